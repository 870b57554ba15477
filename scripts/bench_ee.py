"""EEResidualVisionTransformer at ViT-B/16 dims: the list forward and the shrinking-batch early_exit against the same-dims
ResidualVisionTransformer, all in one process (bench.py is not involved).

    python scripts/bench_ee.py [--batch 2048] [--rounds 3] [--window 1.2] [--out-dir profiles]

224 / patch 16, D 768, 12 heads, MLP 3072, 12 layers, 1000 classes, sigmoid gates on every layer, learnable budget token, budget 0.5, precision
mode "auto"; weights peekvit_amd.synth.ee_state_dict (the ResidualViT loads the tensors the two models share), seeded images with per-image
contrast and brightness so that confidences differ between images.  Configurations:
  (a) ResidualVisionTransformer forward                       (b) the list forward
  (c) early_exit at four thresholds, chosen from the confidences (b) measured so that the mean exit depth is about L, 0.75 L, 0.5 L, 0.25 L
  (d) exit_layers = [2, 5, 8] at the 0.5 L threshold
Method: every configuration is warmed up with the inputs that are timed (a shrinking batch meets its own set of shapes per threshold);
then `rounds` rounds alternate (a), (b), (c), (d); a timed window runs enough forwards to last about `window` seconds and ends in a device
synchronise; reported: the median over rounds and the spread.  Mean depth, count reads and gathers come from the engine's counters over the
timed windows.  The per-kernel split (ops.KernelTimer) and the idle time behind each count read (engine.ee_gaps) are taken in a SEPARATE pass,
one forward per configuration.  Writes <out-dir>/ee_bench.json and <out-dir>/ee_kernel_summary.txt.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from peekvit_amd import engine, ops, synth
from peekvit_amd.models.eeresidualvit import EEResidualVisionTransformer
from peekvit_amd.models.residualvit import ResidualVisionTransformer

CFG = dict(synth.MODEL_CONFIGS["vit_b_16"])
EXTRA = dict(residual_layers=["attention+mlp"] * CFG["num_layers"], gate_temp=1, add_input=False, gate_type="sigmoid", gate_threshold=0.5,
             gate_bias=10, add_budget_token="learnable")
BUDGET = 0.5


def images(batch, dev):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(batch, 3, 224, 224, generator=g)
    gain = 0.3 + 1.4 * torch.rand(batch, 1, 1, 1, generator=g)
    offset = 2.0 * torch.rand(batch, 3, 1, 1, generator=g) - 1.0
    return (x * gain + offset).to(dev)


def depth_for(conf, t, layers=None):
    """Mean number of layers run per image at threshold t (conf fp64 [L, B]; an image that exits at layer i ran i + 1 layers)."""
    L, B = conf.shape
    depth = np.full(B, L)
    for i in sorted(range(L) if layers is None else layers, reverse=True):
        depth[conf[i] >= t] = i + 1
    return float(depth.mean())


def threshold_for(conf, target):
    """The smallest measured confidence value whose mean depth reaches `target` layers (mean depth grows with the threshold)."""
    cand = np.unique(conf)
    lo, hi = 0, len(cand) - 1
    while lo < hi:
        mid = (lo + hi) // 2
        if depth_for(conf, cand[mid]) >= target:
            hi = mid
        else:
            lo = mid + 1
    return float(cand[lo])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.2, help="seconds of work per timed window")
    ap.add_argument("--out-dir", default="profiles")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    L, B = CFG["num_layers"], a.batch
    sd = {k: torch.from_numpy(v.copy()) for k, v in synth.ee_state_dict(dict(CFG, **EXTRA), seed=0).items()}
    ee = EEResidualVisionTransformer(**CFG, **EXTRA).eval()
    ee.load_state_dict(sd, strict=True)
    res = ResidualVisionTransformer(**CFG, **EXTRA).eval()
    missing = res.load_state_dict({k: v for k, v in sd.items() if k in res.state_dict()}, strict=True)
    del sd, missing
    ee, res = ee.to(dev), res.to(dev)
    ee.set_budget(BUDGET)
    res.set_budget(BUDGET)
    x = images(B, dev)

    with torch.no_grad():
        outs = ee(x)
    conf = np.stack([torch.softmax(o.double(), dim=-1).max(dim=-1).values.cpu().numpy() for o in outs[:L]])
    targets = {"L": None, "0.75L": 0.75 * L, "0.5L": 0.5 * L, "0.25L": 0.25 * L}
    thr = {k: (2.0 if t is None else threshold_for(conf, t)) for k, t in targets.items()}
    configs = [("a_residualvit", lambda: res(x), None), ("b_list", lambda: ee(x), None)]
    for k in targets:
        configs.append((f"c_exit_{k}", (lambda t=thr[k]: ee.early_exit(x, t)), dict(threshold=thr[k], predicted_mean_depth=depth_for(conf, thr[k]))))
    configs.append(("d_exit_0.5L_layers_2_5_8", lambda: ee.early_exit(x, thr["0.5L"], exit_layers=[2, 5, 8]),
                    dict(threshold=thr["0.5L"], exit_layers=[2, 5, 8], predicted_mean_depth=depth_for(conf, thr["0.5L"], [2, 5, 8]))))

    # warm-up: every configuration twice with the timed inputs (self-check probe, weight casts, every shape of its shrinking batch), then a
    # timed single forward sizes its window
    steps, info = {}, {}
    with torch.no_grad():
        for name, fn, _ in configs:
            fn()
            fn()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            steps[name] = max(3, math.ceil(a.window / (time.perf_counter() - t0)))
            info[name] = {"guarded": engine.last_forward_guarded()}
        times = {name: [] for name, _, _ in configs}
        counters = {name: [0, 0, 0, 0] for name, _, _ in configs}        # forwards, image-layers, count reads, gathers
        for _ in range(a.rounds):
            for name, fn, _ in configs:
                c0 = (engine.ee_image_layers, engine.ee_syncs, engine.ee_gathers)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(steps[name]):
                    fn()
                torch.cuda.synchronize(dev)
                times[name].append((time.perf_counter() - t0) / steps[name])
                c = counters[name]
                c[0] += steps[name]
                c[1] += engine.ee_image_layers - c0[0]
                c[2] += engine.ee_syncs - c0[1]
                c[3] += engine.ee_gathers - c0[2]

        # separate pass: per-kernel split and the idle time behind each count read
        split, idle = {}, {}
        for name, fn, _ in configs:
            engine.ee_gaps = []
            with ops.KernelTimer() as kt:
                fn()
            torch.cuda.synchronize(dev)
            split[name] = kt.summary()
            idle[name] = {"reads": len(engine.ee_gaps), "idle_ms": round(sum(e0.elapsed_time(e1) for e0, e1 in engine.ee_gaps), 3)}
            engine.ee_gaps = None

    lines = []
    base_b = sorted(times["b_list"])[len(times["b_list"]) // 2]
    base_a = sorted(times["a_residualvit"])[len(times["a_residualvit"]) // 2]
    for name, _, extra in configs:
        ts = sorted(times[name])
        med = ts[len(ts) // 2]
        fw, il, reads, gathers = counters[name]
        line = {"config": name, "batch": B, "img_per_s": round(B / med, 1), "ms_per_step": round(med * 1e3, 3),
                "rounds_ms": [round(t * 1e3, 3) for t in times[name]], "spread_pct": round(100.0 * (ts[-1] - ts[0]) / med, 2),
                "steps_per_window": steps[name], "vs_a": round(base_a / med, 3), "vs_b": round(base_b / med, 3), **info[name], **(extra or {})}
        if name.startswith(("c_", "d_")):
            line.update(mean_depth=round(il / (fw * B), 3), count_reads_per_forward=round(reads / fw, 2), gathers_per_forward=round(gathers / fw, 2),
                        host_read_idle_ms=idle[name]["idle_ms"], ideal_vs_b=round(L / max(il / (fw * B), 1e-9), 3))
        ksum = sum(v["ms"] for v in split[name].values())
        line["kernel_ms"] = {k: round(v["ms"], 3) for k, v in sorted(split[name].items(), key=lambda kv: -kv[1]["ms"])}
        line["kernel_ms_total"] = round(ksum, 3)
        print(json.dumps({k: v for k, v in line.items() if k != "kernel_ms"}), flush=True)
        lines.append(line)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "ee_bench.json"), "w") as f:
        json.dump({"dims": CFG, "budget": BUDGET, "mode": engine._mode(), "confidence_quantiles_per_layer":
                   [[round(float(q), 4) for q in np.quantile(conf[i], [0, 0.25, 0.5, 0.75, 1])] for i in range(L)], "results": lines}, f, indent=1)
    with open(os.path.join(a.out_dir, "ee_kernel_summary.txt"), "w") as f:
        for line in lines:
            f.write(f"{line['config']}: {line['ms_per_step']} ms/step wall, {line['kernel_ms_total']} ms in kernels (one forward, separate pass)\n")
            for k, v in line["kernel_ms"].items():
                f.write(f"    {k:32s} {split[line['config']][k]['launches']:5d} launches {v:10.3f} ms\n")


if __name__ == "__main__":
    main()
