"""One training step of ViT / RankViT / ResidualViT at more than 208 token rows: the HIP training path (streaming attention pair)
against the stock-op composite these shapes trained on before (`PEEKVIT_AMD_TRAIN=torch`).  bench.py is not involved.

    python scripts/bench_long_train.py [--batch 256] [--steps 5] [--warmup 2] [--precision auto] [--out profiles/long_train.json]

Models: the reference's small configs (configs/model/{vit,rankvit,residualvit}.yaml dims: patch 8, hidden 256, mlp 768, 4 layers, 4 heads, so head
dim 64) as VisionTransformer, RankVisionTransformer (keep 0.5 at layers 1 and 2) and ResidualVisionTransformer (sigmoid gates, learnable budget
token), at 160 px (401 / 402 rows) and 224 px (785 / 786 rows).  Timed: forward, cross-entropy, backward, Adam - the median of three segments of
--steps steps with a device synchronise at both ends - and the peak allocated memory.

Without --leg the script is a driver: every (model, image size, side) is a child process of its own under `timeout`, the composite side with
PEEKVIT_AMD_TRAIN=torch in its environment; the legs are chained and the first one that fails, aborts or runs out of time ends the run - nothing
more is started on the device behind it.  The HIP leg also runs one step under ops.KernelTimer: the kernel summary and the attention launches'
share of the step's kernel time."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIMS = dict(patch_size=8, num_layers=4, num_heads=4, hidden_dim=256, mlp_dim=768, num_classes=100)
MODELS = ("vit", "rankvit", "residualvit")
SIZES = (160, 224)
LEG_SECONDS = 300


def _build(name, image_size):
    import torch
    from peekvit_amd.models.rankvit import RankVisionTransformer
    from peekvit_amd.models.residualvit import ResidualVisionTransformer
    from peekvit_amd.models.vit import VisionTransformer
    torch.manual_seed(0)
    cfg = dict(DIMS, image_size=image_size)
    if name == "vit":
        m = VisionTransformer(**cfg)
    elif name == "rankvit":
        m = RankVisionTransformer(**cfg, rankvit_layers=[1, 2])
        m.set_budget(0.5)
    else:
        m = ResidualVisionTransformer(**cfg, gate_type="sigmoid", gate_temp=1, gate_bias=0, gate_threshold=0.5, add_budget_token="learnable")
    with torch.no_grad():
        torch.nn.init.normal_(m.head.weight, std=0.05)          # (the reference's zero head gives the trunk zero gradients)
        torch.nn.init.normal_(m.class_tokens, std=0.02)
    return m


def _time(fn, steps, dev):
    import torch
    segs = []
    for _ in range(3):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize(dev)
        segs.append((time.perf_counter() - t0) / steps)
    return sorted(segs)[1], segs


def leg(a, name, image_size, side):
    import torch
    import torch.nn.functional as F
    from peekvit_amd import engine, ops, synth, train_engine
    assert (os.environ.get("PEEKVIT_AMD_TRAIN", "hip") == "torch") == (side == "torch")
    dev = torch.device("cuda:0")
    with engine.precision(a.precision):
        model = _build(name, image_size).to(dev).train()
        rows = model.seq_length + (1 if name == "residualvit" else 0)
        opt = torch.optim.Adam(model.parameters(), lr=1e-4)
        x = torch.from_numpy(synth.synth_images(a.batch, image_size, seed=0)).to(dev)
        target = torch.arange(a.batch, device=dev) % DIMS["num_classes"]

        def step():
            opt.zero_grad(set_to_none=True)
            F.cross_entropy(model(x), target).backward()
            opt.step()

        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        n0 = ops.launch_count
        dt, segs = _time(step, a.steps, dev)
        line = {"model": name, "image_size": image_size, "rows": rows, "side": side, "batch": a.batch, "precision": a.precision,
                "ms_per_step": round(dt * 1e3, 3), "segments_ms": [round(t * 1e3, 3) for t in segs],
                "peak_mib": round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1), "launches_per_step": (ops.launch_count - n0) / (3 * a.steps),
                "steps_skipped": train_engine.steps_skipped}
        assert (line["launches_per_step"] > 40) == (side == "hip"), line          # a side that ran the other side's path measures nothing
        if side == "hip":
            with ops.KernelTimer() as kt:
                step()
            torch.cuda.synchronize(dev)
            s = kt.summary()
            total = sum(v["ms"] for v in s.values())
            line["kernels_ms"] = round(total, 3)
            line["kernel_summary_ms"] = {k: {"launches": v["launches"], "ms": round(v["ms"], 3)} for k, v in sorted(s.items(), key=lambda kv: -kv[1]["ms"])}
            line["attention_share"] = {k: round(v["ms"] / total, 4) for k, v in s.items() if k.startswith("pv_attention")}
    return line


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--precision", default="auto", choices=["auto", "bf16"])
    p.add_argument("--models", default=",".join(MODELS))
    p.add_argument("--sizes", default=",".join(map(str, SIZES)))
    p.add_argument("--out", default="")
    p.add_argument("--leg", default="")
    a = p.parse_args()
    if a.leg:                                                  # a child: one measurement, one JSON line
        name, size, side = a.leg.split(":")
        print("RESULT " + json.dumps(leg(a, name, int(size), side)), flush=True)
        return 0
    lines = []
    for name in a.models.split(","):
        for size in a.sizes.split(","):
            pair = {}
            for side in ("hip", "torch"):
                env = dict(os.environ)
                env.pop("PEEKVIT_AMD_TRAIN", None)
                if side == "torch":
                    env["PEEKVIT_AMD_TRAIN"] = "torch"
                cmd = ["timeout", "-k", "10", str(LEG_SECONDS), sys.executable, os.path.abspath(__file__), "--leg", f"{name}:{size}:{side}",
                       "--batch", str(a.batch), "--steps", str(a.steps), "--warmup", str(a.warmup), "--precision", a.precision]
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
                res = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                if r.returncode != 0 or not res:
                    print(r.stdout[-4000:])
                    print(f"leg {name}:{size}:{side} ended with status {r.returncode}: nothing further is started", flush=True)
                    return r.returncode or 1
                pair[side] = json.loads(res[-1])
                lines.append(pair[side])
                print(json.dumps({k: v for k, v in pair[side].items() if k != "kernel_summary_ms"}), flush=True)
            speedup = round(pair["torch"]["ms_per_step"] / pair["hip"]["ms_per_step"], 3)
            pair["hip"]["speedup_over_composite"] = speedup
            print(json.dumps({"model": name, "image_size": int(size), "rows": pair["hip"]["rows"], "hip_ms": pair["hip"]["ms_per_step"],
                              "composite_ms": pair["torch"]["ms_per_step"], "speedup": speedup, "hip_peak_mib": pair["hip"]["peak_mib"],
                              "composite_peak_mib": pair["torch"]["peak_mib"]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"legs": lines}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
