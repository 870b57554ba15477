"""One training step of AdaptiveVisionTransformer on the fused dense path (`set_fused_training`), on the packed live rows (`set_packed_training`,
DESIGN.md section 30) and on the fused dense path again (bench.py is not involved).

    python scripts/bench_avit_packed_train.py [--dims avit_t,avit_s] [--gate-centers 30,5] [--batch 256] [--steps 20] [--warmup 3] [--precision auto]
                                              [--halted-depth 3] [--paths dense,packed,dense_again] [--out profiles/avit_packed_train_bench.json]

The set-up is scripts/bench_avit_train.py's: the reference's avit_{t,s}_16_224 dims at 224 pixels, synthetic weights, one model object per configuration
in one process; a step is forward, cross-entropy plus the two A-ViT terms of configs/loss/avit_losses.yaml, backward, Adam.  Per configuration, in
this order: fused dense, packed, fused dense again - ms per step = the median of three timed segments, and the peak allocated memory of each.  The
optimizer steps are real, so the mean depth drifts while the three are timed; `row_share` is the share of the dense rows the packed steps ran
(engine.avit_train_rows / avit_train_dense_rows over the timed steps), `rows_per_layer` that of the last step, layer by layer.

`halted` (gate_center 5 only): the same model is trained on until its mean depth is below --halted-depth, then FROZEN (learning rate 0, so a step costs
what it cost) and both paths are timed on it: the state in which most tokens have halted.

`host_read_ms`: per layer, the GPU time between the end of a pack step and the host's return from reading the next row count (one more packed step
with engine.avit_train_gaps set): what the per-layer synchronisation leaves the GPU idle for.  `kernels_*`: ops.KernelTimer's per-kernel times of one
step of each path.

Past 208 tokens: `--dims ref_small --size 160` (or 224) runs the reference's small dims (patch 8, hidden 256, 4 heads, 4 layers) at
401 / 785 tokens; "dense" is then the LONG fused pass and "packed" the long packed one, and `--composite` first times the same step with both switches
off - the composite step a tree without the long rules takes at these shapes (`composite_ms`, `fused_speedup_vs_composite`).  `break_even_row_share`:
the row share at which the packed step would cost what the fused one does, if its cost above the host reads scaled with its rows
((fused - host reads) / (packed - host reads) x row share)."""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from bench_avit_train import DIMS, TARGET_DEPTH, W_PONDER, W_PRIOR, _measure
from peekvit_amd import engine, ops, synth
from peekvit_amd.losses import AViTDPriorLoss, AViTPonderLoss
from peekvit_amd.models.adavit import AdaptiveVisionTransformer

LONG_DIMS = {"ref_small": dict(num_layers=4, num_heads=4, hidden_dim=256, mlp_dim=768, patch_size=8)}


def _three(model, step, a, dev, line, prefix=""):
    """fused dense -> packed -> fused dense again on `model`; fills `line`."""
    B, S, L = a.batch, model.seq_length, len(model.encoder.layers)
    order = [(tag, packed) for tag, packed in (("dense", False), ("packed", True), ("dense_again", False)) if tag in a.paths]
    for tag, packed in order:
        model.set_packed_training(packed)
        rows0, dense0, syncs0 = engine.avit_train_rows, engine.avit_train_dense_rows, engine.avit_train_syncs
        k = prefix + tag
        line[f"{k}_ms"], line[f"{k}_peak_mib"] = _measure(step, a.steps, a.warmup, dev)
        line[f"{k}_mean_depth"] = round(float(model.encoder.counter_token.mean()), 3)
        ran = engine.avit_train_dense_rows - dense0
        assert (ran > 0) == packed, tag
        if packed:
            line[prefix + "row_share"] = round((engine.avit_train_rows - rows0) / ran, 4)
            line[prefix + "rows_per_layer"] = [round(r / (B * S), 4) for r in engine.avit_train_last_rows]
            line[prefix + "host_reads_per_step"] = (engine.avit_train_syncs - syncs0) / (ran // (B * S * L))
    if len(order) == 3:
        line[prefix + "speedup"] = round(0.5 * (line[prefix + "dense_ms"] + line[prefix + "dense_again_ms"]) / line[prefix + "packed_ms"], 3)
    for tag, packed in order[:2]:
        model.set_packed_training(packed)
        engine.avit_train_gaps = [] if packed else None
        with ops.KernelTimer() as kt:
            step()
        torch.cuda.synchronize(dev)
        s = kt.summary()
        line[f"{prefix}kernels_{tag}_ms"] = round(sum(v["ms"] for v in s.values()), 3)
        line[f"{prefix}kernel_summary_{tag}_ms"] = {k: {"launches": v["launches"], "ms": round(v["ms"], 3)} for k, v in sorted(s.items(), key=lambda kv: -kv[1]["ms"])}
        if packed:
            gaps = [round(e0.elapsed_time(e1), 4) for e0, e1 in engine.avit_train_gaps]
            engine.avit_train_gaps = None
            line[prefix + "host_read_ms"] = gaps
            line[prefix + "host_read_total_ms"] = round(sum(gaps), 3)
    model.set_packed_training(False)


def _config(name, gate_center, a, dev):
    cfg = dict(dict(patch_size=16), **{**DIMS, **LONG_DIMS}[name], image_size=a.size, num_classes=10)
    model = AdaptiveVisionTransformer(**cfg, gate_center=gate_center)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(cfg, seed=0).items()}, strict=True)
    model = model.to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-5)
    x = torch.from_numpy(synth.synth_images(a.batch, a.size, seed=0, name="avit")).to(dev)
    target = torch.arange(a.batch, device=dev) % cfg["num_classes"]
    prior, ponder = AViTDPriorLoss(TARGET_DEPTH), AViTPonderLoss()

    def step():
        opt.zero_grad(set_to_none=True)
        loss = F.cross_entropy(model(x), target) + W_PRIOR * prior(model) + W_PONDER * ponder(model)
        loss.backward()
        opt.step()

    line = {"model": name, "gate_center": gate_center, "batch": a.batch, "precision": a.precision, "tokens": model.seq_length, "image_size": a.size}
    if a.composite:          # both switches off: the stock composite under autograd
        line["composite_ms"], line["composite_peak_mib"] = _measure(step, a.steps, a.warmup, dev)
    model.set_fused_training(True)
    _three(model, step, a, dev, line)
    if a.composite and "dense_ms" in line:
        line["fused_speedup_vs_composite"] = round(line["composite_ms"] / line["dense_ms"], 3)
    if "speedup" in line and "host_read_total_ms" in line:
        fused, gap = 0.5 * (line["dense_ms"] + line["dense_again_ms"]), line["host_read_total_ms"]
        line["break_even_row_share"] = round(line["row_share"] * (fused - gap) / max(line["packed_ms"] - gap, 1e-9), 4)
    if gate_center == 5 and a.halted_depth > 0:
        model.set_packed_training(True)
        extra = 0
        while float(model.encoder.counter_token.mean()) >= a.halted_depth and extra < a.halted_max_steps:
            step()
            extra += 1
        line["halted_extra_steps"] = extra
        for g in opt.param_groups:          # frozen: the optimizer still runs, the parameters stay
            g["lr"] = 0.0
        _three(model, step, a, dev, line, prefix="halted_")
    return line


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--dims", default="avit_t,avit_s")
    p.add_argument("--gate-centers", default="30,5")
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--precision", default="auto", choices=["auto", "bf16"])
    p.add_argument("--halted-depth", type=float, default=3.0)
    p.add_argument("--halted-max-steps", type=int, default=400)
    p.add_argument("--paths", default="dense,packed,dense_again", help="which of the three measurements to run (one alone: a profiler's run of that path)")
    p.add_argument("--size", type=int, default=224, help="image size (with --dims ref_small: 160 -> 401 tokens, 224 -> 785)")
    p.add_argument("--composite", action="store_true", help="first time the step with both switches off (the stock composite under autograd)")
    p.add_argument("--out", default="")
    a = p.parse_args()
    a.paths = a.paths.split(",")
    dev = torch.device("cuda:0")
    lines = []
    with engine.precision(a.precision):
        for name in a.dims.split(","):
            for gc in a.gate_centers.split(","):
                line = _config(name, float(gc), a, dev)
                lines.append(line)
                print(json.dumps({k: v for k, v in line.items() if "kernel_summary" not in k}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "configs": lines}, f, indent=1)


if __name__ == "__main__":
    main()
