"""One training step of AdaptiveVisionTransformer with `set_fused_training` off, on and off again (bench.py is not involved).

    python scripts/bench_avit_train.py [--dims avit_t,avit_s] [--gate-centers 30,5] [--batch 256] [--steps 20] [--warmup 3] [--precision auto]
                                       [--out profiles/avit_train_bench.json]

The reference's configs/model/avit_{t,s}_16_224.yaml dims at 224 pixels, synthetic weights (peekvit_amd.synth), one model object per configuration in
one process.  A step is forward, cross-entropy plus the two A-ViT terms of configs/loss/avit_losses.yaml (peekvit_amd.losses, the yaml's weights),
backward, Adam.  Per configuration, in this order: switch off (the stock-op composite under autograd - what the model does without this feature),
switch on, switch off again - ms per step = the median of three timed segments, and the peak allocated memory of each.  With the switch on,
peekvit_amd.ops.KernelTimer gives the time of every kernel of one step: `act_share` is the share of the step's kernel time spent in the two halting
kernels (pv_avit_act_fwd, pv_avit_act_bwd), `kernels_ms` their sum over all kernels (the rest of a step is stock ops and the host)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from peekvit_amd import engine, ops, synth
from peekvit_amd.losses import AViTDPriorLoss, AViTPonderLoss
from peekvit_amd.models.adavit import AdaptiveVisionTransformer

DIMS = {"avit_t": dict(num_layers=12, num_heads=3, hidden_dim=192, mlp_dim=768), "avit_s": dict(num_layers=12, num_heads=6, hidden_dim=384, mlp_dim=1536)}
W_PRIOR, W_PONDER, TARGET_DEPTH = 0.2, 0.0005, 11          # configs/loss/avit_losses.yaml


def _time(fn, steps, dev):
    segs = []
    for _ in range(3):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize(dev)
        segs.append((time.perf_counter() - t0) / steps)
    return sorted(segs)[1]


def _measure(fn, steps, warmup, dev):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    t = _time(fn, steps, dev)
    return round(t * 1e3, 3), round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1)


def _config(name, gate_center, a, dev):
    cfg = dict(DIMS[name], image_size=224, patch_size=16, num_classes=10)
    model = AdaptiveVisionTransformer(**cfg, gate_center=gate_center)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(cfg, seed=0).items()}, strict=True)
    model = model.to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-5)
    x = torch.from_numpy(synth.synth_images(a.batch, 224, seed=0, name="avit")).to(dev)
    target = torch.arange(a.batch, device=dev) % cfg["num_classes"]
    prior, ponder = AViTDPriorLoss(TARGET_DEPTH), AViTPonderLoss()

    def step():
        opt.zero_grad(set_to_none=True)
        loss = F.cross_entropy(model(x), target) + W_PRIOR * prior(model) + W_PONDER * ponder(model)
        loss.backward()
        opt.step()

    line = {"model": name, "gate_center": gate_center, "batch": a.batch, "precision": a.precision}
    for tag, on in (("off", False), ("on", True), ("off_again", False)):
        model.set_fused_training(on)
        n0 = ops.launch_count
        line[f"step_{tag}_ms"], line[f"step_{tag}_peak_mib"] = _measure(step, a.steps, a.warmup, dev)
        line[f"launches_{tag}"] = ops.launch_count - n0          # C-ABI launches over warm-up and timed steps: 0 with the switch off (stock ops only)
        assert on or line[f"launches_{tag}"] == 0, tag
        assert not on or line[f"launches_{tag}"] > 0, tag
        line[f"mean_depth_{tag}"] = round(float(model.encoder.counter_token.mean()), 3)
    model.set_fused_training(True)
    with ops.KernelTimer() as kt:
        step()
    torch.cuda.synchronize(dev)
    s = kt.summary()
    total = sum(v["ms"] for v in s.values())
    act = sum(s[k]["ms"] for k in ("pv_avit_act_fwd", "pv_avit_act_bwd"))
    line["kernels_ms"] = round(total, 3)
    line["act_kernels_ms"] = {k: {"launches": s[k]["launches"], "ms": round(s[k]["ms"], 4)} for k in ("pv_avit_act_fwd", "pv_avit_act_bwd")}
    line["act_share"] = round(act / total, 4)
    line["kernel_summary_ms"] = {k: {"launches": v["launches"], "ms": round(v["ms"], 3)} for k, v in sorted(s.items(), key=lambda kv: -kv[1]["ms"])}
    line["speedup"] = round(0.5 * (line["step_off_ms"] + line["step_off_again_ms"]) / line["step_on_ms"], 3)
    return line


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--dims", default="avit_t,avit_s")
    p.add_argument("--gate-centers", default="30,5")
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--precision", default="auto", choices=["auto", "bf16"])
    p.add_argument("--out", default="")
    a = p.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    with engine.precision(a.precision):
        for name in a.dims.split(","):
            for gc in a.gate_centers.split(","):
                line = _config(name, float(gc), a, dev)
                lines.append(line)
                print(json.dumps({k: v for k, v in line.items() if k != "kernel_summary_ms"}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "configs": lines}, f, indent=1)


if __name__ == "__main__":
    main()
