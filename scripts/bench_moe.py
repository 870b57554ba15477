"""Routed top-1 MoE forward vs the plain VisionTransformer of the same dims and vs the reference's dense-expert composite (bench.py is not involved).

    python scripts/bench_moe.py [--batch 2048] [--steps 5] [--out profiles/moe_bench.json]

ViT-B/16 dims (224 / patch 16, D 768, 12 heads, MLP 3072, 12 layers), synthetic weights, random images.  Lines: the ViT forward; the same dims
with mlp_moes = [1, 8] * 6 (routed MLP experts on alternate layers); the same with attn_moes = [1, 4] * 6 as well; and the stock-op composite of
the MLP MoE model on the GPU (every expert on every token, then the one-hot einsum: the reference's arithmetic).  Each: img/s and ms/step, the
median of three timed segments, package power and shader clock over the segments (peekvit_amd/telemetry.py).  One JSON line per configuration.
Weights: peekvit_amd.synth.moe_state_dict (the generator bench.py's ViT-B/16 weights come from; ~20 s of host time for the 330 M parameters);
the ViT line loads the same tensors as the one-expert halves.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from peekvit_amd import engine, synth, telemetry
from peekvit_amd.models.moevit import VisionTransformerMoE
from peekvit_amd.models.vit import VisionTransformer

DIMS = dict(image_size=224, patch_size=16, num_layers=12, num_heads=12, hidden_dim=768, mlp_dim=3072, num_classes=1000)


def _time(fn, steps, dev, sampler):
    segs = []
    with sampler.window() as pw:
        for _ in range(3):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize(dev)
            segs.append((time.perf_counter() - t0) / steps)
    return sorted(segs)[1], segs, pw.result()


def _moe(mlp_moes=None, attn_moes=None):
    m = VisionTransformerMoE(**DIMS, mlp_moes=mlp_moes, attn_moes=attn_moes).eval()
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.moe_state_dict(DIMS, mlp_moes, attn_moes, seed=0).items()})
    return m


def _vit_from(moe):
    sd = {}
    for k, v in moe.state_dict().items():
        if "gating_network" in k:
            continue
        sd["class_tokens" if k == "class_token" else k.replace("self_attention.experts.0.", "self_attention.").replace("mlp.experts.0.", "mlp.")] = v
    vit = VisionTransformer(**DIMS).eval()
    vit.load_state_dict({k: v for k, v in sd.items() if k in vit.state_dict()})
    return vit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--composite-steps", type=int, default=1)
    ap.add_argument("--out", default="")
    ap.add_argument("--configs", default="vit,mlp,composite,attn", help="subset of vit, mlp, composite, attn (a profiler run takes one)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sampler = telemetry.sampler(0)
    x = torch.randn(a.batch, 3, 224, 224, generator=torch.Generator().manual_seed(0)).to(dev)
    lines, base = [], None

    def run(name, model, fn, steps):
        nonlocal base
        with torch.no_grad():
            for _ in range(a.warmup):
                fn()
            n0 = engine.moe_routed_layers
            dt, segs, pw = _time(fn, steps, dev, sampler)
            routed = (engine.moe_routed_layers - n0) / (3 * steps)
        line = {"config": name, "batch": a.batch, "img_per_s": round(a.batch / dt, 1), "ms_per_step": round(dt * 1e3, 3),
                "segments_ms": [round(t * 1e3, 3) for t in segs], "routed_halves_per_forward": routed,
                "guarded": engine.last_forward_guarded(), "power": pw}
        if base is None:
            base = dt
        line["vs_vit"] = round(base / dt, 3)
        print(json.dumps(line), flush=True)
        lines.append(line)
        return dt

    want = set(a.configs.split(","))
    moe = _moe(mlp_moes=[1, 8] * 6)
    if "vit" in want:
        vit = _vit_from(moe).to(dev)
        run("vit_b16", vit, lambda: vit(x), a.steps)
        del vit
    moe = moe.to(dev)
    dt_moe = dt_comp = None
    if "mlp" in want:
        dt_moe = run("vit_b16 dims, mlp_moes=[1,8]*6 (routed)", moe, lambda: moe(x), a.steps)
    if "composite" in want:
        dt_comp = run("vit_b16 dims, mlp_moes=[1,8]*6 (stock-op composite: every expert on every token)", moe,
                      lambda: moe._composite_forward(x), a.composite_steps)
    if dt_moe and dt_comp:
        lines[-1]["routed_speedup_vs_composite"] = round(dt_comp / dt_moe, 3)
        print(json.dumps({"routed_speedup_vs_composite": round(dt_comp / dt_moe, 3)}), flush=True)
    del moe
    torch.cuda.empty_cache()
    if "attn" in want:
        moe = _moe(mlp_moes=[1, 8] * 6, attn_moes=[1, 4] * 6).to(dev)
        run("vit_b16 dims, mlp_moes=[1,8]*6, attn_moes=[1,4]*6 (routed)", moe, lambda: moe(x), a.steps)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
