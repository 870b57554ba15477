"""PointCloudTransformer on the HIP path vs the same class's stock-op composite on the GPU (bench.py is not involved).

    python scripts/bench_pct.py [--batch 256] [--points 1024,2048] [--steps 5] [--out profiles/pct_bench.json]

The reference's configs/model/pct.yaml dims (4 layers, 4 heads, 128 / 256, 40 classes), synthetic weights (peekvit_amd.synth.pct_state_dict),
uniform clouds.  Per cloud size: the forward end to end on both paths, the stem alone on both paths (pv_arpe_embed against ARPE.forward), and
the HIP forward's time per kernel (peekvit_amd.ops.KernelTimer; GEMMs split by (N, K, epilogue)).  ms per step = the median of three timed
segments.  The composite materialises [B, N, N] distances and [B, N, k, 6] pair features chunk by chunk; --composite-batch bounds what it is
timed on (its time is scaled to --batch, and the line says so).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from peekvit_amd import engine, ops, synth
from peekvit_amd.models.pct import PointCloudTransformer

DIMS = dict(num_layers=4, num_heads=4, hidden_dim=128, mlp_dim=256, num_classes=40)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--composite-batch", type=int, default=32)
    ap.add_argument("--points", default="1024,2048")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for n in [int(v) for v in a.points.split(",")]:
        kw = dict(DIMS, num_points=n)
        model = PointCloudTransformer(**kw).eval()
        model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.pct_state_dict(kw, 0).items()})
        model = model.to(dev)
        x = torch.from_numpy(synth.synth_points(a.batch, n, seed=0)).to(dev)
        xc = x[:a.composite_batch].contiguous()
        scale = a.batch / xc.shape[0]
        with torch.no_grad():
            for _ in range(a.warmup):
                y = model(x)
            ref = model._composite_forward(xc)
            err = float((y[:xc.shape[0]] - ref).norm() / ref.norm())
            guarded = engine.last_forward_guarded()
            hip = _time(lambda: model(x), a.steps, dev)
            stem = _time(lambda: engine.pct_embed(model, x), a.steps, dev)
            comp = _time(lambda: model._composite_forward(xc), 1, dev) * scale
            comp_stem = _time(lambda: model.embedder(xc), 1, dev) * scale
            with ops.KernelTimer() as kt, engine.precision("f16"):
                engine.pct_forward(model, x)
            torch.cuda.synchronize(dev)
        kernels = {k: {"launches": v["launches"], "ms": round(v["ms"], 4)} for k, v in kt.summary().items()}
        gemms = {str(k): {"launches": v["launches"], "ms": round(v["ms"], 4)} for k, v in kt.members("pv_gemm_bf16").items()}
        line = {"num_points": n, "batch": a.batch, "k": model.embedder.k, "clouds_per_s": round(a.batch / hip, 1), "hip_ms": round(hip * 1e3, 3),
                "composite_ms": round(comp * 1e3, 3), "composite_timed_on_batch": int(xc.shape[0]), "speedup": round(comp / hip, 2),
                "stem_hip_ms": round(stem * 1e3, 3), "stem_composite_ms": round(comp_stem * 1e3, 3), "stem_speedup": round(comp_stem / stem, 2),
                "rel_l2_vs_composite": err, "guarded": guarded, "kernels_ms": kernels, "gemms_ms": gemms}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del model, x, xc
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
