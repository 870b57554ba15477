"""PointCloudTransformer on the HIP path vs the same class's stock-op composite on the GPU (bench.py is not involved).

    python scripts/bench_pct.py [--batch 256] [--points 1024,2048] [--steps 5] [--out profiles/pct_bench.json]

The reference's configs/model/pct.yaml dims (4 layers, 4 heads, 128 / 256, 40 classes), synthetic weights (peekvit_amd.synth.pct_state_dict),
uniform clouds.  Per cloud size: the forward end to end on both paths, the stem alone on both paths (pv_arpe_embed against ARPE.forward), and
the HIP forward's time per kernel (peekvit_amd.ops.KernelTimer; GEMMs split by (N, K, epilogue)).  ms per step = the median of three timed
segments.  The composite materialises [B, N, N] distances and [B, N, k, 6] pair features chunk by chunk; --composite-batch bounds what it is
timed on (its time is scaled to --batch, and the line says so).

    python scripts/bench_pct.py --ranked [--out profiles/pct_rank_infer_bench.json]

RankPointCloudTransformer (every block sorting) at budgets 0.25 / 0.5 / 0.75 / 1.0 with set_fused_inference on (engine.rank_pct_forward) and off (the
composite, on --composite-batch clouds, scaled), next to the dense PointCloudTransformer forward of the same dims; the forward's time per kernel; the
logits against the composite REPLAYING the forward's kept rows; the clouds whose narrowest keep boundary is under engine.RANK_TIE_GAP.  Then the two
ranking kernels alone on the same norms: pv_rank_order_gap (a sort) against pv_rank_topk_gap (all pairs) at B = --batch, N = 255 / 1023 / 2047 / 4096,
k = N / 2.
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
from peekvit_amd.models.pct import PointCloudTransformer, RankPointCloudTransformer

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


def _load(cls, kw, dev):
    model = cls(**kw).eval()
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.pct_state_dict(kw, 0).items()})
    return model.to(dev)


def _event_ms(fn, reps, dev):
    """ms per call of a launch sequence: `reps` calls between two events on the current stream, the median of three such segments."""
    segs = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        segs.append(e0.elapsed_time(e1) / reps)
    return sorted(segs)[1]


def ranked(a, dev):
    lines = []
    for n in [int(v) for v in a.points.split(",")]:
        kw = dict(DIMS, num_points=n)
        x = torch.from_numpy(synth.synth_points(a.batch, n, seed=0)).to(dev)
        xc = x[:a.composite_batch].contiguous()
        scale = a.batch / xc.shape[0]
        with torch.no_grad():
            dense = _load(PointCloudTransformer, kw, dev)
            for _ in range(a.warmup):
                dense(x)
            dense_ms = _time(lambda: dense(x), a.steps, dev) * 1e3
            del dense
            model = _load(RankPointCloudTransformer, kw, dev)
            model.enable_ranking(True)
            for budget in (0.25, 0.5, 0.75, 1.0):
                model.set_budget(budget)
                model.set_fused_inference(True)
                for _ in range(a.warmup):
                    y = model(x)
                guarded = engine.last_forward_guarded()
                hip = _time(lambda: model(x), a.steps, dev)
                with engine.rank_gaps(a.batch, dev) as gap:
                    y = model(x).clone()
                ties = engine.rank_pct_note_gaps(gap)
                ref = model._replay_probe(xc)
                err = float((y[:xc.shape[0]] - ref).norm() / ref.norm())
                with ops.KernelTimer() as kt, engine.precision("f16"):
                    engine.rank_pct_forward(model, x)
                torch.cuda.synchronize(dev)
                lengths = engine.rank_pct_lengths(model, n)
                model.set_fused_inference(False)
                comp = _time(lambda: model(xc), 1, dev) * scale
                own = model(xc)
                err_own = float((y[:xc.shape[0]] - own).norm() / own.norm())
                kernels = {k: {"launches": v["launches"], "ms": round(v["ms"], 4)} for k, v in kt.summary().items()}
                line = {"ranked": True, "num_points": n, "batch": a.batch, "budget": budget, "kept_lengths": lengths, "hip_ms": round(hip * 1e3, 3),
                        "clouds_per_s": round(a.batch / hip, 1), "composite_ms": round(comp * 1e3, 3), "composite_timed_on_batch": int(xc.shape[0]),
                        "speedup": round(comp / hip, 2), "dense_pct_hip_ms": round(dense_ms, 3), "rel_l2_vs_replaying_composite": err,
                        "rel_l2_vs_composite_own_rows": err_own, "near_ties": ties, "rank_tie_gap": engine.RANK_TIE_GAP, "guarded": guarded,
                        "selfcheck_last": list(engine.selfcheck_last) if engine.selfcheck_last else None, "kernels_ms": kernels}
                print(json.dumps(line), flush=True)
                lines.append(line)
        del model, x, xc
        torch.cuda.empty_cache()
    # the two ranking kernels alone, on the same norms
    for n in (255, 1023, 2047, 4096):
        g = torch.Generator().manual_seed(n)
        norms = (torch.rand(a.batch, n, generator=g) * 0.01 + 1.0).to(dev)          # norms of a cloud lie within a percent of each other
        k = n // 2
        gap = torch.full((a.batch,), float("inf"), device=dev)
        assert torch.equal(ops.rank_order(norms, k, gap), ops.rank_topk(norms, k, gap))
        sort_ms = _event_ms(lambda: ops.rank_order(norms, k, gap), 20, dev)
        pairs_ms = _event_ms(lambda: ops.rank_topk(norms, k, gap), 20, dev)
        line = {"rank_kernels": True, "batch": a.batch, "N": n, "k": k, "pv_rank_order_gap_ms": round(sort_ms, 4), "pv_rank_topk_gap_ms": round(pairs_ms, 4),
                "speedup": round(pairs_ms / sort_ms, 2)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--composite-batch", type=int, default=32)
    ap.add_argument("--points", default="1024,2048")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--ranked", action="store_true", help="RankPointCloudTransformer's HIP eval forward over budgets, and the two ranking kernels")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.ranked:
        lines = ranked(a, dev)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(lines, f, indent=1)
        return
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
