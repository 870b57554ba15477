"""ResidualViT token compaction vs the dense forward (bench.py is not involved).

    python scripts/bench_residual_sparse.py [--batch 2048] [--steps 5] [--out profiles/residual_sparse_bench.json]
    python scripts/bench_residual_sparse.py --dense-only --package-root DIR --out parent.json      # the dense numbers of another checkout
    python scripts/bench_residual_sparse.py --parent parent.json --out profiles/residual_sparse_bench.json
    python scripts/bench_residual_sparse.py --dims small --image-size 160 ...      # patch 8, hidden 256, 4 heads, 4 layers
    python scripts/bench_residual_sparse.py --switch-point                         # resident vs streaming ragged attention on segments <= 208

ViT-B/16 dims, random images, precision mode `f16`, two weight sets: "sparse" = synth.residual_sparse_state_dict (gate weights x 4) with
gate_bias=1, whose gates mask about half of the tokens, and "stock" = the plain synthetic weights with gate_bias=10, which mask nothing (full
row share).  Per weight set and budget 0.2 / 0.5 / 0.8: img/s of the dense forward in THREE repeats of three timed segments each (their
spread is what a difference must exceed), img/s of the compacting forward, the executed row share, the GPU time behind each per-layer host
read, and the per-kernel table of one compacting and one dense forward (a separate pass: ops.KernelTimer brackets every launch).
--dense-only measures the dense forward alone with the package found under --package-root (a checkout of the parent commit: this script
needs nothing the parent lacks); --parent merges such a file.  A failed step raises: nothing is started after it.
--dims small --image-size S measures the ResidualViT the reference ships (patch 8, hidden 256, 4 heads of 64, 4 layers, mlp 768) at S px: past 208
rows per image the compacting forward is the long path, and a line also carries every layer's longest segment, the layers that ran the streaming
ragged attention and the fraction of that kernel's workgroups that found no query of their segment to work on.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

_a = argparse.ArgumentParser()
_a.add_argument("--batch", type=int, default=2048)
_a.add_argument("--steps", type=int, default=5)
_a.add_argument("--warmup", type=int, default=2)
_a.add_argument("--budgets", default="0.2,0.5,0.8")
_a.add_argument("--weights", default="sparse,stock")
_a.add_argument("--gate-gain", type=float, default=4.0)
_a.add_argument("--dims", default="b16", choices=("b16", "small"))
_a.add_argument("--image-size", type=int, default=224)
_a.add_argument("--switch-point", action="store_true", help="time the resident against the streaming ragged attention on segments <= 208 and exit")
_a.add_argument("--dense-only", action="store_true")
_a.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
_a.add_argument("--parent", default="", help="JSON written by a --dense-only run of the parent commit")
_a.add_argument("--out", default="")
ARGS = _a.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.package_root))

import numpy as np
import torch

from peekvit_amd import engine, ops, synth
from peekvit_amd.models.residualvit import ResidualVisionTransformer

MODE = "f16"
EXTRA = dict(gate_type="sigmoid", gate_temp=1, add_budget_token="learnable", gate_threshold=0.5)
SMALL = dict(patch_size=8, num_layers=4, num_heads=4, hidden_dim=256, mlp_dim=768, num_classes=10)      # the ResidualViT the reference ships


def _state_dict(cfg, which):
    sd = synth.synth_state_dict(cfg, "residualvit", 0)
    if which == "sparse":           # synth.residual_sparse_state_dict, restated so that a parent checkout without it measures the same weights
        for k in sd:
            if k.endswith("residual_gate.projection.weight"):
                sd[k] = synth.round_to_bf16((sd[k].astype(np.float64) * ARGS.gate_gain).astype(np.float32))
    return {k: torch.from_numpy(v.copy()) for k, v in sd.items()}


def _segments(fn, steps, dev):
    segs = []
    for _ in range(3):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize(dev)
        segs.append((time.perf_counter() - t0) / steps)
    return segs


def _kernels(fn, dev):
    with ops.KernelTimer() as kt:
        fn()
        torch.cuda.synchronize(dev)
    return {k: {"launches": v["launches"], "ms": round(v["ms"], 3)} for k, v in sorted(kt.summary().items(), key=lambda kv: -kv[1]["ms"])}


def _empty_workgroups(model, x, dev):
    """One compacting forward with every streaming ragged attention launch recorded: per such layer (longest segment, fraction of the launch's
    B * H * ceil(longest / 64) workgroups whose first query lies past their own segment)."""
    real, seen = ops.attention_varlen_w_stream, []
    ops.attention_varlen_w_stream = lambda qkv, out, seg, lm, max_len, H, dh: (seen.append((seg, max_len)), real(qkv, out, seg, lm, max_len, H, dh))[1]
    try:
        model(x)
        torch.cuda.synchronize(dev)
    finally:
        ops.attention_varlen_w_stream = real
    out = []
    for seg, max_len in seen:
        lens = (seg[1:] - seg[:-1]).long()
        nqb = (max_len + 63) // 64
        out.append({"longest": int(max_len), "empty_fraction": round(1.0 - float(((lens + 63) // 64).sum()) / (lens.numel() * nqb), 4)})
    return out


def switch_point(dev):
    """The resident and the streaming ragged attention on the same packed rows, every segment <= 208: ms per launch, median of three segments."""
    from peekvit_amd import _lib
    H, dh, B = 4, 64, ARGS.batch
    res = []
    with engine.precision(MODE):
        for lo, hi in ((40, 100), (100, 208), (180, 208), (208, 208)):
            g = torch.Generator().manual_seed(hi)
            lens = torch.randint(lo, hi + 1, (B,), generator=g)
            lens[0] = hi
            seg = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)]).to(torch.int32).to(dev)
            R_ = int(lens.sum())
            qkv = torch.randn(R_, 3 * H * dh, generator=g).to(_lib.operand_dtype()).to(dev)
            lm = torch.zeros(R_, device=dev)
            out = torch.empty((R_, H * dh), dtype=qkv.dtype, device=dev)
            line = {"segments": [lo, hi], "batch": B, "rows": R_, "heads": H}
            for name, fn in (("resident", ops.attention_varlen_w), ("streaming", ops.attention_varlen_w_stream)):
                run = lambda: fn(qkv, out, seg, lm, hi, H, dh)
                for _ in range(3):
                    run()
                line[name + "_ms"] = round(sorted(_segments(run, 20, dev))[1] * 1e3, 4)
            line["streaming_vs_resident"] = round(line["streaming_ms"] / line["resident_ms"], 3)
            print(json.dumps(line), flush=True)
            res.append(line)
    return res


def main():
    a = ARGS
    dev = torch.device("cuda:0")
    if a.switch_point:
        res = switch_point(dev)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        return
    x = torch.randn(a.batch, 3, a.image_size, a.image_size, generator=torch.Generator().manual_seed(0)).to(dev)
    base = dict(synth.MODEL_CONFIGS["vit_b_16"], image_size=a.image_size) if a.dims == "b16" else dict(SMALL, image_size=a.image_size)
    parent = {(r["weights"], r["budget"]): r for r in json.load(open(a.parent))} if a.parent else {}
    lines = []
    for which in a.weights.split(","):
        gate_bias = 1 if which == "sparse" else 10
        cfg = dict(base, **EXTRA, gate_bias=gate_bias)
        model = ResidualVisionTransformer(**cfg).eval()
        model.load_state_dict(_state_dict(cfg, which))
        model = model.to(dev)
        for budget in [float(v) for v in a.budgets.split(",")]:
            model.set_budget(budget)
            fwd = lambda: model(x)
            with torch.no_grad(), engine.precision(MODE):
                for _ in range(a.warmup):
                    fwd()
                repeats = [_segments(fwd, a.steps, dev) for _ in range(3)]
                med = [sorted(s)[1] for s in repeats]
                line = {"weights": which, "gate_bias": gate_bias, "gate_gain": a.gate_gain if which == "sparse" else 1.0, "budget": budget,
                        "batch": a.batch, "mode": MODE, "dims": a.dims, "image_size": a.image_size, "rows_per_image": synth.seq_length(cfg) + 1,
                        "dense_img_per_s_repeats": [round(a.batch / t, 1) for t in med],
                        "dense_segments_ms": [[round(t * 1e3, 3) for t in s] for s in repeats],
                        "dense_img_per_s": round(a.batch / sorted(med)[1], 1),
                        "dense_spread_rel": round((max(med) - min(med)) / sorted(med)[1], 5)}
                if not a.dense_only:
                    line["dense_kernels"] = _kernels(fwd, dev)
                    model.set_token_compaction(True)
                    for _ in range(a.warmup):
                        fwd()
                    r0, d0, s0, f0 = engine.sparse_rows, engine.sparse_dense_rows, engine.sparse_syncs, engine.sparse_dense_forwards
                    segs = _segments(fwd, a.steps, dev)
                    n_fwd = 3 * a.steps
                    syncs = (engine.sparse_syncs - s0) / n_fwd
                    if engine.sparse_dense_forwards != f0 or engine.sparse_rows == r0:
                        raise RuntimeError("the compacting forward took the dense path")
                    share = (engine.sparse_rows - r0) / float(engine.sparse_dense_rows - d0)
                    engine.sparse_gaps = []
                    fwd()
                    torch.cuda.synchronize(dev)
                    gaps = [e0.elapsed_time(e1) for e0, e1 in engine.sparse_gaps]
                    engine.sparse_gaps = None
                    dt = sorted(segs)[1]
                    line.update({"compact_img_per_s": round(a.batch / dt, 1), "compact_segments_ms": [round(t * 1e3, 3) for t in segs],
                                 "executed_row_share": round(share, 4), "rows_per_layer": list(engine.sparse_last_rows),
                                 "host_syncs_per_forward": syncs,
                                 "sync_gap_ms_per_layer": [round(g, 4) for g in gaps], "sync_gap_ms_per_forward": round(sum(gaps), 3),
                                 "compact_vs_dense": round(sorted(med)[1] / dt, 4), "compact_kernels": _kernels(fwd, dev)})
                    line.update({"longest_segment_per_layer": list(engine.sparse_last_max_len),
                                 "streaming_attention_layers": _empty_workgroups(model, x, dev)})
                    model.set_token_compaction(False)
                    p = parent.get((which, budget))
                    if p is not None:
                        line.update({"parent_dense_img_per_s": p["dense_img_per_s"], "parent_dense_img_per_s_repeats": p["dense_img_per_s_repeats"],
                                     "compact_vs_parent_dense": round(line["compact_img_per_s"] / p["dense_img_per_s"], 4),
                                     "dense_vs_parent_dense": round(line["dense_img_per_s"] / p["dense_img_per_s"], 4)})
            print(json.dumps({k: v for k, v in line.items() if not k.endswith("_kernels")}), flush=True)
            lines.append(line)
        del model
    if a.out:
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
