"""ResidualViT training on the packed live rows vs the dense training step (bench.py is not involved).

    python scripts/bench_residual_sparse_train.py [--batch 1024] [--steps 3] [--out profiles/residual_sparse_train_bench.json]
    python scripts/bench_residual_sparse_train.py --dense-only --package-root DIR --out parent.json      # the dense step of another checkout
    python scripts/bench_residual_sparse_train.py --parent parent.json --out profiles/residual_sparse_train_bench.json
    python scripts/bench_residual_sparse_train.py --dims small --image-size 160 --batch 256 ...      # patch 8, hidden 256, 4 heads, 4 layers

One training step = forward, cross-entropy + the budget loss of configs/loss/crossentropy_mse.yaml, backward, Adam.  ViT-B/16 dims, random images,
fp16 operands under the loss scale (precision mode "auto", what training uses by default), two weight sets: "sparse" =
synth.residual_sparse_state_dict (gate weights x 4) with gate_bias=1 and "stock" = the plain synthetic weights with gate_bias=10, which mask
nothing.  Budgets: fixed 0.2 / 0.5 / 0.8 for every image (budget_interval = [b, b]) and "interval" = one budget per image sampled in [0, 1].
Per case, switch off and on in ONE process: step ms in three repeats of three timed segments (the scheme of scripts/bench_residual_sparse.py;
their spread is what a difference must exceed), peak memory, the share of rows run, and - in a separate pass, ops.KernelTimer brackets every
launch - the kernel-time split (pack step, attention forward, attention backward, GEMMs, the rest).
--dims small --image-size S measures the ResidualViT the reference ships (patch 8, hidden 256, 4 heads of 64, 4 layers, mlp 768; the budget loss on
every layer) at S px: past 208 rows per image (402 at 160 px, 786 at 224 px) the packed step runs the chunked pack step and, per layer, the streaming
ragged attention pair; the lines then also carry the longest segment per layer of the last step and how many layers streamed per step.
--dense-only measures the dense step alone with the package found under --package-root (a checkout of the parent commit: this script needs
nothing the parent lacks); --parent merges such a file.  A failed step raises: nothing is started after it."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

_a = argparse.ArgumentParser()
_a.add_argument("--batch", type=int, default=1024)
_a.add_argument("--steps", type=int, default=3)
_a.add_argument("--warmup", type=int, default=2)
_a.add_argument("--budgets", default="0.2,0.5,0.8,interval")
_a.add_argument("--weights", default="sparse,stock")
_a.add_argument("--gate-gain", type=float, default=4.0)
_a.add_argument("--dims", default="b16", choices=("b16", "small"))
_a.add_argument("--image-size", type=int, default=224)
_a.add_argument("--dense-only", action="store_true")
_a.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
_a.add_argument("--parent", default="", help="JSON written by a --dense-only run of the parent commit")
_a.add_argument("--out", default="")
ARGS = _a.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.package_root))

import numpy as np
import torch

from peekvit_amd import engine, ops, synth, train_engine
from peekvit_amd.losses import LossCompose
from peekvit_amd.models.residualvit import ResidualVisionTransformer

MODE = "auto"
EXTRA = dict(gate_type="sigmoid", gate_temp=1, add_budget_token="learnable", gate_threshold=0.5)
# configs/loss/crossentropy_mse.yaml's additional loss, spelled out so that the script does not depend on the harness of the checkout it measures
BUDGET_LOSS = {"mse": {"_target_": "peekvit_amd.losses.MSELoss", "weight": 0.01, "strict": False, "budget": None, "per_layer": False,
                       "skip_layers": [0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11]}}
SMALL = dict(patch_size=8, num_layers=4, num_heads=4, hidden_dim=256, mlp_dim=768, num_classes=10)      # the ResidualViT the reference ships
GROUPS = (("pack_step", ("pv_residual_pack_step", "pv_residual_gate")),
          ("attention_fwd", ("pv_attention_varlen_w_lse", "pv_attention_varlen_w_stream_lse", "pv_attention_bf16", "pv_attention_lse", "pv_attention_stream_lse")),
          ("attention_bwd", ("pv_attention_varlen_w_bwd16", "pv_attention_varlen_w_stream_bwd16", "pv_attention_bwd", "pv_attention_stream_bwd")),
          ("gemm", ("pv_gemm",)))


def _state_dict(cfg, which):
    sd = synth.synth_state_dict(cfg, "residualvit", 0)
    if which == "sparse":           # synth.residual_sparse_state_dict, restated so that a parent checkout measures the same weights
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


def _split(fn, dev):
    with ops.KernelTimer() as kt:
        fn()
        torch.cuda.synchronize(dev)
    out = {name: 0.0 for name, _ in GROUPS}
    out["other"] = 0.0
    for k, v in kt.summary().items():
        for name, prefixes in GROUPS:
            if k.startswith(prefixes):
                out[name] += v["ms"]
                break
        else:
            out["other"] += v["ms"]
    return {k: round(v, 3) for k, v in out.items()}


def _measure(step, steps, warmup, dev):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    repeats = [_segments(step, steps, dev) for _ in range(3)]
    med = [sorted(s)[1] for s in repeats]
    return {"step_ms": round(sorted(med)[1] * 1e3, 3), "step_ms_repeats": [round(t * 1e3, 3) for t in med],
            "segments_ms": [[round(t * 1e3, 3) for t in s] for s in repeats], "spread_rel": round((max(med) - min(med)) / sorted(med)[1], 5),
            "peak_memory_mib": round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1)}


def main():
    a = ARGS
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    base = dict(synth.MODEL_CONFIGS["vit_b_16"], image_size=a.image_size) if a.dims == "b16" else dict(SMALL, image_size=a.image_size)
    x = torch.randn(a.batch, 3, a.image_size, a.image_size, generator=gen).to(dev)
    y = torch.randint(0, base["num_classes"], (a.batch,), generator=gen).to(dev)
    parent = {(r["weights"], str(r["budget"])): r for r in json.load(open(a.parent))
              if (r.get("dims", "b16"), r.get("image_size", 224)) == (a.dims, a.image_size)} if a.parent else {}
    extra_loss = LossCompose(BUDGET_LOSS if a.dims == "b16" else {"mse": dict(BUDGET_LOSS["mse"], skip_layers=[])})
    lines = []
    for which in a.weights.split(","):
        gate_bias = 1 if which == "sparse" else 10
        for budget in a.budgets.split(","):
            interval = (0.0, 1.0) if budget == "interval" else (float(budget), float(budget))
            cfg = dict(base, **EXTRA, gate_bias=gate_bias, budget_interval=interval)
            model = ResidualVisionTransformer(**cfg)
            model.load_state_dict(_state_dict(cfg, which))
            model = model.to(dev).train()
            opt = torch.optim.Adam(model.parameters(), lr=1e-5)

            def step():
                opt.zero_grad(set_to_none=True)
                loss = torch.nn.functional.cross_entropy(model(x), y)
                loss = loss + extra_loss.compute(model, budget=model.current_budget, return_dict=False)
                loss.backward()
                opt.step()

            line = {"weights": which, "gate_bias": gate_bias, "gate_gain": a.gate_gain if which == "sparse" else 1.0, "budget": budget,
                    "batch": a.batch, "mode": MODE, "dims": a.dims, "image_size": a.image_size, "rows_per_image": synth.seq_length(cfg) + 1}
            with engine.precision(MODE):
                line["dense"] = _measure(step, a.steps, a.warmup, dev)
                if not a.dense_only:
                    line["dense"]["kernel_ms"] = _split(step, dev)
                    model.set_compact_training(True)
                    f0 = engine.sparse_train_dense_forwards
                    for _ in range(a.warmup):
                        step()
                    r0, d0, l0, s0 = engine.sparse_rows, engine.sparse_dense_rows, engine.sparse_train_long_layers, engine.sparse_syncs
                    line["packed"] = _measure(step, a.steps, 0, dev)
                    line["packed"]["layers_streamed_per_step"] = round((engine.sparse_train_long_layers - l0) * cfg["num_layers"] / float(engine.sparse_syncs - s0), 3)
                    line["packed"]["longest_segment_per_layer"] = list(engine.sparse_last_max_len)
                    if engine.sparse_train_dense_forwards != f0 or engine.sparse_rows == r0:
                        raise RuntimeError("the packed training step took the dense path")
                    line["packed"]["executed_row_share"] = round((engine.sparse_rows - r0) / float(engine.sparse_dense_rows - d0), 4)
                    line["packed"]["kernel_ms"] = _split(step, dev)
                    line["packed_vs_dense"] = round(line["dense"]["step_ms"] / line["packed"]["step_ms"], 4)
                    model.set_compact_training(False)
            line["steps_skipped"] = train_engine.steps_skipped
            p = parent.get((which, budget))
            if p is not None:
                line["parent_dense"] = p["dense"]
                line["dense_vs_parent_dense"] = round(p["dense"]["step_ms"] / line["dense"]["step_ms"], 4)
            print(json.dumps(line), flush=True)
            lines.append(line)
            del model, opt
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
