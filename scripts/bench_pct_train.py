"""One training step of PointCloudTransformer with the stem's pair stage on the HIP training kernels (peekvit_amd.pct_train) and with
PEEKVIT_AMD_TRAIN=torch, the stock-op composite (bench.py is not involved).

    python scripts/bench_pct_train.py [--batch 64] [--points 1024,2048] [--steps 3] [--out profiles/pct_train_bench.json]
    python scripts/bench_pct_train.py --fused-attention [--precision f16] [--out profiles/pct_train_attn_bench.json]
    python scripts/bench_pct_train.py --fused-blocks [--precision f16] [--out profiles/pct_train_block_bench.json]
    python scripts/bench_pct_train.py --ranked [--precision f16] [--budgets 0.25,0.5,0.75,1.0] [--out profiles/pct_train_ranked_bench.json]

The reference's configs/model/pct.yaml dims (4 layers, 4 heads, 128 / 256, 40 classes), synthetic weights (peekvit_amd.synth.pct_state_dict),
uniform clouds.  Per cloud size and per path, in one process and the same order: a full training step (forward, cross-entropy, backward,
Adam) and the stem alone (forward + backward of model.embedder), ms per step = the median of three timed segments, and the peak allocated
memory of each.  The knob is read per call, so both paths run on the same model object.  Where MIOpen's BatchNorm backward (a stock op)
fails to build for a shape, both paths of that size are measured on torch's native BatchNorm kernels and the line says so.  With the path on,
the stem's time per kernel (peekvit_amd.ops.KernelTimer) says where it goes; what the kernels do not account for is the fp64 finalisation on
stock ops and lin2 / bn2.

--fused-attention measures the encoder's opt-in switch instead (model.set_fused_attention): the same training step with
the switch off (the path above with PEEKVIT_AMD_TRAIN=hip) and on, on the same model object in one process - ms per step, peak allocated
memory, and with the switch on the time of the streaming attention forward and backward kernels per step (KernelTimer).

--fused-blocks measures model.set_fused_blocks by the same protocol: one process, one model object, three configurations in
turn - fused attention only, fused blocks, fused attention only again - ms per step, peak allocated memory, and the time of every kernel of a step
with fused attention only and with fused blocks (KernelTimer; "all kernels" is their sum: the rest of a step is stock ops and the host).

--ranked measures RankPointCloudTransformer.set_fused_ranking on a model with enable_ranking(True), per budget, by the same
protocol: one process, one model object, three configurations in turn - fused attention only (the best path a sorting model has without the switch),
fused ranking, fused attention only again - ms per step, peak allocated memory, and kernel time and launch count of a step of the first two.
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
import torch.nn.functional as F

from peekvit_amd import ops, pct_train, synth
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


def _measure(fn, steps, warmup, dev):
    """(ms per call, peak allocated MiB over the timed calls, pair-stage forwards per call)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    n0 = pct_train.stem_passes
    t = _time(fn, steps, dev)
    return t * 1e3, torch.cuda.max_memory_allocated(dev) / 2 ** 20, (pct_train.stem_passes - n0) / (3 * steps)


def _config(n, a, dev):
    kw = dict(DIMS, num_points=n)
    model = PointCloudTransformer(**kw)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.pct_state_dict(kw, 0).items()})
    model = model.to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    x = torch.from_numpy(synth.synth_points(a.batch, n, seed=0)).to(dev)
    target = torch.arange(a.batch, device=dev) % DIMS["num_classes"]

    def step():
        opt.zero_grad(set_to_none=True)
        F.cross_entropy(model(x), target).backward()
        opt.step()

    def stem():
        model.embedder.zero_grad(set_to_none=True)
        model.embedder(x).square().mean().backward()

    line = {"num_points": n, "batch": a.batch, "k": model.embedder.k, "batchnorm": "miopen" if torch.backends.cudnn.enabled else "native"}
    for tag, knob in (("hip", "hip"), ("torch", "torch")):
        os.environ["PEEKVIT_AMD_TRAIN"] = knob
        try:
            ms, mib, passes = _measure(step, a.steps, a.warmup, dev)
            sms, smib, spasses = _measure(stem, a.steps, a.warmup, dev)
        except RuntimeError as e:
            raise RuntimeError(f"with PEEKVIT_AMD_TRAIN={knob}: {e}") from e
        assert passes == spasses == (1.0 if tag == "hip" else 0.0), (tag, passes, spasses)          # the path that was asked for ran
        line.update({f"step_{tag}_ms": round(ms, 3), f"step_{tag}_peak_mib": round(mib, 1), f"stem_{tag}_ms": round(sms, 3),
                     f"stem_{tag}_peak_mib": round(smib, 1)})
    os.environ["PEEKVIT_AMD_TRAIN"] = "hip"
    with ops.KernelTimer() as kt:
        stem()
    torch.cuda.synchronize(dev)
    line["stem_kernels_ms"] = {k: {"launches": v["launches"], "ms": round(v["ms"], 4)} for k, v in kt.summary().items()}
    line["step_speedup"] = round(line["step_torch_ms"] / line["step_hip_ms"], 2)
    line["stem_speedup"] = round(line["stem_torch_ms"] / line["stem_hip_ms"], 2)
    return line


def _config_attn(n, a, dev):
    """The training step with the fused attention switch off and on (PEEKVIT_AMD_TRAIN=hip both times: the stem is on its kernels)."""
    from peekvit_amd import engine
    kw = dict(DIMS, num_points=n)
    model = PointCloudTransformer(**kw)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.pct_state_dict(kw, 0).items()})
    model = model.to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    x = torch.from_numpy(synth.synth_points(a.batch, n, seed=0)).to(dev)
    target = torch.arange(a.batch, device=dev) % DIMS["num_classes"]
    os.environ["PEEKVIT_AMD_TRAIN"] = "hip"

    def step():
        opt.zero_grad(set_to_none=True)
        F.cross_entropy(model(x), target).backward()
        opt.step()

    B, H, D, L = a.batch, DIMS["num_heads"], DIMS["hidden_dim"], DIMS["num_layers"]
    line = {"num_points": n, "batch": B, "precision": a.precision, "batchnorm": "miopen" if torch.backends.cudnn.enabled else "native",
            "stock_scores_mib_per_layer": round(4 * B * H * n * n / 2 ** 20, 1), "fused_saved_mib_per_layer": round(B * n * (8 * D + 4 * H) / 2 ** 20, 1)}
    with engine.precision(a.precision):
        for tag, on in (("off", False), ("on", True), ("off_again", False)):          # (off twice: drift between the first and the last segment shows)
            model.set_fused_attention(on)
            n0 = pct_train.attn_passes
            ms, mib, _ = _measure(step, a.steps, a.warmup, dev)
            passes = (pct_train.attn_passes - n0) / (a.warmup + 3 * a.steps)
            assert passes == (L if on else 0), (tag, passes)          # the path that was asked for ran
            line.update({f"step_{tag}_ms": round(ms, 3), f"step_{tag}_peak_mib": round(mib, 1)})
        model.set_fused_attention(True)
        with ops.KernelTimer() as kt:
            step()
        torch.cuda.synchronize(dev)
    model.set_fused_attention(False)
    line["kernels_ms_per_step"] = {k: {"launches": v["launches"], "ms": round(v["ms"], 4), "tflops": round(v["flops"] / v["ms"] / 1e9, 1) if v["ms"] else 0.0}
                                   for k, v in kt.summary().items() if "attention_stream" in k}
    line["step_speedup"] = round(line["step_off_ms"] / line["step_on_ms"], 2)
    line["peak_ratio"] = round(line["step_off_peak_mib"] / line["step_on_peak_mib"], 2)
    return line


def _config_blocks(n, a, dev):
    """The training step with fused attention only (the best path without the block switch), with fused blocks, and with fused attention only
    again (PEEKVIT_AMD_TRAIN=hip every time: the stem is on its kernels)."""
    from peekvit_amd import engine
    kw = dict(DIMS, num_points=n)
    model = PointCloudTransformer(**kw)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.pct_state_dict(kw, 0).items()})
    model = model.to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    x = torch.from_numpy(synth.synth_points(a.batch, n, seed=0)).to(dev)
    target = torch.arange(a.batch, device=dev) % DIMS["num_classes"]
    os.environ["PEEKVIT_AMD_TRAIN"] = "hip"

    def step():
        opt.zero_grad(set_to_none=True)
        F.cross_entropy(model(x), target).backward()
        opt.step()

    B, H, D, Mh, L = a.batch, DIMS["num_heads"], DIMS["hidden_dim"], DIMS["mlp_dim"], DIMS["num_layers"]
    line = {"num_points": n, "batch": B, "precision": a.precision, "batchnorm": "miopen" if torch.backends.cudnn.enabled else "native",
            "block_saved_mib_per_layer": round(B * n * pct_train.block_saved_bytes_per_row(D, H, Mh) / 2 ** 20, 1)}
    kernels = {}
    model.set_fused_attention(True)
    with engine.precision(a.precision):
        for tag, on in (("attention", False), ("blocks", True), ("attention_again", False)):      # (twice: drift between the first and the last segment shows)
            model.set_fused_blocks(on)
            n0, a0 = pct_train.block_passes, pct_train.attn_passes
            ms, mib, _ = _measure(step, a.steps, a.warmup, dev)
            calls = a.warmup + 3 * a.steps
            ran = ((pct_train.block_passes - n0) / calls, (pct_train.attn_passes - a0) / calls)
            assert ran == ((L, 0) if on else (0, L)), (tag, ran)          # the path that was asked for ran
            line.update({f"step_{tag}_ms": round(ms, 3), f"step_{tag}_peak_mib": round(mib, 1)})
            if tag != "attention_again":
                with ops.KernelTimer() as kt:
                    step()
                torch.cuda.synchronize(dev)
                kernels[tag] = {k: {"launches": v["launches"], "ms": round(v["ms"], 4)} for k, v in sorted(kt.summary().items())}
                kernels[tag]["all kernels"] = {"launches": sum(v["launches"] for v in kt.summary().values()), "ms": round(sum(v["ms"] for v in kt.summary().values()), 4)}
    model.set_fused_blocks(False)
    model.set_fused_attention(False)
    line["kernels_ms_per_step"] = kernels
    line["step_speedup"] = round(min(line["step_attention_ms"], line["step_attention_again_ms"]) / line["step_blocks_ms"], 2)
    line["peak_ratio"] = round(line["step_attention_peak_mib"] / line["step_blocks_peak_mib"], 2)
    return line


def _config_ranked(n, a, dev):
    """A sorting model's training step per budget: fused attention only, fused ranking, fused attention only again (PEEKVIT_AMD_TRAIN=hip every time)."""
    from peekvit_amd import engine
    from peekvit_amd.models.pct import RankPointCloudTransformer
    kw = dict(DIMS, num_points=n)
    model = RankPointCloudTransformer(**kw)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.pct_state_dict(kw, 0).items()})
    model = model.to(dev).train()
    model.enable_ranking(True)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    x = torch.from_numpy(synth.synth_points(a.batch, n, seed=0)).to(dev)
    target = torch.arange(a.batch, device=dev) % DIMS["num_classes"]
    os.environ["PEEKVIT_AMD_TRAIN"] = "hip"

    def step():
        opt.zero_grad(set_to_none=True)
        F.cross_entropy(model(x), target).backward()
        opt.step()

    B, H, D, Mh, L = a.batch, DIMS["num_heads"], DIMS["hidden_dim"], DIMS["mlp_dim"], DIMS["num_layers"]
    line = {"num_points": n, "batch": B, "precision": a.precision, "batchnorm": "miopen" if torch.backends.cudnn.enabled else "native", "budgets": {}}
    model.set_fused_attention(True)
    with engine.precision(a.precision):
        for budget in [float(v) for v in a.budgets.split(",")]:
            model.set_budget(budget)
            keep = pct_train.ranked_keep(model.encoder.layers[0], n)
            rows = keep + 1 + (1 if keep < n - 1 else 0)
            r = {"keep": keep, "compact_rows": rows, "saved_mib_per_layer": round((B * rows * pct_train.block_saved_bytes_per_row(D, H, Mh) + 4 * B * keep) / 2 ** 20, 1)}
            kernels = {}
            for tag, on in (("attention", False), ("ranked", True), ("attention_again", False)):      # (twice: drift between the first and the last segment shows)
                model.set_fused_ranking(on)
                n0, a0, b0 = pct_train.ranked_passes, pct_train.attn_passes, pct_train.block_passes
                ms, mib, _ = _measure(step, a.steps, a.warmup, dev)
                calls = a.warmup + 3 * a.steps
                ran = ((pct_train.ranked_passes - n0) / calls, (pct_train.attn_passes - a0) / calls, pct_train.block_passes - b0)
                assert ran == ((L, 0, 0) if on else (0, L, 0)), (tag, budget, ran)          # the path that was asked for ran
                r.update({f"step_{tag}_ms": round(ms, 3), f"step_{tag}_peak_mib": round(mib, 1)})
                if tag != "attention_again":
                    with ops.KernelTimer() as kt:
                        step()
                    torch.cuda.synchronize(dev)
                    kernels[tag] = {k: {"launches": v["launches"], "ms": round(v["ms"], 4)} for k, v in sorted(kt.summary().items())}
                    kernels[tag]["all kernels"] = {"launches": sum(v["launches"] for v in kt.summary().values()), "ms": round(sum(v["ms"] for v in kt.summary().values()), 4)}
            r["kernels_ms_per_step"] = kernels
            r["step_speedup"] = round(min(r["step_attention_ms"], r["step_attention_again_ms"]) / r["step_ranked_ms"], 2)
            r["peak_ratio"] = round(r["step_attention_peak_mib"] / r["step_ranked_peak_mib"], 2)
            line["budgets"][str(budget)] = r
    model.set_fused_ranking(False)
    model.set_fused_attention(False)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fused-attention", action="store_true", help="measure the encoder's fused-attention switch off / on instead of the stem's knob")
    ap.add_argument("--fused-blocks", action="store_true", help="measure the encoder's fused-block switch against fused attention alone")
    ap.add_argument("--ranked", action="store_true", help="measure RankPointCloudTransformer's fused-ranking switch against fused attention alone, per budget")
    ap.add_argument("--budgets", default="0.25,0.5,0.75,1.0", help="--ranked: the budgets to measure")
    ap.add_argument("--precision", default="f16", choices=["bf16", "f16"], help="operand type of the fused attention (engine.precision)")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--points", default="1024,2048")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    config = _config_ranked if a.ranked else _config_blocks if a.fused_blocks else _config_attn if a.fused_attention else _config
    for n in [int(v) for v in a.points.split(",")]:
        try:
            line = config(n, a, dev)
        except RuntimeError as e:
            # MIOpen's BatchNorm backward does not build for every shape (a stock op, on either path): measure both paths of this size on
            # torch's native BatchNorm kernels instead, and say so in the line
            if "miopen" not in str(e).lower():
                raise
            torch.cuda.empty_cache()
            with torch.backends.cudnn.flags(enabled=False):
                line = config(n, a, dev)
            line["miopen_error"] = str(e)
        print(json.dumps(line), flush=True)
        lines.append(line)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
