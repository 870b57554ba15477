#!/usr/bin/env python3
"""Headline benchmark: images/sec of the ViT-B/16 forward at batch 2048 per GPU, 224x224 (BASELINE.json).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Both forms work: started WITHOUT a launcher and with --gpus N > 1, this process - before it makes any GPU call - starts
`python -m torch.distributed.run` with N ranks as a child, relays the child's single JSON line and exits with its code.

One process per GPU.  A "step" is ONE forward pass of the hot path (VisionTransformer.forward on the MI355X
kernels) over one device-resident synthetic batch.  The path shards along the batch: every
rank runs an independent replica on its own 2048-image batch, no data-path collective ("scaling": "weak");
the only communication is the timing barrier + MAX-over-ranks reduction over RCCL.

A plain run sets up, warms up, times the K steps and prints ONE JSON line (rank 0) with the contract keys (metric, value, unit,
higher_is_better, dtype, ms_per_step, ...).  --dump-outputs DIR also writes what the last timed step computed as DIR/<name>.npy.
--full adds everything else, timed after the headline in the same process:
  roofline      the dominant kernel (pv_gemm_bf16): algorithmic FLOPs / HIP-event time, from the K steps run again with events
  power         package power / shader clock over the timed steps
  cpu_baseline  the CPU oracle (oracle/vit_oracle.py, fp32, = the reference's arithmetic) timed on the host cores, and the GPU
                logits scored against it
  bf16_mode, all_rows_mode, reference_loop, pipeline_loop, extra_configs
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch

MFMA_BF16_PEAK_TFLOPS = 2500.0      # dense bf16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md "Peak BF16/FP16 MFMA"
HBM_PEAK_GBS = 8000.0               # HBM3E spec, same guide
# measured on this box (scripts/mfma_peak.hip, profiles/r01_mfma_peak.txt): register-only MFMA loop with data-like operand toggling;
# reported next to the nominal peak, never used for `frac`
MFMA_BF16_SUSTAINED_MEASURED_TFLOPS = 2003.0
HBM_ACHIEVABLE_GBS = 6290.0         # measured float4 copy, same guide ("HBM3E peak BW": 6.29 TB/s = 79 % of spec); the ridge below uses it
RIDGE_FLOP_PER_BYTE = MFMA_BF16_PEAK_TFLOPS * 1e12 / (HBM_ACHIEVABLE_GBS * 1e9)      # 397: a GEMM below it is HBM-bound by its ALGORITHMIC bytes


def gemm_members(kt, name, steps, cfg):
    """Per-member roofline of the GEMM family (one C-ABI entry point, four roofline cases): each member against the bound its algorithmic
    intensity puts it under - MFMA for the in-projection and fc1, HBM for the out-projection and fc2, whose fp32 residual in + out and
    16-bit copy make them move more bytes than 2.5 PFLOP/s could feed."""
    D, Mh = cfg["hidden_dim"], cfg["mlp_dim"]
    from peekvit_amd._lib import PV_EPI_BIAS_POS_F32
    names = {(3 * D, D): "qkv in-projection", (2 * D, D): "k|v in-projection of the last block (class-token rows only)",
             (D, D): "attention out-projection (+ fp32 residual, 16-bit copy, row statistics)",
             (Mh, D): "fc1 + GELU", (D, Mh): "fc2 (+ fp32 residual, 16-bit copy, row statistics)"}
    out = []
    for (N, K, epi), d in sorted(kt.members(name).items(), key=lambda kv: -kv[1]["ms"]):
        if out and d["ms"] / steps < 0.1:  # (the last block's class-row GEMMs: 2048 rows, tens of microseconds)
            continue
        sec = d["ms"] * 1e-3
        inten = d["flops"] / d["bytes"]
        bound = "mfma" if inten >= RIDGE_FLOP_PER_BYTE else "hbm"
        m = {"member": "patch embedding (+ bias, positional embedding)" if epi == PV_EPI_BIAS_POS_F32 else names.get((N, K), f"N={N} K={K}"), "N": N, "K": K, "epilogue": epi,
             "launches_per_step": d["launches"] // steps, "avg_launch_ms": round(d["ms"] / d["launches"], 4), "ms_per_step": round(d["ms"] / steps, 3),
             "algorithmic_flop_per_byte": round(inten, 1), "bound": bound,
             "tflops": round(d["flops"] / sec / 1e12, 1), "algo_gbs": round(d["bytes"] / sec / 1e9, 1)}
        if bound == "mfma":
            m.update(achieved=m["tflops"], peak=MFMA_BF16_PEAK_TFLOPS, unit="TFLOP/s", frac=round(m["tflops"] / MFMA_BF16_PEAK_TFLOPS, 4))
        else:
            m.update(achieved=m["algo_gbs"], peak=HBM_PEAK_GBS, unit="GB/s", frac=round(m["algo_gbs"] / HBM_PEAK_GBS, 4),
                     frac_of_achievable_hbm=round(m["algo_gbs"] / HBM_ACHIEVABLE_GBS, 4))
        out.append(m)
    return out


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", default="vit_b_16")
    ap.add_argument("--batch", type=int, default=2048, help="images per GPU per step")
    ap.add_argument("--rank-budget", type=float, default=None, help="run RankViT (rankvit_layers 3,6,9) at this budget")
    ap.add_argument("--train", action="store_true",
                    help="BASELINE.json configs[2]/[4]: a step = forward + cross-entropy + backward (HIP backward kernels); with N > 1 "
                         "ranks the parameter gradients are all-reduced over RCCL (data-parallel training path)")
    ap.add_argument("--no-optimizer", action="store_true",
                    help="--train: stop the step after loss.backward() (+ all-reduce).  Default: the reference's whole step (train/train.py:112-121) "
                         "- zero_grad, forward, cross-entropy, backward, [all-reduce], clip_grad_norm_(1.0), Adam(1e-3).step()")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also measure and check everything else: per-kernel roofline, power, CPU baseline and oracle "
                         "checks, bf16 / all-rows modes, reference and pipeline loops, extra_configs (off: the headline only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (logits; with --train also a fixed sample of the parameter gradients) "
                         "as DIR/<name>.npy, float32")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline and the oracle checks")
    ap.add_argument("--no-extra", action="store_true", help="--full: skip the extra_configs (BASELINE configs 2, 4 and config 3's training "
                                                             "step, timed after the headline in the same process) and the reference-loop value")
    ap.add_argument("--cpu-batch", type=int, default=64, help="images of the CPU-oracle sample (64: large enough that the GPU path scored "
                                                                "against it takes the same kernels / LayerNorm folding as the timed batch)")
    ap.add_argument("--cpu-iters", type=int, default=4)
    ap.add_argument("--precision", default="auto", choices=["auto", "bf16", "f16", "bf16x3"],
                    help="operand precision of the MFMA products: auto (default = the package default: IEEE fp16 operands behind the "
                         "operand-range guard with bf16 fallback for inference - meets the 1e-3 logits tolerance; bf16 operands for "
                         "training), bf16 (4e-3), f16 (unguarded), bf16x3 (split operands, 1e-5)")
    ap.add_argument("--streams", type=int, default=0, help="forward on this many batch slices / HIP streams (0 = package default)")
    ap.add_argument("--bucket-kib", type=int, default=25 << 10, help="gradient all-reduce bucket size (KiB), --train with N > 1")
    ap.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL over xGMI); gloo only to rehearse N>1 on one GPU")
    return ap.parse_args()


def cpu_baseline(cfg, batch, iters, gpu_model=None, dev=None):
    """The CPU oracle (bit-equal to the reference on CPU, tests/test_oracle_golden.py) on a bounded sample.  As the checker it
    also scores the GPU path on the same sample: relative L2 of the logits per operand-precision mode."""
    from oracle import vit_oracle as O
    from peekvit_amd import synth
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(cfg).items()}
    x = torch.randn(batch, 3, cfg["image_size"], cfg["image_size"], generator=torch.Generator().manual_seed(0))
    # the GPU box gives one-GPU jobs a 16-CPU share of a 256-thread host: size the pool to the share, not the host
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    cores = max(1, min(cores, int(os.environ.get("PV_CPU_THREADS", "16"))))
    torch.set_num_threads(cores)
    with torch.no_grad():
        ref = O.vit_forward(x, sd, cfg, "fp32")                 # warm-up
        t0 = time.perf_counter()
        for _ in range(iters):
            O.vit_forward(x, sd, cfg, "fp32")
        dt = time.perf_counter() - t0
    out = {"value": round(batch * iters / dt, 2), "unit": "images/sec", "cores": torch.get_num_threads(), "kind": "port",
           "sample": f"{iters} forwards of batch {batch} (fp32, torch CPU, oracle/vit_oracle.py), {dt:.1f} s, on {torch.get_num_threads()} "
                     f"threads (this job's CPU share) of a host with {os.cpu_count()} hardware threads"}
    if gpu_model is not None:
        from peekvit_amd import engine
        err = {}
        with torch.no_grad():
            for mode in ("auto", "bf16", "f16"):
                with engine.precision(mode):
                    got = gpu_model(x.to(dev)).float().cpu()
                err[mode] = float(f"{((got - ref).norm() / ref.norm()).item():.3e}")
        out["gpu_logits_rel_l2_vs_oracle"] = err       # tolerance of BASELINE.json: 1e-3
    return out


def oracle_error(model, cfg, dev, images, train=False, rank=None):
    """Relative L2 of the GPU path's logits against the CPU oracle's fp32 logits (= the reference's arithmetic) on a small seeded batch."""
    from oracle import vit_oracle as O
    from peekvit_amd import synth
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(cfg).items()}
    x = torch.randn(images, 3, cfg["image_size"], cfg["image_size"], generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        ref = O.vit_forward(x, sd, cfg, "fp32", **({"rankvit_layers": rank[0], "budget": rank[1]} if rank else {}))
    with (torch.enable_grad() if train else torch.no_grad()):
        got = model(x.to(dev)).detach().float().cpu()
    return float(f"{((got - ref).norm() / ref.norm()).item():.3e}")


def extra_config(kind, dev, steps, warmup):
    """One more BASELINE.json configuration, timed in THIS process after the headline (same barrier + synchronize bracket around exactly
    `steps` steps), so that the driver's one invocation also times configs 2, 4 and the training step of config 3."""
    from peekvit_amd import engine, ops, synth
    from peekvit_amd.models.rankvit import RankVisionTransformer
    from peekvit_amd.models.vit import VisionTransformer
    name, batch, train, rank = {"vit_small_fwd": ("vit_small", 512, False, None), "rankvit_b16_fwd": ("vit_b_16", 2048, False, ([3, 6, 9], 0.5)),
                                "vit_b_16_train_step": ("vit_b_16", 2048, True, None), "vit_b_16_hostile_weights_fwd": ("vit_b_16", 256, False, None),
                                "vit_b_16_trained_like_weights_fwd": ("vit_b_16", 2048, False, None)}[kind]
    hostile = kind == "vit_b_16_hostile_weights_fwd"
    trained_like = kind == "vit_b_16_trained_like_weights_fwd"
    cfg = synth.MODEL_CONFIGS[name]
    seqs = None
    if rank:
        import math
        model = RankVisionTransformer(**cfg, rankvit_layers=rank[0])
        model.set_budget(rank[1])
        S, seqs = synth.seq_length(cfg), []
        for i in range(cfg["num_layers"]):
            if i in rank[0]:
                S = 1 + math.ceil((S - 1) * rank[1])
            seqs.append(S)
    else:
        model = VisionTransformer(**cfg)
    synth.load_synth_weights(model, cfg)
    if hostile:
        # what mode auto's guards COST when they trip (round 3 ADVICE): the reference-checked hostile weights (tests/golden/hostile.npz: six decades of
        # weight magnitudes, x100 outlier channels, a massive token) raise the attention-score guard on every forward - after three trips the model
        # stays in the split-operand mode, which is what gets timed
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.hostile_variants(cfg)["hostile"].items()})
    if trained_like:
        # what a TRAINED ViT looks like to the guards (round 5; tests/golden/hostile.npz holds the real reference's logits for it): attention logits of
        # 47 - 58 in every third layer, two massive-activation channels, no x100 gains: the score guard names layers 1, 4, 7, 10 on the first forward
        # and only THEIR attention half runs in split precision from then on
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.hostile_variants(cfg)["trained_like"].items()})
    model = (model.train() if train else model.eval()).to(dev)
    gen = torch.Generator(device=dev).manual_seed(4321)
    x = torch.randn(batch, 3, cfg["image_size"], cfg["image_size"], generator=gen, device=dev).to(torch.bfloat16).to(torch.float32)
    if train:
        y = torch.randint(0, cfg["num_classes"], (batch,), generator=gen, device=dev)
        params = [p for p in model.parameters() if p.requires_grad]
        opt = torch.optim.Adam(params, lr=1e-3, fused=True)

        def step():
            for p in params:
                p.grad = None
            torch.nn.functional.cross_entropy(model(x), y).backward()
            torch.nn.utils.clip_grad_norm_(params, 1.0, foreach=True)
            opt.step()
    else:
        def step():
            model(x)
    f0 = engine.fallback_count
    rep0 = getattr(engine, "rank_repaired_images", 0)
    sc0 = dict(engine.selfcheck_totals)           # (before the oracle check below: the first forward of a key is where its first probe runs)
    engine.selfcheck_totals["worst_rel_l2"] = 0.0
    if hostile:
        import warnings
        warnings.simplefilter("ignore", RuntimeWarning)
        err = None
    elif trained_like:
        import warnings
        warnings.simplefilter("ignore", RuntimeWarning)
        from oracle import vit_oracle as O
        sd = {k: torch.from_numpy(v.copy()) for k, v in synth.hostile_variants(cfg)["trained_like"].items()}
        xc = torch.randn(16, 3, cfg["image_size"], cfg["image_size"], generator=torch.Generator().manual_seed(0))
        with torch.no_grad():
            ref = O.vit_forward(xc, sd, cfg, "fp32")
            got = model(xc.to(dev)).float().cpu()
        err = float(f"{((got - ref).norm() / ref.norm()).item():.3e}")
    else:
        err = oracle_error(model, cfg, dev, 16 if rank else 64, train, rank)        # before the optimizer moves the weights
    engine.selfcheck_last = None
    from peekvit_amd import telemetry
    sampler = telemetry.sampler(dev.index or 0)
    with (torch.enable_grad() if train else torch.no_grad()):
        for _ in range(warmup):
            step()
        import gc
        gc.collect()                  # (see the headline's warm-up)
        # the median of three back-to-back timed segments of `steps` steps each (a 5 ms step on a shared host: one 25 ms hiccup inside a single segment
        # of 50 steps read as -10 % in one of round 4's runs; round 6: the training step too - its single segment of ten 0.23 s steps was the review's item 7)
        segs = []
        with sampler.window() as pw:
            for _seg in range(3):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(steps):
                    step()
                torch.cuda.synchronize(dev)
                segs.append(time.perf_counter() - t0)
        dt = sorted(segs)[len(segs) // 2]
        with ops.KernelTimer() as kt:
            step()
            torch.cuda.synchronize(dev)
    ks = kt.summary()
    flops_exec = sum(v["flops"] for v in ks.values()) / batch
    value = batch * steps / dt
    out = {"config": kind, "workload": (f"{name} train step (fwd, cross-entropy, bwd, clip 1.0, Adam)" if train else
                                        f"rank{name} layers={rank[0]} budget={rank[1]} forward" if rank else f"{name} forward" + (" on the hostile-weights fixture" if hostile else " on the trained-like fixture" if trained_like else "")) + f", batch {batch}, {cfg['image_size']}x{cfg['image_size']}",
           "value": round(value, 1), "unit": "images/sec", "steps": steps, "warmup": warmup, "ms_per_step": round(dt / steps * 1e3, 3),
           "timed_segments_ms_per_step": [round(t / steps * 1e3, 3) for t in segs],
           "dtype": _train_dtype(model) if train else ("bf16x3" if engine.fallback_count > f0 else "f16"),
           "gflop_per_image": round(synth.fwd_flops_per_image(cfg, seqs) * (3 if train else 1) / 1e9, 3), "gflop_per_image_executed": round(flops_exec / 1e9, 3),
           "model_mfma_roofline_frac": round(value * flops_exec / (MFMA_BF16_PEAK_TFLOPS * 1e12), 4),
           ("train_forward_logits_rel_l2_vs_oracle" if train else "logits_rel_l2_vs_oracle"): err,
           "logits_sample_images": 16 if rank else 64,
           "top_kernels_ms": {k: round(v["ms"], 3) for k, v in sorted(ks.items(), key=lambda kv: -kv[1]["ms"])[:4]},
           # package power / shader clock over the three timed segments (read-only sysfs sampling on a host thread, peekvit_amd/telemetry.py)
           "power": pw.result()}
    if hostile:
        out.pop("logits_rel_l2_vs_oracle"); out.pop("logits_sample_images")
        out["guard"] = {"whole_forward_fallbacks": engine.fallback_count - f0, "sticky_split_operand_mode": bool(engine.guard_state(model).unsafe),
                        "hybrid_layers": sorted(engine.guard_state(model).hybrid), "mlp_halves_split": bool(engine.guard_state(model).mlp_hybrid),
                        "note": "the attention-score guard trips on these weights (scores ~1e3 in every layer): round 5 repeats the forward ONCE with the attention half "
                                "of the tripped layers in split precision (LayerNorm -> [hi|lo|hi], in-projection as three bf16 products, split-operand scores) and remembers "
                                "the layers; everything else stays fp16 (inside 1e-3: tests/test_hip_precision.py::HOSTILE_CASES).  On THIS entry's noise images that measures 1.15e-3: the "
                                "self-check's first escalation step (round 6: the MLP half of every layer in split precision) brings it to 0.83e-3 over the batch but not under the "
                                "9e-4 limit on the probe images, so bf16x3 answers, as in rounds 3-5 (8.2 k img/s); what is left is the out-projection and P.V in 16 bits on the "
                                "class row (scripts/dbg/hostile_sites.py)"}
    if trained_like:
        st = engine.guard_state(model)
        out["logits_sample_images"] = 16
        out["guard"] = {"whole_forward_fallbacks": engine.fallback_count - f0, "hybrid_layers": sorted(st.hybrid), "local_fallbacks": engine.hybrid_fallback_count,
                        "note": "attention logits ~50 in layers 1, 4, 7, 10 + massive-activation channels: those four layers' attention half runs in split precision, the rest on fp16 operands"}
    if not train and not hostile and engine.selfcheck_last is not None:
        sc = engine.selfcheck_last
        out["self_check"] = {"fp16_vs_bf16x3_logits_rel_l2": float(f"{sc[0]:.3e}"), "images_compared": sc[1] - sc[2], "limit": engine.SELFCHECK_LIMIT}
        tot = engine.selfcheck_totals
        out["self_check"]["all_probes_of_this_entry"] = {"probes": tot["probes"] - sc0["probes"], "images": tot["images"] - sc0["images"],
                                                         "worst_fp16_vs_bf16x3_logits_rel_l2": float(f"{tot['worst_rel_l2']:.3e}")}
        if rank:
            # CUMULATIVE over every probe of this entry (oracle check, warm-up, timed segments) - round 5 reported the last probe only
            out["self_check"]["rank_tie_flips"] = {"images": tot["tie_flips"] - sc0["tie_flips"], "of": tot["images"] - sc0["images"], "last_probe": {"images": sc[2], "of": sc[1]},
                                                   "repaired_images": getattr(engine, "rank_repaired_images", 0) - rep0,
                                                   "note": "probe images in which a ranked layer kept a different token SET than the "
                                                   "split-operand arithmetic did (a near-tie at the keep boundary resolved by 16-bit noise in the norms): their logits move "
                                                   "by a median 6.5e-4 (profiles/r06_rank_tie_calibration.json: beyond operand rounding, within the order of the contract) and they are excluded from the comparison above; PEEKVIT_AMD_RANK_STRICT=1 sends the model to bf16x3 instead"}
    if train:
        from peekvit_amd import train_engine
        st = train_engine.train_state(model)
        out["loss_scale"] = {"scale": st.scale, "target_max_entering_gradient": st.target, "steps": st.steps, "steps_skipped_for_overflow": st.skipped}
        out["logits_note"] = ("training runs the inference path's fp16 operands with a power-of-two loss scale for the 16-bit gradients (peekvit_amd/train_engine.py): its forward "
                              "is inside the 1e-3 contract; gradients are asserted at 2e-3 against the reference's training step (tests/test_hip_backward.py)")
    del model, x
    torch.cuda.empty_cache()
    return out


def _train_dtype(model):
    """The 16-bit operand type the training steps of `model` ran on (fp16 with a loss scale in mode auto; bf16 after a forward overflow / in mode bf16)."""
    from peekvit_amd import train_engine
    return train_engine.pass_operand(model)


DUMP_MAX_ELEMS = {"logits": 12 << 20, "grad_sample": 1 << 20}      # float32 elements: 52 MB at most in all


def last_step_outputs(out, grads=None):
    """What a caller of the timed path received from its last step, as float32 host arrays: the logits (a seeded sample of rows when
    there are more than DUMP_MAX_ELEMS of them) and, for a training step, a seeded sample of the flattened parameter gradients (in
    parameters() order).  The samples depend only on the shapes, so two builds run with the same arguments dump the same elements."""
    import numpy as np
    arrays = {}
    logits = out.detach().float()
    rows = max(1, DUMP_MAX_ELEMS["logits"] // max(1, logits[0].numel()))
    if logits.shape[0] > rows:
        keep = torch.randperm(logits.shape[0], generator=torch.Generator().manual_seed(0))[:rows].sort().values
        logits = logits[keep.to(logits.device)]
    arrays["logits"] = logits.cpu().numpy().astype(np.float32)
    if grads is not None:
        flat = torch.cat([g.detach().reshape(-1).float() for g in grads])
        idx = torch.randint(0, flat.numel(), (min(flat.numel(), DUMP_MAX_ELEMS["grad_sample"]),), generator=torch.Generator().manual_seed(1))
        arrays["grad_sample"] = flat[idx.sort().values.to(flat.device)].cpu().numpy().astype(np.float32)
    return arrays


def write_outputs(dirname, arrays):
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), a)


def reference_loop(model, cfg, batch, steps, dev):
    """images/sec as the REFERENCE defines it (validate/test.py:113-124): wall clock around the evaluation loop, host batches moved with a
    synchronous .to(device), argmax + metric update per batch - here `steps` batches from one pinned host batch.  Never `value`."""
    host = torch.randn(batch, 3, cfg["image_size"], cfg["image_size"], generator=torch.Generator().manual_seed(7)).pin_memory()
    labels = torch.randint(0, cfg["num_classes"], (batch,), generator=torch.Generator().manual_seed(8)).pin_memory()
    correct = torch.zeros((), dtype=torch.int64, device=dev)
    with torch.no_grad():
        for _ in range(2):
            model(host.to(dev))
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            b, l = host.to(dev), labels.to(dev)
            correct += (torch.argmax(model(b), 1) == l).sum()
        _ = int(correct.item())
        dt = time.perf_counter() - t0
    return {"value": round(batch * steps / dt, 1), "unit": "images/sec", "ms_per_step": round(dt / steps * 1e3, 3),
            "definition": "validate/test.py:113-124: wall clock of the loop incl. a synchronous host-to-device copy of every fp32 batch (pinned, "
                          f"{host.numel() * 4 / 1e9:.2f} GB) and the argmax / accuracy update"}


def pipeline_loop(model, cfg, batch, steps, dev):
    """The same definition of images/sec (validate/test.py:113-124: wall clock around the loop, argmax + accuracy update per batch) over the loop
    peekvit_amd.harness.test.evaluate runs: uint8 NHWC host batches (the normalisation is fused into the patch gather) through the DevicePrefetcher
    - batch i + 1 is copied on a side stream while batch i is computed - and the guard word of batch i read after batch i + 1 has been launched
    (engine.deferred_flags).  `steps` batches cycling through three pinned host batches.  Never `value`."""
    from peekvit_amd import engine
    from peekvit_amd.harness.pipeline import DevicePrefetcher
    g = torch.Generator().manual_seed(7)
    R = cfg["image_size"]
    hosts = [torch.randint(0, 256, (batch, R, R, 3), generator=g, dtype=torch.uint8).pin_memory() for _ in range(3)]
    labels = [torch.randint(0, cfg["num_classes"], (batch,), generator=g).pin_memory() for _ in range(3)]

    def loader(n):
        for i in range(n):
            yield hosts[i % 3], labels[i % 3]

    def sweep(n):
        hits = torch.zeros((), dtype=torch.int64, device=dev)
        prev = None
        with engine.deferred_flags():
            for b, l in DevicePrefetcher(loader(n), dev, keep=1):
                out = model(b)
                if prev is not None:
                    hits += (engine.resolve(prev[0]).argmax(1) == prev[1]).sum()
                prev = (out, l)
            hits += (engine.resolve(prev[0]).argmax(1) == prev[1]).sum()
        return int(hits.item())                     # the loop's one read-back

    with torch.no_grad():
        sweep(3)                                    # (first forward of the uint8 key: its self-check runs here, outside the timing)
        torch.cuda.synchronize(dev)
        f0 = engine.fallback_count
        t0 = time.perf_counter()
        sweep(steps)
        dt = time.perf_counter() - t0
    return {"value": round(batch * steps / dt, 1), "unit": "images/sec", "ms_per_step": round(dt / steps * 1e3, 3), "batches": steps,
            "fallback_forwards": engine.fallback_count - f0,
            "definition": "validate/test.py:113-124's wall clock over harness.test.evaluate's loop: uint8 NHWC host batches "
                          f"({hosts[0].numel() / 1e9:.2f} GB each, pinned) copied one batch ahead on a side stream, normalisation fused into the patch gather, "
                          "guard word read one batch late, one read-back at the end"}


def small_model_entry(dev, steps=200):
    """BASELINE config 1's model on the GPU: vit_tiny 160x160, batch 32 - launch-bound (~100 launches of a few microseconds): eager, and as ONE
    hipGraph replay (peekvit_amd.graph.GraphedForward: capture once, bit-identical replays)."""
    from peekvit_amd import engine, synth
    from peekvit_amd.graph import GraphedForward
    from peekvit_amd.models.vit import VisionTransformer
    cfg = synth.MODEL_CONFIGS["vit_tiny"]
    model = VisionTransformer(**cfg)
    synth.load_synth_weights(model, cfg)
    model = model.eval().to(dev)
    B = 32
    x = torch.randn(B, 3, cfg["image_size"], cfg["image_size"], generator=torch.Generator(device=dev).manual_seed(99), device=dev).to(torch.bfloat16).float()
    err = oracle_error(model, cfg, dev, 32)
    out = {"config": "vit_tiny_fwd_b32", "workload": f"vit_tiny forward, batch {B}, {cfg['image_size']}x{cfg['image_size']} (BASELINE config 1's model on the GPU)",
           "gflop_per_image": round(synth.fwd_flops_per_image(cfg) / 1e9, 3), "logits_rel_l2_vs_oracle": err, "dtype": "f16"}
    from peekvit_amd import autograph
    with torch.no_grad():
        def timed():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(steps):
                model(x)
            torch.cuda.synchronize(dev)
            return time.perf_counter() - t0
        # (a) every launch issued by the host (what round 5 called "eager"): the engine's own choice of hipGraph replay switched off
        autograph.ENABLED = False
        for _ in range(5):
            ref = model(x)
        f0 = engine.fallback_count
        dt = timed()
        out["eager_launches"] = {"value": round(B * steps / dt, 1), "unit": "images/sec", "ms_per_step": round(dt / steps * 1e3, 4)}
        # (b) the DEFAULT path (round 6): mode auto captures a launch-bound key after a few clean forwards and replays it (peekvit_amd/autograph.py)
        autograph.ENABLED = True
        r0, c0 = autograph.replays, autograph.captures
        for _ in range(autograph.WARM + 2):
            got = model(x)
        dt = timed()
        out["eager"] = {"value": round(B * steps / dt, 1), "unit": "images/sec", "ms_per_step": round(dt / steps * 1e3, 4),
                        "note": "the default call `model(x)`: the engine replays its own hipGraph for this launch-bound shape",
                        "auto_graph": {"captures": autograph.captures - c0, "replays": autograph.replays - r0, "bit_identical_to_launches": bool(torch.equal(got, ref))}}
        if engine.fallback_count > f0:
            out["dtype"] = "bf16x3"
        g = GraphedForward(model, x)
        for _ in range(5):
            y = g(x)
        same = bool(torch.equal(y, ref))
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            g(x)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        out["hipgraph_replay"] = {"value": round(B * steps / dt, 1), "unit": "images/sec", "ms_per_step": round(dt / steps * 1e3, 4), "bit_identical_to_eager": same,
                                  "model_mfma_roofline_frac": round(B * steps / dt * synth.fwd_flops_per_image(cfg) / (MFMA_BF16_PEAK_TFLOPS * 1e12), 4)}
    del model, g
    torch.cuda.empty_cache()
    return out


def self_launch(args) -> int:
    """--gpus N > 1 without a launcher: start N ranks as a CHILD `python -m torch.distributed.run` (this process has made no GPU
    call - replacing a process that has initialised the GPU is forbidden on this pool), relay its output, return its exit code."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), PV_BENCH_CHILD="1")
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    for ln in proc.stdout.splitlines():
        if ln not in lines:
            print(ln, file=sys.stderr)
    if proc.returncode == 0 and len(lines) == 1:
        print(lines[0], flush=True)
        return 0
    print(f"bench.py: the {args.gpus}-rank run failed (exit {proc.returncode}, {len(lines)} result lines)", file=sys.stderr)
    return proc.returncode or 1


def main():
    args = parse()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # (dmabuf IPC only on this pool: RCCL's buffer exchange needs it; before the first HIP call)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: the launcher's rank count and --gpus must agree")
    dist = world > 1
    ndev = torch.cuda.device_count()
    if args.dist_backend == "gloo":
        local = local % max(ndev, 1)       # rehearsal: several ranks may share one GPU
    elif ndev < world:
        raise SystemExit(f"--gpus {world} over RCCL needs {world} visible GPUs, found {ndev} (rehearse with --dist-backend gloo)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if dist:
        import torch.distributed as td
        if args.dist_backend == "nccl":
            td.init_process_group("nccl", device_id=dev)
        else:
            td.init_process_group("gloo")

    from peekvit_amd import ops, synth
    from peekvit_amd.models.rankvit import RankVisionTransformer
    from peekvit_amd.models.vit import VisionTransformer

    cfg = synth.MODEL_CONFIGS[args.model]
    seqs = None
    if args.rank_budget is None:
        model = VisionTransformer(**cfg)
        workload = f"{args.model} forward, batch {args.batch}/GPU, {cfg['image_size']}x{cfg['image_size']}"
    else:
        layers = [3, 6, 9] if cfg["num_layers"] >= 10 else list(range(1, cfg["num_layers"]))
        model = RankVisionTransformer(**cfg, rankvit_layers=layers)
        model.set_budget(args.rank_budget)
        import math
        S, seqs = synth.seq_length(cfg), []
        for i in range(cfg["num_layers"]):
            if i in layers and args.rank_budget != 1:
                S = 1 + math.ceil((S - 1) * args.rank_budget)
            seqs.append(S)
        workload = f"rank{args.model} layers={layers} budget={args.rank_budget} forward, batch {args.batch}/GPU"
    synth.load_synth_weights(model, cfg)
    model = (model.train() if args.train else model.eval()).to(dev)
    infer_model = model
    flops_img = synth.fwd_flops_per_image(cfg, seqs) * (3 if args.train else 1)      # backward = dgrad + wgrad = 2x forward
    if args.train:
        workload = workload.replace("forward", "train step (fwd, cross-entropy, bwd" + (f", gradient all-reduce over {args.dist_backend}" if world > 1 else "")
                                    + (")" if args.no_optimizer else ", clip 1.0, Adam)"))

    # random (never zero-filled) device-resident input, bf16-representable like the parity fixtures
    gen = torch.Generator(device=dev).manual_seed(1234 + rank)
    x = torch.randn(args.batch, 3, cfg["image_size"], cfg["image_size"], generator=gen, device=dev)
    x = x.to(torch.bfloat16).to(torch.float32)

    def barrier():
        if dist:
            td.barrier()
        torch.cuda.synchronize(dev)

    from peekvit_amd import engine
    if args.train:
        from peekvit_amd import dist as pvdist
        y = torch.randint(0, cfg["num_classes"], (args.batch,), generator=gen, device=dev)
        infer = model
        n_buckets = 0
        reducer = pvdist.OverlappedGradReducer(infer.parameters(), bucket_bytes=args.bucket_kib << 10, model=infer) if dist else None      # ~25 MB buckets leave during backward

        # the reference's optimizer (configs/optimizer/adam.yaml: torch.optim.Adam, lr 1e-3) and clip (train/train.py:120); stock
        # multi-tensor PyTorch kernels over the 86.6 M fp32 parameters - plumbing around the path, ~1 % of the step
        params = [p for p in infer.parameters() if p.requires_grad]
        opt = None if args.no_optimizer else torch.optim.Adam(params, lr=1e-3, fused=True)

        def train_step(inp):
            nonlocal n_buckets
            if reducer is not None:
                reducer.zero_grad()          # gradients accumulate straight into the flat all-reduce buckets (their slices are p.grad)
            else:
                for p in params:
                    p.grad = None
            logits = infer(inp)
            torch.nn.functional.cross_entropy(logits, y).backward()
            if dist:
                n_buckets = reducer.finish()
            if opt is not None and not (reducer is not None and reducer.skip_step):      # (an overflowed fp16 step is skipped on every rank alike)
                torch.nn.utils.clip_grad_norm_(params, 1.0, foreach=True)
                opt.step()
            return logits.detach()

        model = train_step
    if args.streams:
        engine._STREAMS = args.streams
    fallbacks0 = engine.fallback_count
    train_fwd_err = None
    if args.full and args.train and world == 1 and not args.no_cpu_baseline and args.rank_budget is None:
        with engine.precision(args.precision):       # BEFORE the optimizer moves the weights away from the oracle's (round 5: rounds 1-4 compared afterwards)
            train_fwd_err = oracle_error(infer_model, cfg, dev, args.cpu_batch, train=True)
    dumped = None
    elapsed_instr = 0.0
    with (torch.enable_grad() if args.train else torch.no_grad()), engine.precision(args.precision):
        for _ in range(args.warmup):
            out = model(x)
        # (Python's first full garbage collection of the process - ~85 ms over the module trees and tensors built so far - otherwise lands somewhere
        # in the first few dozen steps, i.e. inside a short timed region, instead of in start-up where it belongs: scripts/dbg/train_step_times.py)
        import gc
        gc.collect()
        # (1) the contract's timed region: exactly K steps between barrier + synchronize, nothing else on the stream
        if args.full:
            from peekvit_amd import telemetry
            sampler = telemetry.sampler(local)
            window = sampler.window()
        else:
            import contextlib
            window = contextlib.nullcontext()
        barrier()
        t0 = time.perf_counter()
        with window as pw_headline:
            for _ in range(args.steps):
                out = model(x)
            barrier()
        elapsed = time.perf_counter() - t0
        if args.dump_outputs and rank == 0:
            # copied to the host now: the steps below may overwrite buffers the last timed step returned
            dumped = last_step_outputs(out, [p.grad for p in infer_model.parameters()] if args.train else None)
        if args.full:
            # (2) the same K steps again with two HIP events around EVERY launch (on the launch stream) for the per-kernel
            # roofline numbers; the ~200 extra stream commands per step cost ~3 %, which is why (1) is timed without them
            barrier()
            with ops.KernelTimer() as kt:
                t1 = time.perf_counter()
                for _ in range(args.steps):
                    out = model(x)
                barrier()
                elapsed_instr = time.perf_counter() - t1
    assert torch.isfinite(out).all()
    if args.train:
        grads = [p.grad for p in infer_model.parameters()]
        assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads), "non-finite parameter gradient"
    if dumped is not None:
        write_outputs(args.dump_outputs, dumped)
    if dist:
        t = torch.tensor([elapsed, elapsed_instr], device=dev if args.dist_backend == "nccl" else "cpu", dtype=torch.float64)
        td.all_reduce(t, op=td.ReduceOp.MAX)
        elapsed, elapsed_instr = float(t[0].item()), float(t[1].item())

    # the 16-bit operand type the timed steps really computed in: training -> bf16; inference in mode auto -> fp16 unless a guard
    # sent forwards to the fallback mode (split bf16 operands)
    fallbacks = engine.fallback_count - fallbacks0
    if args.precision == "auto":
        dtype = _train_dtype(infer_model) if args.train else ("bf16x3" if (fallbacks or engine.guard_state(infer_model).unsafe) else "f16")
    else:
        dtype = args.precision

    def kernel_report():
        """--full: the per-kernel table and the roofline of the dominant kernel from the instrumented pass (2)."""
        ks = kt.summary()
        dom = max(ks, key=lambda k: ks[k]["ms"])
        d = ks[dom]
        if d["flops"] > 0:
            roof = {"kernel": dom, "bound": "mfma", "achieved": round(d["flops"] / (d["ms"] * 1e-3) / 1e12, 1),
                    "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s", "traffic": None,
                    "peak_sustained_mfma_only_measured": MFMA_BF16_SUSTAINED_MEASURED_TFLOPS}
        else:
            roof = {"kernel": dom, "bound": "hbm", "achieved": round(d["bytes"] / (d["ms"] * 1e-3) / 1e9, 1),
                    "peak": HBM_PEAK_GBS, "unit": "GB/s", "traffic": None}
        roof["frac"] = round(roof["achieved"] / roof["peak"], 4)
        roof["launches_per_step"] = d["launches"] // args.steps
        roof["avg_launch_ms"] = round(d["ms"] / d["launches"], 4)
        roof["algorithmic_per_launch"] = round((d["flops"] if d["flops"] > 0 else d["bytes"]) / d["launches"] / (1e12 if d["flops"] > 0 else 1e9), 4)
        if dom.startswith("pv_gemm_bf16"):
            # The GEMM entry point is four roofline cases.  `roofline` itself = the member the step spends most time in, against ITS bound;
            # `members` = all of them; `family` = every GEMM launch lumped against the MFMA peak (what rounds 1-3 reported as `frac`).
            members = gemm_members(kt, dom, args.steps, cfg)
            top = members[0]
            family = dict(roof)
            roof = {"kernel": f"{dom} [{top['member']}: N={top['N']} K={top['K']}]", "bound": top["bound"], "achieved": top["achieved"], "peak": top["peak"],
                    "unit": top["unit"], "frac": top["frac"], "traffic": None, "launches_per_step": top["launches_per_step"], "avg_launch_ms": top["avg_launch_ms"],
                    "algorithmic_per_launch": round((top["tflops"] if top["bound"] == "mfma" else top["algo_gbs"]) * top["avg_launch_ms"] * 1e-3, 4),
                    "algorithmic_flop_per_byte": top["algorithmic_flop_per_byte"], "ridge_flop_per_byte": round(RIDGE_FLOP_PER_BYTE, 1),
                    "members": members, "family": family}
        # HBM/fabric bytes per launch from the committed PMC passes of this same command (separate FETCH_SIZE / WRITE_SIZE runs, FETCH_SIZE
        # doubled per MI355X_MICROARCH.md "HBM"): profiles/rNN_kernel_summary.json, keyed by the rocprof kernel name - the 256^2 kernel's template
        # argument is the epilogue, so the in-projection (<0>) and fc1 (<1>) have their own rows, the two residual GEMMs share <2>
        try:
            prof = next(f for f in ("r06_kernel_summary.json", "r05_kernel_summary.json", "r04_kernel_summary.json", "r03_kernel_summary.json", "r02_kernel_summary.json") if os.path.exists(os.path.join(ROOT, "profiles", f)))
            summ = json.load(open(os.path.join(ROOT, "profiles", prof)))["kernels"]
            if dom.startswith("pv_gemm_bf16") and args.model == "vit_b_16" and args.batch == 2048 and args.rank_budget is None and not args.train:
                for m in roof["members"]:
                    key = f"pv_gemm256_pf<{m['epilogue']}>"
                    split = key + (" [short]" if m["K"] == cfg["hidden_dim"] else " [long]")      # (out-proj / fc2 share a kernel name: split by duration in the summary)
                    row = summ.get(split) or summ.get(key)
                    if row and "hbm_read_MB" in row:
                        m["traffic"] = round((row["hbm_read_MB"] + row["hbm_write_MB"]) * 1e6)
                        m["traffic_note"] = "bytes/launch, PMC FETCH_SIZE x2 + WRITE_SIZE" + (" (kernel name shared by out-proj and fc2: their launch-weighted mean)" if split not in summ and m["epilogue"] == 2 else "")
                roof["traffic"] = roof["members"][0].get("traffic")
                roof["traffic_source"] = "profiles/" + prof
                roof["traffic_unit"] = "bytes/launch (PMC FETCH_SIZE x2 + WRITE_SIZE) of the dominant member's kernel"
                fam = [v for k, v in summ.items() if k.startswith("pv_gemm") and "hbm_read_MB" in v]
                n = sum(v["launches"] for v in fam)
                roof["family"]["traffic"] = round(sum((v["hbm_read_MB"] + v["hbm_write_MB"]) * 1e6 * v["launches"] for v in fam) / n)
        except (OSError, KeyError, ValueError, StopIteration, ZeroDivisionError):
            pass
        flops_exec = sum(v["flops"] for v in ks.values()) / (args.steps * args.batch)
        # the EMPIRICAL roofline (scripts/power_roofline.hip, profiles/r02_power_roofline.json): what a dependency-free loop with a 256^2 GEMM tile's
        # LDS / L2 operand traffic sustains on this part at the dominant kernel's HBM bytes per FLOP - `peak` above stays the nominal 2.5 PFLOP/s
        try:
            if d["flops"] > 0 and d["bytes"] > 0:
                pr_ = json.load(open(os.path.join(ROOT, "profiles", "r02_power_roofline.json")))
                pts = sorted((r["bytes_per_kflop_hbm"], r["tflops"]) for r in pr_["synthetic"] if r["lds_per_16mfma"] == 6 and r["l2_per_16mfma"] == 2)
                bpk = d["bytes"] / d["flops"] * 1e3
                lo = max((q for q in pts if q[0] <= bpk), default=pts[0]); hi = min((q for q in pts if q[0] >= bpk), default=pts[-1])
                emp = lo[1] if hi[0] == lo[0] else lo[1] + (hi[1] - lo[1]) * (bpk - lo[0]) / (hi[0] - lo[0])
                (roof.get("family") or roof)["empirical"] = {"algorithmic_hbm_bytes_per_kflop": round(bpk, 3), "sustained_by_dependency_free_mix_tflops": round(emp, 1),
                                                             "frac": round(d["flops"] / (d["ms"] * 1e-3) / 1e12 / emp, 4), "source": "profiles/r02_power_roofline.json"}
        except (OSError, KeyError, ValueError, IndexError, ZeroDivisionError):
            pass
        kernels = {k: {"ms_per_step": round(v["ms"] / args.steps, 3),
                       "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1) if v["flops"] else None,
                       "algo_gbs": round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1) if v["bytes"] else None}
                   for k, v in sorted(ks.items(), key=lambda kv: -kv[1]["ms"])}
        return ks, roof, kernels, flops_exec

    if rank == 0:
        value = world * args.batch * args.steps / elapsed
        line = {
            "metric": "images/sec ViT-B/16 fwd @ batch 2048, 224x224" if args.model == "vit_b_16" and args.batch == 2048 and args.rank_budget is None and not args.train
                      else f"images/sec {workload}",
            "value": round(value, 1), "unit": "images/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": dtype, "data": "synthetic",
            "config": {"workload": workload, "global_batch": world * args.batch,
                       "parallelism": (f"dp{world} (batch-sharded, gradient all-reduce over {args.dist_backend})" if args.train and dist
                                       else f"replicas x{world} (batch-sharded, no collective)"),
                       "gflop_per_image": round(flops_img / 1e9, 3),
                       "precision_mode": args.precision, "streams": engine._STREAMS,
                       "operands": {"f16": "IEEE fp16 operands, fp32 accumulate (same MFMA rate as bf16), range-guarded" if args.precision == "auto"
                                    else "IEEE fp16 operands, fp32 accumulate", "bf16": "bf16 operands, fp32 accumulate",
                                    "bf16x3": "split bf16 hi+lo operands (3 products), fp32 accumulate"}[dtype],
                       "range_guard_fallbacks": fallbacks,
                       "self_check": (None if args.train or engine.selfcheck_last is None else
                                      {"fp16_vs_bf16x3_logits_rel_l2": float(f"{engine.selfcheck_last[0]:.3e}"), "images": engine.selfcheck_last[1],
                                       "limit": engine.SELFCHECK_LIMIT, "note": "mode auto's own measurement on the first forward of this batch size (engine.run_guarded)"})},
        }
        if args.full:
            ks, roof, kernels, flops_exec = kernel_report()
            line["ms_per_step_instrumented"] = round(elapsed_instr / args.steps * 1e3, 3)
            line["config"]["gflop_per_image_executed"] = round(flops_exec / 1e9, 3)
            line["config"]["last_block"] = ("class-token rows only (k|v for all tokens; q, out-proj, MLP for the rows the head reads; same logits)"
                                            if "pv_attention_rows_bf16" in ks else "all rows")
            # MFMA FLOPs the kernels really executed per second (their own algorithmic counts) over the dense bf16 peak - NOT the
            # reference formula's FLOPs, of which the last block skips the rows nobody reads
            line["model_mfma_roofline_frac"] = round(value / world * flops_exec / (MFMA_BF16_PEAK_TFLOPS * 1e12), 4)
            line["roofline"], line["kernels"] = roof, kernels
            # the operating point the timed region ran at (round 6, review item 3): mean package power and shader clock over exactly the K timed steps of rank 0,
            # the board's power cap, and the empirical (dependency-free instruction mix at this bytes/FLOP) roofline of the GEMM family next to the nominal one
            pw = pw_headline.result()
            line["power_w"], line["sclk_mhz"] = pw.get("power_w"), pw.get("sclk_mhz")
            line["power"] = dict(pw, cap_w=sampler.cap_w(), source="sysfs hwmon power1_average / freq1_input of this GPU, ~50 Hz host thread (peekvit_amd/telemetry.py)")
            emp = (roof.get("family") or roof).get("empirical")
            if emp:
                line["empirical_roofline"] = emp
        if args.full and args.train and world == 1 and not args.no_cpu_baseline and args.rank_budget is None:
            # the forward of the TRAINING arithmetic (fp16 operands + loss scale since round 5) against the fp32 oracle, next to `dtype`
            line["train_forward_logits_rel_l2_vs_oracle"] = train_fwd_err
            line["train_forward_logits_note"] = "train-mode forward on the initial weights; contract: 1e-3; gradients are asserted at 2e-3 against the reference's training step"
            from peekvit_amd import train_engine as _te
            _st = _te.train_state(infer_model)
            line["loss_scale"] = {"scale": _st.scale, "target_max_entering_gradient": _st.target, "steps": _st.steps, "steps_skipped_for_overflow": _st.skipped}
        if args.train and dist:
            line["grad_allreduce"] = {"buckets_per_step": n_buckets, "launched_during_backward_total": reducer.launched_before_finish,
                                      "bucket_bytes": reducer.bucket_bytes}
        if args.full and not args.no_cpu_baseline and world == 1:
            plain = args.rank_budget is None and not args.train
            line["cpu_baseline"] = cpu_baseline(cfg, args.cpu_batch, args.cpu_iters, infer_model if plain else None, dev)
            if plain and args.precision == "auto":
                # the same forward on bf16 operands (the explicit "bf16" mode), for the record
                with torch.no_grad(), engine.precision("bf16"):
                    for _ in range(2):
                        infer_model(x)
                    torch.cuda.synchronize(dev)
                    t2 = time.perf_counter()
                    for _ in range(args.steps):
                        infer_model(x)
                    torch.cuda.synchronize(dev)
                    dtb = time.perf_counter() - t2
                line["bf16_mode"] = {"value": round(args.batch * args.steps / dtb, 1), "unit": "images/sec",
                                     "ms_per_step": round(dtb / args.steps * 1e3, 3), "dtype": "bf16"}
            if plain and engine._LAST_BLOCK_ROWS:
                # the same forward with the last block computing all S rows, as the reference does (PEEKVIT_AMD_LAST_BLOCK_ROWS=0)
                engine._LAST_BLOCK_ROWS = False
                try:
                    with torch.no_grad(), engine.precision(args.precision):
                        for _ in range(2):
                            infer_model(x)
                        torch.cuda.synchronize(dev)
                        t2 = time.perf_counter()
                        for _ in range(args.steps):
                            infer_model(x)
                        torch.cuda.synchronize(dev)
                        dta = time.perf_counter() - t2
                finally:
                    engine._LAST_BLOCK_ROWS = True
                line["all_rows_mode"] = {"value": round(args.batch * args.steps / dta, 1), "unit": "images/sec",
                                         "ms_per_step": round(dta / args.steps * 1e3, 3), "gflop_per_image": round(flops_img / 1e9, 3)}
            err = line["cpu_baseline"].get("gpu_logits_rel_l2_vs_oracle", {}).get(args.precision)
            if plain and err is not None:
                line["logits_rel_l2_vs_oracle"] = err
                line["logits_tolerance"] = 1e-3
                if dtype == "f16" and not err <= 1e-3:
                    # the reported operand type is the one that is supposed to meet BASELINE.json's contract: refuse to report otherwise
                    print(json.dumps(line), file=sys.stderr, flush=True)
                    raise SystemExit(f"bench.py: dtype {dtype} logits are {err:.2e} from the CPU oracle, outside the 1e-3 contract: no result line")
        if args.full and world == 1 and not args.no_extra and args.model == "vit_b_16" and args.batch == 2048 and args.rank_budget is None and not args.train \
                and args.precision == "auto":
            # (c) the reference's own images/sec definition as a second value; (b) BASELINE configs 2, 4 and config 3's training step in the same
            # invocation: the driver's one `bench.py --gpus 1` then times them too.  `value` above is untouched by these.
            line["reference_loop"] = reference_loop(infer_model, cfg, args.batch, args.steps, dev)
            # ... and the same definition over the loop the harness runs: uint8 batches, prefetcher, deferred guard read (round 5)
            line["pipeline_loop"] = pipeline_loop(infer_model, cfg, args.batch, args.steps, dev)
            del x, out
            infer_model.to("cpu")
            torch.cuda.empty_cache()
            # (a 5 ms step wants more than 20 of them behind one synchronize: vit_small runs 5x the steps and warm-up, half a second in all)
            ex_steps = {"vit_small_fwd": 5 * args.steps, "rankvit_b16_fwd": args.steps}
            ex_warm = {"vit_small_fwd": 4 * (min(args.warmup, 3) + 2)}
            line["extra_configs"] = [extra_config(k, dev, ex_steps.get(k, max(5, args.steps // 2)), ex_warm.get(k, min(args.warmup, 3) + 2))
                                     for k in ("vit_small_fwd", "rankvit_b16_fwd", "vit_b_16_train_step", "vit_b_16_trained_like_weights_fwd", "vit_b_16_hostile_weights_fwd")]
            line["extra_configs"].append(small_model_entry(dev))
        print(json.dumps(line), flush=True)
    if dist:
        td.barrier()
        td.destroy_process_group()


if __name__ == "__main__":
    main()
