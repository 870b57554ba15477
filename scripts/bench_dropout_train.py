"""One training step of a ViT with dropout, `set_fused_dropout` off and on, and what the mask generator costs the streaming attention kernels
(bench.py is not involved; DESIGN.md section 31 holds the numbers).

    python scripts/bench_dropout_train.py [--model vit_b_16] [--batch 256] [--steps 10] [--warmup 2] [--precision auto] [--out FILE.json]

Without --leg the script is a driver: every measurement ("leg") is a child process of its own under `timeout`, the legs are chained and the first one
that fails, aborts or runs out of time ends the run - nothing more is started on the device behind it.

  step:<dropout>:<attention_dropout>   a ViT-B/16 training step (forward, cross-entropy, backward, SGD) at the given batch with the switch off - the
                                        parent's behaviour: the stock composite under dropout, the HIP training path at (0, 0) - then on, then off
                                        again, in one process: ms per step (median of three timed segments, a device synchronise at both ends) and the
                                        peak allocated memory of each.  One KernelTimer step with the switch on lists the kernels.
  kernels                               the streaming attention forward and 16-bit backward entry points with DROP off and on (p = 0.1) at
                                        B = 256, H = 12, S = 197, dh = 64, alternating, by device events around 200 launches each: the difference is
                                        the generator.  The resident forward and the persistent backward the dropout-free step uses are timed too."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = ((0.0, 0.0), (0.1, 0.0), (0.1, 0.1))
LEG_SECONDS = {"step": 420, "kernels": 180}


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
    return sorted(segs)[1]


def _measure(fn, steps, warmup, dev):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    t = _time(fn, steps, dev)
    return round(t * 1e3, 3), round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1)


def leg_step(a, dropout, attention_dropout):
    import torch
    import torch.nn.functional as F
    from peekvit_amd import engine, ops, synth
    from peekvit_amd.models.vit import VisionTransformer
    dev = torch.device("cuda:0")
    cfg = synth.MODEL_CONFIGS[a.model]
    with engine.precision(a.precision):
        model = VisionTransformer(**cfg, dropout=dropout, attention_dropout=attention_dropout)
        synth.load_synth_weights(model, cfg)
        model = model.to(dev).train()
        opt = torch.optim.SGD(model.parameters(), lr=1e-6)
        x = torch.from_numpy(synth.synth_images(a.batch, cfg["image_size"], seed=0)).to(dev)
        target = torch.arange(a.batch, device=dev) % cfg["num_classes"]

        def step():
            opt.zero_grad(set_to_none=True)
            F.cross_entropy(model(x), target).backward()
            opt.step()

        line = {"leg": "step", "model": a.model, "batch": a.batch, "precision": a.precision, "dropout": dropout, "attention_dropout": attention_dropout}
        active = max(dropout, attention_dropout) > 0
        for tag, on in (("off", False), ("on", True), ("off_again", False)):
            model.set_fused_dropout(on)
            n0 = ops.launch_count
            line[f"step_{tag}_ms"], line[f"step_{tag}_peak_mib"] = _measure(step, a.steps, a.warmup, dev)
            line[f"launches_{tag}"] = ops.launch_count - n0          # C-ABI launches: 0 on the stock composite
            assert (line[f"launches_{tag}"] > 0) == (on or not active), (tag, line)
        model.set_fused_dropout(True)
        with ops.KernelTimer() as kt:
            step()
        torch.cuda.synchronize(dev)
        s = kt.summary()
        line["kernels_ms"] = round(sum(v["ms"] for v in s.values()), 3)
        line["kernel_summary_ms"] = {k: {"launches": v["launches"], "ms": round(v["ms"], 3)} for k, v in sorted(s.items(), key=lambda kv: -kv[1]["ms"])}
        line["speedup_on_over_off"] = round(0.5 * (line["step_off_ms"] + line["step_off_again_ms"]) / line["step_on_ms"], 3)
    return line


def leg_kernels(a):
    import torch
    from peekvit_amd import _lib, engine, ops
    dev = torch.device("cuda:0")
    B, H, S, dh, p, reps = a.batch, 12, 197, 64, 0.1, 200
    D, nb, qscale = H * dh, (S + 63) // 64, dh ** -0.5
    line = {"leg": "kernels", "B": B, "H": H, "S": S, "dh": dh, "p": p, "precision": a.precision}
    with engine.precision("f16" if a.precision == "auto" else "bf16"):          # the operand build a training pass uses in that mode
        dt = _lib.operand_dtype()
        line["operands"] = str(dt)
        g = torch.Generator(device="cuda").manual_seed(0)
        qkv = torch.randn(B, S, 3 * D, generator=g, device=dev)
        qkv[..., :D] *= qscale
        qkv = qkv.to(dt)
        dout = (torch.randn(B, S, D, generator=g, device=dev) * 0.1).to(dt)
        out, lse = torch.empty((B, S, D), dtype=dt, device=dev), torch.empty((B, H, S), device=dev)
        dq, dbp, dl = torch.empty((B, S, 3 * D), dtype=dt, device=dev), torch.empty((B, nb, 3 * D), device=dev), torch.empty((B, H, S), device=dev)
        dbp1 = torch.empty((B, 3 * D), device=dev)
        calls = {
            "stream_fwd": lambda: ops.attention_stream(qkv, out, lse, B, S, H, dh),
            "stream_fwd_drop": lambda: ops.attention_stream_drop(qkv, out, lse, B, S, H, dh, p, 1234, 7),
            "stream_bwd16": lambda: ops.attention_stream_bwd16(qkv, dout, out, lse, dq, B, S, H, dh, qscale, dbias_partial=dbp, delta_ws=dl),
            "stream_bwd16_drop": lambda: ops.attention_stream_bwd16_drop(qkv, dout, out, lse, dq, B, S, H, dh, qscale, p, 1234, 7, dbias_partial=dbp, delta_ws=dl),
            "resident_fwd_lse": lambda: ops.attention(qkv, out, B, S, H, dh, lse=lse),
            "persistent_bwd_lse": lambda: ops.attention_bwd_lse(qkv, dout, out, lse, dq, B, S, H, dh, qscale, dbias_partial=dbp1),
        }
        times = {k: [] for k in calls}
        for fn in calls.values():                              # warm up every shape
            for _ in range(3):
                fn()
        torch.cuda.synchronize(dev)
        for _round in range(3):                                # alternate the versions; the median of three rounds
            for name, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) / reps)
        for name, ts in times.items():
            line[name + "_ms"] = round(sorted(ts)[1], 4)
            line[name + "_spread_ms"] = round(max(ts) - min(ts), 4)
        line["generator_fwd_ms"] = round(line["stream_fwd_drop_ms"] - line["stream_fwd_ms"], 4)
        line["generator_bwd_ms"] = round(line["stream_bwd16_drop_ms"] - line["stream_bwd16_ms"], 4)
    return line


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="vit_b_16")
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--precision", default="auto", choices=["auto", "bf16"])
    p.add_argument("--out", default="")
    p.add_argument("--leg", default="")
    a = p.parse_args()
    if a.leg:                                                  # a child: one measurement, one JSON line
        kind, _, rest = a.leg.partition(":")
        line = leg_kernels(a) if kind == "kernels" else leg_step(a, *[float(v) for v in rest.split(":")])
        print("RESULT " + json.dumps(line), flush=True)
        return 0
    legs = [f"step:{d}:{ad}" for d, ad in CONFIGS] + ["kernels"]
    lines = []
    for leg in legs:
        cmd = ["timeout", "-k", "10", str(LEG_SECONDS[leg.partition(":")[0]]), sys.executable, os.path.abspath(__file__), "--leg", leg, "--model", a.model,
               "--batch", str(a.batch), "--steps", str(a.steps), "--warmup", str(a.warmup), "--precision", a.precision]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        res = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not res:
            print(r.stdout[-4000:])
            print(f"leg {leg} ended with status {r.returncode}: nothing further is started", flush=True)
            return r.returncode or 1
        line = json.loads(res[-1])
        lines.append(line)
        print(json.dumps({k: v for k, v in line.items() if k != "kernel_summary_ms"}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"legs": lines}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
