"""A-ViT packed-halting forward vs the plain VisionTransformer of the same dims (bench.py is not involved).

    python scripts/bench_avit.py [--batch 2048] [--steps 5] [--out profiles/avit_bench.json]

For avit_s (D 384, 6 heads) and avit_t (D 192, 3 heads) dims at 224 / patch 16 / 12 layers, synthetic weights (peekvit_amd.synth), random images:
img/s and ms/step of the A-ViT forward at gate_center 30 / 5 / 2 (mean depth 11.7 / 6.7 / lower on these weights) and of the ViT forward, each the
median of three timed segments; mean token depth, the fraction of the dense model's rows the A-ViT layers ran, the GPU time of the per-layer host
read of the next row count, and package power / shader clock over the segments (peekvit_amd/telemetry.py).  One JSON line per configuration.

Past 208 tokens: `--dims ref_small --size 160` (or 224) runs the reference's small dims (patch 8, hidden 256, 4 heads, 4 layers)
at 401 / 785 tokens; every line then also carries the stock composite on the same GPU (`composite_*`: what a parent without the long path runs at
these shapes) and the layers per forward whose attention streamed.
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
from peekvit_amd.models.adavit import AdaptiveVisionTransformer
from peekvit_amd.models.vit import VisionTransformer

DIMS = {"avit_s": dict(hidden_dim=384, mlp_dim=1536, num_heads=6), "avit_t": dict(hidden_dim=192, mlp_dim=768, num_heads=3),
        "ref_small": dict(hidden_dim=256, mlp_dim=768, num_heads=4, patch_size=8, num_layers=4)}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dims", default="avit_s,avit_t")
    ap.add_argument("--centers", default="30,5,2")
    ap.add_argument("--out", default="")
    ap.add_argument("--size", type=int, default=224, help="image size (with --dims ref_small: 160 -> 401 tokens, 224 -> 785)")
    ap.add_argument("--composite", action="store_true", help="also time the stock-op composite of the A-ViT on the same GPU")
    ap.add_argument("--mode", default="auto", help="precision mode of the A-ViT forwards (the ViT line always runs in the default mode)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sampler = telemetry.sampler(0)
    x = torch.randn(a.batch, 3, a.size, a.size, generator=torch.Generator().manual_seed(0)).to(dev)
    lines = []
    for dname in a.dims.split(","):
        cfg = dict(dict(image_size=a.size, patch_size=16, num_layers=12, num_classes=1000), **DIMS[dname])
        L = cfg["num_layers"]
        sd = {k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(cfg, seed=0).items()}
        vit = VisionTransformer(**cfg).eval()
        vit.load_state_dict(sd)
        vit = vit.to(dev)
        with torch.no_grad():
            for _ in range(a.warmup):
                vit(x)
            dt_vit, segs_vit, pw_vit = _time(lambda: vit(x), a.steps, dev, sampler)
        del vit
        for gc in [float(v) for v in a.centers.split(",")]:
            model = AdaptiveVisionTransformer(**cfg, gate_center=gc).eval()
            model.load_state_dict(sd)
            model = model.to(dev)
            with torch.no_grad(), engine.precision(a.mode):
                for _ in range(a.warmup):
                    model(x)
                r0, s0, l0 = engine.act_rows, engine.act_syncs, engine.avit_long_layers
                dt, segs, pw = _time(lambda: model(x), a.steps, dev, sampler)
                n_fwd = 3 * a.steps
                rows = (engine.act_rows - r0) / n_fwd
                syncs = (engine.act_syncs - s0) / n_fwd
                streamed = (engine.avit_long_layers - l0) / n_fwd
                engine.act_gaps = []
                model(x)
                torch.cuda.synchronize(dev)
                gaps = [e0.elapsed_time(e1) for e0, e1 in engine.act_gaps]
                engine.act_gaps = None
            S = model.seq_length
            depth = float(model.encoder.counter_token.float().mean())
            comp = {}
            if a.composite:
                with torch.no_grad():
                    for _ in range(a.warmup):
                        model._composite_forward(x)
                    dt_c, segs_c, _ = _time(lambda: model._composite_forward(x), a.steps, dev, sampler)
                comp = {"composite_img_per_s": round(a.batch / dt_c, 1), "composite_ms_per_step": round(dt_c * 1e3, 3),
                        "composite_segments_ms": [round(t * 1e3, 3) for t in segs_c], "speedup_vs_composite": round(dt_c / dt, 3)}
            line = {"model": f"{dname} dims (D {cfg['hidden_dim']}, {cfg['num_heads']} heads, {L} layers, {a.size}/{cfg['patch_size']})", "gate_center": gc,
                    "tokens": S, "streamed_layers_per_forward": streamed, **comp,
                    "batch": a.batch, "mode": a.mode, "fell_back": a.mode == "auto" and not engine.last_forward_guarded(),
                    "avit_img_per_s": round(a.batch / dt, 1), "avit_ms_per_step": round(dt * 1e3, 3),
                    "avit_segments_ms": [round(t * 1e3, 3) for t in segs],
                    "vit_img_per_s": round(a.batch / dt_vit, 1), "vit_ms_per_step": round(dt_vit * 1e3, 3),
                    "vit_segments_ms": [round(t * 1e3, 3) for t in segs_vit],
                    "speedup_vs_vit": round(dt_vit / dt, 3), "mean_depth": round(depth, 3),
                    "rows_executed_frac": round(rows / (L * a.batch * S), 4), "host_syncs_per_forward": syncs,
                    "sync_gap_ms_per_forward": round(sum(gaps), 3), "sync_gap_ms_per_layer_median": round(sorted(gaps)[len(gaps) // 2], 4) if gaps else None,
                    "power_avit": pw, "power_vit": pw_vit}
            print(json.dumps(line), flush=True)
            lines.append(line)
            del model
    if a.out:
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
