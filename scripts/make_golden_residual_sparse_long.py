"""Generate tests/golden/residualvit_sparse_long.npz + residualvit_sparse_long_meta.json by running the REAL reference ResidualVisionTransformer
(models/residualvit.py) on CPU at more than 208 rows per image, with gates that actually mask tokens.

Run in the build container only (the reference never travels to the GPU box):

    python scripts/make_golden_residual_sparse_long.py

scripts/make_golden_residual_sparse.py at the dims of the ResidualViT the reference ships (patch 8, hidden 256, 4 heads of 64, 4 layers, mlp 768,
10 classes) and at two image sizes: 120 px (15 x 15 patches + class + budget row = 227 rows: the first layers stream, later ones fit the resident
kernel) and 160 px (402 rows).  Weights: peekvit_amd.synth.residual_sparse_state_dict(cfg, gate_gain=4.0) with gate_bias=1; images:
synth.synth_images(2, size, seed=0).  Both are pure functions of name + seed, so the fixture holds OUTPUTS only, per size and budget 0.2 / 0.5 / 0.8:

    s{size}_b{budget}_logits      fp32 [2, 10]         the reference's logits
    s{size}_b{budget}_masks       fp32 [4, 2, N, 1]    every block's mask (N = (size / 8)^2)
    s{size}_b{budget}_thresholds  fp32 [4, 2]          sigmoid(budget_token_gate(budget token)) per block and image
    s{size}_b{budget}_margin      fp32 [4, 2, N]       every token's gate margin |sigmoid - threshold| in its block
    s{size}_b{budget}_rows_share  fp64 []              rows the compacting forward runs / rows the dense forward runs, by an fp64 restatement

The GPU test compares a token's state (collapsed or live) except where the recorded margin is under 5e-3; this script asserts that no more than
2 % of the (block, image, token) entries of any size and budget are left out that way, and that the fp64 restatement of the compacting forward
(tests/residual_sparse_ref.py) agrees with the reference on every token's state.
"""
from __future__ import annotations

import hashlib
import inspect
import json
import os
import sys

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np
import torch

from peekvit_amd import synth
from oracle import make_golden as MG
import residual_sparse_ref as R            # (tests/: the fp64 restatement of the compacting forward; before the reference import takes the
                                           #  repository off sys.path)

GOLD = os.path.join(REPO, "tests", "golden")
REF_FILES = ("models/residualvit.py", "models/blocks.py")
DIMS = dict(patch_size=8, num_layers=4, num_heads=4, hidden_dim=256, mlp_dim=768, num_classes=10)
SIZES = (120, 160)
BUDGETS = (0.2, 0.5, 0.8)
MARGIN, MAX_EXCLUDED = 5e-3, 0.02
BATCH, GAIN = 2, 4.0


def main():
    _, _, ResVT = MG.import_reference()
    src = os.path.realpath(inspect.getsourcefile(ResVT))
    if not src.startswith(MG.REF_ROOT + "/"):
        raise SystemExit(f"resolved ResidualVisionTransformer to {src}, not the reference: refusing to write fixtures")
    torch.set_num_threads(8)
    extra = dict(residual_layers=["attention+mlp"] * DIMS["num_layers"], gate_temp=1, add_input=False, gate_type="sigmoid", gate_threshold=0.5,
                 gate_bias=1, add_budget_token="learnable")
    L = DIMS["num_layers"]
    arrays, info = {}, {}
    for size in SIZES:
        cfg = dict(DIMS, image_size=size)
        scfg = dict(cfg, **extra)
        torch.manual_seed(0)
        model = ResVT(**cfg, **extra).eval()
        sd = synth.residual_sparse_state_dict(scfg, gate_gain=GAIN, seed=0)
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
        x = torch.from_numpy(synth.synth_images(BATCH, size, seed=0))
        sd64 = {k: torch.from_numpy(v.copy()).double() for k, v in sd.items()}
        S = synth.seq_length(cfg) + 1
        info[str(size)] = {"rows": S, "budget": {}}
        for b in BUDGETS:
            model.set_budget(b)
            thr, sig, hooks = [], [], []
            for blk in model.encoder.layers:
                # the gate's sigmoid (before the threshold is subtracted) and the threshold, as the reference computes them
                hooks.append(blk.residual_gate.gate.register_forward_hook(lambda m, i, o, acc=sig: acc.append(o.detach().clone())))
                hooks.append(blk.budget_token_gate.register_forward_hook(lambda m, i, o, acc=thr: acc.append(torch.sigmoid(o.detach()))))
            with torch.no_grad():
                logits = model(x)
            for h in hooks:
                h.remove()
            masks = torch.stack([blk.mask.detach() for blk in model.encoder.layers])           # [L, B, N, 1]
            thr = torch.stack(thr).reshape(L, BATCH)
            sig = torch.stack(sig).reshape(L, BATCH, -1)
            margin = (sig - thr[:, :, None]).abs()
            assert torch.equal(masks.squeeze(-1) == 0, (sig - thr[:, :, None]) <= 0)
            _, m64, _, rows = R.packed_forward(x.double(), sd64, scfg, b)
            assert torch.equal(m64 == 0, masks == 0), "the fp64 restatement and the reference disagree on a token's state"
            share = sum(rows) / float(len(rows) * BATCH * S)
            excluded = float((margin < MARGIN).float().mean())
            assert excluded <= MAX_EXCLUDED, f"{size} px budget {b}: {excluded:.4f} of the tokens have a gate margin under {MARGIN}"
            key = f"s{size}_b{b}_"
            arrays[key + "logits"] = logits.numpy()
            arrays[key + "masks"] = masks.numpy()
            arrays[key + "thresholds"] = thr.numpy()
            arrays[key + "margin"] = margin.numpy()
            arrays[key + "rows_share"] = np.float64(share)
            info[str(size)]["budget"][str(b)] = {"rows_share": share, "excluded_fraction": excluded, "min_margin": float(margin.min()),
                                                 "rows_per_layer": [int(r) for r in rows],
                                                 "mask_zero_fraction": [float((masks[i] == 0).float().mean()) for i in range(L)]}
            print(f"{size} px budget {b}: rows share {share:.3f}, excluded {excluded:.4f}, rows per layer {rows} of {BATCH * S}")
    np.savez_compressed(os.path.join(GOLD, "residualvit_sparse_long.npz"), **arrays)
    meta = {"torch": torch.__version__, "reference_class": "models/residualvit.py:ResidualVisionTransformer",
            "reference_sha256": {f: hashlib.sha256(open(os.path.join(MG.REF_ROOT, f), "rb").read()).hexdigest() for f in REF_FILES},
            "dims": DIMS, "sizes": list(SIZES), "kwargs": extra, "gate_gain": GAIN, "batch": BATCH, "budgets": list(BUDGETS), "margin": MARGIN,
            "max_excluded_fraction": MAX_EXCLUDED,
            "weights": "peekvit_amd.synth.residual_sparse_state_dict(cfg, gate_gain, seed=0); images: synth.synth_images(batch, size, seed=0)",
            "size": info}
    with open(os.path.join(GOLD, "residualvit_sparse_long_meta.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print(os.path.getsize(os.path.join(GOLD, "residualvit_sparse_long.npz")), "bytes")


if __name__ == "__main__":
    main()
