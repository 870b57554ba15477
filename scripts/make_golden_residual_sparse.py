"""Generate tests/golden/residualvit_sparse.npz + residualvit_sparse_meta.json by running the REAL reference ResidualVisionTransformer
(models/residualvit.py) on CPU, with gates that actually mask tokens.

Run in the build container only (the reference never travels to the GPU box):

    python scripts/make_golden_residual_sparse.py [--gate-gain G]

The reference is imported through oracle.make_golden.import_reference; a class that does not resolve to a file under the reference checkout
is refused.  Weights: peekvit_amd.synth.residual_sparse_state_dict(cfg, gate_gain) with gate_bias=1 on ViT-B/16 dims; images:
synth.synth_images(2, 224, seed=0).  Both are pure functions of name + seed, so the fixture holds OUTPUTS only, per budget 0.2 / 0.5 / 0.8:

    b{budget}_logits      fp32 [2, 1000]        the reference's logits
    b{budget}_masks       fp32 [12, 2, 196, 1]  every block's mask
    b{budget}_thresholds  fp32 [12, 2]          sigmoid(budget_token_gate(budget token)) per block and image
    b{budget}_margin      fp32 [12, 2, 196]     every token's gate margin |sigmoid - threshold| in its block
    b{budget}_rows_share  fp64 []               rows the compacting forward runs / rows the dense forward runs, by an fp64 restatement

A mask is relu(sigmoid - threshold): whether a token is collapsed (mask exactly 0) or live in a block is a comparison, and a margin near 0
can resolve differently under 16-bit operands.  The GPU test compares that state token by token except where the recorded margin is under
5e-3; this script asserts that no more than 2 % of the (block, image, token) entries of any budget are left out that way.
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
import residual_sparse_ref as R            # (tests/: the fp64 restatement of the compacting forward, for the rows-run share; before the
                                           #  reference import takes the repository off sys.path)

GOLD = os.path.join(REPO, "tests", "golden")
REF_FILES = ("models/residualvit.py", "models/blocks.py")
BUDGETS = (0.2, 0.5, 0.8)
MARGIN, MAX_EXCLUDED = 5e-3, 0.02
BATCH = 2


def main():
    gain = float(sys.argv[sys.argv.index("--gate-gain") + 1]) if "--gate-gain" in sys.argv else 4.0
    _, _, ResVT = MG.import_reference()
    src = os.path.realpath(inspect.getsourcefile(ResVT))
    if not src.startswith(MG.REF_ROOT + "/"):
        raise SystemExit(f"resolved ResidualVisionTransformer to {src}, not the reference: refusing to write fixtures")
    torch.set_num_threads(8)
    cfg = dict(synth.MODEL_CONFIGS["vit_b_16"])
    extra = dict(residual_layers=["attention+mlp"] * cfg["num_layers"], gate_temp=1, add_input=False, gate_type="sigmoid", gate_threshold=0.5,
                 gate_bias=1, add_budget_token="learnable")
    scfg = dict(cfg, **extra)
    torch.manual_seed(0)
    model = ResVT(**cfg, **extra).eval()
    sd = synth.residual_sparse_state_dict(scfg, gate_gain=gain, seed=0)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    x = torch.from_numpy(synth.synth_images(BATCH, cfg["image_size"], seed=0))
    sd64 = {k: torch.from_numpy(v.copy()).double() for k, v in sd.items()}
    arrays, info = {}, {}
    for b in BUDGETS:
        model.set_budget(b)
        thr, sig = [], []
        hooks = []
        for blk in model.encoder.layers:
            # the gate's sigmoid (before the threshold is subtracted) and the threshold, as the reference computes them
            hooks.append(blk.residual_gate.gate.register_forward_hook(lambda m, i, o, acc=sig: acc.append(o.detach().clone())))
            hooks.append(blk.budget_token_gate.register_forward_hook(lambda m, i, o, acc=thr: acc.append(torch.sigmoid(o.detach()))))
        with torch.no_grad():
            logits = model(x)
        for h in hooks:
            h.remove()
        masks = torch.stack([blk.mask.detach() for blk in model.encoder.layers])           # [L, B, N, 1]
        thr = torch.stack(thr).reshape(cfg["num_layers"], BATCH)
        margin = (torch.stack(sig).reshape(cfg["num_layers"], BATCH, -1) - thr[:, :, None]).abs()
        assert torch.equal(masks.squeeze(-1) == 0, (torch.stack(sig).reshape(margin.shape) - thr[:, :, None]) <= 0)
        _, m64, _, rows = R.packed_forward(x.double(), sd64, scfg, b)
        assert torch.equal(m64 == 0, masks == 0), "the fp64 restatement and the reference disagree on a token's state"
        share = sum(rows) / float(len(rows) * BATCH * (synth.seq_length(cfg) + 1))
        excluded = float((margin < MARGIN).float().mean())
        assert excluded <= MAX_EXCLUDED, f"budget {b}: {excluded:.4f} of the tokens have a gate margin under {MARGIN}"
        arrays[f"b{b}_logits"] = logits.numpy()
        arrays[f"b{b}_masks"] = masks.numpy()
        arrays[f"b{b}_thresholds"] = thr.numpy()
        arrays[f"b{b}_margin"] = margin.numpy()
        arrays[f"b{b}_rows_share"] = np.float64(share)
        info[str(b)] = {"rows_share": share, "excluded_fraction": excluded, "min_margin": float(margin.min()),
                        "mask_zero_fraction": [float((masks[i] == 0).float().mean()) for i in range(cfg["num_layers"])]}
        print(f"budget {b}: rows share {share:.3f}, excluded {excluded:.4f}, zeros {['%.2f' % z for z in info[str(b)]['mask_zero_fraction']]}")
    np.savez_compressed(os.path.join(GOLD, "residualvit_sparse.npz"), **arrays)
    sig = inspect.signature(ResVT.__init__)
    meta = {"torch": torch.__version__, "reference_class": "models/residualvit.py:ResidualVisionTransformer",
            # the reference's constructor, so that the test of the opt-in switch can pin the whole signature
            "constructor_parameters": [k for k in sig.parameters if k != "self"],
            "constructor_defaults": {k: p.default for k, p in sig.parameters.items() if k != "self" and p.default is not inspect.Parameter.empty},
            "reference_sha256": {f: hashlib.sha256(open(os.path.join(MG.REF_ROOT, f), "rb").read()).hexdigest() for f in REF_FILES},
            "model": "vit_b_16", "kwargs": extra, "gate_gain": gain, "batch": BATCH, "budgets": list(BUDGETS), "margin": MARGIN,
            "max_excluded_fraction": MAX_EXCLUDED,
            "weights": "peekvit_amd.synth.residual_sparse_state_dict(cfg, gate_gain, seed=0); images: synth.synth_images(batch, 224, seed=0)",
            "budget": info}
    with open(os.path.join(GOLD, "residualvit_sparse_meta.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print(os.path.getsize(os.path.join(GOLD, "residualvit_sparse.npz")), "bytes")


if __name__ == "__main__":
    main()
