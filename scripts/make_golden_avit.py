"""Generate tests/golden/avit*.npz + avit_meta.json by running the REAL reference A-ViT (/root/reference/models/adavit.py) on CPU.

Run in the build container only (the reference never travels to the GPU box):

    python scripts/make_golden_avit.py

The reference is imported exactly as oracle/make_golden.py does it (a /tmp symlink named `peekvit` on sys.path, the repository's own
`peekvit` package taken off it, torchvision replaced by placeholders); a class that does not resolve to a file under the reference checkout
is refused.  The reference hard-codes `.cuda()` for its halting state (models/adavit.py:147-151, :187): `torch.Tensor.cuda` is patched to
the identity while the fixtures are captured, and restored afterwards.

As for the other fixtures, weights and images come from peekvit_amd.synth (pure functions of name + seed, bf16-representable), so a
fixture holds the inputs and the OUTPUTS: logits, rho_token, counter_token, halting_score_layer, and the per-layer token halting scores
h_token [L, B, S] (recorded by wrapping every block's forward_act), from which a test knows each token's distance to the threshold.
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

import numpy as np
import torch

from peekvit_amd import synth
from oracle import make_golden as MG

GOLD = os.path.join(REPO, "tests", "golden")
REF_FILES = ("models/adavit.py", "models/blocks.py")

_MICRO = dict(image_size=32, patch_size=8, num_layers=4, num_heads=2, hidden_dim=128, mlp_dim=256, num_classes=10)
_T224 = dict(image_size=224, patch_size=16, num_layers=12, num_heads=3, hidden_dim=192, mlp_dim=768, num_classes=10)
_S224 = dict(image_size=224, patch_size=16, num_layers=12, num_heads=6, hidden_dim=384, mlp_dim=1536, num_classes=10)

# name -> (model kwargs, batch)
CASES = {
    "avit_micro": (dict(_MICRO, gate_center=2.0), 4),
    "avit_t224_gc5": (dict(_T224, gate_center=5), 2),
    "avit_s224_gc30": (dict(_S224, gate_center=30), 2),
    "avit_s224_gc5": (dict(_S224, gate_center=5), 2),
    "avit_cls2_reg2": (dict(_MICRO, num_class_tokens=2, num_registers=2, gate_center=2.0), 4),
    "avit_allhalt": (dict(_MICRO, gate_center=-40.0), 4),          # h = 1 at layer 0: every token halts after one layer
}


def import_reference():
    """The reference's AdaptiveVisionTransformer, imported as oracle/make_golden.py imports the other classes."""
    if not os.path.isdir(MG.REF_ROOT):
        raise SystemExit("reference checkout not present: golden vectors can only be made in the build container")
    MG.import_reference()                        # symlink, sys.path, torchvision placeholders, purge of the repository's `peekvit`
    from peekvit.models.adavit import AdaptiveVisionTransformer
    src = os.path.realpath(inspect.getsourcefile(AdaptiveVisionTransformer))
    if not src.startswith(MG.REF_ROOT + "/"):
        raise SystemExit(f"resolved AdaptiveVisionTransformer to {src}, not the reference: refusing to write fixtures")
    return AdaptiveVisionTransformer


def run_case(cls, kw, batch, seed=0):
    cfg = {k: kw[k] for k in ("image_size", "patch_size", "num_layers", "num_heads", "hidden_dim", "mlp_dim", "num_classes")}
    cfg.update({k: kw[k] for k in ("num_class_tokens", "num_registers") if k in kw})
    torch.manual_seed(seed)
    model = cls(**kw).eval()
    sd = {k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(cfg, seed=seed).items()}
    model.load_state_dict(sd, strict=True)
    x = torch.from_numpy(synth.synth_images(batch, kw["image_size"], seed=seed, name="avit"))
    hs = []
    for blk in model.encoder.layers:
        orig = blk.forward_act

        def wrapped(*a, _orig=orig, **k):
            out, h = _orig(*a, **k)
            hs.append(h[1].detach().clone())
            return out, h
        blk.forward_act = wrapped
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        with torch.no_grad():
            logits = model(x)
    finally:
        torch.Tensor.cuda = cuda
    enc = model.encoder
    arrays = {"images": x.numpy(), "logits": logits.numpy(), "rho_token": enc.rho_token.numpy(), "counter_token": enc.counter_token.numpy(),
              "halting_score_layer": torch.stack(enc.halting_score_layer).numpy(), "h_token": torch.stack(hs).numpy()}
    keys = {k: list(v.shape) for k, v in model.state_dict().items()}
    return arrays, cfg, keys


def main():
    cls = import_reference()
    sig = inspect.signature(cls.__init__)
    defaults = {k: p.default for k, p in sig.parameters.items() if k != "self" and p.default is not inspect.Parameter.empty}
    meta = {"torch": torch.__version__, "reference_class": "models/adavit.py:AdaptiveVisionTransformer",
            "reference_sha256": {f: hashlib.sha256(open(os.path.join(MG.REF_ROOT, f), "rb").read()).hexdigest() for f in REF_FILES},
            "constructor_parameters": [k for k in sig.parameters if k != "self"], "constructor_defaults": defaults,
            "weights": "peekvit_amd.synth.synth_state_dict(cfg, seed=0); images: synth.synth_images(batch, image_size, seed=0, name='avit')",
            "cases": {}}
    for name, (kw, batch) in CASES.items():
        arrays, cfg, keys = run_case(cls, kw, batch)
        if arrays["images"].size > 100_000:
            del arrays["images"]                 # (224-pixel inputs: regenerated by synth.synth_images, recipe in the meta)
        np.savez_compressed(os.path.join(GOLD, name + ".npz"), **arrays)
        depth = arrays["counter_token"]
        meta["cases"][name] = {"kwargs": kw, "batch": batch, "synth_cfg": cfg, "state_dict": keys,
                               "mean_depth": float(depth.mean()), "depth_min": float(depth.min()), "depth_max": float(depth.max())}
        print(f"{name}: batch {batch}, mean depth {depth.mean():.2f} (min {depth.min():.0f}, max {depth.max():.0f}), "
              f"logits |max| {np.abs(arrays['logits']).max():.3g}")
    with open(os.path.join(GOLD, "avit_meta.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
