"""Generate tests/golden/moe_*.npz + moe_meta.json by running the REAL reference VisionTransformerMoE (/root/reference/models/moevit.py) on CPU.

Run in the build container only (the reference never travels to the GPU box):

    python scripts/make_golden_moe.py

The reference is imported exactly as oracle/make_golden.py does it (a /tmp symlink named `peekvit` on sys.path, the repository's own `peekvit`
package taken off it, torchvision replaced by placeholders); a class that does not resolve to a file under the reference checkout is refused.

Weights come from peekvit_amd.synth.moe_state_dict and images from synth.synth_images (pure functions of name + seed, bf16-representable), so
a fixture holds the OUTPUTS: logits, every MoE module's gating_probs [B, S, E] (module names in the meta), and every MoE module's gate logits
[B, S, E] (a forward hook on gating_network.gate), from which a test knows each token's top-1 / top-2 gap.
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
REF_FILES = ("models/moevit.py", "models/blocks.py", "configs/model/moevit.yaml")

_MICRO = dict(image_size=32, patch_size=8, num_layers=4, num_heads=2, hidden_dim=128, mlp_dim=256, num_classes=10)
_S224 = dict(image_size=224, patch_size=16, num_layers=12, num_heads=6, hidden_dim=384, mlp_dim=1536, num_classes=10)
_YAML = dict(image_size=160, patch_size=8, num_layers=4, num_heads=4, hidden_dim=256, mlp_dim=768, num_classes=10)   # configs/model/moevit.yaml dims

# name -> (model kwargs, batch, dominant expert or None)
CASES = {
    "moe_micro": (dict(_MICRO, mlp_moes=[1, 4, 2, 1], attn_moes=[1, 1, 3, 1]), 4, None),
    "moe_s224": (dict(_S224, mlp_moes=[1, 8] * 6), 2, None),
    "moe_yaml160": (dict(_YAML, mlp_moes=[2, 1, 4, 1], attn_moes=[1, 2, 1, 1]), 2, None),          # 401 tokens
    "moe_onehot": (dict(_MICRO, mlp_moes=[1, 4, 4, 1], attn_moes=[1, 3, 1, 1]), 4, 1),             # expert 1 takes every token
}


def import_reference():
    """The reference's VisionTransformerMoE and MoE base class, imported as oracle/make_golden.py imports the other classes."""
    if not os.path.isdir(MG.REF_ROOT):
        raise SystemExit("reference checkout not present: golden vectors can only be made in the build container")
    MG.import_reference()
    from peekvit.models.moevit import MoE, VisionTransformerMoE
    for cls in (MoE, VisionTransformerMoE):
        src = os.path.realpath(inspect.getsourcefile(cls))
        if not src.startswith(MG.REF_ROOT + "/"):
            raise SystemExit(f"resolved {cls.__name__} to {src}, not the reference: refusing to write fixtures")
    return VisionTransformerMoE, MoE


def synth_cfg(kw):
    return {k: kw[k] for k in ("image_size", "patch_size", "num_layers", "num_heads", "hidden_dim", "mlp_dim", "num_classes")}


def run_case(cls, moe_cls, kw, batch, dominant, seed=0):
    cfg = synth_cfg(kw)
    torch.manual_seed(seed)
    model = cls(**kw).eval()
    sd = {k: torch.from_numpy(v.copy()) for k, v in synth.moe_state_dict(cfg, kw.get("mlp_moes"), kw.get("attn_moes"), seed, dominant).items()}
    model.load_state_dict(sd, strict=True)
    x = torch.from_numpy(synth.synth_images(batch, kw["image_size"], seed=seed, name="moe"))
    moes = [(n, m) for n, m in model.named_modules() if isinstance(m, moe_cls) and m.num_experts > 1]     # utils/utils.py get_moes
    gate_logits = {}
    hooks = [m.gating_network.gate.register_forward_hook(lambda mod, i, o, n=n: gate_logits.__setitem__(n, o.detach().clone())) for n, m in moes]
    with torch.no_grad():
        logits = model(x)
    for h in hooks:
        h.remove()
    arrays = {"images": x.numpy(), "logits": logits.numpy()}
    for j, (n, m) in enumerate(moes):
        arrays[f"gating_probs_{j}"] = m.gating_probs.numpy()
        arrays[f"gate_logits_{j}"] = gate_logits[n].numpy()
    keys = {k: list(v.shape) for k, v in model.state_dict().items()}
    return arrays, cfg, keys, [n for n, _ in moes]


def main():
    cls, moe_cls = import_reference()
    sig = inspect.signature(cls.__init__)
    defaults = {k: p.default for k, p in sig.parameters.items() if k != "self" and p.default is not inspect.Parameter.empty}
    meta = {"torch": torch.__version__, "reference_class": "models/moevit.py:VisionTransformerMoE",
            "reference_sha256": {f: hashlib.sha256(open(os.path.join(MG.REF_ROOT, f), "rb").read()).hexdigest() for f in REF_FILES},
            "constructor_parameters": [k for k in sig.parameters if k != "self"], "constructor_defaults": defaults,
            "weights": "peekvit_amd.synth.moe_state_dict(cfg, mlp_moes, attn_moes, seed=0, dominant); "
                       "images: synth.synth_images(batch, image_size, seed=0, name='moe')",
            "cases": {}}
    for name, (kw, batch, dominant) in CASES.items():
        arrays, cfg, keys, moe_names = run_case(cls, moe_cls, kw, batch, dominant)
        if arrays["images"].size > 100_000:
            del arrays["images"]                 # (large inputs: regenerated by synth.synth_images, recipe in the meta)
        np.savez_compressed(os.path.join(GOLD, name + ".npz"), **arrays)
        gaps = []
        for j in range(len(moe_names)):
            s = np.sort(arrays[f"gate_logits_{j}"], axis=-1)
            gaps.append(float((s[..., -1] - s[..., -2]).min()))
        meta["cases"][name] = {"kwargs": kw, "batch": batch, "dominant": dominant, "synth_cfg": cfg, "state_dict": keys, "moes": moe_names,
                               "min_gate_gap": gaps}
        print(f"{name}: batch {batch}, {len(moe_names)} MoE modules, min top-1/top-2 gate gap {min(gaps):.3g}, "
              f"logits |max| {np.abs(arrays['logits']).max():.3g}")
    with open(os.path.join(GOLD, "moe_meta.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
