"""Generate tests/golden/ee_*.npz + ee_meta.json by running the REAL reference EEResidualVisionTransformer (models/eeresidualvit.py) on CPU.

Run in the build container only (the reference never travels to the GPU box):

    python scripts/make_golden_ee.py

The reference is imported through oracle.make_golden.import_reference (a symlink named `peekvit` on sys.path, the repository's own `peekvit`
package taken off it, torchvision replaced by placeholders); a class that does not resolve to a file under the reference checkout is refused.

Weights come from peekvit_amd.synth.ee_state_dict and images from synth.ee_images (pure functions of name + seed, bf16-representable), so
a fixture holds the OUTPUTS: the full list [exit_0 .. exit_{L-1}, final] (out_0 .. out_L, with the reference's shapes), every block's mask,
the max softmax of every list element (fp64), and for two thresholds the exit layer of every image, by an fp64 restatement of select_exits
written here in numpy over the reference's list.

FIXTURE CONDITION.  An exit decision is a comparison; a confidence that sits on the threshold can flip under 16-bit operands.  The tests
exclude no image - the inputs are chosen instead: from a pool of synthetic images the first run of B is kept among those whose confidence at EVERY layer is at
least m away from BOTH thresholds, m = max(0.02, 4 * 0.5 * 1e-3 * max ||outs[i][b]||_2 over the pool): four times what BASELINE's 1e-3
relative-L2 logit tolerance can move a softmax probability (|dp| <= p (1 - p) * 2 ||dz||_inf <= 0.5 ||dz||_2).  Cases of three or more
images must exit at three or more distinct layers, "final" among them, at each threshold.  Both conditions are asserted; m, the thresholds,
the pool indices kept and the exit histograms go into the meta.
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
REF_FILES = ("models/eeresidualvit.py", "models/residualvit.py", "models/blocks.py", "configs/model/eeresidualvit.yaml")

_GATED = dict(gate_type="sigmoid", gate_temp=1, gate_bias=1, gate_threshold=0.5, add_input=False)
_MICRO = dict(image_size=32, patch_size=8, num_layers=4, num_heads=2, hidden_dim=128, mlp_dim=256, num_classes=10,
              residual_layers=["attention+mlp"] * 4, add_budget_token="learnable", **_GATED)
# configs/model/eeresidualvit.yaml on imagenette (160 px, 10 classes), dropout 0
_YAML = dict(image_size=160, patch_size=8, num_layers=4, num_heads=4, hidden_dim=256, mlp_dim=768, num_classes=10, dropout=0.0,
             attention_dropout=0.0, residual_layers=["attention+mlp"] * 4, add_budget_token="learnable", **_GATED)
_S224 = dict(image_size=224, patch_size=16, num_layers=12, num_heads=6, hidden_dim=384, mlp_dim=1536, num_classes=10,
             residual_layers=["attention+mlp"] * 12, add_budget_token="learnable", **_GATED)

# name -> (model kwargs, batch, pool, budget, thresholds, train)
CASES = {
    "ee_micro": (_MICRO, 8, 128, 0.7, (0.4, 0.55), False),
    "ee_yaml160": (_YAML, 4, 32, 0.7, (0.5, 0.7), False),
    "ee_s224": (_S224, 6, 32, 0.7, (0.8, 0.9), False),
    "ee_batch1": (_MICRO, 1, 16, 0.7, (0.4, 0.55), False),
    "ee_2cls1reg": (dict(_MICRO, num_class_tokens=2, num_registers=1), 6, 128, 0.7, (0.4, 0.55), False),
    # train mode: dropout 0 and a float add_budget_token, so that no RNG enters
    "ee_train": (dict(_MICRO, add_budget_token=0.7), 4, 64, None, (0.5, 0.7), True),
}
GRAD_KEYS = ("class_tokens", "conv_proj.bias", "encoder.ln.weight", "head.weight", "head.bias")
GRAD_SUFFIXES = ("residual_gate.projection.weight", "ln_1.weight")


def import_reference():
    MG.import_reference()
    from peekvit.models.eeresidualvit import EEResidualVisionTransformer
    from peekvit.models.residualvit import ResidualViTBlock
    for cls in (EEResidualVisionTransformer, ResidualViTBlock):
        src = os.path.realpath(inspect.getsourcefile(cls))
        if not src.startswith(MG.REF_ROOT + "/"):
            raise SystemExit(f"resolved {cls.__name__} to {src}, not the reference: refusing to write fixtures")
    return EEResidualVisionTransformer


def synth_cfg(kw):
    keys = ("image_size", "patch_size", "num_layers", "num_heads", "hidden_dim", "mlp_dim", "num_classes", "residual_layers",
            "add_budget_token", "num_class_tokens", "num_registers")
    return {k: kw[k] for k in keys if k in kw}


def max_softmax64(z):
    z = np.asarray(z, dtype=np.float64)
    z = z - z.max(axis=-1, keepdims=True)
    e = np.exp(z)
    return (e / e.sum(axis=-1, keepdims=True)).max(axis=-1)


def select_exits64(outs, threshold):
    """outs [L + 1, B, C] -> exit layer per image: the first i < L with max softmax >= threshold, else L."""
    L, B = outs.shape[0] - 1, outs.shape[1]
    layer = np.full(B, L, dtype=np.int64)
    for i in range(L - 1, -1, -1):
        layer[max_softmax64(outs[i]) >= threshold] = i
    return layer


def run_case(cls, kw, batch, pool, budget, thresholds, train, seed=0):
    cfg = synth_cfg(kw)
    torch.manual_seed(seed)
    model = cls(**kw)
    sd = {k: torch.from_numpy(v.copy()) for k, v in synth.ee_state_dict(cfg, seed).items()}
    model.load_state_dict(sd, strict=True)
    model.train(train)
    if budget is not None:
        model.set_budget(budget)
    L, C = kw["num_layers"], kw["num_classes"]
    imgs = torch.from_numpy(synth.ee_images(pool, kw["image_size"], seed=seed))
    with torch.no_grad():
        pooled = model(imgs)
    po = np.stack([o.reshape(pool, C).numpy() for o in pooled])                 # [L + 1, pool, C]
    conf = max_softmax64(po)                                                   # [L + 1, pool]
    m = max(0.02, 4 * 0.5 * 1e-3 * float(np.sqrt((po.astype(np.float64) ** 2).sum(-1)).max()))
    ok = np.ones(pool, dtype=bool)
    for t in thresholds:
        ok &= (np.abs(conf[:L] - t) >= m).all(axis=0)
    elig = np.nonzero(ok)[0]
    assert len(elig) >= batch, f"only {int(ok.sum())} of {pool} pool images are {m:.3g} away from {thresholds} at every layer"
    idx = None
    for s in range(len(elig) - batch + 1):           # the first run of B eligible images that also meets the histogram condition
        cand = elig[s:s + batch]
        hists = [set(select_exits64(po[:, cand], t).tolist()) for t in thresholds]
        if batch < 3 or all(len(h) >= 3 and L in h for h in hists):
            idx = cand
            break
    assert idx is not None, f"no run of {batch} eligible images exits at three layers including the final head at {thresholds}"
    x = imgs[idx].clone()
    y = torch.tensor([(7 * int(i) + 3) % C for i in idx])
    arrays = {"images": x.numpy(), "pool_index": idx.astype(np.int64), "labels": y.numpy()}
    if train:
        outs = model(x)
        loss = sum(torch.nn.functional.cross_entropy(o.reshape(batch, C), y) for o in outs)
        loss.backward()
        arrays["loss"] = np.float32(loss.item())
        grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
        for k, g in grads.items():
            if k in GRAD_KEYS or k.endswith(GRAD_SUFFIXES) or k.startswith("encoder.early_exit_heads."):
                arrays["grad/" + k] = g.numpy()
        outs = [o.detach() for o in outs]
    else:
        with torch.no_grad():
            outs = model(x)
    assert isinstance(outs, list) and len(outs) == L + 1
    for i, o in enumerate(outs):
        arrays[f"out_{i}"] = o.numpy()
    for i, blk in enumerate(model.encoder.layers):
        arrays[f"mask_{i}"] = blk.mask.detach().numpy()
    stacked = np.stack([o.reshape(batch, C).numpy() for o in outs])
    arrays["conf"] = max_softmax64(stacked)
    hist = {}
    for t in thresholds:
        layer = select_exits64(stacked, t)
        arrays[f"exit_layer_{t}"] = layer
        hist[str(t)] = {int(k): int(v) for k, v in zip(*np.unique(layer, return_counts=True))}
        assert (np.abs(arrays["conf"][:L] - t) >= m).all()
        if batch >= 3:
            assert len(hist[str(t)]) >= 3 and L in hist[str(t)], f"threshold {t}: exit histogram {hist[str(t)]}"
    keys = {k: list(v.shape) for k, v in model.state_dict().items()}
    info = {"kwargs": kw, "batch": batch, "pool": pool, "budget": budget, "train": train, "thresholds": list(thresholds), "margin": m,
            "synth_cfg": cfg, "state_dict": keys, "exit_histogram": hist, "out_shapes": [list(o.shape) for o in outs],
            "block_special_tokens": [int(b.num_special_tokens) for b in model.encoder.layers],
            "mask_zero_fraction": [float((arrays[f"mask_{i}"] == 0).mean()) for i in range(L)]}
    return arrays, info


def main():
    cls = import_reference()
    sig = inspect.signature(cls.__init__)
    defaults = {k: p.default for k, p in sig.parameters.items() if k != "self" and p.default is not inspect.Parameter.empty}
    meta = {"torch": torch.__version__, "reference_class": "models/eeresidualvit.py:EEResidualVisionTransformer",
            "reference_sha256": {f: hashlib.sha256(open(os.path.join(MG.REF_ROOT, f), "rb").read()).hexdigest() for f in REF_FILES},
            "constructor_parameters": [k for k in sig.parameters if k != "self"], "constructor_defaults": defaults,
            "weights": "peekvit_amd.synth.ee_state_dict(synth_cfg, seed=0); images: synth.ee_images(pool, image_size, seed=0)"
                       "[pool_index]; labels (7 * pool_index + 3) % classes",
            "cases": {}}
    for name, (kw, batch, pool, budget, thresholds, train) in CASES.items():
        arrays, info = run_case(cls, kw, batch, pool, budget, thresholds, train)
        if arrays["images"].size > 100_000:
            del arrays["images"]                 # (large inputs: regenerated by synth.ee_images + pool_index, recipe in the meta)
        np.savez_compressed(os.path.join(GOLD, name + ".npz"), **arrays)
        meta["cases"][name] = info
        print(f"{name}: batch {batch}, margin {info['margin']:.3g}, exits {info['exit_histogram']}, conf {arrays['conf'].min():.3f} .. "
              f"{arrays['conf'].max():.3f}, zero mask fraction {['%.2f' % z for z in info['mask_zero_fraction']]}, "
              f"{os.path.getsize(os.path.join(GOLD, name + '.npz'))} bytes")
    with open(os.path.join(GOLD, "ee_meta.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
