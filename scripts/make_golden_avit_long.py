"""Generate tests/golden/avit_long.npz + avit_long_meta.json by running the REAL reference A-ViT (models/adavit.py of the reference checkout,
oracle.make_golden.REF_ROOT) on CPU at more than 208 tokens per image.

Run in the build container only (the reference never travels to the GPU box):

    python scripts/make_golden_avit_long.py            # writes the fixtures
    python scripts/make_golden_avit_long.py --scan     # prints depth spread, longest segments and margins over a grid of gate_center values

The reference is imported as scripts/make_golden_avit.py imports it, and a case runs through that script's run_case: weights and images come from
peekvit_amd.synth (pure functions of name + the case's seed), so the fixture holds OUTPUTS only - logits, rho_token, counter_token, halting_score_layer
and the per-layer token halting scores h_token [L, B, S] - under the keys "<case>/<array>" of one archive.

Four cases on the micro dims (hidden 128, 2 heads, mlp 256, 4 layers, patch 8, 10 classes): 226, 257, 260 (the 257-token image with 2 class tokens
+ 2 registers) and 442 tokens.
gate_center is chosen per case so that the depths spread over 1 .. 4; the meta records the longest segment of packed rows behind every layer (one
case keeps it above 256 behind layer 0, another drops to 208 or fewer) and every token's smallest distance |c - (1 - eps)| over the layers it runs.
Before anything is written, the repository's composite in fp64 must reproduce the reference's counter_token on every image of every case: a case
that does not gets another gate_center here, never a weaker test."""
from __future__ import annotations

import hashlib
import inspect
import json
import os
import sys

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

import numpy as np
import torch

from peekvit_amd import synth
from oracle import make_golden as MG
import make_golden_avit as GA

GOLD = os.path.join(REPO, "tests", "golden")
_DIMS = dict(patch_size=8, num_layers=4, num_heads=2, hidden_dim=128, mlp_dim=256, num_classes=10)

# name -> (model kwargs, batch, synth seed).  gate_center and seed: of a grid of gate_center 0.5 .. 8 in steps of 0.25 and seeds 0 .. 3 (--scan), the
# pair whose third-largest per-image margin in the REFERENCE's own run is the largest - three of four images keep every token at least 1e-3 (442
# tokens) / 1.5e-3 (226, 257, 260) from the threshold.  Nothing of the code under test enters the choice.
CASES = {
    "avit_long_226": (dict(_DIMS, image_size=120, gate_center=1.25), 4, 0),
    "avit_long_257": (dict(_DIMS, image_size=128, gate_center=0.5), 4, 3),
    "avit_long_260": (dict(_DIMS, image_size=128, num_class_tokens=2, num_registers=2, gate_center=0.5), 4, 2),
    "avit_long_442": (dict(_DIMS, image_size=168, gate_center=6.75), 4, 1),
}
ARRAYS = ("logits", "rho_token", "counter_token", "halting_score_layer", "h_token")


def margins(h_token: np.ndarray, eps: float = 0.01) -> np.ndarray:
    """Smallest |c - (1 - eps)| over the layers each token runs (tests/test_hip_avit.py's _margins), [B, S]."""
    thr = np.float32(torch.tensor(1 - eps, dtype=torch.float32).item())
    L, B, S = h_token.shape
    c, live, mm = np.zeros((B, S), np.float32), np.ones((B, S), bool), np.full((B, S), np.inf)
    for l in range(L - 1):
        c = np.where(live, c + h_token[l], c)
        mm = np.where(live, np.minimum(mm, np.abs(c - thr)), mm)
        live &= c < thr
    return mm


def longest_segments(counter: np.ndarray) -> list:
    """Rows of the longest packed segment that ENTERS layer 1, 2, ..: the tokens still running (counter_token > layer) plus one representative row
    when any token of the image has halted."""
    L = int(counter.max())
    S = counter.shape[1]
    out = []
    for l in range(1, L):
        live = (counter > l).sum(axis=1)
        out.append(int((live + (live < S)).max()))
    return out


def composite_fp64(kw: dict, cfg: dict, batch: int, seed: int):
    """The repository's stock-op composite of the same model in fp64 on the CPU: (counter_token, logits)."""
    from peekvit_amd.models.adavit import AdaptiveVisionTransformer
    model = AdaptiveVisionTransformer(**kw).eval()
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(cfg, seed=seed).items()}, strict=True)
    model = model.double()
    x = torch.from_numpy(synth.synth_images(batch, kw["image_size"], seed=seed, name="avit")).double()
    with torch.no_grad():
        logits = model._composite_forward(x)
    return model.encoder.counter_token.numpy(), logits.numpy()


def describe(arrays: dict) -> dict:
    depth, mm = arrays["counter_token"], margins(arrays["h_token"])
    return {"mean_depth": float(depth.mean()), "depth_histogram": [int((depth == d).sum()) for d in range(1, int(depth.max()) + 1)],
            "longest_segment_into_layer": longest_segments(depth), "min_margin_per_image": [float(v) for v in mm.min(axis=1)],
            "tokens_within_2e-3": int((mm < 2e-3).sum())}


def scan(cls):
    for name, (kw, batch, _) in CASES.items():
        for seed in range(4):
            for gc in np.arange(0.5, 8.01, 0.25):
                arrays, _, _ = GA.run_case(cls, dict(kw, gate_center=float(gc)), batch, seed=seed)
                print(name, "seed", seed, "gate_center", float(gc), json.dumps(describe(arrays)))


def main():
    cls = GA.import_reference()
    if "--scan" in sys.argv:
        return scan(cls)
    sig = inspect.signature(cls.__init__)
    meta = {"torch": torch.__version__, "reference_class": "models/adavit.py:AdaptiveVisionTransformer",
            "reference_sha256": {f: hashlib.sha256(open(os.path.join(MG.REF_ROOT, f), "rb").read()).hexdigest() for f in GA.REF_FILES},
            "reference_files": list(GA.REF_FILES), "constructor_parameters": [k for k in sig.parameters if k != "self"],
            "weights": "peekvit_amd.synth.synth_state_dict(cfg, seed=seed); images: synth.synth_images(batch, image_size, seed=seed, name='avit')",
            "arrays": list(ARRAYS), "cases": {}}
    out = {}
    for name, (kw, batch, seed) in CASES.items():
        arrays, cfg, keys = GA.run_case(cls, kw, batch, seed=seed)
        d = describe(arrays)
        depth = arrays["counter_token"]
        assert set(np.unique(depth)) == {1.0, 2.0, 3.0, 4.0}, (name, np.unique(depth))          # the depths spread over 1 .. 4
        cnt64, lg64 = composite_fp64(kw, cfg, batch, seed)
        assert (cnt64 == depth).all(), f"{name}: the fp64 composite decides {(cnt64 != depth).sum()} tokens differently from the reference"
        d["fp64_composite_logits_rel_l2"] = float(np.linalg.norm(lg64 - arrays["logits"]) / np.linalg.norm(arrays["logits"]))
        for k in ARRAYS:
            out[f"{name}/{k}"] = arrays[k]
        out[f"{name}/margin"] = margins(arrays["h_token"]).astype(np.float32)
        meta["cases"][name] = dict(d, kwargs=kw, batch=batch, seed=seed, synth_cfg=cfg, state_dict=keys, tokens=int(depth.shape[1]))
        print(name, json.dumps(d))
    longest = [c["longest_segment_into_layer"] for c in meta["cases"].values()]
    assert any(l[0] > 256 for l in longest), "no case keeps a segment above 256 rows behind layer 0"
    assert any(min(l) <= 208 for l in longest), "no case drops to 208 rows or fewer"
    np.savez_compressed(os.path.join(GOLD, "avit_long.npz"), **out)
    with open(os.path.join(GOLD, "avit_long_meta.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
