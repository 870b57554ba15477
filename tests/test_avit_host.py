"""A-ViT (reference models/adavit.py) without a GPU: the module surface against the reference's constructor and state-dict keys, the stock-op
composite against the reference's golden outputs (scripts/make_golden_avit.py), the ponder loss's gradient, and the argument checks of the two
packed-halting C entry points (include/peekvit_hip.h pv_attention_varlen_bf16, pv_act_step)."""
import ctypes as C
import importlib
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
from peekvit_amd import synth

META = json.load(open(os.path.join(GOLDEN, "avit_meta.json")))
CASES = sorted(META["cases"])


def _model(name):
    from peekvit_amd.models.adavit import AdaptiveVisionTransformer
    case = META["cases"][name]
    model = AdaptiveVisionTransformer(**case["kwargs"]).eval()
    sd = {k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(case["synth_cfg"], seed=0).items()}
    model.load_state_dict(sd, strict=True)
    return model


def _images(name, g):
    case = META["cases"][name]
    if "images" in g:
        return torch.from_numpy(g["images"])
    return torch.from_numpy(synth.synth_images(case["batch"], case["kwargs"]["image_size"], seed=0, name="avit"))


def test_target_resolves_and_surface_matches_reference():
    mod = importlib.import_module("peekvit.models.adavit")
    cls = mod.AdaptiveVisionTransformer
    from peekvit_amd.models.adavit import AdaptiveVisionTransformer, AViTBlock, AViTEncoder
    assert cls is AdaptiveVisionTransformer and mod.AViTBlock is AViTBlock and mod.AViTEncoder is AViTEncoder
    sig = inspect.signature(cls.__init__)
    assert [k for k in sig.parameters if k != "self"] == META["constructor_parameters"]
    defaults = {k: p.default for k, p in sig.parameters.items() if k != "self" and p.default is not inspect.Parameter.empty}
    assert defaults == META["constructor_defaults"]
    for name in CASES:
        m = cls(**META["cases"][name]["kwargs"])
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == META["cases"][name]["state_dict"], name
        assert float(m.head.weight.abs().sum()) == 0.0 and float(m.head.bias.abs().sum()) == 0.0


def test_harness_configs_instantiate():
    from peekvit_amd.harness import config
    for name, gc in (("avit_t_16_224", 5), ("avit_s_16_224", 30)):
        cfg = config.load_config("test_config", [f"model={name}", "dataset.num_classes=10"])
        m = cfg["model"]
        assert m["_target_"] == "peekvit.models.adavit.AdaptiveVisionTransformer" and m["gate_center"] == gc and m["timm_pretrained_weights"] is None


@pytest.mark.parametrize("name", CASES)
def test_composite_matches_reference_golden(name, golden):
    g = golden(name)
    model = _model(name)
    with torch.no_grad():
        logits = model(_images(name, g))
    enc = model.encoder
    np.testing.assert_allclose(logits.numpy(), g["logits"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(enc.counter_token.numpy(), g["counter_token"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(enc.rho_token.numpy(), g["rho_token"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(torch.stack(enc.halting_score_layer).numpy(), g["halting_score_layer"], rtol=0, atol=1e-5)
    assert len(enc.halting_score_layer) == META["cases"][name]["kwargs"]["num_layers"]


def test_all_halt_case_runs_one_layer_and_batch_one_score_is_nan():
    g = np.load(os.path.join(GOLDEN, "avit_allhalt.npz"))
    assert (g["counter_token"] == 1).all()
    model = _model("avit_micro")
    with torch.no_grad():
        model(torch.from_numpy(g["images"][:1]))
    assert all(torch.isnan(s) for s in model.encoder.halting_score_layer)       # mean over images 1.. of a batch of one (the reference's slice)
    assert model.encoder.rho_token.shape == (1, model.seq_length)                # state re-made for the new batch size


def test_ponder_loss_backpropagates_into_the_blocks():
    model = _model("avit_micro").train()
    g = np.load(os.path.join(GOLDEN, "avit_micro.npz"))
    x = torch.from_numpy(g["images"])
    logits = model(x)
    loss = model.encoder.rho_token.mean() + logits.pow(2).mean()
    loss.backward()
    for i, blk in enumerate(model.encoder.layers):
        grads = [p.grad for p in blk.parameters()]
        assert all(gr is not None and torch.isfinite(gr).all() for gr in grads), i
        assert sum(float(gr.abs().sum()) for gr in grads) > 0, f"layer {i}: no gradient from the ponder loss"
    # the ponder term alone reaches the halting gate's input (channel 0 of every block output)
    model.zero_grad()
    model(x)
    model.encoder.rho_token.mean().backward()
    assert float(model.encoder.layers[0].mlp.fc2.bias.grad[0].abs()) > 0


def _header_arity(name):
    header = open(os.path.join(REPO, "include", "peekvit_hip.h")).read()
    m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_new_entry_points_are_exported_declared_and_validate_arguments():
    from peekvit_amd import _lib
    lib = _lib.load()
    for name in ("pv_attention_varlen_bf16", "pv_act_step"):
        assert name in _lib.SIGNATURES and _header_arity(name) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(_lib.load("f16"), name)
    p = C.c_void_p(256)                 # never dereferenced: every call below is refused before anything is launched
    null = C.c_void_p(0)
    att = lambda qkv, seg, nh, B, max_len, H, dh: lib.pv_attention_varlen_bf16(qkv, p, seg, nh, B, max_len, H, dh, null, null)
    assert att(p, p, p, 4, 209, 3, 64) == -2                    # longer than the tile bound
    assert att(p, p, p, 4, 197, 6, 48) == -2                    # dh != 64
    assert att(p, p, p, 4, 197, 3, 32) == -2
    assert att(p, null, p, 4, 197, 3, 64) == -1                 # null segment table
    assert att(p, p, null, 4, 197, 3, 64) == -1                 # null multiplicities
    assert att(null, p, p, 4, 197, 3, 64) == -1
    assert att(p, p, p, 0, 197, 3, 64) == -1 and att(p, p, p, 4, 0, 3, 64) == -1

    def act(B=4, S=197, D=192, nc=1, last=0, nxt=True, y=p, seg=p, pos=p):
        n = p if nxt else null
        return lib.pv_act_step(y, seg, p, pos, B, S, D, p, p, p, p, p, p, nc, p, 10.0, 5.0, 0.99, last, n, n, n, n, n, n, null)
    assert act(seg=null) == -1 and act(pos=null) == -1 and act(y=null) == -1
    assert act(nxt=False) == -1                                 # the next tables are required unless it is the last layer
    assert act(B=0) == -1 and act(nc=0) == -1 and act(nc=198) == -1
    assert act(S=257) == -2 and act(nc=17, S=200) == -2 and act(D=190) == -2
