"""VisionTransformerMoE (reference models/moevit.py) without a GPU: the Hydra targets, the module surface against the reference's constructor and
state-dict keys (tests/golden/moe_meta.json), the stock-op composite against the reference's golden outputs (scripts/make_golden_moe.py), the
reference's get_moes / get_last_forward_gates walk, training through the composite, the harness config, a test ledger for
include/peekvit_hip_moe.h and the argument checks of its entry points."""
import ast
import ctypes as C
import importlib
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, rel_l2
from peekvit_amd import synth

META = json.load(open(os.path.join(GOLDEN, "moe_meta.json")))
CASES = sorted(META["cases"])


def _model(name):
    from peekvit_amd.models.moevit import VisionTransformerMoE
    case = META["cases"][name]
    kw = case["kwargs"]
    model = VisionTransformerMoE(**kw).eval()
    sd = synth.moe_state_dict(case["synth_cfg"], kw.get("mlp_moes"), kw.get("attn_moes"), seed=0, dominant=case["dominant"])
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return model


def _images(name, g):
    case = META["cases"][name]
    if "images" in g:
        return torch.from_numpy(g["images"])
    return torch.from_numpy(synth.synth_images(case["batch"], case["kwargs"]["image_size"], seed=0, name="moe"))


def get_moes(model):
    """utils/utils.py:61-78 of the reference, restated."""
    from peekvit.models.moevit import MoE
    return {n: m for n, m in model.named_modules() if isinstance(m, MoE) and m.num_experts > 1}


def get_last_forward_gates(model):
    """utils/utils.py:81-94 of the reference, restated."""
    from peekvit.models.moevit import MoE
    return {n: m.gating_probs for n, m in model.named_modules() if isinstance(m, MoE) and m.num_experts > 1}


def test_hydra_targets_resolve():
    from peekvit_amd.harness import config
    from peekvit_amd.models.moevit import VisionTransformerMoE
    mod = importlib.import_module("peekvit.models.moevit")
    assert mod.VisionTransformerMoE is VisionTransformerMoE and mod.MoEVisionTransformer is VisionTransformerMoE
    kw = dict(image_size=32, patch_size=8, num_layers=2, num_heads=2, hidden_dim=128, mlp_dim=256, num_classes=10, mlp_moes=[1, 3])
    for target in ("peekvit.models.moevit.VisionTransformerMoE", "peekvit.models.moevit.MoEVisionTransformer"):   # (the latter: the reference's yaml)
        m = config.instantiate({"_target_": target, **kw})
        assert isinstance(m, VisionTransformerMoE) and m.encoder.layers[1].mlp.num_experts == 3


def test_surface_matches_reference():
    mod = importlib.import_module("peekvit.models.moevit")
    for name in ("MoE", "TopKGate", "MLPMoE", "AttentionMoE", "ViTBlockMoE", "ViTEncoderMoE", "VisionTransformerMoE"):
        assert inspect.isclass(getattr(mod, name)), name
    assert issubclass(mod.MLPMoE, mod.MoE) and issubclass(mod.AttentionMoE, mod.MoE)
    cls = mod.VisionTransformerMoE
    sig = inspect.signature(cls.__init__)
    assert [k for k in sig.parameters if k != "self"] == META["constructor_parameters"]
    defaults = {k: p.default for k, p in sig.parameters.items() if k != "self" and p.default is not inspect.Parameter.empty}
    assert defaults == META["constructor_defaults"]
    for name in CASES:
        m = cls(**META["cases"][name]["kwargs"])
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == META["cases"][name]["state_dict"], name
        assert float(m.head.weight.abs().sum()) == 0.0 and float(m.head.bias.abs().sum()) == 0.0
        assert m.mlp_moes == (META["cases"][name]["kwargs"].get("mlp_moes") or [1] * m.num_layers)


def test_get_moes_and_last_forward_gates_walk():
    model = _model("moe_micro")
    names = META["cases"]["moe_micro"]["moes"]
    assert list(get_moes(model)) == names and [n for n, _ in zip(names, model.moes())] == names
    with torch.no_grad():
        model(torch.from_numpy(synth.synth_images(2, 32, seed=3, name="moe")))
    gates = get_last_forward_gates(model)
    assert list(gates) == names
    for n, g in gates.items():
        E = get_moes(model)[n].num_experts
        assert g.shape == (2, 17, E) and g.dtype == torch.float32
        assert torch.equal(g.sum(-1), torch.ones(2, 17)) and bool(((g == 0) | (g == 1)).all())
    # one-expert halves are plain modules: no gating_probs attribute, as in the reference (forward_one)
    assert not hasattr(model.encoder.layers[0].mlp, "gating_probs")


@pytest.mark.parametrize("name", CASES)
def test_composite_matches_reference_golden(name, golden):
    g = golden(name)
    model = _model(name)
    with torch.no_grad():
        logits = model(_images(name, g))
    assert rel_l2(logits, g["logits"]) < 1e-3
    np.testing.assert_allclose(logits.numpy(), g["logits"], rtol=0, atol=1e-5)
    moes = model.moes()
    assert len(moes) == len(META["cases"][name]["moes"])
    for j, m in enumerate(moes):
        assert np.array_equal(m.gating_probs.numpy(), g[f"gating_probs_{j}"]), (name, j)
        assert np.array_equal(g[f"gating_probs_{j}"].argmax(-1), g[f"gate_logits_{j}"].argmax(-1))
    if META["cases"][name]["dominant"] is not None:
        d = META["cases"][name]["dominant"]
        assert all(bool((m.gating_probs.argmax(-1) == d).all()) for m in moes)


def test_training_through_the_composite_reaches_experts_and_gates():
    torch.manual_seed(0)
    model = _model("moe_micro").train()
    x = torch.from_numpy(synth.synth_images(4, 32, seed=1, name="moe"))
    loss = torch.nn.functional.cross_entropy(model(x), torch.arange(4) % 10)
    loss.backward()
    blk = model.encoder.layers[1]
    assert float(blk.mlp.gating_network.gate.weight.grad.abs().sum()) > 0          # straight-through Gumbel softmax
    assert any(float(e.fc1.weight.grad.abs().sum()) > 0 for e in blk.mlp.experts)
    g = blk.mlp.gating_probs
    assert g.requires_grad and torch.allclose(g.detach().sum(-1), torch.ones(4, 17))


def test_harness_config_builds_the_model():
    from peekvit_amd.harness import config
    from peekvit_amd.models.moevit import VisionTransformerMoE
    cfg = config.load_config("test_config", ["model=moevit", "dataset.num_classes=10", "dataset.image_size=160"])
    m = cfg["model"]
    assert m["_target_"] == "peekvit.models.moevit.VisionTransformerMoE" and m["mlp_moes"] is None and m["attn_moes"] is None
    model = config.instantiate(m)
    assert isinstance(model, VisionTransformerMoE) and model.patch_size == 8 and model.seq_length == 401 and not model.moes()


# ---- include/peekvit_hip_moe.h: every declared entry point has a test that calls it directly ----
LEDGER = {
    "pv_moe_packed_rows": ["test_moe_host.py::test_packed_rows_and_scratch_size"],
    "pv_moe_route_scratch_size": ["test_moe_host.py::test_packed_rows_and_scratch_size"],
    "pv_moe_route": ["test_hip_moe.py::test_route_against_fp64", "test_hip_moe.py::test_route_exact_tie_and_single_expert",
                     "test_hip_moe.py::test_route_strided_input_is_bit_identical_to_contiguous"],
    "pv_gemm_grouped_bf16": ["test_hip_moe.py::test_grouped_gemm_against_fp64_and_sentinels",
                             "test_hip_moe.py::test_grouped_gemm_bit_identical_to_per_expert_gemm"],
    "pv_moe_gather_bf16": ["test_hip_moe.py::test_gather_exact", "test_hip_moe.py::test_gather_from_padded_planes_and_past_one_grid_sweep"],
}


def _declared():
    src = open(os.path.join(REPO, "include", "peekvit_hip_moe.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pv_\w+)\s*\(", src, flags=re.M))


def test_moe_ledger_names_a_direct_test_for_every_declared_entry_point():
    from peekvit_amd import _lib
    declared = _declared()
    assert set(LEDGER) == declared == set(_lib.SIGNATURES_MOE), declared ^ set(LEDGER)
    ops_src = open(os.path.join(REPO, "peekvit_amd", "ops.py")).read()
    wrappers = {}
    for node in ast.parse(ops_src).body:
        if isinstance(node, ast.FunctionDef):
            for sym in re.findall(r"\b(pv_\w+)\(", ast.get_source_segment(ops_src, node)):
                wrappers.setdefault(sym, set()).add(node.name)
    for entry, ids in LEDGER.items():
        for tid in ids:
            fname, _, name = tid.partition("::")
            src = open(os.path.join(REPO, "tests", fname)).read()
            fn = next((n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == name), None)
            assert fn is not None, f"{entry}: {tid} does not exist"
            body = ast.get_source_segment(src, fn)
            assert re.search(rf"\b{entry}\b", body) or any(re.search(rf"\bops\.{w}\(", body) for w in wrappers.get(entry, ())), tid


def _arity(name):
    header = open(os.path.join(REPO, "include", "peekvit_hip_moe.h")).read()
    m = re.search(r"\b(?:int|int64_t) " + name + r"\(([^;]*)\);", header)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_packed_rows_and_scratch_size():
    from peekvit_amd import _lib
    lib = _lib.load()
    for name, (_, args) in _lib.SIGNATURES_MOE.items():
        assert _arity(name) == len(args), name
        assert hasattr(_lib.load("f16"), name)
    assert lib.pv_moe_packed_rows(1, 1) == 512 and lib.pv_moe_packed_rows(256, 8) == 9 * 256 and lib.pv_moe_packed_rows(403456, 8) == (1576 + 8) * 256
    assert lib.pv_moe_packed_rows(0, 2) == -1 and lib.pv_moe_packed_rows(10, 0) == -1 and lib.pv_moe_packed_rows(10, 65) == -1
    assert lib.pv_moe_route_scratch_size(403456, 8) == (1576 * 8 + 64) * 4 and lib.pv_moe_route_scratch_size(-1, 8) == -1
    assert lib.pv_moe_route_scratch_size(5, 65) == -1


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from peekvit_amd import _lib
    from peekvit_amd._lib import GemmArgs, PV_EPI_BIAS_GELU_BF16, PV_EPI_BIAS_RES_F32, PV_EPI_BIAS_BF16
    lib = _lib.load()
    p = C.c_void_p(256)                 # never dereferenced: every call below is refused before anything is launched
    null = C.c_void_p(0)

    def route(x=p, ldx=768, M=1000, D=768, E=8, gw=p, expert=p, perm=p, xln=null, scratch=p, nbytes=1 << 20, probs=null):
        return lib.pv_moe_route(x, ldx, M, D, p, p, 1e-5, gw, p, E, expert, null, probs, p, perm, p, xln, scratch, nbytes, null)
    assert route(x=null) == -1 and route(gw=null) == -1 and route(expert=null) == -1 and route(perm=null) == -1 and route(scratch=null) == -1
    assert route(E=0) == -1 and route(E=65) == -1 and route(M=0) == -1 and route(D=0) == -1
    assert route(D=770, ldx=772) == -2 and route(D=8192, ldx=8192) == -2          # D % 4, D > 4096
    assert route(ldx=766) == -1 and route(ldx=770) == -1                         # stride below D / not a multiple of 4
    assert route(x=C.c_void_p(260)) == -1 and route(xln=C.c_void_p(258)) == -1 and route(probs=C.c_void_p(258)) == -1
    assert route(nbytes=100) == -1                                              # scratch smaller than pv_moe_route_scratch_size

    def gemm(epi=PV_EPI_BIAS_GELU_BF16, M=1024, N=3072, K=768, tiles=4, E=8, ws=3072 * 768, perm=p, rows=900, te=p, **kw):
        a = GemmArgs(A=256, W=256, bias=256, out=256, res=256, M=M, N=N, K=K, lda=K, ldw=K, ldo=N, ldr=N, epilogue=epi, qscale=1.0)
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.pv_gemm_grouped_bf16(C.byref(a), te, tiles, E, ws, perm, rows, null)
    assert gemm(te=null) == -1 and gemm(E=0) == -1 and gemm(E=65) == -1 and gemm(tiles=3) == -1          # M != tiles * 256
    assert gemm(epi=PV_EPI_BIAS_BF16) == -2 and gemm(K=704, lda=704, ldw=704, ws=3072 * 704) == -2 and gemm(N=3068, ldo=3068, ldr=3068, ws=3068 * 768) == -2
    assert gemm(ws=100) == -1 and gemm(A=0) == -1 and gemm(A=264) == -1 and gemm(lda=772) == -1 and gemm(ldo=3000) == -1
    assert gemm(row_scale=256) == -1 and gemm(ksplit=2) == -1 and gemm(qcols=64) == -1 and gemm(ln_out=256) == -1
    assert gemm(struct_size=8) == -1
    assert gemm(epi=PV_EPI_BIAS_RES_F32, N=768, ldo=768, ldr=768, ws=768 * 768, perm=null) == -1          # the residual form needs perm
    assert gemm(epi=PV_EPI_BIAS_RES_F32, N=768, ldo=768, ldr=768, ws=768 * 768, rows=0) == -1
    assert gemm(epi=PV_EPI_BIAS_RES_F32, N=768, ldo=768, ldr=768, ws=768 * 768, res=0) == -1

    def gather(src=p, stride=1000 * 768, ld=768, M=1000, Mp=3072, D=768, E=8, out=p, perm=p):
        return lib.pv_moe_gather_bf16(src, stride, ld, p, perm, M, Mp, D, E, out, null)
    assert gather(src=null) == -1 and gather(out=null) == -1 and gather(perm=null) == -1 and gather(E=0) == -1 and gather(E=65) == -1
    assert gather(D=764, ld=764) == -1 and gather(ld=760) == -1 and gather(stride=999 * 768) == -1 and gather(out=C.c_void_p(264)) == -1
