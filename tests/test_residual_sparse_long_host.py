"""ResidualViT exact token compaction past 208 rows per image without a GPU: the eligibility rule of the long packed path, a
test ledger for include/peekvit_hip_sparse_long.h and the argument checks of its entry points, the fixture of
scripts/make_golden_residual_sparse_long.py, and the torch restatement of the packed algorithm against the dense forward in fp64 at 227 rows."""
import ast
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
from peekvit_amd import synth
import residual_sparse_ref as R

META = json.load(open(os.path.join(GOLDEN, "residualvit_sparse_long_meta.json")))
EXTRA = dict(gate_type="sigmoid", gate_temp=1, add_budget_token="learnable", gate_threshold=0.5)
HEADER = os.path.join(REPO, "include", "peekvit_hip_sparse_long.h")


# ---- eligibility ----
def _model(**over):
    from peekvit_amd.models.residualvit import ResidualVisionTransformer
    kw = dict(image_size=240, patch_size=16, num_layers=2, num_heads=1, hidden_dim=64, mlp_dim=64, **EXTRA)
    return ResidualVisionTransformer(**dict(kw, **over)).eval()


class _Cuda:              # (is_cuda is all the rule reads of the tensor; real GPU tensors are exercised in tests/test_hip_residual_sparse_long.py)
    is_cuda = True


def test_long_eligibility_rules():
    m = _model()
    ok = lambda model: model._long_compaction_ok(_Cuda())
    assert m.seq_length + 1 == 227 and ok(m) and not m._compaction_ok(_Cuda())          # the resident rule keeps its answer
    assert not m._long_compaction_ok(torch.zeros(1))                                    # a CPU tensor
    # the admitted rows per image (the rule reads seq_length; a square patch grid cannot land on the four edges)
    for rows, long_ok, resident_ok in ((208, False, True), (209, True, False), (4096, True, False), (4097, False, False), (3, False, True)):
        m.seq_length = rows - 1
        assert ok(m) is long_ok and m._compaction_ok(_Cuda()) is resident_ok, rows
    m.seq_length = 226
    m.train()
    assert not ok(m)                                                                    # eval only
    m.eval()
    h = m.encoder.layers[1].mlp.register_forward_hook(lambda *a: None)
    assert not ok(m)
    h.remove()
    h = m.encoder.register_forward_pre_hook(lambda *a: None)
    assert not ok(m)
    h.remove()
    assert ok(m)
    keep = m.encoder.layers[0]
    m.encoder.layers[0] = torch.nn.Identity()
    assert not ok(m)
    m.encoder.layers[0] = keep
    assert ok(m)
    del m.encoder.layers[1]
    assert not ok(m)
    assert not ok(_model(dropout=0.1)) and not ok(_model(attention_dropout=0.1))
    assert not ok(_model(num_heads=2))                                                  # head dim 32
    assert not ok(_model(residual_layers=["attention+mlp", "mlp"])) and not ok(_model(gate_type="gumbel"))
    assert ok(_model(hidden_dim=256, num_heads=4, mlp_dim=768))                         # the dims of the fixture


def test_cpu_model_past_208_rows_with_compaction_on_is_the_dense_path():
    from peekvit_amd import engine
    m = _model(image_size=240, num_classes=10)
    x = torch.from_numpy(synth.synth_images(1, 240, seed=2))
    m.set_budget(0.5)
    with torch.no_grad():
        off = m(x)
    m.set_token_compaction(True)
    n0, r0, l0 = engine.sparse_dense_forwards, engine.sparse_rows, engine.sparse_long_layers
    with torch.no_grad():
        on = m(x)
    assert torch.equal(on, off)
    assert engine.sparse_dense_forwards == n0 + 1 and engine.sparse_rows == r0 and engine.sparse_long_layers == l0
    assert isinstance(engine.sparse_last_max_len, list)


# ---- include/peekvit_hip_sparse_long.h: every declared entry point is exported, bound, wrapped and has a test that calls it directly ----
LEDGER = {
    "pv_attention_varlen_w_stream_bf16": ["test_hip_residual_sparse_long.py::test_attention_stream_matches_fp64_with_random_multiplicities",
                                          "test_hip_residual_sparse_long.py::test_attention_stream_equals_dense_attention_over_repeated_rows",
                                          "test_hip_residual_sparse_long.py::test_attention_stream_has_the_bits_of_the_streaming_forward",
                                          "test_hip_residual_sparse_long.py::test_attention_stream_refuses_what_it_does_not_take"],
    "pv_residual_pack_step_long": ["test_hip_residual_sparse_long.py::test_pack_step_long_against_the_restatement",
                                   "test_hip_residual_sparse_long.py::test_pack_step_long_has_the_bits_of_the_resident_step",
                                   "test_hip_residual_sparse_long.py::test_pack_step_long_refuses_more_rows_than_it_holds"],
}
WRAPPERS = {"pv_attention_varlen_w_stream_bf16": "attention_varlen_w_stream", "pv_residual_pack_step_long": "residual_pack_step_long"}


def _arity(name, header=HEADER):
    m = re.search(r"\b(?:int|int64_t) " + name + r"\(([^;]*)\);", open(header).read())
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_ledger_names_a_direct_test_for_every_declared_entry_point():
    from peekvit_amd import _build, _lib, ops
    assert "peekvit_hip_sparse_long.h" in _build.HEADERS
    assert _build.FILE_FLAGS.get("pv_sparse_long.hip") == _build.FILE_FLAGS["pv_sparse.hip"]            # the flags of its sibling
    assert os.path.exists(os.path.join(REPO, "peekvit_amd", "csrc", "pv_sparse_long.hip"))
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pv_\w+)\s*\(", src, flags=re.M))
    assert set(LEDGER) == declared == set(_lib.SIGNATURES_SPARSE_LONG) == set(WRAPPERS), declared ^ set(LEDGER)
    others = [getattr(_lib, n) for n in dir(_lib) if n.startswith("SIGNATURES") and n != "SIGNATURES_SPARSE_LONG"]
    assert len(others) >= 14 and not any(set(_lib.SIGNATURES_SPARSE_LONG) & set(d) for d in others)         # a dict of their own
    sibling_header = os.path.join(REPO, "include", "peekvit_hip_sparse.h")
    for name, sibling in (("pv_attention_varlen_w_stream_bf16", "pv_attention_varlen_w_bf16"), ("pv_residual_pack_step_long", "pv_residual_pack_step")):
        _, args = _lib.SIGNATURES_SPARSE_LONG[name]
        assert _arity(name) == len(args) == _arity(sibling, sibling_header), name                            # the sibling's argument list
        assert args == _lib.SIGNATURES_SPARSE[sibling][1]
        assert hasattr(_lib.load(), name) and hasattr(_lib.load("f16"), name)                                # exported by both libraries
        assert re.search(rf"\b{name}\(", ast.get_source_segment(open(ops.__file__).read(), next(
            n for n in ast.parse(open(ops.__file__).read()).body if isinstance(n, ast.FunctionDef) and n.name == WRAPPERS[name])))
    assert _lib.load().pv_version() == 10 and _lib.load("f16").pv_version() == 10                            # ABI unchanged
    assert re.search(r"#define PV_SPARSE_LONG_MAX_LEN 4096\b", open(HEADER).read()) and ops.SPARSE_LONG_MAX_LEN == 4096
    for entry, ids in LEDGER.items():
        for tid in ids:
            fname, _, name = tid.partition("::")
            tsrc = open(os.path.join(REPO, "tests", fname)).read()
            funcs = {n.name: n for n in ast.parse(tsrc).body if isinstance(n, ast.FunctionDef)}
            assert name in funcs, f"{entry}: {tid} is not a test of {fname}"
            helpers = {c.func.id for c in ast.walk(funcs[name]) if isinstance(c, ast.Call) and isinstance(c.func, ast.Name) and c.func.id in funcs}
            body = "\n".join(ast.get_source_segment(tsrc, funcs[f]) for f in {name} | helpers)
            assert re.search(rf"\b{entry}\b", body) or re.search(rf"\bops\.{WRAPPERS[entry]}\b", body), f"{tid} never calls {entry}"


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from peekvit_amd import _lib
    p, q, null = C.c_void_p(256), C.c_void_p(1 << 30), C.c_void_p(0)       # never dereferenced: every call below is refused before a launch
    for op in ("bf16", "f16"):
        lib = _lib.load(op)

        def attn(qkv=p, out=q, seg=p, lm=p, B=4, max_len=402, H=4, dh=64):
            return lib.pv_attention_varlen_w_stream_bf16(qkv, out, seg, lm, B, max_len, H, dh, null, null)
        assert attn(qkv=null) == -1 and attn(out=null) == -1 and attn(seg=null) == -1 and attn(lm=null) == -1
        assert attn(B=0) == -1 and attn(H=0) == -1 and attn(max_len=0) == -1
        assert attn(qkv=C.c_void_p(264)) == -1 and attn(out=C.c_void_p((1 << 30) + 4)) == -1                 # misaligned
        assert attn(seg=C.c_void_p(258)) == -1 and attn(lm=C.c_void_p(257)) == -1
        assert attn(dh=32) == -2 and attn(dh=128) == -2 and attn(max_len=4097) == -2
        assert attn(B=1 << 31, H=2) == -2 and attn(B=1 << 25, max_len=4096) == -2                            # grid above 2^31 - 1

        def pack(x=p, seg=p, mult=p, tok=p, B=4, N=400, D=256, wg=p, bg=p, wb=p, bb=p, temp=1.0, mrow=p, xn=q, rs=p, mn=p, lm=p, sn=p, tn=p,
                 mo=p, th=p, tot=p, g=null, b=null, ln=null):
            return lib.pv_residual_pack_step_long(x, seg, mult, tok, B, N, D, wg, bg, wb, bb, temp, 0.0, mrow, xn, rs, mn, lm, sn, tn, mo, th, tot,
                                                  g, b, 1e-6, ln, null)
        for k in ("x", "seg", "mult", "tok", "wg", "bg", "wb", "bb", "mrow", "xn", "rs", "mn", "lm", "sn", "tn", "mo", "th", "tot"):
            assert pack(**{k: null}) == -1, k
        assert pack(B=0) == -1 and pack(D=0) == -1 and pack(N=-1) == -1 and pack(temp=0.0) == -1
        assert pack(xn=p) == -1                                          # in place
        assert pack(ln=p) == -1 and pack(ln=p, g=p) == -1                # LayerNorm output without its affine
        assert pack(D=770) == -2 and pack(D=8192) == -2 and pack(N=4095) == -2 and pack(B=1 << 31) == -2
        assert pack(x=C.c_void_p(260)) == -2 and pack(xn=C.c_void_p((1 << 30) + 8)) == -2 and pack(wg=C.c_void_p(264)) == -2
        assert pack(ln=C.c_void_p(516), g=p, b=p) == -2 and pack(ln=p, g=C.c_void_p(260), b=p) == -2


# ---- fixture ----
def test_long_fixture_and_its_metadata():
    g = np.load(os.path.join(GOLDEN, "residualvit_sparse_long.npz"))
    assert META["dims"] == dict(patch_size=8, num_layers=4, num_heads=4, hidden_dim=256, mlp_dim=768, num_classes=10)
    assert META["sizes"] == [120, 160] and META["batch"] == 2 and META["budgets"] == [0.2, 0.5, 0.8] and META["gate_gain"] == 4.0
    assert META["kwargs"]["gate_bias"] == 1 and META["margin"] == 5e-3 and META["max_excluded_fraction"] == 0.02
    assert set(META["reference_sha256"]) == {"models/residualvit.py", "models/blocks.py"}
    L = META["dims"]["num_layers"]
    for size, rows in ((120, 227), (160, 402)):
        N = (size // 8) ** 2
        assert META["size"][str(size)]["rows"] == rows == N + 2
        for b in META["budgets"]:
            key = f"s{size}_b{b}_"
            assert g[key + "logits"].shape == (2, 10) and g[key + "masks"].shape == (L, 2, N, 1)
            assert g[key + "thresholds"].shape == (L, 2) and g[key + "margin"].shape == (L, 2, N)
            assert float((g[key + "margin"] < META["margin"]).mean()) <= META["max_excluded_fraction"]
            assert 0.3 < float(g[key + "rows_share"]) < 0.7 and bool((g[key + "masks"] == 0).any())
            # a mask is zero exactly where sigmoid <= threshold: margin and mask agree
            assert bool(((g[key + "masks"][..., 0] > 0) <= (g[key + "margin"] > 0)).all())
            rec = META["size"][str(size)]["budget"][str(b)]
            assert abs(sum(rec["rows_per_layer"]) / (L * 2 * rows) - float(g[key + "rows_share"])) < 1e-12
    assert len(g.files) == 2 * 3 * 5
    assert os.path.getsize(os.path.join(GOLDEN, "residualvit_sparse_long.npz")) < 1 << 20


# ---- the checker of the GPU tests at more than 208 rows ----
def test_packed_restatement_equals_the_dense_forward_in_fp64_at_227_rows():
    torch.set_num_threads(min(8, torch.get_num_threads()))
    cfg = dict(META["dims"], image_size=120, **META["kwargs"])
    sd = R.sparse_sd(cfg, META["gate_gain"], torch.float64)
    x = torch.from_numpy(synth.synth_images(META["batch"], 120, seed=0)).double()
    S = synth.seq_length(cfg) + 1
    assert S == 227
    g = np.load(os.path.join(GOLDEN, "residualvit_sparse_long.npz"))
    for b in META["budgets"]:
        ld, md, td, _ = R.dense_forward(x, sd, cfg, b)
        lp, mp, tp, rows = R.packed_forward(x, sd, cfg, b)
        assert ld.dtype == lp.dtype == torch.float64
        assert R.rel_l2(lp, ld) < 1e-12
        assert torch.equal(mp == 0, md == 0) and float((mp - md).abs().max()) < 1e-12 and float((tp - td).abs().max()) < 1e-12
        assert bool((md == 0).any()) and sum(rows) < len(rows) * META["batch"] * S
        # ... and it is what the fixture recorded from the real reference
        assert rows == META["size"]["120"]["budget"][str(b)]["rows_per_layer"]
        assert R.rel_l2(lp.numpy(), g[f"s120_b{b}_logits"]) < 1e-4 and np.array_equal(mp.numpy() == 0, g[f"s120_b{b}_masks"] == 0)
