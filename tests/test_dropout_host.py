"""Dropout on the training path without a GPU (include/peekvit_hip_dropout.h): the statistics of the mask generator as
tests/dropout_ref.py restates it, the fp64 restatement of attention under a mask (all-ones mask = no dropout; the hand-written backward = autograd;
a fully dropped row is exactly zero), the argument checks of the entry points in both builds (every refusal comes before a launch), the header's
ledger, and the dispatch of the switch on CPU tensors (`set_fused_dropout`: off by default, the composite for a CPU tensor, `train_eligible` unchanged)."""
import ast
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import attn_backward_ref as R
import dropout_ref as DR
from conftest import REPO

HEADER = os.path.join(REPO, "include", "peekvit_hip_dropout.h")
REFUSAL = "test_dropout_host.py::test_entry_points_refuse_bad_arguments_without_a_gpu"
LEDGER = {
    "pv_dropout_keep_u8": ["test_hip_dropout.py::test_mask_bits_equal_the_numpy_generator", REFUSAL],
    "pv_dropout_f32": ["test_hip_dropout.py::test_row_kernels", REFUSAL],
    "pv_dropout_residual": ["test_hip_dropout.py::test_row_kernels", REFUSAL],
    "pv_dropout_bwd16": ["test_hip_dropout.py::test_row_kernels", REFUSAL],
    "pv_attention_stream_lse_drop_bf16": ["test_hip_dropout.py::test_attention_forward_rows", REFUSAL],
    "pv_attention_stream_bwd16_drop_bf16": ["test_hip_dropout.py::test_attention_backward_rows", REFUSAL],
}
WRAPPERS = {"pv_dropout_keep_u8": "dropout_keep", "pv_dropout_f32": "dropout_f32", "pv_dropout_residual": "dropout_residual",
            "pv_dropout_bwd16": "dropout_bwd16", "pv_attention_stream_lse_drop_bf16": "attention_stream_drop",
            "pv_attention_stream_bwd16_drop_bf16": "attention_stream_bwd16_drop"}


# ---- the generator ----
ROWS, COLS = 2048, 1024


@pytest.fixture(scope="module")
def site_words():
    """The 32-bit words of the four sites the statistics need, computed once: (key 1234, site 7), its neighbour site and its neighbour key."""
    return {"main": DR.words(1234, 7, ROWS, COLS), "site8": DR.words(1234, 8, ROWS, COLS), "key1235": DR.words(1235, 7, ROWS, COLS)}


def _std(keep, q):
    return (keep.astype(np.float64) - q) / np.sqrt(q * (1.0 - q))


def _corr(a, b):
    """normalised correlation of two standardised arrays times sqrt(n): a unit normal for independent fair draws"""
    return float((a * b).mean() * np.sqrt(a.size))


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_generator_statistics(site_words, p):
    thr = DR.threshold(p)
    q = 1.0 - float(thr) / 2.0 ** 32                       # the exact keep probability
    assert abs((1.0 - q) - float(np.float32(p))) <= 2.0 ** -32
    keep = site_words["main"] >= thr
    n = keep.size
    z = (keep.mean() - q) / np.sqrt(q * (1.0 - q) / n)
    x = _std(keep, q)
    stats = {"lag-1 columns": _corr(x[:, :-1], x[:, 1:]), "lag-4 columns": _corr(x[:, :-4], x[:, 4:]), "lag-1 rows": _corr(x[:-1], x[1:]),
             "diagonal": _corr(x[:-1, :-1], x[1:, 1:]), "site 8": _corr(x, _std(site_words["site8"] >= thr, q)),
             "key 1235": _corr(x, _std(site_words["key1235"] >= thr, q))}
    row_dev = float(np.abs(keep.mean(1) - q).max() / np.sqrt(q * (1.0 - q) / COLS))
    col_dev = float(np.abs(keep.mean(0) - q).max() / np.sqrt(q * (1.0 - q) / ROWS))
    print(f"p = {p}: keep fraction z = {z:.2f}; " + ", ".join(f"{k} {v:.2f}" for k, v in stats.items()) + f"; row means {row_dev:.2f} sigma, column means {col_dev:.2f} sigma")
    assert abs(z) <= 4.0
    assert all(abs(v) <= 4.0 for v in stats.values()), stats
    assert row_dev <= 5.0 and col_dev <= 5.0


def test_generator_edges():
    assert DR.threshold(0.0) == 0 and DR.keep_mask(1, 2, 5, 7, 0.0).all()                     # p = 0 keeps everything, and the factor is 1
    assert DR.scale(0.0) == 1.0 and DR.scale(0.5) == 2.0
    a = DR.keep_mask(1234, 7, 40, 33, 0.5)
    assert np.array_equal(a[10:20], DR.keep_mask(1234, 7, 10, 33, 0.5, row0=10))              # a pure function of (row, col): any window agrees
    assert np.array_equal(a[:, :9], DR.keep_mask(1234, 7, 40, 9, 0.5))
    assert DR.sm64(0) == np.uint64(0xE220A8397B1DCDAF)                                       # splitmix64's first output for seed 0
    assert DR.keep_tensor(9, 1, (2, 3, 4, 5), 0.3).shape == (2, 3, 4, 5)
    assert np.array_equal(DR.keep_tensor(9, 1, (2, 3, 4, 5), 0.3).reshape(24, 5).numpy().astype(np.uint8), DR.keep_mask(9, 1, 24, 5, 0.3))


# ---- the fp64 restatement ----
def test_all_ones_mask_is_the_dropout_free_attention():
    B, S, H, dh = 2, 13, 2, 32
    qkv, dout = R.inputs(B, S, H, dh, torch.bfloat16)
    ones = torch.ones(B, H, S, S)
    want = R.fp64(qkv, dout, B, S, H, dh, dh ** -0.5)
    got = DR.fp64_attention(qkv, dout, ones, 0.0, B, S, H, dh, dh ** -0.5)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    out_m, g_m = DR.fp64_attention_manual(qkv, dout, ones, 0.0, B, S, H, dh, dh ** -0.5)
    assert (out_m - want[0]).abs().max() <= 1e-12 and (g_m - want[2]).abs().max() <= 1e-12
    # the fp32 restatements with an all-ones mask are attn_backward_ref's
    assert torch.equal(DR.restated_forward(qkv, ones, 0.0, B, S, H, dh)[0], R.restated_forward(qkv, B, S, H, dh, block=64)[0])
    assert torch.equal(DR.restated_forward(qkv, ones, 0.0, B, S, H, dh)[1], R.restated_forward(qkv, B, S, H, dh, block=64)[1])


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_hand_written_backward_equals_autograd(p):
    B, S, H, dh = 2, 70, 2, 32
    qkv, dout = R.inputs(B, S, H, dh, torch.float16)
    mask = DR.attention_mask(77, 3, B, H, S, p)
    out_a, _, g_a = DR.fp64_attention(qkv, dout, mask, p, B, S, H, dh, dh ** -0.5)
    out_m, g_m = DR.fp64_attention_manual(qkv, dout, mask, p, B, S, H, dh, dh ** -0.5)
    assert (out_a - out_m).abs().max() <= 1e-12 and (g_a - g_m).abs().max() <= 1e-12
    assert g_a.abs().max() > 1e-3


FULL_DROP = DR.FULL_DROP          # (shared with tests/test_hip_dropout.py)


def test_a_fully_dropped_row_is_exactly_zero():
    f = FULL_DROP
    B, H, S, dh, p = f["B"], f["H"], f["S"], f["dh"], f["p"]
    mask = DR.attention_mask(f["key"], f["site"], B, H, S, p)
    dead = ~mask.any(-1)                                   # [B, H, S]
    assert dead.any() and (~dead).any()                    # the fixture holds a fully dropped row and one that is not
    qkv, dout = R.inputs(B, S, H, dh, torch.bfloat16)
    out_a, _, g_a = DR.fp64_attention(qkv, dout, mask, p, B, S, H, dh, dh ** -0.5)
    out_m, g_m = DR.fp64_attention_manual(qkv, dout, mask, p, B, S, H, dh, dh ** -0.5)
    out_r = DR.restated_forward(qkv, mask, p, B, S, H, dh)[0]
    g_r = DR.restated_backward(qkv, dout, mask, p, B, S, H, dh, dh ** -0.5)
    for out, g in ((out_a, g_a), (out_m, g_m), (out_r, g_r)):
        assert torch.isfinite(out).all() and torch.isfinite(g).all()
        assert (R.heads(out, B, S, H, dh)[dead] == 0).all()                                   # the row's output ...
        assert (R.heads(g[..., :H * dh], B, S, H, dh)[dead] == 0).all()                       # ... and its query gradient, exactly
        assert (R.heads(out, B, S, H, dh)[~dead] != 0).any()
    # a key no query kept contributes to no output: its value gradient is exactly zero (its key gradient is not - the softmax is of all keys)
    unseen = ~mask.any(-2)
    if unseen.any():
        assert (R.heads(g_m[..., 2 * H * dh:], B, S, H, dh)[unseen] == 0).all() and (R.heads(g_r[..., 2 * H * dh:], B, S, H, dh)[unseen] == 0).all()


# ---- the C ABI ----
def _declared():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pv_\w+)\s*\(", src, flags=re.M))


def _arity(name):
    m = re.search(r"\bint " + name + r"\(([^;]*)\);", open(HEADER).read())
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_dropout_ledger_names_a_direct_test_for_every_declared_entry_point():
    from peekvit_amd import _build, _lib
    assert "peekvit_hip_dropout.h" in _build.HEADERS and os.path.join(_build.CSRC, "pv_dropout.hip") in _build.sources()
    assert _build.FILE_FLAGS["pv_dropout.hip"] == ["-fno-slp-vectorize"] == _build.FILE_FLAGS["pv_rowops.hip"]
    declared = _declared()
    assert set(LEDGER) == declared == set(_lib.SIGNATURES_DROPOUT) == set(WRAPPERS), declared ^ set(LEDGER)
    others = [getattr(_lib, n) for n in dir(_lib) if n.startswith("SIGNATURES") and n != "SIGNATURES_DROPOUT"]
    assert len(others) >= 13 and not any(set(_lib.SIGNATURES_DROPOUT) & set(d) for d in others)          # a dict of their own
    for name, (_, args) in _lib.SIGNATURES_DROPOUT.items():
        assert _arity(name) == len(args), name
        assert hasattr(_lib.load(), name) and hasattr(_lib.load("f16"), name)            # exported by both libraries
    assert _lib.load().pv_version() == 10 and _lib.load("f16").pv_version() == 10        # ABI unchanged
    ops_src = open(os.path.join(REPO, "peekvit_amd", "ops.py")).read()
    wrappers = {}
    for node in ast.parse(ops_src).body:
        if isinstance(node, ast.FunctionDef):
            for sym in re.findall(r"\b(pv_\w+)\(", ast.get_source_segment(ops_src, node)):
                wrappers.setdefault(sym, set()).add(node.name)
    assert all(wrappers.get(sym) == {w} for sym, w in WRAPPERS.items()), {s: wrappers.get(s) for s in WRAPPERS}          # one wrapper per entry point
    for entry, ids in LEDGER.items():
        for tid in ids:
            fname, _, name = tid.partition("::")
            src = open(os.path.join(REPO, "tests", fname)).read()
            funcs = {n.name: n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef)}
            assert name in funcs, f"{entry}: {tid} is not a test of {fname}"
            reach = {name}
            for _ in range(3):                             # the test, the helpers it calls, theirs
                for fn in list(reach):
                    reach |= {n.func.id for n in ast.walk(funcs[fn]) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id in funcs}
            body = "\n".join(ast.get_source_segment(src, funcs[fn]) for fn in reach)
            assert re.search(rf"\b{entry}\(", body) or re.search(rf"\bops\.{WRAPPERS[entry]}\(", body), f"{tid} never calls {entry}"


def test_the_attention_entry_points_instantiate_the_existing_kernels():
    """Call, do not copy: dropout is a template flag of the three streaming kernels, not a fourth kernel; the mask is one device function."""
    from peekvit_amd import _build
    read = lambda f: open(os.path.join(_build.CSRC, f)).read()
    stream, attn, drop, gen = read("pv_attention_stream.hip"), read("pv_attention.hip"), read("pv_dropout.hip"), read("pv_dropout.h")
    assert 'extern "C" int pv_attention_stream_lse_drop_bf16(' in stream and 'extern "C" int pv_attention_stream_bwd16_drop_bf16(' in stream
    # (one launcher per direction instantiates the kernels from its own template flags; the entry points name the flags where they call it)
    assert "pv_attn_stream_dq_kernel<DH, O16, W, DROP>" in stream and "pv_attn_stream_dkv_kernel<DH, O16, W, DROP>" in stream
    assert "pv_dispatch_attn_stream_bwd<true, false, true>(" in stream
    assert "pv_attn_stream_kernel<DH, LSE, W, DROP>" in attn and "pv_dispatch_attn_stream_lse<false, true>(" in attn
    assert "pv_launch_attn_stream_lse_drop(" in stream
    for f in sorted(os.listdir(_build.CSRC)):
        text = read(f)
        assert len(re.findall(r"__global__[^;{]*\bpv_attn_stream_d(?:q|kv)_kernel\(", text)) == (2 if f == "pv_attention_stream.hip" else 0), f
        assert len(re.findall(r"__global__[^;{]*\bpv_attn_stream_kernel\(", text)) == (1 if f == "pv_attention.hip" else 0), f
        assert len(re.findall(r"__global__[^;{]*\bpv_attn_stream_var_kernel\(", text)) == (1 if f == "pv_attention.hip" else 0), f
        assert len(re.findall(r"\bpv_drop_lb32\(uint32_t", text)) == (1 if f == "pv_dropout.h" else 0), f          # the generator exists once
    # the uniform and the ragged forward share ONE body: its score product is written once
    assert attn.count("PV_MFMA_16x16x32(*reinterpret_cast<const bf16x8*>(Ks + koff[ks] + kt * (16 * DHP * 2)), qf[ks], a, 0, 0, 0)") == 1
    assert attn.count("pv_attn_stream_body<DH, LSE, W, DROP, false>(") == 1 and attn.count("pv_attn_stream_body<DH, false, false, false, true>(") == 1
    for text in (stream, attn, drop):
        assert "pv_drop_keep(" in text and "pv_drop_row_key(" in text
    assert '#include "pv_rows.h"' in drop and all(piece in drop for piece in ("RowRegs<NCH>", "pv_load_row<NCH>", "pv_store_row<NCH>", "pv_store_row16<NCH>"))
    assert "atomic" not in drop.replace("no atomics", "") and "atomic" not in gen


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from peekvit_amd import _lib
    p, q, null = C.c_void_p(256), C.c_void_p(1 << 30), C.c_void_p(0)       # never dereferenced: every call below is refused before a launch
    odd16, odd8, odd4 = C.c_void_p(264), C.c_void_p(260), C.c_void_p(258)  # off a 16-byte / an 8-byte / a 4-byte boundary
    bad_p = (-0.1, 1.0, float("nan"), 1.5, float("inf"))
    for op in ("bf16", "f16"):
        lib = _lib.load(op)

        def keep(k=p, rows=5, cols=7, pp=0.1):
            return lib.pv_dropout_keep_u8(k, 1234, 7, rows, cols, pp, null)

        def f32(x=p, out=q, rows=5, D=64, pp=0.1):
            return lib.pv_dropout_f32(x, out, 1234, 7, rows, D, pp, null)

        def res(x=p, u=p, out=q, rows=5, D=64, pp=0.1):
            return lib.pv_dropout_residual(x, u, out, 1234, 7, rows, D, pp, null)

        def b16(d=p, du=q, rows=5, D=64, pp=0.1):
            return lib.pv_dropout_bwd16(d, du, 1234, 7, rows, D, pp, null)

        assert keep(k=null) == -1
        for call, ptrs, wide in ((f32, ("x", "out"), ("x", "out")), (res, ("x", "u", "out"), ("x", "out")), (b16, ("d", "du"), ())):
            for name in ptrs:
                assert call(**{name: null}) == -1, name                                           # nulls
                assert call(**{name: odd4}) == -1, name                                           # misaligned for either element size
                if name in wide:
                    assert call(**{name: odd16}) == -1 and call(**{name: odd8}) == -1, name       # fp32 rows: 16-byte aligned
            assert call(D=62) == -2 and call(D=4100) == -2 and call(D=8192) == -2                 # D % 4, D > 4096
        assert b16(du=p) == -1                                                                    # out of place only
        for call in (keep, f32, res, b16):
            assert call(rows=0) == -1 and call(rows=-3) == -1
            for pp in bad_p:
                assert call(pp=pp) == -1, pp                                                      # p < 0, p >= 1, NaN
        assert keep(cols=0) == -1 and keep(cols=-1) == -1 and keep(cols=1 << 33) == -2
        for call in (f32, res, b16):
            assert call(D=0) == -1 and call(D=-64) == -1

        def fwd(qkv=p, out=q, lse=q, flag=null, B=2, S=65, H=2, dh=32, pp=0.1):
            return lib.pv_attention_stream_lse_drop_bf16(qkv, out, lse, B, S, H, dh, pp, 1234, 7, flag, null)

        def bwd(qkv=p, dout=p, out=p, lse=p, dqkv16=q, dbias=q, delta=q, B=2, S=65, H=2, dh=32, pp=0.1):
            return lib.pv_attention_stream_bwd16_drop_bf16(qkv, dout, out, lse, dqkv16, dbias, delta, B, S, H, dh, 1.0, pp, 1234, 7, null)

        for call, ptrs, wide in ((fwd, ("qkv", "out", "lse"), ("qkv", "out")), (bwd, ("qkv", "dout", "out", "lse", "dqkv16", "delta"), ("qkv", "dout", "out", "dqkv16"))):
            for name in ptrs:
                assert call(**{name: null}) == -1, name                                           # nulls (the flag word / dbias may be null)
                assert call(**{name: odd4}) == -1, name
                if name in wide:
                    assert call(**{name: odd16}) == -1, name                                      # 16-bit arrays: 16-byte aligned
            for dim in ("B", "S", "H"):
                assert call(**{dim: 0}) == -1 and call(**{dim: -1}) == -1, dim
            for dh in (16, 40, 80, 96, 128, 33):
                assert call(dh=dh) == -2, dh                                                      # dh outside {32, 48, 64}
            assert call(dh=0) == -1 and call(dh=-32) == -1
            for pp in bad_p:
                assert call(pp=pp) == -1, pp
            assert call(B=1 << 31) == -2 and call(B=1 << 20, H=1 << 11) == -2 and call(B=1 << 16, H=1 << 10, S=64 * 32 + 1) == -2 and call(S=1 << 31) == -2
        assert fwd(flag=odd4) == -1 and bwd(dbias=odd4) == -1


# ---- the switch ----
def _vit(**kw):
    from peekvit_amd.models.vit import VisionTransformer
    return VisionTransformer(image_size=32, patch_size=8, num_layers=2, num_heads=2, hidden_dim=64, mlp_dim=128, num_classes=10, **kw)


def test_switch_exists_is_off_by_default_and_leaves_cpu_tensors_on_the_composite():
    from peekvit_amd import ops, train_engine
    from peekvit_amd.models import adavit, moevit, rankvit, residualvit, vit
    assert hasattr(vit.VisionTransformer, "set_fused_dropout") and hasattr(rankvit.RankVisionTransformer, "set_fused_dropout")
    for cls in (residualvit.ResidualVisionTransformer, adavit.AdaptiveVisionTransformer, moevit.VisionTransformerMoE):
        assert not hasattr(cls, "set_fused_dropout"), cls                                        # the other models keep their behaviour: no switch
    model = _vit(dropout=0.1, attention_dropout=0.1)
    torch.nn.init.normal_(model.head.weight, std=0.02)
    assert not getattr(model, "_pv_fused_dropout", False)                                         # off by default
    x = torch.randn(2, 3, 32, 32)
    assert not model._fused_dropout_ok(x)
    n0 = ops.launch_count
    torch.manual_seed(5)
    want = model(x)
    model.set_fused_dropout(True)
    assert model._pv_fused_dropout and "_pv_fused_dropout" not in model.state_dict()
    assert not model._fused_dropout_ok(x)                                                         # a CPU tensor
    torch.manual_seed(5)
    got = model(x)
    assert torch.equal(got, want) and ops.launch_count == n0                                      # the stock composite, its random stream, bit for bit
    assert train_engine.train_state(model).dropout_record is None
    assert train_engine.live_dropout_p(model) == [0.1] * 5
    model.encoder.layers[1].dropout.p = 0.25                                                      # the live values, not the constructor's
    assert train_engine.live_dropout_p(model) == [0.1, 0.1, 0.1, 0.25, 0.1]
    model.set_fused_dropout(False)
    assert not model._pv_fused_dropout


def test_train_eligible_keeps_its_meaning(monkeypatch):
    """`dropout > 0 in train mode` still means "not eligible" for every caller that does not ask otherwise (ResidualViT, A-ViT, MoE, the point-cloud
    models and a block called on its own pin it); the switch has a predicate of its own, which is false outside a pass that runs with fused dropout."""
    from peekvit_amd import engine, train_engine
    assert list(inspect.signature(train_engine.train_eligible).parameters) == ["x", "module", "dropout_p"]
    monkeypatch.delenv("PEEKVIT_AMD_BACKEND", raising=False)
    monkeypatch.delenv("PEEKVIT_AMD_TRAIN", raising=False)
    gpu_like = types.SimpleNamespace(is_cuda=True, numel=lambda: 8)           # (only what the predicate reads)
    blk = _vit(dropout=0.1).encoder.layers[0]
    with engine.precision("auto"), torch.enable_grad():
        assert blk.training and not train_engine.train_eligible(gpu_like, blk, 0.1) and train_engine.train_eligible(gpu_like, blk, 0.0)
        blk.eval()
        assert train_engine.train_eligible(gpu_like, blk, 0.1)
        blk.train()
        assert not train_engine.dropout_eligible(gpu_like, blk)                                   # no pass: a block on its own keeps the composite
        assert not train_engine.train_eligible(torch.zeros(2, 5, 64), blk, 0.0)                   # a CPU tensor
    with engine.precision("bf16x3"), torch.enable_grad():
        assert not train_engine.train_eligible(gpu_like, blk, 0.0)


def test_harness_flag_defaults_to_off():
    text = open(os.path.join(REPO, "peekvit_amd", "harness", "configs", "training", "base.yaml")).read()
    assert re.search(r"^fused_dropout: false\b", text, flags=re.M)
    src = open(os.path.join(REPO, "peekvit_amd", "harness", "train.py")).read()
    assert 'tr.get("fused_dropout", False)' in src and "model.set_fused_dropout(True)" in src
