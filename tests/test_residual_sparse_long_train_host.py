"""ResidualViT packed training past 208 rows per image without a GPU: the fp64 restatement against the dense composite on
the three cases the GPU step test uses (with the preconditions that keep the comparison from passing vacuously), the eligibility rule, a test ledger
for include/peekvit_hip_sparse_long_train.h with the argument checks of its four entry points, and a CPU step with the switch on at 402 rows."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from peekvit_amd import synth
import residual_sparse_ref as R
import test_residual_sparse_train_host as host
from test_long_train_host import _Cuda

HEADER = os.path.join(REPO, "include", "peekvit_hip_sparse_long_train.h")
RESIDENT = 208
MARGIN_ROWS = 20            # how far a layer's longest segment stays from the switch point, so that fp32 gates cannot move it across
KNEE = 1e-3

ROWS402 = dict(image_size=80, patch_size=4, num_layers=3, num_heads=2, hidden_dim=128, mlp_dim=256, num_classes=10)
ROWS227 = dict(image_size=60, patch_size=4, num_layers=2, num_heads=2, hidden_dim=128, mlp_dim=256, num_classes=10)
# name -> (model dims, batch, per-image budgets, gate gain, gate_bias, seed, layers whose longest segment exceeds 208 rows)
CASES = {
    "all_stream": (ROWS402, 3, [0.1, 0.5, 0.95], 4.0, 1.0, 0, [True, True, True]),
    "first_streams": (ROWS402, 3, [0.1, 0.5, 0.95], 4.0, 0.0, 1, [True, False, False]),
    "rows227": (ROWS227, 3, [0.1, 0.5, 0.9], 4.0, 0.0, 1, [False, False]),
}


def build(name):
    """test_residual_sparse_train_host.build for the cases above: (cfg, model in double and train mode with fixed budgets, x, y, budgets)."""
    from peekvit_amd.models.residualvit import ResidualVisionTransformer
    dims, batch, budgets, g, gb, seed, _ = CASES[name]
    cfg = dict(dims, **host.EXTRA, gate_bias=gb)
    sd = R.sparse_sd(cfg, g, torch.float64, seed=seed)
    model = ResidualVisionTransformer(**cfg).double()
    model.load_state_dict(sd)
    model.train()
    bud = torch.tensor(budgets, dtype=torch.float64)
    model._sample_budget = lambda n: bud.clone()
    x = torch.from_numpy(synth.synth_images(batch, cfg["image_size"], seed=seed)).double()
    y = torch.arange(batch) % cfg["num_classes"]
    return cfg, model, x, y, budgets


def segment_lengths(masks):
    """Rows of every image's packed segment behind each layer's pack step, from the dense masks: class row + one row per live class of tokens + one
    zero row if anything is masked + budget row.  (Tokens masked together form one class from then on.)"""
    B, N = masks[0].shape[:2]
    label = np.arange(B * N).reshape(B, N)
    nxt = B * N
    out = []
    for m in masks:
        z = (m[..., 0] == 0).numpy()
        lens = []
        for b in range(B):
            lens.append(2 + len(set(label[b][~z[b]].tolist())) + int(z[b].any()))
            if z[b].any():
                label[b][z[b]] = nxt
                nxt += 1
        out.append(lens)
    return out


def knee_share(m64, x):
    """The share of tokens within KNEE of the relu's knee in the fp64 composite, over every block."""
    out, hooks = [], []

    def pre(blk, inp):
        t = inp[0]
        thr = torch.sigmoid(blk.budget_token_gate(t[:, -1:]))
        sig = torch.sigmoid(blk.residual_gate.projection(t[:, 1:-1]) / blk.residual_gate.temp + blk.residual_gate.sigmoid_bias)
        out.append((sig - thr).abs().reshape(-1).detach())
    for blk in m64.encoder.layers:
        hooks.append(blk.register_forward_pre_hook(pre))
    with torch.no_grad():
        m64(x)
    for h in hooks:
        h.remove()
    return float((torch.cat(out) < KNEE).double().mean())


# ---- 1. the checker of the GPU step test: the packed restatement is the dense composite past 208 rows ----
@pytest.mark.parametrize("name", list(CASES))
def test_packed_training_step_equals_the_dense_composite_in_fp64_past_208_rows(name):
    torch.set_num_threads(min(8, torch.get_num_threads()))
    cfg, model, x, y, budgets = build(name)
    S = synth.seq_length(cfg) + 1
    assert S == (227 if name == "rows227" else 402)
    dense = host.dense_step(model, x, y)
    lens = segment_lengths(dense[2])
    shares, relive, nothing = host.mask_facts(dense[2])
    share = knee_share(model, x)
    print(f"\n{name}: segment lengths per layer {lens}, masked share per block {['%.2f' % s for s in shares]}, a merged class live again: {relive}, "
          f"an image that masks nothing: {nothing}, tokens within {KNEE} of the knee {share:.4f}")
    # the case's own preconditions, so that neither this comparison nor the GPU test's can pass vacuously
    streams = CASES[name][6]
    assert len(lens) == len(streams)
    for layer, (ln, stream) in enumerate(zip(lens, streams)):
        assert (max(ln) >= RESIDENT + 1 + MARGIN_ROWS) if stream else (max(ln) <= RESIDENT - MARGIN_ROWS), (layer, ln)
    assert share <= 0.05                                             # the cap of the GPU test's mask comparison
    if name == "all_stream":
        assert relive and nothing
        assert any(min(ln) < RESIDENT for ln in lens)                # short and long segments in one launch
    packed = host.packed_step(model, cfg, x, y, budgets)
    assert packed[5] > 0, "the mask loss is zero: its gradient would not be exercised"
    assert sum(packed[4]) < len(packed[4]) * x.shape[0] * S          # row share < 1
    assert packed[4] == [sum(ln) for ln in lens]
    for md, mp in zip(dense[2], packed[2]):
        assert torch.equal(md == 0, mp == 0) and float((md - mp).abs().max()) < 1e-12
    errs = host.compare(dense, packed)
    worst = max(errs, key=errs.get)
    print(f"{name}: loss {errs['loss']:.3g}, logits {errs['logits']:.3g}, worst gradient {worst} {errs[worst]:.3g} over {len(errs) - 2} tensors, "
          f"rows share {sum(packed[4]) / (len(packed[4]) * x.shape[0] * S):.3f}")
    assert errs[worst] < host.LIMIT, (worst, errs[worst])


# ---- 2. eligibility ----
def _model(**over):
    from peekvit_amd.models.residualvit import ResidualVisionTransformer
    kw = dict(image_size=240, patch_size=16, num_layers=2, num_heads=1, hidden_dim=64, mlp_dim=64, **host.EXTRA)
    return ResidualVisionTransformer(**dict(kw, **over)).train()


def test_long_compact_training_eligibility():
    with torch.enable_grad():
        m = _model()
        ok = lambda model: model._long_compact_training_ok(_Cuda())
        assert m.seq_length + 1 == 227 and ok(m)
        assert not m._compaction_ok(_Cuda(), training=True) and not m._long_compaction_ok(_Cuda())      # today's answers
        assert not m._long_compact_training_ok(torch.zeros(1))                                          # a CPU tensor
        for rows, long_ok, resident_ok in ((208, False, True), (209, True, False), (227, True, False), (402, True, False), (4096, True, False),
                                           (4097, False, False)):
            m.seq_length = rows - 1
            assert ok(m) is long_ok and m._compaction_ok(_Cuda(), training=True) is resident_ok, rows
            assert not m._long_compaction_ok(_Cuda()) and not m._compaction_ok(_Cuda())                  # train mode: not the inference rules' business
        m.seq_length = 401
        m.eval()
        assert not ok(m) and m._long_compaction_ok(_Cuda()) and not m._compaction_ok(_Cuda(), training=True)
        m.train()
        assert ok(m)
        with torch.no_grad():
            assert not ok(m)                                                                            # nothing to train
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
        assert not ok(_model(dropout=0.1)) and not ok(_model(attention_dropout=0.1))
        assert not ok(_model(num_heads=2))                                                              # head dim 32
        assert ok(_model(hidden_dim=256, num_heads=4, mlp_dim=768, image_size=160, patch_size=8))       # the reference's small model at 160 px


# ---- 3. include/peekvit_hip_sparse_long_train.h: every declared entry point is exported, bound, wrapped and has a test that calls it directly ----
GPU_TESTS = "test_hip_residual_sparse_long_train.py"
LEDGER = {
    "pv_attention_varlen_w_stream_lse_bf16": [GPU_TESTS + "::test_streaming_ragged_attention_pair_against_fp64"],
    "pv_attention_varlen_w_stream_bwd16_bf16": [GPU_TESTS + "::test_streaming_ragged_attention_pair_against_fp64",
                                                GPU_TESTS + "::test_a_weighted_key_beyond_row_255_is_seen"],
    "pv_residual_pack_step_long_train": [GPU_TESTS + "::test_pack_step_long_train_and_its_backward_against_fp64_autograd"],
    "pv_residual_pack_step_long_bwd": [GPU_TESTS + "::test_pack_step_long_train_and_its_backward_against_fp64_autograd"],
}
SIBLINGS = {"pv_attention_varlen_w_stream_lse_bf16": ("attention_varlen_w_stream_lse", "pv_attention_varlen_w_lse_bf16"),
            "pv_attention_varlen_w_stream_bwd16_bf16": ("attention_varlen_w_stream_bwd16", "pv_attention_varlen_w_bwd16_bf16"),
            "pv_residual_pack_step_long_train": ("residual_pack_step_long_train", "pv_residual_pack_step_train"),
            "pv_residual_pack_step_long_bwd": ("residual_pack_step_long_bwd", "pv_residual_pack_step_bwd")}


def test_ledger_names_a_direct_test_for_every_declared_entry_point():
    from peekvit_amd import _build, _lib
    header = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pv_\w+)\s*\(", src, flags=re.M))
    assert "peekvit_hip_sparse_long_train.h" in _build.HEADERS
    assert '#include "peekvit_hip_sparse_train.h"' in header and '#include "peekvit_hip_sparse_long.h"' in header
    assert _build.FILE_FLAGS["pv_sparse_long_train.hip"] == _build.FILE_FLAGS["pv_sparse_long.hip"]
    assert set(LEDGER) == declared == set(_lib.SIGNATURES_SPARSE_LONG_TRAIN) == set(SIBLINGS), declared ^ set(LEDGER)
    ops_src = open(os.path.join(REPO, "peekvit_amd", "ops.py")).read()
    for name, (_, args) in _lib.SIGNATURES_SPARSE_LONG_TRAIN.items():
        wrapper, sibling = SIBLINGS[name]
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == len(args), name
        assert args == _lib.SIGNATURES_SPARSE_TRAIN[sibling][1], name                                  # the sibling's argument list
        assert hasattr(_lib.load(), name) and hasattr(_lib.load("f16"), name)                          # exported by both libraries
        assert re.search(rf"def {wrapper}\(", ops_src) and f"{name}(" in ops_src and f'_timed("{name}"' in ops_src
        for tid in LEDGER[name]:
            fname, _, test = tid.partition("::")
            body = open(os.path.join(REPO, "tests", fname)).read()
            assert f"def {test}(" in body and re.search(rf"\bops\.{wrapper}\b", body), tid
    assert _lib.load().pv_version() == 10 and _lib.load("f16").pv_version() == 10                      # ABI unchanged


def check_argument_validation():
    """Every refusal below happens before a launch: the pointers are never dereferenced."""
    from peekvit_amd import _lib
    p, q, r, null, odd16, odd8, odd4 = (C.c_void_p(v) for v in (256, 1 << 30, 1 << 31, 0, 264, 260, 258))
    for op in ("bf16", "f16"):
        lib = _lib.load(op)

        def fwd(qkv=p, out=q, lse=p, seg=p, lm=p, B=4, max_len=402, H=4, dh=64, flag=null):
            return lib.pv_attention_varlen_w_stream_lse_bf16(qkv, out, lse, seg, lm, B, max_len, H, dh, flag, null)
        for k in ("qkv", "out", "lse", "seg", "lm"):
            assert fwd(**{k: null}) == -1, k
        assert fwd(B=0) == -1 and fwd(H=0) == -1 and fwd(max_len=0) == -1
        assert fwd(qkv=odd16) == -1 and fwd(out=odd8) == -1 and fwd(lse=odd4) == -1 and fwd(lm=odd4) == -1 and fwd(seg=odd4) == -1 and fwd(flag=odd4) == -1
        assert fwd(dh=32) == -2 and fwd(dh=128) == -2 and fwd(max_len=4097) == -2
        assert fwd(B=1 << 31, H=2) == -2 and fwd(B=1 << 25, max_len=4096) == -2                        # grid above 2^31 - 1

        def bwd(qkv=p, dout=p, out=p, lse=p, seg=p, lm=p, g=q, part=p, delta=p, B=4, max_len=402, H=4, dh=64):
            return lib.pv_attention_varlen_w_stream_bwd16_bf16(qkv, dout, out, lse, seg, lm, g, part, delta, B, max_len, H, dh, 0.125, null)
        for k in ("qkv", "dout", "out", "lse", "seg", "lm", "g", "delta"):
            assert bwd(**{k: null}) == -1, k
        assert bwd(B=0) == -1 and bwd(H=0) == -1 and bwd(max_len=0) == -1
        for k in ("qkv", "dout", "out", "g"):
            assert bwd(**{k: odd16}) == -1, k
        for k in ("lse", "seg", "lm", "part", "delta"):
            assert bwd(**{k: odd4}) == -1, k
        assert bwd(dh=32) == -2 and bwd(max_len=4097) == -2 and bwd(B=1 << 30, H=2) == -2 and bwd(B=1 << 25, max_len=4096) == -2

        def pack(x=p, seg=p, mult=p, tok=p, B=4, N=400, D=256, wg=p, bg=p, wb=p, bb=p, temp=1.0, mrow=p, xn=q, rs=p, mn=p, lm=p, sn=p, tn=p,
                 mo=p, th=p, tot=p, g=null, b=null, ln=null, ga=p, src=p):
            return lib.pv_residual_pack_step_long_train(x, seg, mult, tok, B, N, D, wg, bg, wb, bb, temp, 0.0, mrow, xn, rs, mn, lm, sn, tn, mo, th, tot,
                                                        g, b, 1e-6, ln, ga, src, null)
        for k in ("x", "seg", "mult", "tok", "wg", "bg", "wb", "bb", "mrow", "xn", "rs", "mn", "lm", "sn", "tn", "mo", "th", "tot", "ga", "src"):
            assert pack(**{k: null}) == -1, k
        assert pack(B=0) == -1 and pack(D=0) == -1 and pack(N=-1) == -1 and pack(temp=0.0) == -1
        assert pack(xn=p) == -1                                          # in place
        assert pack(ln=p) == -1 and pack(ln=p, g=p) == -1                # LayerNorm output without its affine
        assert pack(D=770) == -2 and pack(D=8192) == -2 and pack(N=4095) == -2 and pack(B=1 << 31) == -2
        assert pack(x=odd8) == -2 and pack(xn=C.c_void_p((1 << 30) + 8)) == -2 and pack(wg=odd16) == -2
        assert pack(ln=C.c_void_p(516), g=p, b=p) == -2 and pack(ln=p, g=odd8, b=p) == -2

        def pbwd(x=p, seg=p, tok=p, mrow=p, ga=p, thr=p, sn=p, src=p, g=q, drs=p, dm=p, B=4, N=400, D=256, wg=p, wb=p, temp=1.0, dx=r, dmr=p, dwg=p,
                 dwb=p, scal=p):
            return lib.pv_residual_pack_step_long_bwd(x, seg, tok, mrow, ga, thr, sn, src, g, drs, dm, B, N, D, wg, wb, temp, dx, dmr, dwg, dwb, scal, null)
        for k in ("x", "seg", "tok", "mrow", "ga", "thr", "sn", "src", "g", "drs", "wg", "wb", "dx", "dmr", "dwg", "dwb", "scal"):
            assert pbwd(**{k: null}) == -1, k                                    # a null pointer (dm alone may be null)
        assert pbwd(B=0) == -1 and pbwd(D=0) == -1 and pbwd(N=-1) == -1 and pbwd(temp=0.0) == -1
        for k in ("x", "g", "dx", "wg", "wb", "dwg", "dwb", "scal"):
            assert pbwd(**{k: odd16}) == -1, k                                   # a misaligned pointer
        assert pbwd(dx=p) == -1 and pbwd(dx=q) == -1                             # in place
        assert pbwd(N=4095) == -2 and pbwd(D=770) == -2 and pbwd(D=8192) == -2 and pbwd(B=1 << 31) == -2
        # the entry points of peekvit_hip_sparse_train.h keep their limit
        assert lib.pv_attention_varlen_w_lse_bf16(p, q, p, p, p, 4, 209, 4, 64, null, null) == -2
        assert lib.pv_attention_varlen_w_bwd16_bf16(p, p, p, p, p, p, q, p, p, 4, 209, 4, 64, 0.125, null) == -2


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    check_argument_validation()


# ---- 4. the public switch on the CPU at 402 rows ----
def test_a_cpu_step_past_208_rows_with_the_switch_on_is_the_dense_path():
    from peekvit_amd import engine
    torch.set_num_threads(min(8, torch.get_num_threads()))
    cfg, m, x, y, _ = build("first_streams")
    assert m.seq_length + 1 == 402
    off = host.dense_step(m, x, y)
    m.set_compact_training(True)
    n0, r0, l0 = engine.sparse_train_dense_forwards, engine.sparse_rows, engine.sparse_train_long_layers
    on = host.dense_step(m, x, y)
    assert engine.sparse_train_dense_forwards == n0 + 1 and engine.sparse_rows == r0 and engine.sparse_train_long_layers == l0
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    assert all(torch.equal(on[3][k], off[3][k]) for k in on[3] if on[3][k] is not None) and any(g is not None for g in on[3].values())
