"""A sorting point-cloud block's training kernels without a GPU: a test ledger for include/peekvit_hip_rank_train.h, the argument checks of its entry
points (every refusal comes before a launch), where their kernels live, the fused-ranking switch of RankPointCloudTransformer on CPU tensors (off by
default, no state-dict key, the composite bit for bit) and - in fp64 on stock ops - the equivalence of the compact restatement the kernels run (live
rows plus one weighted tail row) with RankingPCTBlock itself."""
import ast
import ctypes as C
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import REPO
from peekvit_amd import synth

HEADER = os.path.join(REPO, "include", "peekvit_hip_rank_train.h")
REFUSAL = "test_rank_train_host.py::test_entry_points_refuse_bad_arguments_without_a_gpu"

# ---- include/peekvit_hip_rank_train.h: every declared entry point is exported and has a test that calls it directly ----
LEDGER = {
    "pv_rank_pack_f32": ["test_hip_rank_train.py::test_pack_expand_unpack_against_index_ops", REFUSAL],
    "pv_rank_expand_f32": ["test_hip_rank_train.py::test_pack_expand_unpack_against_index_ops", REFUSAL],
    "pv_rank_unpack_grad_f32": ["test_hip_rank_train.py::test_pack_expand_unpack_against_index_ops", REFUSAL],
    "pv_rank_reduce_f32": ["test_hip_rank_train.py::test_reduce_copies_the_live_rows_and_sums_the_tail_in_a_fixed_order", REFUSAL],
    "pv_layernorm_f32_bf16_masked": ["test_hip_rank_train.py::test_masked_layernorm_forward", REFUSAL],
    "pv_layernorm_bwd_sum_masked": ["test_hip_rank_train.py::test_masked_layernorm_backward_of_a_sum", REFUSAL],
    "pv_attention_stream_lse_w_bf16": ["test_hip_rank_train.py::test_weighted_stream_attention", REFUSAL],
    "pv_attention_stream_bwd16_w_bf16": ["test_hip_rank_train.py::test_weighted_stream_attention", REFUSAL],
}
WRAPPERS = {"pv_rank_pack_f32": "rank_pack", "pv_rank_expand_f32": "rank_expand", "pv_rank_unpack_grad_f32": "rank_unpack_grad",
            "pv_rank_reduce_f32": "rank_reduce", "pv_layernorm_f32_bf16_masked": "layernorm_f32_bf16_masked",
            "pv_layernorm_bwd_sum_masked": "layernorm_bwd_sum_masked", "pv_attention_stream_lse_w_bf16": "attention_stream_w",
            "pv_attention_stream_bwd16_w_bf16": "attention_stream_bwd16_w"}


def _declared():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pv_\w+)\s*\(", src, flags=re.M))


def _arity(name):
    m = re.search(r"\b(?:int|int64_t) " + name + r"\(([^;]*)\);", open(HEADER).read())
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_rank_train_ledger_names_a_direct_test_for_every_declared_entry_point():
    from peekvit_amd import _build, _lib
    assert "peekvit_hip_rank_train.h" in _build.HEADERS
    declared = _declared()
    assert set(LEDGER) == declared == set(_lib.SIGNATURES_RANK_TRAIN) == set(WRAPPERS), declared ^ set(LEDGER)
    others = (_lib.SIGNATURES, _lib.SIGNATURES_MOE, _lib.SIGNATURES_EE, _lib.SIGNATURES_SPARSE, _lib.SIGNATURES_PCT, _lib.SIGNATURES_PCT_TRAIN,
              _lib.SIGNATURES_ATTN_STREAM, _lib.SIGNATURES_PCT_BLOCK)
    assert not any(set(_lib.SIGNATURES_RANK_TRAIN) & set(d) for d in others)              # a dict of their own
    for name, (_, args) in _lib.SIGNATURES_RANK_TRAIN.items():
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

    def reaches(entry, name, funcs, src, seen):
        if name in seen or name not in funcs:
            return False
        seen.add(name)
        body = ast.get_source_segment(src, funcs[name])
        if re.search(rf"\b{entry}\(", body) or re.search(rf"\bops\.{WRAPPERS[entry]}\(", body):
            return True
        called = {n.func.id for n in ast.walk(funcs[name]) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name)}
        return any(reaches(entry, c, funcs, src, seen) for c in called if c.startswith("_"))

    for entry, ids in LEDGER.items():
        for tid in ids:
            fname, _, name = tid.partition("::")
            src = open(os.path.join(REPO, "tests", fname)).read()
            funcs = {n.name: n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef)}
            assert name.startswith("test_") and name in funcs, f"{entry}: {tid} is not a test of {fname}"
            assert reaches(entry, name, funcs, src, set()), f"{tid} never calls {entry}"


def test_the_new_entry_points_instantiate_the_existing_kernels():
    """Call, do not copy: each of the four derived entry points sits in the source of the kernel it instantiates (the streaming
    forward is launched from pv_attention.hip, where its kernel is, as pv_attention_stream_lse_bf16's is), under that source's flags; no second
    LayerNorm or streaming-attention kernel exists; the row movers have a source of their own built from pv_rows.h's pieces."""
    from peekvit_amd import _build
    read = lambda f: open(os.path.join(_build.CSRC, f)).read()
    rowops, pct, stream, attn, rank = (read(f) for f in ("pv_rowops.hip", "pv_pct.hip", "pv_attention_stream.hip", "pv_attention.hip", "pv_rank_train.hip"))
    assert 'extern "C" int pv_layernorm_bwd_sum_masked(' in rowops and "pv_layernorm_bwd_kernel<N, false, true, true>" in rowops
    assert "pv_layernorm_bwd_kernel<N, false, true>" in rowops                          # (the unmasked instantiation is where it was)
    assert 'extern "C" int pv_layernorm_f32_bf16_masked(' in pct and "pv_layernorm_f32_bf16_kernel<N_, true>" in pct
    assert 'extern "C" int pv_attention_stream_lse_w_bf16(' in stream and 'extern "C" int pv_attention_stream_bwd16_w_bf16(' in stream
    # (one launcher per direction instantiates the kernels from its own template flags; the entry points name the flags where they call it)
    assert "pv_attn_stream_dq_kernel<DH, O16, W, DROP>" in stream and "pv_attn_stream_dkv_kernel<DH, O16, W, DROP>" in stream
    assert "pv_dispatch_attn_stream_bwd<true, true, false>(" in stream                # the W instantiations
    assert "pv_dispatch_attn_stream_bwd<true, false, false>(" in stream               # (the unweighted O16 instantiations are where they were)
    assert "pv_attn_stream_kernel<DH, LSE, W, DROP>" in attn and "pv_dispatch_attn_stream_lse<true, false>(" in attn
    assert "pv_launch_attn_stream_lse_w(" in stream
    for f in sorted(os.listdir(_build.CSRC)):
        text = read(f)
        assert len(re.findall(r"__global__[^;{]*\bpv_layernorm_bwd_kernel\(", text)) == (1 if f == "pv_rowops.hip" else 0), f
        assert len(re.findall(r"__global__[^;{]*\bpv_layernorm_f32_bf16_kernel\(", text)) == (1 if f == "pv_pct.hip" else 0), f
        assert len(re.findall(r"__global__[^;{]*\bpv_attn_stream_d(?:q|kv)_kernel\(", text)) == (2 if f == "pv_attention_stream.hip" else 0), f
        assert len(re.findall(r"__global__[^;{]*\bpv_attn_stream_kernel\(", text)) == (1 if f == "pv_attention.hip" else 0), f
        assert len(re.findall(r'extern "C" int pv_rank_(?:pack|expand|reduce|unpack_grad)_f32\(', text)) == (4 if f == "pv_rank_train.hip" else 0), f
    assert '#include "pv_rows.h"' in rank and all(piece in rank for piece in ("RowRegs<NCH>", "pv_load_row<NCH>", "pv_store_row<NCH>"))
    assert "atomic" not in rank.replace("no atomics", "")
    assert _build.FILE_FLAGS["pv_rank_train.hip"] == ["-fno-slp-vectorize"] == _build.FILE_FLAGS["pv_rowops.hip"] == _build.FILE_FLAGS["pv_pct.hip"]
    assert _build.FILE_FLAGS["pv_attention_stream.hip"] == ["-mllvm", "-amdgpu-mfma-vgpr-form=1"] == _build.FILE_FLAGS["pv_attention.hip"]


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from peekvit_amd import _lib
    p, q, null = C.c_void_p(256), C.c_void_p(1 << 30), C.c_void_p(0)       # never dereferenced: every call below is refused before a launch
    odd16, odd8, odd4 = C.c_void_p(264), C.c_void_p(260), C.c_void_p(258)  # off a 16-byte / an 8-byte / a 4-byte boundary
    inf, nan = float("inf"), float("nan")
    for op in ("bf16", "f16"):
        lib = _lib.load(op)

        # ---- the row movers ----
        def pack(fn, a=p, keep=p, b=q, B=2, S=13, k=5, D=64):
            return fn(a, keep, b, B, S, k, D, null)

        def tail(fn, a=p, b=q, B=2, S=13, L=6, D=64):
            return fn(a, b, B, S, L, D, null)

        for fn in (lambda *args: lib.pv_rank_pack_f32(*args), lambda *args: lib.pv_rank_unpack_grad_f32(*args)):
            for name in ("a", "keep", "b"):
                assert pack(fn, **{name: null}) == -1, name                                       # nulls
                assert pack(fn, **{name: odd4}) == -1, name                                       # misaligned for either element size
            assert pack(fn, a=odd16) == -1 and pack(fn, b=odd16) == -1 and pack(fn, a=odd8) == -1 # fp32 arrays: 16-byte aligned
            for dim in ("B", "S", "k", "D"):
                assert pack(fn, **{dim: 0}) == -1 and pack(fn, **{dim: -4}) == -1, dim            # sizes < 1
            assert pack(fn, S=1, k=1) == -1                                                       # no row to rank
            assert pack(fn, k=13) == -1 and pack(fn, k=100) == -1 and pack(fn, S=2, k=2) == -1    # k > S - 1
            assert pack(fn, D=62) == -2 and pack(fn, D=1028) == -2 and pack(fn, D=2048) == -2     # D % 4, D > 1024
            assert pack(fn, S=4098, k=7) == -2 and pack(fn, B=1 << 16) == -2                      # S - 1 > 4096, B > 65535
        for fn in (lambda *args: lib.pv_rank_expand_f32(*args), lambda *args: lib.pv_rank_reduce_f32(*args)):
            for name in ("a", "b"):
                assert tail(fn, **{name: null}) == -1, name
                assert tail(fn, **{name: odd16}) == -1 and tail(fn, **{name: odd8}) == -1 and tail(fn, **{name: odd4}) == -1, name
            for dim in ("B", "S", "L", "D"):
                assert tail(fn, **{dim: 0}) == -1 and tail(fn, **{dim: -4}) == -1, dim
            assert tail(fn, L=13) == -1 and tail(fn, L=14) == -1 and tail(fn, S=2, L=2) == -1     # L >= S: no masked row, nothing to expand or reduce
            assert tail(fn, D=62) == -2 and tail(fn, D=1028) == -2 and tail(fn, D=2048) == -2
            assert tail(fn, S=4098) == -2 and tail(fn, B=1 << 16) == -2

        # ---- the masked LayerNorms ----
        def lnf(x=p, gamma=p, beta=p, row_scale=p, out16=q, out32=q, rows=5, D=128):
            return lib.pv_layernorm_f32_bf16_masked(x, gamma, beta, row_scale, out16, out32, rows, D, 1e-6, null)

        for name in ("x", "gamma", "beta", "row_scale", "out16", "out32"):
            assert lnf(**{name: null}) == -1, name
            assert lnf(**{name: odd4}) == -1, name
        for name in ("x", "gamma", "beta", "out32"):
            assert lnf(**{name: odd16}) == -1 and lnf(**{name: odd8}) == -1, name                 # fp32 arrays: 16-byte aligned
        assert lnf(out16=odd8) == -1                                                              # 16-bit rows: 8-byte aligned
        for dim in ("rows", "D"):
            assert lnf(**{dim: 0}) == -1 and lnf(**{dim: -4}) == -1, dim
        assert lnf(D=126) == -2 and lnf(D=1028) == -2 and lnf(D=2048) == -2
        assert lnf(out32=p) == -1                                                                 # the fp32 rows on the rows being read

        def lnb(x=p, dy16=p, dy32=p, gamma=p, row_scale=p, dx_out=q, dx16=q, dgb=q, ws=q, ws_floats=3 * 128 * 2, rows=5, D=128, accumulate=0):
            return lib.pv_layernorm_bwd_sum_masked(x, dy16, dy32, gamma, row_scale, dx_out, dx16, dgb, ws, ws_floats, rows, D, 1e-6, accumulate, null)

        for name in ("x", "gamma", "row_scale", "dgb", "ws"):
            assert lnb(**{name: null}) == -1, name
        assert lnb(dy16=null, dy32=null) == -1 and lnb(dx_out=null, dx16=null) == -1
        for name in ("x", "dy32", "gamma", "dx_out", "dgb", "ws"):
            assert lnb(**{name: odd16}) == -1 and lnb(**{name: odd4}) == -1, name
        for name in ("dy16", "dx16"):
            assert lnb(**{name: odd8}) == -1 and lnb(**{name: odd4}) == -1, name
        assert lnb(row_scale=odd4) == -1
        for dim in ("rows", "D"):
            assert lnb(**{dim: 0}) == -1 and lnb(**{dim: -4}) == -1, dim
        assert lnb(D=126) == -2 and lnb(D=1028, ws_floats=1 << 20) == -2 and lnb(D=2048, ws_floats=1 << 20) == -2
        assert lnb(ws_floats=3 * 128 * 2 - 1) == -1 and lnb(ws_floats=0) == -1 and lnb(rows=1 << 20, ws_floats=1024 * 3 * 128 - 1) == -1

        # ---- the weighted streaming attention ----
        def fwd(qkv=p, out=q, lse=q, flag=null, B=2, S=65, H=2, dh=32, t=0.5):
            return lib.pv_attention_stream_lse_w_bf16(qkv, out, lse, B, S, H, dh, t, flag, null)

        def bwd(qkv=p, dout=p, out=p, lse=p, dqkv16=q, dbias=q, delta=q, B=2, S=65, H=2, dh=32, t=0.5):
            return lib.pv_attention_stream_bwd16_w_bf16(qkv, dout, out, lse, dqkv16, dbias, delta, B, S, H, dh, 1.0, t, null)

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
            assert call(B=1 << 31) == -2 and call(B=1 << 20, H=1 << 11) == -2 and call(B=1 << 16, H=1 << 10, S=64 * 32 + 1) == -2 and call(S=1 << 31) == -2
            for t in (-0.5, -1e-30, inf, -inf, nan):
                assert call(t=t) == -1, t                                                         # tail_log_mult: finite and >= 0
        assert fwd(flag=odd4) == -1 and bwd(dbias=odd4) == -1


def _tiny(seed=0, **extra):
    from peekvit_amd.models.pct import RankPointCloudTransformer
    torch.manual_seed(seed)
    m = RankPointCloudTransformer(num_points=32, num_layers=2, num_heads=2, hidden_dim=64, mlp_dim=128, num_classes=5, **extra).train()
    m.enable_ranking(True)
    m.set_budget(0.5)
    return m


def test_fused_ranking_switch_is_off_by_default_and_adds_no_state():
    from peekvit_amd.models.pct import PointCloudTransformer
    m = _tiny()
    assert [blk.fused_ranking for blk in m.encoder.layers] == [False, False] and [blk.last_train_keep for blk in m.encoder.layers] == [None, None]
    keys, nparam, nbuf = list(m.state_dict()), len(list(m.parameters())), len(list(m.buffers()))
    m.set_fused_ranking()
    assert [blk.fused_ranking for blk in m.encoder.layers] == [True, True]
    assert [(blk.fused_attention, blk.fused_block) for blk in m.encoder.layers] == [(False, False)] * 2          # a switch of its own
    assert list(m.state_dict()) == keys and len(list(m.parameters())) == nparam and len(list(m.buffers())) == nbuf
    m.set_fused_ranking(False)
    assert [blk.fused_ranking for blk in m.encoder.layers] == [False, False]
    assert not hasattr(PointCloudTransformer, "set_fused_ranking")                         # the ranking model's switch


def test_cpu_tensors_run_the_composite_bit_for_bit_with_the_switch_on(monkeypatch):
    from peekvit_amd import ops, pct_train
    from peekvit_amd.models.pct import RankingPCTBlock
    x = torch.from_numpy(synth.synth_points(3, 32, 1))
    calls = []
    stock = RankingPCTBlock.sort_order
    monkeypatch.setattr(RankingPCTBlock, "sort_order", staticmethod(lambda t: (calls.append(1), stock(t))[1]))
    results = []
    for on in (False, True):
        m = _tiny()
        if on:
            m.set_fused_ranking(True)
            m.set_fused_blocks(True)
            blk = m.encoder.layers[0]
            assert not pct_train.ranked_block_eligible(blk, torch.zeros(3, 32, 64)) and not pct_train.block_eligible(blk, torch.zeros(3, 32, 64))
        n0, b0, l0, c0 = pct_train.ranked_passes, pct_train.ranked_backwards, ops.launch_count, len(calls)
        loss = m(x).square().sum()
        loss.backward()
        assert (pct_train.ranked_passes, pct_train.ranked_backwards, ops.launch_count) == (n0, b0, l0)          # zero launches
        assert len(calls) - c0 == 2                                                        # sort_order is still called once per sorting block
        assert all(blk.last_train_keep is None for blk in m.encoder.layers)
        results.append((loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
    (l_off, g_off), (l_on, g_on) = results
    assert torch.equal(l_off, l_on) and set(g_off) == set(g_on) and all(torch.equal(g_off[n], g_on[n]) for n in g_off)


def test_eligibility_shares_block_eligible_conditions():
    from peekvit_amd import pct_train
    from peekvit_amd.models.pct import PCTBlock, RankingPCTBlock
    assert pct_train.RANK_MAX_N == 4096
    blk = RankingPCTBlock(num_heads=2, hidden_dim=64, mlp_dim=128, dropout=0.0, attention_dropout=0.0).train()
    blk.sort, blk.fused_ranking, blk.fused_block = True, True, True
    x = torch.zeros(2, 9, 64)
    assert not pct_train.ranked_block_eligible(blk, x) and not pct_train.block_eligible(blk, x)          # CPU tensors
    assert not pct_train.ranked_block_eligible(PCTBlock(2, 64, 128, 0.0, 0.0), x)                        # not a ranking block
    for S, budget, keep in ((9, 0.5, 4), (9, 1.0, 8), (9, 2.0, 8), (9, 0.01, 1), (9, 0.0, 0), (130, 0.5, 65), (2, 0.5, 1)):
        blk.set_budget(budget)
        assert pct_train.ranked_keep(blk, S) == keep, (S, budget)
        assert pct_train.ranked_keep(blk, S) == min(S - 1, int(blk.mask_tokens(torch.ones(1, S, 1))[0, 1:, 0].sum()))          # mask_tokens' own count
    assert pct_train.block_saved_bytes_per_row(128, 4, 256) == 20 * 128 + 4 * 256 + 4 * 4


# ---- the compact restatement, in fp64 on stock ops ---------------------------------------------------------------------------------------
def _compact_block(blk, x):
    """RankingPCTBlock.forward (train, sort on) restated as the kernels run it: L = 1 + keep live rows plus ONE tail row per image that stands for the m
    masked ones - its x is 0, both its LayerNorm outputs are masked, its key gets + ln m on its score - and whose output is broadcast to rows L .. S - 1
    (autograd's transpose of that broadcast is the sum of dout over those rows)."""
    B, S, D = x.shape
    keep = min(S - 1, math.ceil((S - 1) * blk.current_budget))
    L, m = 1 + keep, S - 1 - keep
    order = torch.argsort(torch.norm(x[:, 1:], dim=-1), dim=-1, descending=True, stable=True)[:, :keep] + 1
    rows = torch.cat([torch.zeros_like(order[:, :1]), order], dim=1)
    xc = torch.gather(x, 1, rows[:, :, None].expand(-1, -1, D))
    scale = torch.ones(L + (1 if m else 0), 1, dtype=x.dtype)
    if m:
        xc = torch.cat([xc, torch.zeros(B, 1, D, dtype=x.dtype)], dim=1)
        scale[L] = 0.0
    mha = blk.self_attention.self_attention
    H, dh = mha.num_heads, D // mha.num_heads
    u = blk.ln_1(xc) * scale
    q, k, v = (t.reshape(B, -1, H, dh).transpose(1, 2) for t in F.linear(u, mha.in_proj_weight, mha.in_proj_bias).split(D, dim=-1))
    s = (q * dh ** -0.5) @ k.transpose(-1, -2)
    if m:
        bias = torch.zeros(L + 1, dtype=x.dtype)
        bias[L] = math.log(m)
        s = s + bias
    att = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, -1, D)
    vv = F.linear(att, mha.out_proj.weight, mha.out_proj.bias) + u
    yc = blk.mlp(blk.ln_2(vv) * scale) + vv
    return torch.cat([yc[:, :L], yc[:, L:].expand(-1, m, -1)], dim=1) if m else yc


@pytest.mark.parametrize("budget,m", [(1.0, 0), (0.9, 1), (0.5, 6), (0.05, 11)])
def test_compact_restatement_is_the_ranking_block_in_fp64(budget, m):
    from peekvit_amd.models.pct import RankingPCTBlock
    torch.manual_seed(7)
    B, S, D = 3, 13, 64
    blk = RankingPCTBlock(num_heads=2, hidden_dim=D, mlp_dim=96, dropout=0.0, attention_dropout=0.0).double().train()
    with torch.no_grad():
        for p in blk.parameters():
            p.add_(torch.randn_like(p) * 0.05)                     # biases and LayerNorm parameters away from 0 and 1
    blk.sort = True
    blk.set_budget(budget)
    assert S - 1 - math.ceil((S - 1) * budget) == m
    x = torch.randn(B, S, D, dtype=torch.float64)
    g = torch.randn(B, S, D, dtype=torch.float64)
    results = []
    for fn in (blk, lambda t: _compact_block(blk, t)):
        xg = x.clone().requires_grad_(True)
        out = fn(xg)
        results.append((out.detach(), torch.autograd.grad(out, [xg] + list(blk.parameters()), g)))
    (o_ref, g_ref), (o_c, g_c) = results
    names = ["x"] + [n for n, _ in blk.named_parameters()]
    worst = max([float((o_ref - o_c).abs().max())] + [float((a - b).abs().max() / a.abs().max().clamp_min(1e-300)) for a, b in zip(g_ref, g_c)])
    print(f"compact restatement, budget {budget} (m = {m}): worst |difference| of out / relative to each gradient's maximum {worst:.3g}")
    assert o_ref.shape == o_c.shape == (B, S, D)
    assert float((o_ref - o_c).abs().max()) <= 1e-12
    for n, a, b in zip(names, g_ref, g_c):
        assert float((a - b).abs().max()) <= 1e-12, n              # exact arithmetic up to summation order
