"""The point-cloud encoder block's training kernels without a GPU: a test ledger for include/peekvit_hip_pct_block.h, the argument checks of its two
entry points (every refusal comes before a launch), where their kernels live, and the fused-block switch of the point-cloud models on CPU tensors
(off by default, no state-dict key, the composite bit for bit)."""
import ast
import ctypes as C
import os
import re

import torch

from conftest import REPO
from peekvit_amd import synth

HEADER = os.path.join(REPO, "include", "peekvit_hip_pct_block.h")
REFUSAL = "test_pct_block_host.py::test_entry_points_refuse_bad_arguments_without_a_gpu"

# ---- include/peekvit_hip_pct_block.h: every declared entry point is exported and has a test that calls it directly ----
LEDGER = {
    "pv_layernorm_bwd_sum": ["test_hip_pct_block.py::test_layernorm_backward_of_a_sum", REFUSAL],
    "pv_attention_stream_bwd16_bf16": ["test_hip_pct_block.py::test_stream_backward_in_16_bits_with_bias_partials", REFUSAL],
}
WRAPPERS = {"pv_layernorm_bwd_sum": "layernorm_bwd_sum", "pv_attention_stream_bwd16_bf16": "attention_stream_bwd16"}


def _declared():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pv_\w+)\s*\(", src, flags=re.M))


def _arity(name):
    m = re.search(r"\b(?:int|int64_t) " + name + r"\(([^;]*)\);", open(HEADER).read())
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_pct_block_ledger_names_a_direct_test_for_every_declared_entry_point():
    from peekvit_amd import _build, _lib
    assert "peekvit_hip_pct_block.h" in _build.HEADERS
    declared = _declared()
    assert set(LEDGER) == declared == set(_lib.SIGNATURES_PCT_BLOCK), declared ^ set(LEDGER)
    others = (_lib.SIGNATURES, _lib.SIGNATURES_MOE, _lib.SIGNATURES_EE, _lib.SIGNATURES_SPARSE, _lib.SIGNATURES_PCT, _lib.SIGNATURES_PCT_TRAIN,
              _lib.SIGNATURES_ATTN_STREAM)
    assert not any(set(_lib.SIGNATURES_PCT_BLOCK) & set(d) for d in others)               # a dict of their own
    for name, (_, args) in _lib.SIGNATURES_PCT_BLOCK.items():
        assert _arity(name) == len(args), name
        assert hasattr(_lib.load(), name) and hasattr(_lib.load("f16"), name)            # exported by both libraries
    assert _lib.load().pv_version() == 10 and _lib.load("f16").pv_version() == 10        # ABI unchanged
    ops_src = open(os.path.join(REPO, "peekvit_amd", "ops.py")).read()
    wrappers = {}
    for node in ast.parse(ops_src).body:
        if isinstance(node, ast.FunctionDef):
            for sym in re.findall(r"\b(pv_\w+)\(", ast.get_source_segment(ops_src, node)):
                wrappers.setdefault(sym, set()).add(node.name)
    assert all(wrappers.get(sym) == {w} for sym, w in WRAPPERS.items()), {s: wrappers.get(s) for s in WRAPPERS}

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
    """Call, do not copy: each entry point sits in the source of the kernel it instantiates, under that source's flags, and no
    second LayerNorm-backward or streaming-backward kernel exists."""
    from peekvit_amd import _build
    rowops = open(os.path.join(_build.CSRC, "pv_rowops.hip")).read()
    stream = open(os.path.join(_build.CSRC, "pv_attention_stream.hip")).read()
    assert 'extern "C" int pv_layernorm_bwd_sum(' in rowops and "pv_layernorm_bwd_kernel<N, false, true>" in rowops
    assert 'extern "C" int pv_attention_stream_bwd16_bf16(' in stream
    # (one launcher instantiates the two kernels from its own template flags; the entry point names O16 = true where it calls it)
    assert "pv_attn_stream_dq_kernel<DH, O16, W, DROP>" in stream and "pv_attn_stream_dkv_kernel<DH, O16, W, DROP>" in stream
    assert "pv_dispatch_attn_stream_bwd<true, false, false>(" in stream
    for f in sorted(os.listdir(_build.CSRC)):
        text = open(os.path.join(_build.CSRC, f)).read()
        assert len(re.findall(r"__global__[^;{]*\bpv_layernorm_bwd_kernel\(", text)) == (1 if f == "pv_rowops.hip" else 0), f
        assert len(re.findall(r"__global__[^;{]*\bpv_attn_stream_d(?:q|kv)_kernel\(", text)) == (2 if f == "pv_attention_stream.hip" else 0), f
    assert _build.FILE_FLAGS["pv_rowops.hip"] == ["-fno-slp-vectorize"]
    assert _build.FILE_FLAGS["pv_attention_stream.hip"] == ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from peekvit_amd import _lib
    p, q, null = C.c_void_p(256), C.c_void_p(1 << 30), C.c_void_p(0)       # never dereferenced: every call below is refused before a launch
    odd16, odd8, odd4 = C.c_void_p(264), C.c_void_p(260), C.c_void_p(258)  # off a 16-byte / an 8-byte / a 4-byte boundary
    for op in ("bf16", "f16"):
        lib = _lib.load(op)

        def ln(x=p, dy16=p, dy32=p, gamma=p, dx_out=q, dx16=q, dgb=q, ws=q, ws_floats=3 * 128 * 2, rows=5, D=128, accumulate=0):
            return lib.pv_layernorm_bwd_sum(x, dy16, dy32, gamma, dx_out, dx16, dgb, ws, ws_floats, rows, D, 1e-6, accumulate, null)

        for name in ("x", "gamma", "dgb", "ws"):
            assert ln(**{name: null}) == -1, name                                                 # nulls
        assert ln(dy16=null, dy32=null) == -1 and ln(dx_out=null, dx16=null) == -1                # ... both terms, both results
        for name in ("x", "dy32", "gamma", "dx_out", "dgb", "ws"):
            assert ln(**{name: odd16}) == -1 and ln(**{name: odd4}) == -1, name                   # fp32 arrays: 16-byte aligned
        for name in ("dy16", "dx16"):
            assert ln(**{name: odd8}) == -1 and ln(**{name: odd4}) == -1, name                    # 16-bit rows: 8-byte aligned
        for dim in ("rows", "D"):
            assert ln(**{dim: 0}) == -1 and ln(**{dim: -4}) == -1, dim                            # sizes < 1
        assert ln(D=126) == -2 and ln(D=1028, ws_floats=1 << 20) == -2 and ln(D=2048, ws_floats=1 << 20) == -2        # D % 4, D > 1024
        assert ln(ws_floats=3 * 128 * 2 - 1) == -1 and ln(ws_floats=0) == -1                      # ceil(5 / 4) = 2 partial rows of 3 D floats
        assert ln(rows=1 << 20, ws_floats=1024 * 3 * 128 - 1) == -1                               # ... 1024 at the most

        def bwd(qkv=p, dout=p, out=p, lse=p, dqkv16=q, dbias=q, delta=q, B=2, S=65, H=2, dh=32):
            return lib.pv_attention_stream_bwd16_bf16(qkv, dout, out, lse, dqkv16, dbias, delta, B, S, H, dh, 1.0, null)

        for name in ("qkv", "dout", "out", "lse", "dqkv16", "delta"):
            assert bwd(**{name: null}) == -1, name                                                # nulls (dbias may be null)
            assert bwd(**{name: odd4}) == -1, name                                                # misaligned for either element size
            if name not in ("lse", "delta"):
                assert bwd(**{name: odd16}) == -1, name                                           # 16-bit arrays: 16-byte aligned
        assert bwd(dbias=odd4) == -1
        for dim in ("B", "S", "H"):
            assert bwd(**{dim: 0}) == -1 and bwd(**{dim: -1}) == -1, dim                          # sizes < 1
        for dh in (16, 40, 80, 96, 128, 33):
            assert bwd(dh=dh) == -2, dh                                                           # dh outside {32, 48, 64}
        assert bwd(dh=0) == -1 and bwd(dh=-32) == -1
        assert bwd(B=1 << 31) == -2 and bwd(B=1 << 20, H=1 << 11) == -2                           # B * H * ceil(S / 64) workgroups against 2^31
        assert bwd(B=1 << 16, H=1 << 10, S=64 * 32 + 1) == -2 and bwd(S=1 << 31) == -2


def _tiny(cls=None, seed=0, **extra):
    from peekvit_amd.models.pct import PointCloudTransformer
    torch.manual_seed(seed)
    return (cls or PointCloudTransformer)(num_points=32, num_layers=2, num_heads=2, hidden_dim=64, mlp_dim=128, num_classes=5, **extra).train()


def test_fused_block_switch_is_off_by_default_and_adds_no_state():
    from peekvit_amd.models.pct import PointCloudTransformer, RankPointCloudTransformer
    for cls in (PointCloudTransformer, RankPointCloudTransformer):
        m = _tiny(cls)
        assert [blk.fused_block for blk in m.encoder.layers] == [False, False]
        keys, nparam, nbuf = list(m.state_dict()), len(list(m.parameters())), len(list(m.buffers()))
        m.set_fused_blocks()
        assert [blk.fused_block for blk in m.encoder.layers] == [True, True]
        assert [blk.fused_attention for blk in m.encoder.layers] == [False, False]                # a switch of its own
        assert list(m.state_dict()) == keys and len(list(m.parameters())) == nparam and len(list(m.buffers())) == nbuf
        m.set_fused_blocks(False)
        assert [blk.fused_block for blk in m.encoder.layers] == [False, False]


def test_cpu_tensors_run_the_composite_bit_for_bit_with_the_switch_on():
    from peekvit_amd import ops, pct_train
    from peekvit_amd.models.pct import PointCloudTransformer, RankPointCloudTransformer
    x = torch.from_numpy(synth.synth_points(3, 32, 1))
    for cls in (PointCloudTransformer, RankPointCloudTransformer):
        results = []
        for on in (False, True):
            m = _tiny(cls)
            if on:
                m.set_fused_blocks(True)
                assert not pct_train.block_eligible(m.encoder.layers[0], torch.zeros(3, 32, 64))
            n0, b0, l0 = pct_train.block_passes, pct_train.block_backwards, ops.launch_count
            loss = m(x).square().sum()
            loss.backward()
            assert (pct_train.block_passes, pct_train.block_backwards, ops.launch_count) == (n0, b0, l0)
            results.append((loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
        (l_off, g_off), (l_on, g_on) = results
        assert torch.equal(l_off, l_on) and set(g_off) == set(g_on) and all(torch.equal(g_off[n], g_on[n]) for n in g_off)


def test_saved_bytes_formula():
    from peekvit_amd import pct_train
    assert pct_train.block_saved_bytes_per_row(128, 4, 256) == 20 * 128 + 4 * 256 + 4 * 4
