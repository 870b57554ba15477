"""Streaming attention for training without a GPU: a test ledger for include/peekvit_hip_attn_stream.h, the argument checks of its entry points
(every refusal comes before a launch), the build flags of its source, and the fused-attention switch of the point-cloud models on CPU tensors
(off by default, no state-dict key, the composite bit for bit)."""
import ast
import ctypes as C
import os
import re

import torch

from conftest import REPO
from peekvit_amd import synth

HEADER = os.path.join(REPO, "include", "peekvit_hip_attn_stream.h")
REFUSAL = "test_attn_stream_host.py::test_entry_points_refuse_bad_arguments_without_a_gpu"

# ---- include/peekvit_hip_attn_stream.h: every declared entry point is exported and has a test that calls it directly ----
LEDGER = {
    "pv_attention_stream_lse_bf16": ["test_hip_attn_stream.py::test_stream_forward_with_row_statistics", REFUSAL],
    "pv_attention_stream_bwd_bf16": ["test_hip_attn_stream.py::test_stream_backward_against_fp64", REFUSAL],
}


def _declared():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pv_\w+)\s*\(", src, flags=re.M))


def _arity(name):
    m = re.search(r"\b(?:int|int64_t) " + name + r"\(([^;]*)\);", open(HEADER).read())
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_attn_stream_ledger_names_a_direct_test_for_every_declared_entry_point():
    from peekvit_amd import _build, _lib
    assert "peekvit_hip_attn_stream.h" in _build.HEADERS
    declared = _declared()
    assert set(LEDGER) == declared == set(_lib.SIGNATURES_ATTN_STREAM), declared ^ set(LEDGER)
    others = (_lib.SIGNATURES, _lib.SIGNATURES_MOE, _lib.SIGNATURES_EE, _lib.SIGNATURES_SPARSE, _lib.SIGNATURES_PCT, _lib.SIGNATURES_PCT_TRAIN)
    assert not any(set(_lib.SIGNATURES_ATTN_STREAM) & set(d) for d in others)             # a dict of their own
    for name, (_, args) in _lib.SIGNATURES_ATTN_STREAM.items():
        assert _arity(name) == len(args), name
        assert hasattr(_lib.load(), name) and hasattr(_lib.load("f16"), name)            # exported by both libraries
    assert _lib.load().pv_version() == 10 and _lib.load("f16").pv_version() == 10        # ABI unchanged
    ops_src = open(os.path.join(REPO, "peekvit_amd", "ops.py")).read()
    wrappers = {}
    for node in ast.parse(ops_src).body:
        if isinstance(node, ast.FunctionDef):
            for sym in re.findall(r"\b(pv_\w+)\(", ast.get_source_segment(ops_src, node)):
                wrappers.setdefault(sym, set()).add(node.name)
    assert wrappers.get("pv_attention_stream_lse_bf16") == {"attention_stream"} and wrappers.get("pv_attention_stream_bwd_bf16") == {"attention_stream_bwd"}

    def reaches(entry, name, funcs, src, seen):
        if name in seen or name not in funcs:
            return False
        seen.add(name)
        body = ast.get_source_segment(src, funcs[name])
        if re.search(rf"\b{entry}\(", body) or any(re.search(rf"\bops\.{w}\(", body) for w in wrappers.get(entry, ())):
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


def test_build_flags_of_the_streaming_source():
    from peekvit_amd import _build
    assert _build.FILE_FLAGS["pv_attention_stream.hip"] == _build.FILE_FLAGS["pv_attention.hip"] == ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]
    assert os.path.join(_build.CSRC, "pv_attention_stream.hip") in _build.sources()
    # call, do not copy: the helpers both attention sources use are defined once, in the header both include
    texts = {f: open(os.path.join(_build.CSRC, f)).read() for f in ("pv_attention.hip", "pv_attention_stream.hip", "pv_attn.h")}
    for f in ("pv_attention.hip", "pv_attention_stream.hip"):
        assert '#include "pv_attn.h"' in texts[f] and "int pv_swz(" not in texts[f] and "#define PV_P_SHIFT" not in texts[f]
    assert "int pv_swz(" in texts["pv_attn.h"] and "#define PV_P_SHIFT" in texts["pv_attn.h"]


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from peekvit_amd import _lib
    p, q, null = C.c_void_p(256), C.c_void_p(1 << 30), C.c_void_p(0)       # never dereferenced: every call below is refused before a launch
    odd16, odd4 = C.c_void_p(264), C.c_void_p(258)                         # off a 16-byte boundary / off a 4-byte boundary
    for op in ("bf16", "f16"):
        lib = _lib.load(op)

        def fwd(qkv=p, out=q, lse=q, flag=null, B=2, S=65, H=2, dh=32):
            return lib.pv_attention_stream_lse_bf16(qkv, out, lse, B, S, H, dh, flag, null)

        def bwd(qkv=p, dout=p, out=p, lse=p, dqkv=q, delta=q, B=2, S=65, H=2, dh=32):
            return lib.pv_attention_stream_bwd_bf16(qkv, dout, out, lse, dqkv, delta, B, S, H, dh, 1.0, null)

        pointers = {fwd: ("qkv", "out", "lse"), bwd: ("qkv", "dout", "out", "lse", "dqkv", "delta")}
        for fn, names in pointers.items():
            for name in names:
                assert fn(**{name: null}) == -1, (fn.__name__, name)                              # nulls
                assert fn(**{name: odd4}) == -1, (fn.__name__, name)                              # misaligned for either element size
                if name not in ("lse", "delta"):
                    assert fn(**{name: odd16}) == -1, (fn.__name__, name)                         # 16-bit rows and dqkv: 16-byte aligned
            for dim in ("B", "S", "H"):
                assert fn(**{dim: 0}) == -1 and fn(**{dim: -1}) == -1, (fn.__name__, dim)          # sizes < 1
            for dh in (16, 40, 80, 96, 128, 33):
                assert fn(dh=dh) == -2, (fn.__name__, dh)                                         # dh outside {32, 48, 64}
            assert fn(dh=0) == -1 and fn(dh=-32) == -1
            assert fn(B=1 << 31) == -2 and fn(B=1 << 20, H=1 << 11) == -2                         # B * H * ceil(S / 64) workgroups against 2^31
            assert fn(B=1 << 16, H=1 << 10, S=64 * 32 + 1) == -2                                  # ... which only the block count pushes over
            assert fn(S=1 << 31) == -2
        assert fwd(flag=odd4) == -1


def _tiny(seed=0, **extra):
    from peekvit_amd.models.pct import PointCloudTransformer
    torch.manual_seed(seed)
    return PointCloudTransformer(num_points=32, num_layers=2, num_heads=2, hidden_dim=64, mlp_dim=128, num_classes=5, **extra).train()


def test_fused_switch_is_off_by_default_and_adds_no_state():
    from peekvit_amd.models.pct import PointCloudTransformer, RankPointCloudTransformer
    for cls in (PointCloudTransformer, RankPointCloudTransformer):
        torch.manual_seed(0)
        m = cls(num_points=32, num_layers=2, num_heads=2, hidden_dim=64, mlp_dim=128, num_classes=5)
        assert [blk.fused_attention for blk in m.encoder.layers] == [False, False]
        keys, nparam, nbuf = list(m.state_dict()), len(list(m.parameters())), len(list(m.buffers()))
        m.set_fused_attention()
        assert [blk.fused_attention for blk in m.encoder.layers] == [True, True]
        assert list(m.state_dict()) == keys and len(list(m.parameters())) == nparam and len(list(m.buffers())) == nbuf
        m.set_fused_attention(False)
        assert [blk.fused_attention for blk in m.encoder.layers] == [False, False]


def test_cpu_tensors_run_the_composite_bit_for_bit_with_the_switch_on():
    from peekvit_amd import ops, pct_train
    x = torch.from_numpy(synth.synth_points(3, 32, 1))
    results = []
    for on in (False, True):
        m = _tiny()
        if on:
            m.set_fused_attention(True)
            assert not pct_train.attention_eligible(m.encoder.layers[0], torch.zeros(3, 32, 64))
        n0, b0, l0 = pct_train.attn_passes, pct_train.attn_backwards, ops.launch_count
        loss = m(x).square().sum()
        loss.backward()
        assert (pct_train.attn_passes, pct_train.attn_backwards, ops.launch_count) == (n0, b0, l0)
        results.append((loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
    (l_off, g_off), (l_on, g_on) = results
    assert torch.equal(l_off, l_on) and set(g_off) == set(g_on) and all(torch.equal(g_off[n], g_on[n]) for n in g_off)
