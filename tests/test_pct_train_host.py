"""The training path of the point-cloud stem without a GPU: a test ledger for include/peekvit_hip_pct_train.h, the argument checks of its
entry points (every refusal comes before a launch), the build flags of its source, and the dispatch on CPU tensors (the composite)."""
import ast
import ctypes as C
import os
import re

import torch

from conftest import REPO
from peekvit_amd import synth

HEADER = os.path.join(REPO, "include", "peekvit_hip_pct_train.h")
REFUSAL = "test_pct_train_host.py::test_entry_points_refuse_bad_arguments_without_a_gpu"

# ---- include/peekvit_hip_pct_train.h: every declared entry point is exported and has a test that calls it directly ----
LEDGER = {
    "pv_arpe_knn": ["test_hip_pct_train.py::test_knn_lists_equal_the_sort_and_the_eval_kernel", REFUSAL],
    "pv_arpe_pair_moments": ["test_hip_pct_train.py::test_pair_moments_against_fp64", REFUSAL],
    "pv_arpe_pair_max": ["test_hip_pct_train.py::test_pair_max_against_fp64", REFUSAL],
    "pv_arpe_pair_bwd": ["test_hip_pct_train.py::test_pair_bwd_sums_against_fp64", REFUSAL],
}


def _declared():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pv_\w+)\s*\(", src, flags=re.M))


def _arity(name):
    m = re.search(r"\b(?:int|int64_t) " + name + r"\(([^;]*)\);", open(HEADER).read())
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_pct_train_ledger_names_a_direct_test_for_every_declared_entry_point():
    from peekvit_amd import _build, _lib
    assert "peekvit_hip_pct_train.h" in _build.HEADERS
    declared = _declared()
    assert set(LEDGER) == declared == set(_lib.SIGNATURES_PCT_TRAIN), declared ^ set(LEDGER)
    assert not set(_lib.SIGNATURES_PCT_TRAIN) & set(_lib.SIGNATURES_PCT)                # a dict of their own
    for name, (_, args) in _lib.SIGNATURES_PCT_TRAIN.items():
        assert _arity(name) == len(args), name
        assert hasattr(_lib.load(), name) and hasattr(_lib.load("f16"), name)          # exported by both libraries
    assert _lib.load().pv_version() == 10 and _lib.load("f16").pv_version() == 10      # ABI unchanged
    ops_src = open(os.path.join(REPO, "peekvit_amd", "ops.py")).read()
    wrappers = {}
    for node in ast.parse(ops_src).body:
        if isinstance(node, ast.FunctionDef):
            for sym in re.findall(r"\b(pv_\w+)\(", ast.get_source_segment(ops_src, node)):
                wrappers.setdefault(sym, set()).add(node.name)
    assert all(wrappers.get(e) for e in LEDGER), "every entry point has an ops wrapper"

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


def test_build_flags_of_the_training_source():
    from peekvit_amd import _build
    assert _build.FILE_FLAGS["pv_pct_train.hip"] == ["-fno-slp-vectorize"]
    assert os.path.join(_build.CSRC, "pv_pct_train.hip") in _build.sources()


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from peekvit_amd import _lib
    p, q, null = C.c_void_p(256), C.c_void_p(1 << 30), C.c_void_p(0)       # never dereferenced: every call below is refused before a launch
    odd4, odd2 = C.c_void_p(258), C.c_void_p(257)                          # off a 4-byte boundary / off a 2-byte boundary
    for op in ("bf16", "f16"):
        lib = _lib.load(op)

        def knn(pts=p, idx=q, B=2, N=64, k=4):
            return lib.pv_arpe_knn(pts, idx, B, N, k, null)

        def mom(pts=p, idx=p, sh=p, part=q, B=2, N=64, k=4):
            return lib.pv_arpe_pair_moments(pts, idx, sh, part, B, N, k, null)

        def pmax(pts=p, idx=p, w1=p, b1=p, sc=p, sh=p, y=q, arg=q, B=2, N=64, k=4):
            return lib.pv_arpe_pair_max(pts, idx, w1, b1, sc, sh, y, arg, B, N, k, null)

        def bwd(pts=p, arg=p, y=p, g=p, w1=p, b1=p, part=q, B=2, N=64):
            return lib.pv_arpe_pair_bwd(pts, arg, y, g, w1, b1, part, B, N, null)

        pointers = {knn: ("pts", "idx"), mom: ("pts", "idx", "sh", "part"), pmax: ("pts", "idx", "w1", "b1", "sc", "sh", "y", "arg"),
                    bwd: ("pts", "arg", "y", "g", "w1", "b1", "part")}
        for fn, names in pointers.items():
            for name in names:
                assert fn(**{name: null}) == -1, (fn.__name__, name)                              # nulls
                assert fn(**{name: odd2}) == -1, (fn.__name__, name)                              # misaligned for either element size
                if name not in ("idx", "arg"):
                    assert fn(**{name: odd4}) == -1, (fn.__name__, name)                          # fp32 arrays: 4-byte aligned
            assert fn(B=0) == -1 and fn(N=0) == -1 and fn(B=-1) == -1                             # zero sizes
            assert fn(N=15) == -2 and fn(N=4097) == -2                                            # 16 <= N <= 4096
            assert fn(B=1 << 31) == -2
        for fn in (knn, mom, pmax):
            assert fn(k=0) == -1 and fn(k=65) == -1 and fn(k=-3) == -1                            # 1 <= k <= N
            assert fn(N=15, k=1) == -2 and fn(N=4097, k=256) == -2
        assert bwd(arg=odd2) == -1


def test_cpu_tensors_in_train_mode_run_the_composite():
    from peekvit_amd import ops, pct_train
    from peekvit_amd.models.pct import PointCloudTransformer
    torch.manual_seed(0)
    m = PointCloudTransformer(num_points=32, num_layers=1, num_heads=2, hidden_dim=64, mlp_dim=128, num_classes=5).train()
    x = torch.from_numpy(synth.synth_points(3, 32, 1))
    assert not pct_train.eligible(m.embedder, x)
    n0, l0 = pct_train.stem_passes, ops.launch_count
    out = m(x)
    out.square().sum().backward()
    assert pct_train.stem_passes == n0 and ops.launch_count == l0
    assert m.embedder.lin1.weight.grad is not None and int(m.embedder.bn1.num_batches_tracked) == 1
    # ... and an eval forward with grads on
    m.eval()
    y = m.embedder(x)
    assert y.requires_grad and pct_train.stem_passes == n0 and ops.launch_count == l0
