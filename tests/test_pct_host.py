"""Point-cloud transformers without a GPU: a test ledger for include/peekvit_hip_pct.h and the argument checks of its entry points, the
constructors and state-dict keys against the real reference's (tests/golden/pct_meta.json, scripts/make_golden_pct.py), the Hydra targets and
harness configs, the stock-op composite of both classes against the reference's golden outputs, a checkpoint round trip and train mode.

The composite runs the reference's own torch ops, so it is held to an fp32-rounding bound derived from the fixture: the reference's output is
measured against a float64 restatement (the same composite on a .double() model), and the composite may be four times as far from it."""
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

META = json.load(open(os.path.join(GOLDEN, "pct_meta.json")))
HEADER = os.path.join(REPO, "include", "peekvit_hip_pct.h")

# ---- include/peekvit_hip_pct.h: every declared entry point is exported and has a test that calls it directly ----
LEDGER = {
    "pv_arpe_embed": ["test_hip_pct.py::test_arpe_embed_against_fp64", "test_hip_pct.py::test_arpe_embed_duplicates_beyond_k",
                      "test_hip_pct.py::test_arpe_embed_exact_tie_between_distinct_points_goes_to_the_lowest_index",
                      "test_pct_host.py::test_entry_points_refuse_bad_arguments_without_a_gpu"],
    "pv_layernorm_f32_bf16": ["test_hip_pct.py::test_layernorm_both_planes", "test_pct_host.py::test_entry_points_refuse_bad_arguments_without_a_gpu"],
    "pv_mean_pool_f32": ["test_hip_pct.py::test_mean_pool_against_fp64", "test_pct_host.py::test_entry_points_refuse_bad_arguments_without_a_gpu"],
    "pv_pct_head_f32": ["test_hip_pct.py::test_pct_head_against_fp64", "test_pct_host.py::test_entry_points_refuse_bad_arguments_without_a_gpu"],
}


def _declared():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pv_\w+)\s*\(", src, flags=re.M))


def _arity(name):
    m = re.search(r"\b(?:int|int64_t) " + name + r"\(([^;]*)\);", open(HEADER).read())
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_pct_ledger_names_a_direct_test_for_every_declared_entry_point():
    from peekvit_amd import _build, _lib
    assert "peekvit_hip_pct.h" in _build.HEADERS and _build.FILE_FLAGS.get("pv_pct.hip") == ["-fno-slp-vectorize"]
    declared = _declared()
    assert set(LEDGER) == declared == set(_lib.SIGNATURES_PCT), declared ^ set(LEDGER)
    for name, (_, args) in _lib.SIGNATURES_PCT.items():
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


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from peekvit_amd import _lib
    p, q, null = C.c_void_p(256), C.c_void_p(1 << 30), C.c_void_p(0)       # never dereferenced: every call below is refused before a launch
    odd = C.c_void_p(260)
    for op in ("bf16", "f16"):
        lib = _lib.load(op)

        def arpe(pts=p, w1=p, b1=p, s1=p, t1=p, w2=p, b2=p, s2=p, t2=p, tok=q, idx=null, B=2, N=64, k=4, D=128, S=64, off=0):
            return lib.pv_arpe_embed(pts, w1, b1, s1, t1, w2, b2, s2, t2, tok, idx, B, N, k, D, S, off, null)
        for name in ("pts", "w1", "b1", "s1", "t1", "w2", "b2", "s2", "t2", "tok"):
            assert arpe(**{name: null}) == -1, name
        assert arpe(B=0) == -1 and arpe(N=0) == -1 and arpe(D=0) == -1 and arpe(S=0) == -1 and arpe(off=-1) == -1
        assert arpe(k=0) == -1 and arpe(k=65) == -1 and arpe(k=-3) == -1                      # 1 <= k <= N
        assert arpe(N=15, k=1, S=15) == -2 and arpe(N=4097, k=256, S=4097) == -2             # 16 <= N <= 4096
        assert arpe(D=1028) == -2 and arpe(D=130) == -2 and arpe(D=2048) == -2               # D % 4 == 0, D <= 1024
        assert arpe(S=63) == -1 and arpe(S=65, off=2) == -1                                  # the rows [off, off + N) must exist
        assert arpe(tok=odd) == -1 and arpe(w2=odd) == -1 and arpe(idx=C.c_void_p(258)) == -1
        assert arpe(B=1 << 31) == -2

        def ln(x=p, g=p, b=p, o16=q, o32=C.c_void_p(1 << 31), ldx=128, ld32=128, rows=8, D=128):
            return lib.pv_layernorm_f32_bf16(x, ldx, g, b, o16, o32, ld32, rows, D, 1e-5, null)
        for name in ("x", "g", "b", "o16", "o32"):
            assert ln(**{name: null}) == -1, name
        assert ln(rows=0) == -1 and ln(D=0) == -1 and ln(ldx=124) == -1 and ln(ld32=126) == -1 and ln(ldx=130) == -1
        assert ln(D=130, ldx=132, ld32=132) == -2 and ln(D=4100, ldx=4100, ld32=4100) == -2
        assert ln(x=odd) == -1 and ln(o16=C.c_void_p(1028)) == -1 and ln(o32=p) == -1            # (the fp32 rows on top of the input)

        def pool(x=p, out=q, B=2, S=65, D=128):
            return lib.pv_mean_pool_f32(x, out, B, S, D, null)
        assert pool(x=null) == -1 and pool(out=null) == -1 and pool(B=0) == -1 and pool(S=0) == -1 and pool(D=0) == -1
        assert pool(D=130) == -2 and pool(x=odd) == -1

        def head(pooled=p, w1=p, b1=p, s=p, t=p, w2=p, b2=p, out=q, B=2, D=128, Hd=64, Cn=40):
            return lib.pv_pct_head_f32(pooled, w1, b1, s, t, w2, b2, out, B, D, Hd, Cn, null)
        for name in ("pooled", "w1", "s", "t", "w2", "out"):
            assert head(**{name: null}) == -1, name
        assert head(B=0) == -1 and head(D=0) == -1 and head(Hd=0) == -1 and head(Cn=0) == -1
        assert head(D=4097) == -2 and head(Hd=4097) == -2 and head(pooled=C.c_void_p(258)) == -1


# ---- the reference's surface ----
def _classes():
    from peekvit_amd.models.pct import PointCloudTransformer, RankPointCloudTransformer
    return {"PointCloudTransformer": PointCloudTransformer, "RankPointCloudTransformer": RankPointCloudTransformer}


@pytest.mark.parametrize("name", ["PointCloudTransformer", "RankPointCloudTransformer"])
def test_constructor_and_state_dict_equal_the_reference(name):
    cls, ref = _classes()[name], META[name]
    sig = inspect.signature(cls.__init__)
    assert [k for k in sig.parameters if k != "self"] == ref["constructor_parameters"]
    defaults = {k: p.default for k, p in sig.parameters.items() if k != "self" and p.default is not inspect.Parameter.empty}
    assert json.loads(json.dumps(defaults)) == ref["constructor_defaults"]
    m = cls(**META["surface_kwargs"])
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == ref["state_dict"]
    assert list(m.state_dict()) == list(ref["state_dict"]) or set(m.state_dict()) == set(ref["state_dict"])
    assert m.embedder.k == META["surface_kwargs"]["num_points"] // 16
    if name == "RankPointCloudTransformer":
        m.enable_ranking([True, False])
        m.set_budget(0.5)
        assert [b.sort for b in m.encoder.layers] == [True, False] and all(b.current_budget == 0.5 for b in m.encoder.layers)
        assert m.current_budget == 0.5


def test_hydra_targets_resolve_and_harness_configs_instantiate():
    from peekvit_amd.harness import config
    from peekvit_amd.models import pct
    for target, cls in (("peekvit.models.pct.PointCloudTransformer", pct.PointCloudTransformer),
                        ("peekvit.models.rankpct.PointCloudTransformer", pct.PointCloudTransformer),          # what the reference's pct.yaml names
                        ("peekvit.models.rankpct.RankPointCloudTransformer", pct.RankPointCloudTransformer)):
        module, _, attr = target.rpartition(".")
        assert getattr(importlib.import_module(module), attr) is cls
        m = config.instantiate({"_target_": target, "num_points": 32, "num_layers": 1, "num_heads": 2, "hidden_dim": 64, "mlp_dim": 128})
        assert type(m) is cls and m.num_classes == 40
    for model, cls in (("pct", pct.PointCloudTransformer), ("rankpct", pct.RankPointCloudTransformer)):
        cfg = config.load_config("test_config", [f"model={model}", "dataset=synthetic_points", "dataset.num_points=64", "dataset.train_size=4",
                                                 "dataset.val_size=4"])
        m = config.instantiate(cfg["model"])
        assert type(m) is cls and m.embedder.k == 4 and m.hidden_dim == 128 and len(m.encoder.layers) == 4 and m.num_classes == 40
        ds = config.instantiate(cfg["dataset"])
        x, y = ds.val_dataset[0]
        assert tuple(x.shape) == (64, 3) and x.dtype == torch.float32 and 0 <= int(y) < 40 and len(ds.train_dataset) == 4
        with torch.no_grad():
            assert tuple(m.eval()(torch.stack([ds.val_dataset[i][0] for i in range(2)])).shape) == (2, 40)


# ---- the composite against the reference's outputs ----
def _synth_cfg(kw):
    return {k: v for k, v in kw.items() if k in ("num_points", "num_layers", "num_heads", "hidden_dim", "mlp_dim", "num_classes", "num_registers",
                                                 "num_class_tokens")}


def _load(cls, kw):
    m = cls(**kw).eval()
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.pct_state_dict(_synth_cfg(kw), 0).items()}, strict=True)
    return m


def _four_times(got, ref32, ref64, what):
    e_ref, e_got = rel_l2(ref32, ref64), rel_l2(got, ref64)
    m_ref, m_got = float(np.abs(np.asarray(ref32, np.float64) - ref64).max()), float(np.abs(np.asarray(got, np.float64) - ref64).max())
    print(f"{what}: rel L2 {e_got:.3g} (reference {e_ref:.3g}), max abs {m_got:.3g} (reference {m_ref:.3g})")
    assert e_got <= 4 * e_ref and m_got <= 4 * m_ref, (what, e_got, e_ref, m_got, m_ref)


@pytest.mark.parametrize("name", sorted(META["cases"]))
def test_composite_equals_the_reference(name):
    info = META["cases"][name]
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    m = _load(_classes()["PointCloudTransformer"], info["kwargs"])
    assert np.array_equal(z["points"], synth.synth_points(info["batch"], info["kwargs"]["num_points"], info["points_seed"], info["dup_frac"]))
    x = torch.from_numpy(z["points"])
    with torch.no_grad():
        emb, idx = m.embedder(x, return_idx=True)
        logits = m(x)
        m64 = _load(_classes()["PointCloudTransformer"], info["kwargs"]).double()
        emb64, logits64 = m64.embedder(x.double()).numpy(), m64(x.double()).numpy()
    sets = np.sort(idx.numpy(), axis=-1)
    tie = z["tie"]
    assert info["k"] == m.embedder.k and sets.shape == z["neighbours"].shape
    assert np.array_equal(sets[~tie], z["neighbours"][~tie].astype(np.int64))          # (a tie is copies of one point: embeddings only)
    assert int(tie.sum()) == info["tie_queries"] and (info["dup_frac"] == 0) == (int(tie.sum()) == 0)
    _four_times(emb.numpy(), z["embedding"], emb64, name + " embedding")
    _four_times(logits.numpy(), z["logits"], logits64, name + " logits")


@pytest.mark.parametrize("name", sorted(META["rank_cases"]))
def test_rank_composite_equals_the_reference(name):
    info = META["rank_cases"][name]
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cls = _classes()["RankPointCloudTransformer"]
    x = torch.from_numpy(z["points"])

    def run(m, x):
        m.enable_ranking(info["ranking"])
        m.set_budget(info["budget"])
        with torch.no_grad():
            return m(x)
    m = _load(cls, info["kwargs"])
    logits = run(m, x)
    S = info["kwargs"]["num_points"] + info["kwargs"].get("num_registers", 0)
    for i in info["ranked_layers"]:
        keep = np.sort(m.encoder.layers[i].last_keep.numpy(), axis=-1)
        assert np.array_equal(keep, z[f"kept_{i}"].astype(np.int64)) and keep[:, 0].tolist() == [0] * info["batch"]      # row 0 is fixed
        S = int(np.ceil(S * info["budget"]))                    # ceil(S * budget) rows of the WHOLE sequence, not ceil((S - 1) * budget)
        assert keep.shape[1] == S
    m64 = _load(cls, info["kwargs"]).double()
    logits64 = run(m64, x.double())
    same = all(np.array_equal(np.sort(a.last_keep.numpy(), -1), np.sort(b.last_keep.numpy(), -1))
               for a, b in zip((m.encoder.layers[i] for i in info["ranked_layers"]), (m64.encoder.layers[i] for i in info["ranked_layers"])))
    assert same, "the float64 restatement kept other rows: the fixture's boundary gap is too small for this comparison"
    _four_times(logits.numpy(), z["logits"], logits64.numpy(), name + " logits")
    # without ranking the model is the plain one
    plain = _load(_classes()["PointCloudTransformer"], info["kwargs"])
    m.enable_ranking(False)
    with torch.no_grad():
        assert torch.equal(m(x), plain(x))


def test_checkpoint_round_trip(tmp_path):
    from peekvit_amd.harness import checkpoint
    kw = dict(META["cases"]["pct_n64r1"]["kwargs"])
    for cname, cls in _classes().items():
        m = _load(cls, kw)
        args = dict(kw, _target_=f"peekvit.models.rankpct.{cname}")
        f = checkpoint.save_state(str(tmp_path / cname), m, args, epoch=3)
        m2, state = checkpoint.load_state(f, strict=True)
        assert type(m2) is cls and state["model_class"] == cname and state["epoch"] == 3
        x = torch.from_numpy(synth.synth_points(2, 64, 5))
        with torch.no_grad():
            assert torch.equal(m.eval()(x), m2.eval()(x))
        assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))


def test_train_mode_runs_the_composite_and_reaches_every_parameter():
    kw = dict(num_points=32, num_layers=2, num_heads=2, hidden_dim=64, mlp_dim=128, num_classes=7, num_registers=1)
    for cname, cls in _classes().items():
        torch.manual_seed(0)
        m = cls(**kw).train()
        if cname == "RankPointCloudTransformer":
            m.enable_ranking(True)
            m.set_budget(0.5)
        x = torch.from_numpy(synth.synth_points(4, 32, 2))
        before = m.embedder.bn1.running_mean.clone()
        out = m(x)
        assert tuple(out.shape) == (4, 7) and out.requires_grad
        out.square().sum().backward()
        missing = [n for n, p in m.named_parameters() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
        assert missing == ["class_tokens"]                                   # the parameter the forward never uses
        assert not torch.equal(before, m.embedder.bn1.running_mean)          # batch statistics
        assert int(m.head.bn1.num_batches_tracked) == 1


def test_knn_is_direct_differences_with_ties_to_the_lowest_index():
    from peekvit_amd.models.pct import knn_indices
    x = torch.zeros(1, 6, 3)
    x[0, :, 0] = torch.tensor([0.0, 1.0, -1.0, 1.0, 3.0, -1.0])             # rows 1, 3 and rows 2, 5 coincide; 1 and 2 are equally far from 0
    assert knn_indices(x, 3)[0, 0].tolist() == [0, 1, 2] and knn_indices(x, 4)[0, 0].tolist() == [0, 1, 2, 3]
    assert knn_indices(x, 2)[0, 3].tolist() == [1, 3]
    # far from the origin |a|^2 + |b|^2 - 2 a.b cancels; differences do not
    y = torch.tensor([[[1000.0, 0, 0], [1000.001, 0, 0], [1000.003, 0, 0], [999.996, 0, 0]]])
    assert knn_indices(y, 2)[0, 0].tolist() == [0, 1] and knn_indices(y, 2)[0, 2].tolist() == [2, 1]
    assert torch.equal(knn_indices(y, 3), knn_indices(y.double(), 3))
    with pytest.raises(ValueError):
        knn_indices(y, 5)
