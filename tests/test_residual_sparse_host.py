"""ResidualViT exact token compaction without a GPU: the public switch against the reference's constructor and
state-dict contract, a test ledger for include/peekvit_hip_sparse.h and the argument checks of its entry points, the torch restatement of the
packed algorithm (tests/residual_sparse_ref.py, the checker of the GPU tests) against oracle.vit_oracle's dense forward in fp64, the dense
path a CPU model takes with compaction on, the synthetic sparse weights and their fixture, and the harness key."""
import ast
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
from peekvit_amd import synth
import residual_sparse_ref as R

META = json.load(open(os.path.join(GOLDEN, "meta.json")))
SPARSE_META = json.load(open(os.path.join(GOLDEN, "residualvit_sparse_meta.json")))
EXTRA = dict(gate_type="sigmoid", gate_temp=1, add_budget_token="learnable", gate_threshold=0.5)


def _micro(gate_bias=0, **over):
    from peekvit_amd.models.residualvit import ResidualVisionTransformer
    cfg = dict(synth.MODEL_CONFIGS["vit_micro"], **EXTRA, gate_bias=gate_bias)
    m = ResidualVisionTransformer(**dict(cfg, **over))
    synth.load_synth_weights(m, cfg, "residualvit", seed=0)
    return cfg, m.eval()


def test_switch_exists_and_the_reference_surface_is_unchanged(monkeypatch):
    from peekvit_amd.models.residualvit import ResidualVisionTransformer as cls
    cfg = synth.MODEL_CONFIGS["vit_micro"]
    m = cls(**cfg, gate_type="sigmoid", add_budget_token="learnable")
    assert m.token_compaction is False
    assert m.set_token_compaction() is m and m.token_compaction is True
    m.set_token_compaction(False)
    assert m.token_compaction is False
    with pytest.raises(AttributeError):
        m.token_compaction = True                                  # read-only
    # neither a constructor kwarg nor a state-dict entry: both are the reference's
    params = [k for k in inspect.signature(cls.__init__).parameters if k != "self"]
    assert "token_compaction" not in params and not any("compact" in k for k in params)
    m.set_token_compaction(True)
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == META["state_dict"]["residualvit_micro"]
    assert not any("compact" in k for k, _ in m.named_buffers()) and not any("compact" in k for k, _ in m.named_parameters())
    # it survives what a checkpoint round trip does to a module, and the environment switch sets the default
    m2 = cls(**cfg, gate_type="sigmoid", add_budget_token="learnable")
    m2.load_state_dict(m.state_dict())
    assert m2.token_compaction is False
    monkeypatch.setenv("PEEKVIT_AMD_RESIDUAL_COMPACT", "1")
    assert cls(**cfg, gate_type="sigmoid", add_budget_token="learnable").token_compaction is True
    monkeypatch.setenv("PEEKVIT_AMD_RESIDUAL_COMPACT", "0")
    assert cls(**cfg, gate_type="sigmoid", add_budget_token="learnable").token_compaction is False


def test_constructor_signature_equals_the_reference():
    from peekvit_amd.models.residualvit import ResidualVisionTransformer as cls
    sig = inspect.signature(cls.__init__)
    # names, order and defaults of the real reference's constructor, recorded by scripts/make_golden_residual_sparse.py
    assert [k for k in sig.parameters if k != "self"] == SPARSE_META["constructor_parameters"]
    defaults = {k: p.default for k, p in sig.parameters.items() if k != "self" and p.default is not inspect.Parameter.empty}
    assert json.loads(json.dumps(defaults)) == SPARSE_META["constructor_defaults"]
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for k, p in sig.parameters.items())


# ---- include/peekvit_hip_sparse.h: every declared entry point is exported and has a test that calls it directly ----
LEDGER = {
    "pv_attention_varlen_w_bf16": ["test_hip_residual_sparse.py::test_attention_w_matches_fp64_with_random_multiplicities",
                                   "test_hip_residual_sparse.py::test_attention_w_equals_dense_attention_over_repeated_rows",
                                   "test_hip_residual_sparse.py::test_attention_w_every_tile_bound",
                                   "test_hip_residual_sparse.py::test_attention_w_refuses_what_it_does_not_take"],
    "pv_residual_pack_step": ["test_hip_residual_sparse.py::test_pack_step_small_sizes", "test_hip_residual_sparse.py::test_pack_step_production_size",
                              "test_hip_residual_sparse.py::test_pack_step_refuses_bad_arguments"],
}
HEADER = os.path.join(REPO, "include", "peekvit_hip_sparse.h")


def _declared():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pv_\w+)\s*\(", src, flags=re.M))


def _arity(name):
    m = re.search(r"\b(?:int|int64_t) " + name + r"\(([^;]*)\);", open(HEADER).read())
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_sparse_ledger_names_a_direct_test_for_every_declared_entry_point():
    from peekvit_amd import _build, _lib
    assert "peekvit_hip_sparse.h" in _build.HEADERS and _build.FILE_FLAGS.get("pv_sparse.hip") == ["-fno-slp-vectorize"]
    declared = _declared()
    assert set(LEDGER) == declared == set(_lib.SIGNATURES_SPARSE), declared ^ set(LEDGER)
    for name, (_, args) in _lib.SIGNATURES_SPARSE.items():
        assert _arity(name) == len(args), name
        assert hasattr(_lib.load(), name) and hasattr(_lib.load("f16"), name)          # exported by both libraries
    assert _lib.load().pv_version() == 10 and _lib.load("f16").pv_version() == 10      # ABI unchanged
    ops_src = open(os.path.join(REPO, "peekvit_amd", "ops.py")).read()
    wrappers = {}
    for node in ast.parse(ops_src).body:
        if isinstance(node, ast.FunctionDef):
            for sym in re.findall(r"\b(pv_\w+)\(", ast.get_source_segment(ops_src, node)):
                wrappers.setdefault(sym, set()).add(node.name)
    def reaches(entry, name, funcs, src, seen):
        """Does test / helper `name` call the entry point: by its symbol, through its ops wrapper, or through a helper of the same file that does?"""
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
    for op in ("bf16", "f16"):
        lib = _lib.load(op)

        def attn(qkv=p, out=q, seg=p, lm=p, B=4, max_len=198, H=12, dh=64):
            return lib.pv_attention_varlen_w_bf16(qkv, out, seg, lm, B, max_len, H, dh, null, null)
        assert attn(qkv=null) == -1 and attn(out=null) == -1 and attn(seg=null) == -1 and attn(lm=null) == -1
        assert attn(B=0) == -1 and attn(H=0) == -1 and attn(max_len=0) == -1
        assert attn(dh=32) == -2 and attn(dh=128) == -2 and attn(max_len=209) == -2 and attn(B=1 << 31, H=2) == -2

        def pack(x=p, seg=p, mult=p, tok=p, B=4, N=196, D=768, wg=p, bg=p, wb=p, bb=p, temp=1.0, mrow=p, xn=q, rs=p, mn=p, lm=p, sn=p, tn=p,
                 mo=p, th=p, tot=p, g=null, b=null, ln=null):
            return lib.pv_residual_pack_step(x, seg, mult, tok, B, N, D, wg, bg, wb, bb, temp, 0.0, mrow, xn, rs, mn, lm, sn, tn, mo, th, tot,
                                             g, b, 1e-6, ln, null)
        for k in ("x", "seg", "mult", "tok", "wg", "bg", "wb", "bb", "mrow", "xn", "rs", "mn", "lm", "sn", "tn", "mo", "th", "tot"):
            assert pack(**{k: null}) == -1, k
        assert pack(B=0) == -1 and pack(D=0) == -1 and pack(N=-1) == -1 and pack(temp=0.0) == -1
        assert pack(xn=p) == -1                                          # in place
        assert pack(ln=p) == -1 and pack(ln=p, g=p) == -1                # LayerNorm output without its affine
        assert pack(D=770) == -2 and pack(D=8192) == -2 and pack(N=207) == -2 and pack(B=1 << 31) == -2
        assert pack(x=C.c_void_p(260)) == -2 and pack(xn=C.c_void_p((1 << 30) + 8)) == -2 and pack(wg=C.c_void_p(264)) == -2
        assert pack(ln=C.c_void_p(516), g=p, b=p) == -2 and pack(ln=p, g=C.c_void_p(260), b=p) == -2


# ---- the checker of the GPU tests ----
def _sd64(cfg, gain):
    return R.sparse_sd(cfg, gain, torch.float64)


@pytest.mark.parametrize("name,gate_bias,gain,batch", [("vit_micro", 0, 1.0, 4), (SPARSE_META["model"], SPARSE_META["kwargs"]["gate_bias"],
                                                                                 SPARSE_META["gate_gain"], SPARSE_META["batch"])])
def test_packed_restatement_equals_the_oracles_dense_forward_in_fp64(name, gate_bias, gain, batch):
    torch.set_num_threads(min(8, torch.get_num_threads()))
    cfg = dict(synth.MODEL_CONFIGS[name], **EXTRA, gate_bias=gate_bias)
    sd = _sd64(cfg, gain)
    x = torch.from_numpy(synth.synth_images(batch, cfg["image_size"], seed=0)).double()
    S = synth.seq_length(cfg) + 1
    for b in (0.2, 0.5, 0.8):
        ld, md, td, _ = R.dense_forward(x, sd, cfg, b)
        lp, mp, tp, rows = R.packed_forward(x, sd, cfg, b)
        assert ld.dtype == lp.dtype == torch.float64
        err = R.rel_l2(lp, ld)
        print(f"\n{name} budget {b}: packed vs dense in fp64 {err:.3g}, rows share {sum(rows) / (len(rows) * batch * S):.3f}")
        assert err < 1e-12
        assert torch.equal(mp == 0, md == 0) and float((mp - md).abs().max()) < 1e-12 and float((tp - td).abs().max()) < 1e-12
        assert bool((md == 0).any()), "the case masks nothing: it would not exercise the compaction"
        assert sum(rows) < len(rows) * batch * S
    # ... and the dense fp64 forward is the oracle's own fp32 forward up to fp32 rounding
    from oracle import vit_oracle as O
    sd32 = {k: v.float() for k, v in sd.items()}
    l32 = O.residualvit_forward(x.float(), sd32, cfg, 0.8)
    assert R.rel_l2(l32.numpy(), R.dense_forward(x, sd, cfg, 0.8)[0].numpy()) < 1e-4


def test_pack_step_restatement_on_a_hand_made_case():
    """Two images, D = 4, gate = first coordinate: the tables by hand."""
    wg, wb = torch.tensor([1.0, 0, 0, 0]), torch.tensor([0.0, 0, 0, 0])          # thr = sigmoid(0) = 0.5; mask = relu(sigmoid(x0) - 0.5)
    x = torch.tensor([[9.0, 1, 1, 1], [2.0, 0, 0, 0], [-1.0, 5, 5, 5], [3.0, 1, 0, 0], [-2.0, 7, 7, 7], [0.5, 0, 0, 0],      # image 0: cls, 4 rows, budget
                      [9.0, 2, 2, 2], [4.0, 4, 4, 4], [0.5, 0, 0, 0]], dtype=torch.float64)                                    # image 1: cls, 1 row, budget
    seg, mult = np.array([0, 6, 9]), np.array([1, 1, 2, 1, 3, 1, 1, 7, 1])
    tok_row = np.array([[1, 2, 2, 3, 4, 4, 4], [1, 1, 1, 1, 1, 1, 1]])
    st = R.pack_step_ref(x, seg, mult, tok_row, wg, 0.0, wb, 0.0, 1.0, 0.0)
    assert st["seg_next"].tolist() == [0, 5, 8] and st["totals"] == (8, 5)
    assert st["mult_next"].tolist() == [1, 1, 1, 5, 1, 1, 7, 1]                    # rows 2 and 4 of image 0 (2 + 3 tokens) merge into its zero row
    assert st["tok_row_next"].tolist() == [[1, 3, 3, 2, 3, 3, 3], [1] * 7]
    s2, s3, s4 = (float(torch.sigmoid(torch.tensor(v, dtype=torch.float64))) - 0.5 for v in (2.0, 3.0, 4.0))
    assert np.allclose(st["row_scale_next"].numpy(), [1, s2, s3, 0, 1, 1, s4, 1], atol=1e-15)
    assert np.allclose(st["mask_out"].numpy(), [[s2, 0, 0, s3, 0, 0, 0], [s4] * 7], atol=1e-15)
    assert torch.equal(st["x_next"][3], torch.zeros(4, dtype=torch.float64)) and torch.equal(st["x_next"][0], x[0]) and torch.equal(st["x_next"][4], x[5])
    assert torch.allclose(st["x_next"][1], s2 * x[1]) and torch.allclose(st["x_next"][6], s4 * x[7])
    assert torch.allclose(st["log_mult_next"], torch.log(torch.tensor([1, 1, 1, 5, 1, 1, 7, 1], dtype=torch.float64)))


# ---- CPU model, fixture, synthetic weights, harness ----
def test_cpu_model_with_compaction_on_is_the_dense_path_bit_for_bit():
    from peekvit_amd import engine
    cfg, m = _micro(0)
    x = torch.from_numpy(synth.synth_images(3, cfg["image_size"], seed=2))
    m.set_budget(0.5)
    with torch.no_grad():
        off = m(x)
    masks = [blk.mask.clone() for blk in m.encoder.layers]
    m.set_token_compaction(True)
    n0, r0 = engine.sparse_dense_forwards, engine.sparse_rows
    with torch.no_grad():
        on = m(x)
    assert torch.equal(on, off) and all(torch.equal(blk.mask, k) for blk, k in zip(m.encoder.layers, masks))
    assert engine.sparse_dense_forwards == n0 + 1 and engine.sparse_rows == r0
    m.train()
    m(x)                                                              # training: dense as well, counted
    assert engine.sparse_dense_forwards == n0 + 2
    m.eval().set_token_compaction(False)
    with torch.no_grad():
        m(x)
    assert engine.sparse_dense_forwards == n0 + 2


def test_eligibility_rules():
    cfg, m = _micro(0)
    class _Cuda:              # (is_cuda is all the rule reads of the tensor; real GPU tensors are exercised in tests/test_hip_residual_sparse.py)
        is_cuda = True
    ok = lambda model: model._compaction_ok(_Cuda())
    assert ok(m) and not m._compaction_ok(torch.zeros(1))
    m.train()
    assert not ok(m)
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
    del m.encoder.layers[1]
    assert not ok(m)
    assert not ok(_micro(0, dropout=0.1)[1]) and not ok(_micro(0, num_heads=4)[1])                     # dropout above 0; head dim 32
    assert not ok(_micro(0, residual_layers=["attention+mlp", "mlp"])[1]) and not ok(_micro(0, gate_type="gumbel")[1])
    from peekvit_amd.models.residualvit import ResidualVisionTransformer
    big = ResidualVisionTransformer(image_size=240, patch_size=16, num_layers=1, num_heads=1, hidden_dim=64, mlp_dim=64, **EXTRA).eval()
    assert big.seq_length + 1 == 227 and not ok(big)                                                    # more than 208 tokens


def test_sparse_state_dict_and_fixture():
    cfg = dict(synth.MODEL_CONFIGS["vit_b_16"], **EXTRA)
    base, sp = synth.synth_state_dict(cfg, "residualvit"), synth.residual_sparse_state_dict(cfg, gate_gain=4.0)
    assert set(base) == set(sp)
    for k in base:
        if k.endswith("residual_gate.projection.weight"):
            assert np.array_equal(sp[k], synth.round_to_bf16(base[k] * 4.0)) and np.array_equal(sp[k], synth.round_to_bf16(sp[k]))
        else:
            assert np.array_equal(sp[k], base[k]), k
    g = np.load(os.path.join(GOLDEN, "residualvit_sparse.npz"))
    assert SPARSE_META["kwargs"]["gate_bias"] == 1 and SPARSE_META["batch"] == 2 and SPARSE_META["budgets"] == [0.2, 0.5, 0.8]
    assert 0 < SPARSE_META["gate_gain"] <= 4.0
    for b in SPARSE_META["budgets"]:
        assert g[f"b{b}_logits"].shape == (2, 1000) and g[f"b{b}_masks"].shape == (12, 2, 196, 1)
        assert g[f"b{b}_thresholds"].shape == (12, 2) and g[f"b{b}_margin"].shape == (12, 2, 196)
        assert float((g[f"b{b}_margin"] < SPARSE_META["margin"]).mean()) <= SPARSE_META["max_excluded_fraction"] == 0.02
        assert 0.3 < float(g[f"b{b}_rows_share"]) < 0.7 and bool((g[f"b{b}_masks"] == 0).any())
        # a mask is zero exactly where sigmoid <= threshold: margin and mask agree
        assert bool(((g[f"b{b}_masks"][..., 0] > 0) <= (g[f"b{b}_margin"] > 0)).all())
    assert os.path.getsize(os.path.join(GOLDEN, "residualvit_sparse.npz")) < 1 << 20


def test_harness_config_key_parses_and_the_cpu_sweep_reports_the_share():
    from peekvit_amd.harness import config, test as htest
    assert config.load_config("test_config", ["model=residualvit_b_16"])["test"]["compact_tokens"] is False
    assert config.load_config("test_config", ["model=residualvit_b_16", "test.compact_tokens=true"])["test"]["compact_tokens"] is True
    micro = ["model=residualvit_b_16", "model.patch_size=8", "model.hidden_dim=64", "model.mlp_dim=128", "model.num_layers=2", "model.num_heads=1",
             "dataset.image_size=32", "dataset.num_classes=10", "dataset.train_size=16", "dataset.val_size=16", "device=cpu",
             "test.test_batch_size=8", "test.budgets=[0.5,1.0]"]
    res = htest.main(micro + ["test.compact_tokens=true"])
    assert [r["budget"] for r in res] == [0.5, 1.0] and all("executed_row_share" in r and r["executed_row_share"] is None for r in res)
    assert all("executed_row_share" not in r for r in htest.main(micro))


def test_harness_sweep_restores_the_callers_setting():
    from peekvit_amd.harness import test as htest
    cfg, m = _micro(0)
    x = torch.from_numpy(synth.synth_images(4, cfg["image_size"], seed=1))
    loader = [(x, torch.zeros(4, dtype=torch.int64))]
    res = htest.evaluate(m, loader, "cpu", [0.5], 4, compact_tokens=True)
    assert "executed_row_share" in res[0] and m.token_compaction is False       # switched on for the sweep only
    m.set_token_compaction(True)
    htest.evaluate(m, loader, "cpu", [0.5], 4, compact_tokens=True)
    assert m.token_compaction is True                                            # the caller's own setting stays
    assert "executed_row_share" not in htest.evaluate(m, loader, "cpu", [0.5], 4)[0]
