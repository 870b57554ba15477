"""A-ViT training on the packed live rows without a GPU: the packed restatement (tests/avit_packed_train_ref.py: representative
rows, ln n key weights, the per-image scalar G, autograd through the row-wise block only) against the dense fp64 composite of tests/avit_train_ref.py,
the switch and the harness key, and a test ledger plus the argument checks for include/peekvit_hip_avit_pack_train.h."""
import ast
import ctypes as C
import json
import os
import re

import pytest
import torch

import avit_packed_train_ref as pref
import avit_train_ref as ref
from conftest import GOLDEN, REPO, rel_l2
from peekvit_amd import synth
from peekvit_amd.harness import config, train as htrain

META = json.load(open(os.path.join(GOLDEN, "avit_meta.json")))
EXACT = 1e-12           # the restatement differs from the dense composite by fp64 rounding alone (measured: DESIGN.md section 30)


def _avit64(name):
    from peekvit_amd.models.adavit import AdaptiveVisionTransformer
    case = META["cases"][name]
    model = AdaptiveVisionTransformer(**case["kwargs"]).train()
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(case["synth_cfg"], seed=0).items()}, strict=True)
    x = torch.from_numpy(synth.synth_images(6, case["kwargs"]["image_size"], seed=0, name="avit"))
    return model.double(), x, torch.arange(6) % case["kwargs"]["num_classes"]


def _pattern(which, B, S, L, n_cls):
    """A counter_token [B, S] (the layer after which each token halts, 1-based) that forces a decision pattern through the replay argument."""
    g = torch.Generator().manual_seed(5)
    rnd = torch.randint(1, L + 1, (B, S), generator=g).double()
    if which == "free":
        return None
    if which == "random":
        return rnd
    if which == "nobody_halts":
        return torch.full((B, S), float(L), dtype=torch.float64)
    if which == "all_halt_after_layer_1":
        return torch.ones(B, S, dtype=torch.float64)
    if which == "one_image_halted_one_untouched":
        rnd[1] = 1.0           # image 1 (it counts in the layer scores) runs on its representative row alone from layer 2 on
        rnd[2] = float(L)      # image 2 never packs
        return rnd
    assert which == "class_token_halts_early"
    rnd[:, :n_cls] = float(L)
    rnd[0, 0] = 1.0            # in image 0 (no score gradient) and image 3 a class token halts before the last layer
    rnd[3, n_cls - 1] = 2.0
    return rnd


PATTERNS = ["free", "random", "nobody_halts", "all_halt_after_layer_1", "one_image_halted_one_untouched", "class_token_halts_early"]


@pytest.mark.parametrize("kind", ["ce", "ponder", "prior", "yaml"])
@pytest.mark.parametrize("name", ["avit_micro", "avit_cls2_reg2"])
def test_packed_restatement_equals_the_dense_fp64_composite(name, kind):
    """Logits, rho_token, every layer score and every parameter gradient of the packed restatement against the dense fp64 composite replaying the same
    decisions, free-running and under every forced pattern: 1e-12 relative.  A parameter's gradient is measured against its own norm, or against
    1e-3 of the complete gradient's where its own is smaller than that (a gradient that is zero up to cancellation has no relative error of its own)."""
    worst_here = 0.0
    for which in PATTERNS:
        model, x, labels = _avit64(name)
        B, S, L, n_cls = 6, model.seq_length, len(model.encoder.layers), model.num_class_tokens
        counter = _pattern(which, B, S, L, n_cls)
        lg, rho, sc, cnt, _ = ref.model_forward(model, x, counter)
        ref.loss_terms(kind, lg, labels, rho, sc).backward()
        want = {n: p.grad for n, p in model.named_parameters()}
        model.zero_grad(set_to_none=True)
        plg, prho, psc, pcnt, got, rows = pref.packed_model_step(model, x, labels, kind, counter)
        assert torch.equal(pcnt, cnt), which
        if which == "nobody_halts":
            assert rows == [B * S] * L
        if which == "all_halt_after_layer_1":
            assert rows == [B * S] + [B] * (L - 1)
        if which not in ("free", "nobody_halts"):
            assert rows[-1] < B * S
        errs = {"logits": rel_l2(plg, lg), "rho": rel_l2(prho, rho), "scores": rel_l2(torch.stack(psc), torch.stack(sc))}
        total = float(torch.cat([g.reshape(-1) for g in want.values() if g is not None]).norm())
        for n, g64 in want.items():
            if g64 is None:
                assert got[n] is None or float(got[n].abs().max()) <= EXACT * total, (which, n)
                continue
            assert got[n] is not None, (which, n)
            errs[n] = float((got[n] - g64).norm()) / max(float(g64.norm()), 1e-3 * total, 1e-300)
        bad = {k: v for k, v in errs.items() if not v <= EXACT}
        assert not bad, (which, bad)
        worst_here = max(worst_here, max(errs.values()))
    print(name, kind, "worst relative difference", worst_here)


def test_pack_step_restatement_against_the_dense_step_on_one_layer():
    """pack_step_fwd on a hand-made packed input against avit_train_ref.act_step on the expanded dense rows: state, accumulated class rows, score and
    the next tables (a survivor keeps its order, one zero row with ln n, an image that halts everything keeps that one row)."""
    B, S, D, n_cls = 3, 5, 8, 1
    g = torch.Generator().manual_seed(1)
    m = torch.tensor([[1, 1, 0, 1, 0], [1, 1, 1, 1, 1], [0, 0, 0, 0, 0]], dtype=torch.float64)
    y = torch.randn(B, S, D, generator=g, dtype=torch.float64)
    y[:, :, 0] = 3.0 + 0.05 * torch.randn(B, S, generator=g, dtype=torch.float64)
    for b in range(B):
        y[b, m[b] == 0] = y[b, m[b] == 0][:1] if (m[b] == 0).any() else y[b, m[b] == 0]          # halted tokens of an image share one output
    c = torch.rand(B, S, generator=g, dtype=torch.float64) * 0.9
    c[1] = 0.0          # image 1 halts nothing; image 0 halts some
    c[m == 0] = 1.5     # a halted token sits above the threshold for good (its c is the one state entry the packed step leaves alone)
    Rr, rho, cnt = torch.rand(B, S, generator=g, dtype=torch.float64), torch.rand(B, S, generator=g, dtype=torch.float64), torch.ones(B, S, dtype=torch.float64)
    acc = torch.randn(B, n_cls, D, generator=g, dtype=torch.float64)
    d = ref.act_step(y, c, Rr, rho, cnt, m, acc, 10.0, 30.0, 0.99, False, n_cls)
    rows, pos, seg, nh = [], [], [0], []
    for b in range(B):
        live = [t for t in range(S) if m[b, t] == 1]
        rows += [y[b, t] for t in live]
        pos += live
        if len(live) < S:
            rows.append(y[b, [t for t in range(S) if m[b, t] == 0][0]]); pos.append(-1)
        nh.append(S - len(live)); seg.append(len(pos))
    st = pref.pack_step_fwd(torch.stack(rows), seg, nh, pos, (c, Rr, rho, cnt, m), acc, 10.0, 30.0, 0.99, False)
    assert torch.allclose(st["state"][0][m == 1], d[1][m == 1], rtol=1e-14, atol=0) and torch.equal(st["state"][0][m == 0], c[m == 0])
    for a, b_ in zip(st["state"][1:], (d[2], d[3], d[4], d[5])):
        assert torch.allclose(a, b_, rtol=1e-14, atol=0)
    assert torch.allclose(st["acc"], d[6], rtol=1e-14, atol=1e-300)
    assert abs(float(st["h_part"][1:].sum() / ((B - 1) * S) - d[7])) < 1e-15
    m1 = d[5]
    assert st["nh_next"].tolist() == [int(S - m1[b].sum()) for b in range(B)] and st["nh_next"][2] == S and st["seg_next"][3] - st["seg_next"][2] == 1
    assert st["pos_next"].tolist() == sum(([t for t in range(S) if m1[b, t] == 1] + ([-1] if m1[b].sum() < S else []) for b in range(B)), [])
    zero = st["pos_next"] < 0
    assert torch.equal(st["x_next"][zero], torch.zeros(int(zero.sum()), D, dtype=torch.float64)) and torch.equal(st["rs_next"], (~zero).double())
    assert torch.allclose(st["lm_next"][zero].exp(), st["nh_next"][st["nh_next"] > 0].double(), rtol=1e-14)


# ---- interface -------------------------------------------------------------------------------------------------------------------------------------
def test_packed_switch_leaves_cpu_forwards_on_the_composite_and_adds_no_state():
    model, x, _ = _avit64("avit_micro")
    model = model.float()
    keys = set(model.state_dict())
    want = model(x)
    model.set_packed_training(True)
    assert torch.equal(model(x), want) and set(model.state_dict()) == keys and not any("packed" in k for k in keys)
    model.set_fused_training(True)
    assert torch.equal(model(x), want)
    model.set_packed_training(False)
    assert model._pv_packed_training is False


def test_harness_key_defaults_to_off_and_is_wired():
    assert config.load_config("train_config", ["model=avit_t_16_224"])["training"]["packed_training"] is False
    assert config.load_config("train_config", ["model=avit_t_16_224", "training.packed_training=true"])["training"]["packed_training"] is True
    with pytest.raises(ValueError, match="set_packed_training"):
        htrain.main(["model=vit_tiny", "training.packed_training=true", "device=cpu", "dataset.image_size=32", "dataset.num_classes=10", "dataset.train_size=8",
                     "dataset.val_size=8", "training.train_batch_size=8", "training.num_epochs=1"])
    seen = []
    from peekvit_amd.models.adavit import AdaptiveVisionTransformer
    real = AdaptiveVisionTransformer.set_packed_training
    try:
        AdaptiveVisionTransformer.set_packed_training = lambda self, on=True: (seen.append(on), real(self, on))[1]
        htrain.main(["model=avit_t_16_224", "model.image_size=32", "model.patch_size=8", "model.hidden_dim=64", "model.mlp_dim=128", "model.num_layers=2",
                     "model.num_heads=1", "dataset.image_size=32", "dataset.num_classes=10", "dataset.train_size=8", "dataset.val_size=8", "device=cpu",
                     "training.train_batch_size=8", "training.num_epochs=1", "training.packed_training=true"])
    finally:
        AdaptiveVisionTransformer.set_packed_training = real
    assert seen == [True]


# ---- include/peekvit_hip_avit_pack_train.h: every declared entry point is exported, bound and has a test that calls it --------------------------------
LEDGER = {
    "pv_avit_pack_step_train": ["test_hip_avit_packed_train.py::test_pack_step_forward_against_fp64"],
    "pv_avit_pack_step_bwd": ["test_hip_avit_packed_train.py::test_pack_step_backward_against_fp64"],
}
WRAPPER = {"pv_avit_pack_step_train": "avit_pack_step_train", "pv_avit_pack_step_bwd": "avit_pack_step_bwd"}
HEADER = os.path.join(REPO, "include", "peekvit_hip_avit_pack_train.h")


def _declared():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pv_\w+)\s*\(", src, flags=re.M))


def _arity(name):
    m = re.search(r"\b(?:int|int64_t) " + name + r"\(([^;]*)\);", open(HEADER).read())
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_avit_pack_train_ledger_names_a_direct_test_for_every_declared_entry_point():
    from peekvit_amd import _build, _lib
    declared = _declared()
    assert set(LEDGER) == declared == set(_lib.SIGNATURES_AVIT_PACK_TRAIN), declared ^ set(LEDGER)
    assert "peekvit_hip_avit_pack_train.h" in _build.HEADERS and any(s.endswith("pv_avit_pack_train.hip") for s in _build.sources())
    main = re.sub(r"/\*.*?\*/", " ", open(os.path.join(REPO, "include", "peekvit_hip.h")).read(), flags=re.S)
    assert not any(re.search(rf"\b{n}\s*\(", main) for n in declared)          # a header of their own
    for name, (_, args) in _lib.SIGNATURES_AVIT_PACK_TRAIN.items():
        assert _arity(name) == len(args), name
        assert hasattr(_lib.load(), name) and hasattr(_lib.load("f16"), name)          # exported by both libraries
    assert _lib.load().pv_version() == 10 and _lib.load("f16").pv_version() == 10      # ABI unchanged
    ops_src = open(os.path.join(REPO, "peekvit_amd", "ops.py")).read()
    wrappers = {}
    for node in ast.parse(ops_src).body:
        if isinstance(node, ast.FunctionDef):
            for sym in re.findall(r"\b(pv_\w+)\(", ast.get_source_segment(ops_src, node)):
                wrappers.setdefault(sym, set()).add(node.name)
    for entry, fn in WRAPPER.items():
        assert wrappers[entry] == {fn}, entry
    te_src = open(os.path.join(REPO, "peekvit_amd", "train_engine.py")).read()
    assert "ops.avit_pack_step_train(" in te_src and "ops.avit_pack_step_bwd(" in te_src          # AViTPackStepFn
    for entry, ids in LEDGER.items():
        for tid in ids:
            fname, _, name = tid.partition("::")
            src = open(os.path.join(REPO, "tests", fname)).read()
            fn = next((n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == name), None)
            assert fn is not None, f"{entry}: {tid} does not exist"
            body = ast.get_source_segment(src, fn)
            assert re.search(rf"\b{entry}\b", body) and re.search(rf"\bops\.{WRAPPER[entry]}\b", body), tid


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from peekvit_amd import _lib
    null = C.c_void_p(0)
    for op in ("bf16", "f16"):
        lib = _lib.load(op)
        P = [C.c_void_p(4096 + 1024 * i) for i in range(27)]          # never dereferenced: every call below is refused before anything is launched

        def fwd(P=P, B=4, S=197, D=192, R=700, n_cls=1, last=0):
            return lib.pv_avit_pack_step_train(*P[:4], B, S, D, R, *P[4:16], n_cls, P[16], 10.0, 30.0, 0.99, last, *P[17:27], null)
        assert fwd(B=0) == -1 and fwd(B=-3) == -1 and fwd(S=0) == -1 and fwd(D=0) == -1 and fwd(R=0) == -1 and fwd(n_cls=0) == -1 and fwd(n_cls=198) == -1
        for i in range(27):
            assert fwd(P=P[:i] + [null] + P[i + 1:]) == -1, i
        optional = {17, 18, 19, 20, 21, 22, 23, 26}                 # with `last`: the next packed input, its tables, totals and src_next may be null
        for i in set(range(27)) - optional:
            assert fwd(P=P[:i] + [null] + P[i + 1:], last=1) == -1, i
        assert fwd(S=257) == -2 and fwd(D=190) == -2 and fwd(D=4100) == -2 and fwd(n_cls=17) == -2 and fwd(B=1 << 31) == -2 and fwd(R=1 << 31) == -2
        assert fwd(B=(1 << 31) // 197 + 1) == -2
        for i in (0, 14, 15, 17, 25):                                # y, acc_in, acc_out, x_next, ycls: 16 bytes
            assert fwd(P=P[:i] + [C.c_void_p(P[i].value + 8)] + P[i + 1:]) == -1, i
        for i in (1, 2, 3, 4, 9, 16, 18, 19, 20, 21, 22, 23, 24, 26):          # tables, state, h_part, sv, src_next: 4 bytes
            assert fwd(P=P[:i] + [C.c_void_p(P[i].value + 2)] + P[i + 1:]) == -1, i

        Q = P[:16]

        def bwd(Q=Q, B=4, S=197, D=192, R=700, Rn=650, n_cls=1, last=0):
            return lib.pv_avit_pack_step_bwd(*Q, B, S, D, R, Rn, n_cls, 10.0, last, null)
        for i in set(range(16)) - {11, 14}:                          # gh (11) and dy16 (14) are optional
            assert bwd(Q=Q[:i] + [null] + Q[i + 1:]) == -1, i
        for i in (1, 2, 3, 6, 7, 8, 9, 10, 12, 13, 15):
            assert bwd(Q=Q[:i] + [null] + Q[i + 1:], last=1) == -1, i
        assert bwd(B=0) == -1 and bwd(S=-1) == -1 and bwd(D=0) == -1 and bwd(R=0) == -1 and bwd(Rn=0) == -1 and bwd(n_cls=0) == -1 and bwd(n_cls=500) == -1
        assert bwd(Q=Q[:15] + [Q[8]]) == -1                          # dR must not be gR
        assert bwd(S=257) == -2 and bwd(D=194) == -2 and bwd(D=8192) == -2 and bwd(n_cls=17) == -2 and bwd(B=1 << 31) == -2 and bwd(R=1 << 31) == -2
        for i in (0, 7, 10, 13):                                     # g_next, ycls, gacc, dy: 16 bytes
            assert bwd(Q=Q[:i] + [C.c_void_p(Q[i].value + 8)] + Q[i + 1:]) == -1, i
        assert bwd(Q=Q[:14] + [C.c_void_p(Q[14].value + 4)] + Q[15:]) == -1           # dy16: 8 bytes
        for i in (1, 4, 5, 6, 8, 9, 11, 12, 15):
            assert bwd(Q=Q[:i] + [C.c_void_p(Q[i].value + 1)] + Q[i + 1:]) == -1, i
