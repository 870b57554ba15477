"""A-ViT past 208 tokens without a GPU: the four training rules of AdaptiveVisionTransformer side by side, the argument
checks of include/peekvit_hip_avit_long.h's two entry points through ctypes, the fixture of scripts/make_golden_avit_long.py, and the fp64
restatement of the packed pass (tests/avit_packed_train_ref.py) against the dense fp64 composite at 226 and 257 rows."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest
import torch

import avit_packed_train_ref as pref
import avit_train_ref as ref
from conftest import GOLDEN, REPO, rel_l2
from peekvit_amd import synth

META = json.load(open(os.path.join(GOLDEN, "avit_long_meta.json")))
HEADER = os.path.join(REPO, "include", "peekvit_hip_avit_long.h")
EXACT = 1e-12           # tests/test_avit_packed_train_host.py's bound: the restatement differs from the dense composite by fp64 rounding alone


# ---- the rules ----
class _Cuda:              # (what train_eligible reads of a tensor; real GPU tensors are exercised in tests/test_hip_avit_long.py)
    is_cuda = True


def _model(rows=226, dh=64, heads=2, **over):
    """A small A-ViT whose rules are then read at `rows` tokens (every rule reads seq_length; a square patch grid cannot land on every count)."""
    from peekvit_amd.models.adavit import AdaptiveVisionTransformer
    kw = dict(image_size=32, patch_size=8, num_layers=2, num_heads=heads, hidden_dim=dh * heads, mlp_dim=64, num_classes=10)
    m = AdaptiveVisionTransformer(**dict(kw, **over)).train()
    m.seq_length = rows
    return m


RULES = [  # rows, dh, resident packed, resident fused, long fused, long packed
    (197, 64, True, True, False, False),
    (208, 64, True, True, False, False),
    (209, 64, False, False, True, True),
    (226, 64, False, False, True, True),
    (4096, 64, False, False, True, True),
    (4097, 64, False, False, False, False),
    (401, 32, False, True, False, False),
    (416, 32, False, True, False, False),
    (417, 32, False, False, True, False),
    (442, 32, False, False, True, False),
    (442, 48, False, False, True, False),
]


@pytest.mark.parametrize("rows,dh,packed,fused,long_fused,long_packed", RULES)
def test_rule_table(rows, dh, packed, fused, long_fused, long_packed):
    m = _model(rows, dh)
    got = (m._packed_training_ok(), m._fused_training_ok(), m._long_fused_training_ok(), m._long_packed_training_ok())
    assert got == (packed, fused, long_fused, long_packed), (rows, dh, got)
    assert not (got[0] and got[3]) and not (got[1] and got[2])          # a resident rule and its long one never both hold


def test_long_packed_refuses_17_class_tokens_and_models_without_layers():
    assert _model(226, num_class_tokens=16)._long_packed_training_ok()
    m = _model(226, num_class_tokens=17)
    assert not m._long_packed_training_ok() and m._long_fused_training_ok()
    m = _model(226)
    del m.encoder.layers[:]
    assert not m._long_packed_training_ok()


class _CudaTensor(_Cuda):
    def numel(self):
        return 1


def test_cpu_tensors_dropout_and_split_precision_are_refused_as_before():
    """The long rules sit behind train_engine.train_eligible exactly as the resident ones do: what that refuses never reaches them."""
    from peekvit_amd import engine, train_engine
    m = _model(226)
    assert train_engine.train_eligible(_CudaTensor(), m, 0.0)
    assert not train_engine.train_eligible(torch.zeros(1, 3, 32, 32), m, 0.0)          # a CPU tensor
    assert not train_engine.train_eligible(_CudaTensor(), m, 0.1)                      # dropout
    with engine.precision("bf16x3"):
        assert not train_engine.train_eligible(_CudaTensor(), m, 0.0)                  # no split-precision training kernels
    with torch.no_grad():
        assert not train_engine.train_eligible(_CudaTensor(), m, 0.0)


def test_cpu_forward_with_both_switches_on_is_the_composite_at_226_tokens():
    from peekvit_amd.models.adavit import AdaptiveVisionTransformer
    kw = dict(image_size=120, patch_size=8, num_layers=2, num_heads=1, hidden_dim=64, mlp_dim=64, num_classes=10, gate_center=2.0)
    torch.manual_seed(0)
    m = AdaptiveVisionTransformer(**kw).train()
    assert m.seq_length == 226 and m._long_packed_training_ok() and m._long_fused_training_ok()
    assert not m._packed_training_ok() and not m._fused_training_ok()
    x = torch.randn(2, 3, 120, 120, generator=torch.Generator().manual_seed(1))
    a = m(x)
    m.set_fused_training(True)
    m.set_packed_training(True)
    assert torch.equal(m(x), a)
    assert set(m.state_dict()) == set(AdaptiveVisionTransformer(**kw).state_dict())


# ---- the header and its bindings ----
def test_header_declares_what_the_library_exports_and_the_package_binds():
    from peekvit_amd import _build, _lib, ops
    declared = set(re.findall(r"^int (pv_\w+)\(", open(HEADER).read(), re.M))
    assert declared == {"pv_avit_pack_step_long", "pv_avit_pack_step_long_bwd"} == set(_lib.SIGNATURES_AVIT_LONG)
    assert "peekvit_hip_avit_long.h" in _build.HEADERS
    assert _build.FILE_FLAGS["pv_avit_long.hip"] == _build.FILE_FLAGS["pv_avit_pack_train.hip"]          # they must round alike
    assert _lib.SIGNATURES_AVIT_LONG["pv_avit_pack_step_long"] == _lib.SIGNATURES_AVIT_PACK_TRAIN["pv_avit_pack_step_train"]
    assert _lib.SIGNATURES_AVIT_LONG["pv_avit_pack_step_long_bwd"] == _lib.SIGNATURES_AVIT_PACK_TRAIN["pv_avit_pack_step_bwd"]
    assert callable(ops.avit_pack_step_long) and callable(ops.avit_pack_step_long_bwd) and ops.AVIT_LONG_MAX_S == 4096
    assert re.search(r"#define PV_AVIT_LONG_MAX_S 4096\b", open(HEADER).read())
    assert re.search(r"#define PV_AVIT_PACK_MAX_S 256\b", open(os.path.join(REPO, "include", "peekvit_hip_avit_pack_train.h")).read())
    for op in ("bf16", "f16"):
        lib = _lib.load(op)
        assert lib.pv_version() == 10
        for name in declared:
            assert getattr(lib, name).argtypes is not None


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """tests/test_avit_packed_train_host.py's checks of the resident pair, at the long bound - and the rule for the saves."""
    from peekvit_amd import _lib
    null = C.c_void_p(0)
    for op in ("bf16", "f16"):
        lib = _lib.load(op)
        P = [C.c_void_p(4096 + 1024 * i) for i in range(27)]          # never dereferenced: every call below is refused before anything is launched

        def fwd(P=P, B=4, S=442, D=192, R=1700, n_cls=1, last=0):
            return lib.pv_avit_pack_step_long(*P[:4], B, S, D, R, *P[4:16], n_cls, P[16], 10.0, 30.0, 0.99, last, *P[17:27], null)

        def without(*idx):
            return [null if i in idx else p for i, p in enumerate(P)]
        assert fwd(B=0) == -1 and fwd(B=-3) == -1 and fwd(S=0) == -1 and fwd(D=0) == -1 and fwd(R=0) == -1 and fwd(n_cls=0) == -1 and fwd(n_cls=443) == -1
        for i in set(range(27)) - {24, 25, 26}:
            assert fwd(P=without(i)) == -1, i
        optional = {17, 18, 19, 20, 21, 22, 23, 26}                 # with `last`: the next packed input, its tables, totals and src_next may be null
        for i in set(range(27)) - optional - {24, 25}:
            assert fwd(P=without(i), last=1) == -1, i
        # the saves sv (24), ycls (25), src_next (26): all or none
        for last in (0, 1):
            for part in ((24,), (25,), (24, 25), (24, 26), (25, 26)):
                assert fwd(P=without(*part), last=last) == -1, (part, last)
        assert fwd(P=without(26)) == -1                              # a training step that is not the last needs src_next ...
        assert fwd(S=4097) == -2 and fwd(D=190) == -2 and fwd(D=4100) == -2 and fwd(n_cls=17) == -2 and fwd(B=1 << 31) == -2 and fwd(R=1 << 31) == -2
        assert fwd(P=without(26), last=1, S=4097) == -2              # ... the last one does not: it gets as far as the size checks
        assert fwd(P=without(24, 25, 26), S=4097) == -2 and fwd(P=without(24, 25, 26), S=4097, last=1) == -2          # and so does the inference step
        assert fwd(B=(1 << 31) // 442 + 1) == -2
        for i in (0, 14, 15, 17, 25):                                # y, acc_in, acc_out, x_next, ycls: 16 bytes
            assert fwd(P=P[:i] + [C.c_void_p(P[i].value + 8)] + P[i + 1:]) == -1, i
        for i in (1, 2, 3, 4, 9, 16, 18, 19, 20, 21, 22, 23, 24, 26):          # tables, state, h_part, sv, src_next: 4 bytes
            assert fwd(P=P[:i] + [C.c_void_p(P[i].value + 2)] + P[i + 1:]) == -1, i

        Q = P[:16]

        def bwd(Q=Q, B=4, S=442, D=192, R=1700, Rn=1650, n_cls=1, last=0):
            return lib.pv_avit_pack_step_long_bwd(*Q, B, S, D, R, Rn, n_cls, 10.0, last, null)
        for i in set(range(16)) - {11, 14}:                          # gh (11) and dy16 (14) are optional
            assert bwd(Q=Q[:i] + [null] + Q[i + 1:]) == -1, i
        for i in (1, 2, 3, 6, 7, 8, 9, 10, 12, 13, 15):
            assert bwd(Q=Q[:i] + [null] + Q[i + 1:], last=1) == -1, i
        assert bwd(B=0) == -1 and bwd(S=-1) == -1 and bwd(D=0) == -1 and bwd(R=0) == -1 and bwd(Rn=0) == -1 and bwd(n_cls=0) == -1 and bwd(n_cls=500) == -1
        assert bwd(Q=Q[:15] + [Q[8]]) == -1                          # dR must not be gR
        assert bwd(S=4097) == -2 and bwd(D=194) == -2 and bwd(D=8192) == -2 and bwd(n_cls=17) == -2 and bwd(B=1 << 31) == -2 and bwd(R=1 << 31) == -2
        for i in (0, 7, 10, 13):                                     # g_next, ycls, gacc, dy: 16 bytes
            assert bwd(Q=Q[:i] + [C.c_void_p(Q[i].value + 8)] + Q[i + 1:]) == -1, i
        assert bwd(Q=Q[:14] + [C.c_void_p(Q[14].value + 4)] + Q[15:]) == -1           # dy16: 8 bytes
        for i in (1, 4, 5, 6, 8, 9, 11, 12, 15):
            assert bwd(Q=Q[:i] + [C.c_void_p(Q[i].value + 1)] + Q[i + 1:]) == -1, i


# ---- the fixture ----
def test_fixture_and_its_metadata():
    from oracle import make_golden as MG
    g = np.load(os.path.join(GOLDEN, "avit_long.npz"))
    assert set(META["reference_sha256"]) == set(META["reference_files"]) == {"models/adavit.py", "models/blocks.py"}
    if os.path.isdir(MG.REF_ROOT):                                   # (where the reference checkout is: the fixtures were made from THIS revision)
        for f, sha in META["reference_sha256"].items():
            assert hashlib.sha256(open(os.path.join(MG.REF_ROOT, f), "rb").read()).hexdigest() == sha, f
    assert sorted(META["cases"]) == ["avit_long_226", "avit_long_257", "avit_long_260", "avit_long_442"]
    longest = []
    for name, case in META["cases"].items():
        kw, B, S, L = case["kwargs"], case["batch"], case["tokens"], case["kwargs"]["num_layers"]
        assert (kw["hidden_dim"], kw["num_heads"], kw["mlp_dim"], L, kw["patch_size"], kw["num_classes"]) == (128, 2, 256, 4, 8, 10) and B == 4
        assert S == int(name.rsplit("_", 1)[1]) == (kw["image_size"] // 8) ** 2 + kw.get("num_class_tokens", 1) + kw.get("num_registers", 0)
        assert g[name + "/logits"].shape == (B, 10) and g[name + "/rho_token"].shape == g[name + "/counter_token"].shape == (B, S)
        assert g[name + "/halting_score_layer"].shape == (L,) and g[name + "/h_token"].shape == (L, B, S) and g[name + "/margin"].shape == (B, S)
        depth = g[name + "/counter_token"]
        assert set(np.unique(depth)) == {1.0, 2.0, 3.0, 4.0}                         # the depths spread over 1 .. 4
        assert case["depth_histogram"] == [int((depth == d).sum()) for d in (1, 2, 3, 4)]
        live = [(depth > l).sum(axis=1) for l in range(1, L)]
        assert case["longest_segment_into_layer"] == [int((n + (n < S)).max()) for n in live]
        assert np.allclose(g[name + "/margin"].min(axis=1), case["min_margin_per_image"], rtol=0, atol=1e-9)
        assert case["fp64_composite_logits_rel_l2"] < 1e-5
        longest.append(case["longest_segment_into_layer"])
    assert any(l[0] > 256 for l in longest) and any(min(l) <= 208 for l in longest)
    assert META["cases"]["avit_long_260"]["kwargs"]["num_class_tokens"] == 2 and META["cases"]["avit_long_260"]["kwargs"]["num_registers"] == 2
    assert len(g.files) == 4 * 6 and os.path.getsize(os.path.join(GOLDEN, "avit_long.npz")) < 1 << 20


def _long_model(name, batch=None, train=False):
    from peekvit_amd.models.adavit import AdaptiveVisionTransformer
    case = META["cases"][name]
    model = AdaptiveVisionTransformer(**case["kwargs"])
    model = model.train() if train else model.eval()
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(case["synth_cfg"], seed=case["seed"]).items()}, strict=True)
    x = torch.from_numpy(synth.synth_images(batch or case["batch"], case["kwargs"]["image_size"], seed=case["seed"], name="avit"))
    return model, x


@pytest.mark.parametrize("name", sorted(META["cases"]))
def test_the_fp64_composite_reproduces_the_reference_depths_on_every_image(name):
    """What scripts/make_golden_avit_long.py asserted before it wrote the fixture, again on the committed arrays."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    g = np.load(os.path.join(GOLDEN, "avit_long.npz"))
    model, x = _long_model(name)
    with torch.no_grad():
        logits = model.double()._composite_forward(x.double())
    assert np.array_equal(model.encoder.counter_token.numpy(), g[name + "/counter_token"])
    assert rel_l2(logits, g[name + "/logits"]) < 1e-5
    assert np.allclose(model.encoder.rho_token.numpy(), g[name + "/rho_token"], atol=1e-5)


# ---- the checker of the GPU training tests past 208 rows ----
@pytest.mark.parametrize("name", ["avit_long_226", "avit_long_257"])
def test_packed_restatement_equals_the_dense_fp64_composite_past_208_rows(name):
    """tests/avit_packed_train_ref.py (imported, not edited) at 226 and 257 rows: logits, rho_token, layer scores and every parameter gradient under
    the combined loss against the dense fp64 composite on the same decisions, 1e-12 relative (tests/test_avit_packed_train_host.py's measure)."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    model, x = _long_model(name, batch=3, train=True)
    model = model.double()
    labels = torch.arange(3) % 10
    lg, rho, sc, cnt, _ = ref.model_forward(model, x, None)
    ref.loss_terms("yaml", lg, labels, rho, sc).backward()
    want = {n: p.grad for n, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    plg, prho, psc, pcnt, got, rows = pref.packed_model_step(model, x, labels, "yaml", None)
    S = model.seq_length
    assert torch.equal(pcnt, cnt) and rows[0] == 3 * S and rows[-1] < 3 * S and all(a >= b for a, b in zip(rows, rows[1:]))
    errs = {"logits": rel_l2(plg, lg), "rho": rel_l2(prho, rho), "scores": rel_l2(torch.stack(psc), torch.stack(sc))}
    total = float(torch.cat([g.reshape(-1) for g in want.values() if g is not None]).norm())
    for n, g64 in want.items():
        if g64 is None:
            assert got[n] is None or float(got[n].abs().max()) <= EXACT * total, n
            continue
        assert got[n] is not None, n
        errs[n] = float((got[n] - g64).norm()) / max(float(g64.norm()), 1e-3 * total, 1e-300)
    bad = {k: v for k, v in errs.items() if not v <= EXACT}
    assert not bad, bad
