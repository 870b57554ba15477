"""EEResidualVisionTransformer (reference models/eeresidualvit.py) without a GPU: the Hydra target, the module surface against the reference's
constructor and state-dict keys (tests/golden/ee_meta.json), the stock-op composite against the reference's golden lists, masks and
gradients (scripts/make_golden_ee.py), select_exits against the fp64 decisions stored with them, the budget errors, the special-token quirk,
the plain-ViT key contract, the harness config, a checkpoint round trip, the FLOP count, a test ledger for include/peekvit_hip_ee.h and the
argument checks of its entry points."""
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

from conftest import GOLDEN, REPO
from peekvit_amd import synth

META = json.load(open(os.path.join(GOLDEN, "ee_meta.json")))
CASES = sorted(META["cases"])
EVAL_CASES = [n for n in CASES if not META["cases"][n]["train"]]


def _model(name):
    from peekvit_amd.models.eeresidualvit import EEResidualVisionTransformer
    case = META["cases"][name]
    model = EEResidualVisionTransformer(**case["kwargs"])
    sd = synth.ee_state_dict(case["synth_cfg"], seed=0)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    model.train(case["train"])
    if case["budget"] is not None:
        model.set_budget(case["budget"])
    return model


def _images(name, g):
    case = META["cases"][name]
    if "images" in g:
        return torch.from_numpy(g["images"])
    return torch.from_numpy(synth.ee_images(case["pool"], case["kwargs"]["image_size"], seed=0)[g["pool_index"]])


def _golden_list(name, g):
    return [torch.from_numpy(g[f"out_{i}"]) for i in range(META["cases"][name]["kwargs"]["num_layers"] + 1)]


def test_hydra_target_resolves():
    from peekvit_amd.harness import config
    from peekvit_amd.models.eeresidualvit import EEResidualViTEncoder, EEResidualVisionTransformer
    mod = importlib.import_module("peekvit.models.eeresidualvit")
    assert mod.EEResidualVisionTransformer is EEResidualVisionTransformer and mod.EEResidualViTEncoder is EEResidualViTEncoder
    assert callable(mod.select_exits)
    m = config.instantiate({"_target_": "peekvit.models.eeresidualvit.EEResidualVisionTransformer", **META["cases"]["ee_micro"]["kwargs"]})
    assert isinstance(m, EEResidualVisionTransformer) and len(m.encoder.early_exit_heads) == 4


def test_surface_matches_reference():
    from peekvit_amd.models.eeresidualvit import EEResidualVisionTransformer as cls
    from peekvit_amd.models.residualvit import ResidualViTBlock
    sig = inspect.signature(cls.__init__)
    assert [k for k in sig.parameters if k != "self"] == META["constructor_parameters"]
    defaults = {k: p.default for k, p in sig.parameters.items() if k != "self" and p.default is not inspect.Parameter.empty}
    assert defaults == META["constructor_defaults"]
    for name in CASES:
        m = cls(**META["cases"][name]["kwargs"])
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == META["cases"][name]["state_dict"], name
        assert all(type(b) is ResidualViTBlock for b in m.encoder.layers)
        # LayerNorm eps: torch's default on encoder.ln and the exit heads, 1e-6 inside the blocks
        assert m.encoder.ln.eps == 1e-5 and all(h[0].eps == 1e-5 for h in m.encoder.early_exit_heads)
        assert all(b.ln_1.eps == 1e-6 and b.ln_2.eps == 1e-6 for b in m.encoder.layers)
        assert m.current_budget is None
    m = cls(**META["cases"]["ee_micro"]["kwargs"])
    sd = m.state_dict()
    for i in range(4):
        assert sd[f"encoder.early_exit_heads.{i}.0.weight"].shape == (128,) and sd[f"encoder.early_exit_heads.{i}.1.weight"].shape == (10, 128)
        assert sd[f"encoder.early_exit_heads.{i}.0.bias"].shape == (128,) and sd[f"encoder.early_exit_heads.{i}.1.bias"].shape == (10,)
    assert sd["learnable_budget_token_1"].shape == (1, 1, 128) and sd["learnable_budget_token_2"].shape == (1, 1, 128)


@pytest.mark.parametrize("name", EVAL_CASES)
def test_composite_matches_reference_golden(name, golden):
    g = golden(name)
    model = _model(name)
    with torch.no_grad():
        outs = model(_images(name, g))
    L = META["cases"][name]["kwargs"]["num_layers"]
    assert isinstance(outs, list) and len(outs) == L + 1
    assert [list(o.shape) for o in outs] == META["cases"][name]["out_shapes"]
    for i, o in enumerate(outs):
        np.testing.assert_allclose(o.numpy(), g[f"out_{i}"], rtol=0, atol=1e-5, err_msg=f"{name} out_{i}")
    for i, blk in enumerate(model.encoder.layers):
        assert blk.mask.shape == g[f"mask_{i}"].shape
        np.testing.assert_allclose(blk.mask.numpy(), g[f"mask_{i}"], rtol=0, atol=1e-5, err_msg=f"{name} mask_{i}")


def test_batch_one_shapes(golden):
    g = golden("ee_batch1")
    model = _model("ee_batch1")
    with torch.no_grad():
        outs = model(_images("ee_batch1", g))
    assert [tuple(o.shape) for o in outs] == [(10,)] * 4 + [(1, 10)]
    with torch.no_grad():
        outs = model(torch.from_numpy(synth.ee_images(3, 32, seed=1)))
    assert [tuple(o.shape) for o in outs] == [(3, 10)] * 5


def test_eval_without_a_budget_and_budget_zero_raise():
    model = _model("ee_micro")
    x = torch.from_numpy(synth.ee_images(2, 32, seed=0))
    model.current_budget = None
    with pytest.raises(ValueError, match="Budget token not set"), torch.no_grad():
        model(x)
    model.set_budget(0.0)                       # the reference tests truthiness
    with pytest.raises(ValueError, match="Budget token not set"), torch.no_grad():
        model(x)
    with pytest.raises(ValueError, match="Budget token not set"), torch.no_grad():
        model.early_exit(x, 0.5)
    model.set_budget(0.3)
    assert model.current_budget == 0.3 and isinstance(model.current_budget, float)
    with torch.no_grad():
        assert len(model(x)) == 5


def test_two_class_tokens_and_a_register_pin_row_zero_and_one_special_token(golden):
    name = "ee_2cls1reg"
    g = golden(name)
    model = _model(name)
    assert META["cases"][name]["block_special_tokens"] == [1] * 4
    assert all(b.num_special_tokens == 1 for b in model.encoder.layers) and model.encoder.num_class_tokens == 1
    assert model.num_class_tokens == 2 and model.num_registers == 1 and model.num_special_tokens == 3
    seen = []
    hooks = [h.register_forward_hook(lambda m, i, o: seen.append(i[0])) for h in model.encoder.early_exit_heads]
    with torch.no_grad():
        outs = model(_images(name, g))
    for h in hooks:
        h.remove()
    assert all(tuple(t.shape) == (6, 1, 128) for t in seen)                 # every exit head reads row 0 only
    # 16 patches + 2 class tokens + 1 register + the budget token = 20 rows; one special row -> 18 gated rows
    assert all(tuple(b.mask.shape) == (6, 18, 1) for b in model.encoder.layers)
    # ... while the final head sums BOTH class rows of encoder.ln's output
    feats = []
    hook = model.encoder.ln.register_forward_hook(lambda m, i, o: feats.append(o))
    with torch.no_grad():
        model(_images(name, g))
    hook.remove()
    want = model.head(feats[0][:, 0:2].sum(dim=1))
    np.testing.assert_allclose(outs[-1].numpy(), want.detach().numpy(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(outs[-1].numpy(), g["out_4"], rtol=0, atol=1e-5)


def test_train_mode_gradients_match_reference_golden(golden):
    name = "ee_train"
    g = golden(name)
    model = _model(name)
    assert model.training
    x, y = _images(name, g), torch.from_numpy(g["labels"])
    outs = model(x)
    assert isinstance(outs, list) and len(outs) == 5 and model.current_budget == pytest.approx(0.7, abs=1e-6)
    loss = sum(torch.nn.functional.cross_entropy(o, y) for o in outs)
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-5
    for i, o in enumerate(outs):
        np.testing.assert_allclose(o.detach().numpy(), g[f"out_{i}"], rtol=0, atol=1e-5)
    for i, blk in enumerate(model.encoder.layers):
        np.testing.assert_allclose(blk.mask.detach().numpy(), g[f"mask_{i}"], rtol=0, atol=1e-5)
    params = dict(model.named_parameters())
    keys = [k[len("grad/"):] for k in g.files if k.startswith("grad/")]
    assert len(keys) >= 20 and any(k.startswith("encoder.early_exit_heads.3.1") for k in keys)
    for k in keys:
        # the list is held to atol 1e-5 at |logit| ~ 1; a gradient tensor whose largest element is ~8 (class_tokens: the sum over 4 images and 5
        # losses) carries the same RELATIVE fp32 reassociation noise, so the bound scales with the tensor's largest magnitude, never below 1e-5
        want = g["grad/" + k]
        np.testing.assert_allclose(params[k].grad.numpy(), want, rtol=0, atol=1e-5 * max(1.0, float(np.abs(want).max())), err_msg=k)


def test_train_mode_samples_a_budget_per_forward():
    from peekvit_amd.models.eeresidualvit import EEResidualVisionTransformer
    kw = dict(META["cases"]["ee_micro"]["kwargs"])
    x = torch.from_numpy(synth.ee_images(2, 32, seed=0))
    torch.manual_seed(0)
    m = EEResidualVisionTransformer(**dict(kw, add_budget_token=[0.25, 0.5, 0.75])).train()      # the list branch (torch.randint)
    seen = set()
    for _ in range(12):
        m(x)
        seen.add(m.current_budget)
    assert seen <= {0.25, 0.5, 0.75} and len(seen) >= 2
    m = EEResidualVisionTransformer(**dict(kw, add_budget_token="learnable_interpolate")).train()
    m(x)
    b1 = m.current_budget
    outs = m(x)
    assert isinstance(b1, float) and 0.0 <= b1 < 1.0 and m.current_budget != b1
    sum(o.sum() for o in outs).backward()
    assert float(m.learnable_budget_token_1.grad.abs().sum()) > 0 and float(m.learnable_budget_token_2.grad.abs().sum()) > 0
    m = EEResidualVisionTransformer(**kw).train()                       # 'learnable': both tokens exist, only the first is used
    sum(o.sum() for o in m(x)).backward()
    assert float(m.learnable_budget_token_1.grad.abs().sum()) > 0 and m.learnable_budget_token_2.grad is None


@pytest.mark.parametrize("name", CASES)
def test_select_exits_on_the_golden_lists(name, golden):
    from peekvit_amd.models.eeresidualvit import select_exits
    g = golden(name)
    case = META["cases"][name]
    L, B = case["kwargs"]["num_layers"], case["batch"]
    outs = _golden_list(name, g)
    for t in case["thresholds"]:
        res = select_exits(outs, t)
        want = g[f"exit_layer_{t}"]
        assert res.exit_layer.dtype == torch.int64 and np.array_equal(res.exit_layer.numpy(), want), (name, t)
        for b in range(B):
            row = outs[int(want[b])].reshape(B, -1)[b]
            assert torch.equal(res.logits[b], row)                        # bit for bit
            assert abs(float(res.confidence[b]) - float(g["conf"][int(want[b]), b])) < 1e-6
        assert res.live is None
    hist = {int(k): v for k, v in case["exit_histogram"][str(case["thresholds"][0])].items()}
    assert hist == {int(k): int(v) for k, v in zip(*np.unique(g[f"exit_layer_{case['thresholds'][0]}"], return_counts=True))}
    assert L + 1 == len(outs)


def test_fixture_condition_holds(golden):
    """No image of any fixture sits within the recorded margin of a threshold at any layer; cases of three or more images exit at three or
    more layers, the final head among them."""
    for name in CASES:
        g, case = golden(name), META["cases"][name]
        L = case["kwargs"]["num_layers"]
        assert case["margin"] >= 0.02
        for t in case["thresholds"]:
            assert float(np.abs(g["conf"][:L] - t).min()) >= case["margin"], (name, t)
            layers = set(g[f"exit_layer_{t}"].tolist())
            if case["batch"] >= 3:
                assert len(layers) >= 3 and L in layers, (name, t, layers)


def test_select_exits_edge_thresholds_and_exit_layers(golden):
    from peekvit_amd.models.eeresidualvit import select_exits
    g = golden("ee_micro")
    outs = _golden_list("ee_micro", g)
    res = select_exits(outs, 1.0001)
    assert bool((res.exit_layer == 4).all()) and torch.equal(res.logits, outs[4])
    for t in (0.0, -1.0):
        res = select_exits(outs, t)
        assert bool((res.exit_layer == 0).all()) and torch.equal(res.logits, outs[0])
        res = select_exits(outs, t, exit_layers=[2, 3])
        assert bool((res.exit_layer == 2).all()) and torch.equal(res.logits, outs[2])
    t = META["cases"]["ee_micro"]["thresholds"][0]
    full = g[f"exit_layer_{t}"]
    res = select_exits(outs, t, exit_layers=[1, 3])
    conf = g["conf"]
    want = np.where(conf[1] >= t, 1, np.where(conf[3] >= t, 3, 4))
    assert np.array_equal(res.exit_layer.numpy(), want) and not np.array_equal(want, full)
    assert np.array_equal(select_exits(outs, t, exit_layers=(3, 1, 3)).exit_layer.numpy(), want)
    with pytest.raises(ValueError):
        select_exits(outs, t, exit_layers=[4])
    # exactly on the threshold exits: two equal logits give p = 0.5
    tie = [torch.tensor([[1.0, 1.0], [0.0, 1.0]]), torch.tensor([[0.0, 0.0], [0.0, 0.0]])]
    assert select_exits(tie, 0.5).exit_layer.tolist() == [0, 0] and select_exits(tie, 0.75).exit_layer.tolist() == [1, 1]
    # on CPU early_exit is select_exits(self(x))
    model = _model("ee_micro")
    x = _images("ee_micro", g)
    with torch.no_grad():
        a, b = model.early_exit(x, t, exit_layers=[1, 3]), select_exits(model(x), t, exit_layers=[1, 3])
    assert torch.equal(a.logits, b.logits) and torch.equal(a.exit_layer, b.exit_layer) and torch.equal(a.confidence, b.confidence)
    assert np.array_equal(a.exit_layer.numpy(), want)


def test_plain_vit_state_dict_leaves_only_heads_gates_and_budget_tokens_missing():
    from peekvit_amd.models.vit import VisionTransformer
    kw = META["cases"]["ee_micro"]["kwargs"]
    vit = VisionTransformer(**{k: kw[k] for k in ("image_size", "patch_size", "num_layers", "num_heads", "hidden_dim", "mlp_dim", "num_classes")})
    model = _model("ee_micro")
    res = model.load_state_dict(vit.state_dict(), strict=False)
    assert list(res.unexpected_keys) == []
    want = {"learnable_budget_token_1", "learnable_budget_token_2"}
    for i in range(4):
        want |= {f"encoder.early_exit_heads.{i}.{j}.{p}" for j in (0, 1) for p in ("weight", "bias")}
        want |= {f"encoder.layers.{i}.residual_gate.projection.{p}" for p in ("weight", "bias")}
        want |= {f"encoder.layers.{i}.budget_token_gate.{p}" for p in ("weight", "bias")}
    assert set(res.missing_keys) == want
    assert torch.equal(model.encoder.layers[2].mlp.fc1.weight, vit.encoder.layers[2].mlp.fc1.weight)


def test_harness_config_builds_the_model():
    from peekvit_amd.harness import config
    from peekvit_amd.models.eeresidualvit import EEResidualVisionTransformer
    cfg = config.load_config("test_config", ["model=eeresidualvit", "dataset.num_classes=10", "dataset.image_size=160"])
    m = cfg["model"]
    assert m["_target_"] == "peekvit.models.eeresidualvit.EEResidualVisionTransformer"
    assert (m["patch_size"], m["hidden_dim"], m["mlp_dim"], m["num_layers"], m["num_heads"]) == (8, 256, 768, 4, 4)
    assert m["dropout"] == 0.1 and m["attention_dropout"] == 0.1 and m["gate_type"] == "sigmoid" and m["gate_bias"] == 1
    assert m["add_budget_token"] == "learnable" and list(m["residual_layers"]) == ["attention+mlp"] * 4 and m["add_input"] is False
    model = config.instantiate(m)
    assert isinstance(model, EEResidualVisionTransformer) and model.seq_length == 401 and len(model.encoder.early_exit_heads) == 4


def test_checkpoint_round_trip_reproduces_the_list(tmp_path, golden):
    from peekvit_amd.harness import checkpoint
    from peekvit_amd.models.eeresidualvit import EEResidualVisionTransformer
    g = golden("ee_micro")
    model = _model("ee_micro")
    args = {"_target_": "peekvit.models.eeresidualvit.EEResidualVisionTransformer", **META["cases"]["ee_micro"]["kwargs"]}
    file = checkpoint.save_state(str(tmp_path), model, args)
    loaded, state = checkpoint.load_state(file)
    assert type(loaded) is EEResidualVisionTransformer and state["model_class"] == "EEResidualVisionTransformer"
    loaded.eval().set_budget(0.7)
    x = _images("ee_micro", g)
    with torch.no_grad():
        a, b = model(x), loaded(x)
    assert len(a) == len(b) == 5 and all(torch.equal(p, q) for p, q in zip(a, b))


def test_flops_count_blocks_as_residualvit_plus_exit_heads():
    from peekvit_amd import flops
    from peekvit_amd.models.residualvit import ResidualVisionTransformer
    kw = dict(META["cases"]["ee_micro"]["kwargs"])
    ee = _model("ee_micro")
    res = ResidualVisionTransformer(**kw)
    D, Cn, L = 128, 10, 4
    assert flops.model_flops(ee) - flops.model_flops(res) == 2.0 * L * (2 * D + D * Cn + Cn)
    x = torch.from_numpy(synth.ee_images(2, 32, seed=0))
    f, sparsity = flops.measured_flops(ee, x)
    assert f > 0 and 0.0 <= sparsity < 1.0
    per = flops.hook_macs(ee, x)["per_module_macs"]
    assert per["encoder.early_exit_heads.3.1"] == (D * Cn + Cn) * 2 and per["head"] == (D * Cn + Cn) * 2


# ---- include/peekvit_hip_ee.h: every declared entry point is exported and has a test that calls it directly ----
LEDGER = {
    "pv_exit_head_f32": ["test_hip_ee.py::test_exit_head_bit_identical_to_cls_pool_and_head", "test_hip_ee.py::test_exit_head_against_fp64"],
    "pv_exit_step": ["test_hip_ee.py::test_exit_step_against_torch_and_fp64", "test_hip_ee.py::test_exit_step_threshold_ties_and_extremes"],
    "pv_gather_images_f32": ["test_hip_ee.py::test_gather_images_exact"],
}


def _declared():
    src = open(os.path.join(REPO, "include", "peekvit_hip_ee.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pv_\w+)\s*\(", src, flags=re.M))


def _arity(name):
    header = open(os.path.join(REPO, "include", "peekvit_hip_ee.h")).read()
    m = re.search(r"\b(?:int|int64_t) " + name + r"\(([^;]*)\);", header)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_ee_ledger_names_a_direct_test_for_every_declared_entry_point():
    from peekvit_amd import _lib
    declared = _declared()
    assert set(LEDGER) == declared == set(_lib.SIGNATURES_EE), declared ^ set(LEDGER)
    for name, (_, args) in _lib.SIGNATURES_EE.items():
        assert _arity(name) == len(args), name
        assert hasattr(_lib.load(), name) and hasattr(_lib.load("f16"), name)          # exported by both libraries
    assert _lib.load().pv_version() == 10                                              # ABI unchanged
    ops_src = open(os.path.join(REPO, "peekvit_amd", "ops.py")).read()
    wrappers = {}
    for node in ast.parse(ops_src).body:
        if isinstance(node, ast.FunctionDef):
            for sym in re.findall(r"\b(pv_\w+)\(", ast.get_source_segment(ops_src, node)):
                wrappers.setdefault(sym, set()).add(node.name)
    for entry, ids in LEDGER.items():
        for tid in ids:
            fname, _, name = tid.partition("::")
            src = open(os.path.join(REPO, "tests", fname)).read()
            fn = next((n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == name), None)
            assert fn is not None, f"{entry}: {tid} does not exist"
            body = ast.get_source_segment(src, fn)
            assert re.search(rf"\b{entry}\b", body) or any(re.search(rf"\bops\.{w}\(", body) for w in wrappers.get(entry, ())), tid


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from peekvit_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(256)                 # never dereferenced: every call below is refused before anything is launched
    q = C.c_void_p(1 << 30)             # a second "buffer", far from the first
    null = C.c_void_p(0)

    def head(x=p, stride=197 * 768, g=p, b=p, w=p, bias=p, out=q, B=64, D=768, Cn=1000):
        return lib.pv_exit_head_f32(x, stride, g, b, 1e-5, w, bias, out, B, D, Cn, null)
    assert head(x=null) == -1 and head(g=null) == -1 and head(b=null) == -1 and head(w=null) == -1 and head(out=null) == -1
    assert head(B=0) == -1 and head(D=0) == -1 and head(Cn=0) == -1
    assert head(D=770, stride=772) == -2 and head(D=8192, stride=8192) == -2            # D % 4, D > 4096
    assert head(stride=764) == -1 and head(stride=197 * 768 + 2) == -1                  # stride below D / not a multiple of 4
    assert head(x=C.c_void_p(260)) == -1 and head(w=C.c_void_p(264)) == -1 and head(g=C.c_void_p(260)) == -1      # misaligned
    assert head(out=C.c_void_p(258)) == -1 and head(bias=C.c_void_p(258)) == -1

    def step(logits=p, ldl=1000, live=p, n=64, Cn=1000, thr=0.5, conf=p, out=q, ldo=1000, layer=p, oconf=p, total=2048, nxt=p, src=p, cnt=p):
        return lib.pv_exit_step(logits, ldl, live, n, Cn, thr, 3, conf, out, ldo, layer, oconf, total, nxt, src, cnt, null)
    for k in ("logits", "live", "conf", "out", "layer", "oconf", "nxt", "src", "cnt"):
        assert step(**{k: null}) == -1, k
    assert step(n=0) == -1 and step(n=-5) == -1 and step(Cn=0) == -1 and step(total=0) == -1
    assert step(ldl=999) == -1 and step(ldo=999) == -1 and step(thr=float("nan")) == -1
    assert step(logits=C.c_void_p(258)) == -1 and step(layer=C.c_void_p(260)) == -1 and step(cnt=C.c_void_p(257)) == -1
    assert step(out=p) == -1 and step(out=C.c_void_p(256 + 4000)) == -1                 # out_logits over the rows being read
    assert step(n=1 << 31) == -2 and step(total=1 << 31) == -2

    def gather(x=p, n_in=64, src=p, n_out=10, elems=197 * 768, out=q):
        return lib.pv_gather_images_f32(x, n_in, src, n_out, elems, out, null)
    assert gather(x=null) == -1 and gather(src=null) == -1 and gather(out=null) == -1
    assert gather(n_in=0) == -1 and gather(n_out=0) == -1 and gather(elems=0) == -1
    assert gather(elems=197 * 768 + 2) == -2                                            # not a multiple of 4 floats
    assert gather(x=C.c_void_p(260)) == -1 and gather(out=C.c_void_p((1 << 30) + 8)) == -1 and gather(src=C.c_void_p(258)) == -1
    assert gather(out=p) == -1 and gather(out=C.c_void_p(256 + 197 * 768 * 4)) == -1    # out aliases x
