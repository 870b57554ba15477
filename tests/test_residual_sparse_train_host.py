"""ResidualViT packed training without a GPU: plain autograd of the packed restatement
(tests/residual_sparse_train_ref.py) against the dense composite model (peekvit_amd.models on the CPU in double, train mode) - loss, logits
and the gradient of EVERY parameter, in fp64.  fp64 rounding lands near 1e-14; a semantic slip (a forgotten multiplicity, a merged row that
keeps gradient, a mask-loss gradient not summed over a row's members) shows at 1e-4 or more: the limit is 1e-9."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from peekvit_amd import losses, synth
import residual_sparse_ref as R
import residual_sparse_train_ref as T

EXTRA = dict(gate_type="sigmoid", gate_temp=1, add_budget_token="learnable", gate_threshold=0.5)
LIMIT = 1e-9
LOSS_BUDGET = 0.02          # budget_mse's budget: below every image's kept share, so the relu inside it is open and every mask carries gradient

# name -> (model dims, batch, per-image budgets, gate gain, gate_bias, seed); seeds, budgets and gate_bias were picked on the CPU so that the
# preconditions asserted in test_packed_training_step_equals_the_dense_composite_in_fp64 hold
MICRO = dict(image_size=32, patch_size=4, num_layers=3, num_heads=2, hidden_dim=128, mlp_dim=256, num_classes=10)
ROWS198 = dict(image_size=56, patch_size=4, num_layers=2, num_heads=2, hidden_dim=128, mlp_dim=256, num_classes=10)
CASES = {
    "micro": (MICRO, 5, [0.05, 0.3, 0.5, 0.7, 0.95], 4.0, 0.0, 0),
    "rows198": (ROWS198, 2, [0.3, 0.8], 4.0, 0.0, 0),
}


def build(name, gate_bias=None, gain=None):
    """(cfg, model in double and train mode with fixed budgets, x, y, budgets) of one case."""
    from peekvit_amd.models.residualvit import ResidualVisionTransformer
    dims, batch, budgets, g, gb, seed = CASES[name]
    g, gb = g if gain is None else gain, gb if gate_bias is None else gate_bias
    cfg = dict(dims, **EXTRA, gate_bias=gb)
    sd = R.sparse_sd(cfg, g, torch.float64, seed=seed)
    model = ResidualVisionTransformer(**cfg).double()
    model.load_state_dict(sd)
    model.train()
    bud = torch.tensor(budgets, dtype=torch.float64)
    model._sample_budget = lambda n: bud.clone()                 # both sides see the same budgets
    x = torch.from_numpy(synth.synth_images(batch, cfg["image_size"], seed=seed)).double()
    y = torch.arange(batch) % cfg["num_classes"]
    return cfg, model, x, y, budgets


def dense_step(model, x, y):
    """One step of the dense composite: (loss, logits, masks [L][B, N, 1], {name: grad})."""
    model.zero_grad(set_to_none=True)
    logits = model(x)
    loss = F.cross_entropy(logits, y) + losses.budget_mse(model, LOSS_BUDGET)
    loss.backward()
    masks = [blk.mask.detach() for blk in model.encoder.layers]
    return loss.detach(), logits.detach(), masks, {k: p.grad for k, p in model.named_parameters()}


def packed_step(model, cfg, x, y, budgets):
    params = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    logits, masks, thrs, rows = T.packed_train_forward(x, params, cfg, budgets)
    mloss = T.budget_mse_ref(masks, LOSS_BUDGET)
    loss = F.cross_entropy(logits, y) + mloss
    loss.backward()
    return loss.detach(), logits.detach(), [m.detach() for m in masks], {k: p.grad for k, p in params.items()}, rows, float(mloss.detach())


def mask_facts(masks):
    """What the dense masks say about the case: the masked share per block, whether some class of tokens masked together (more than one
    token) is live again in a later block, whether some image masks nothing in some block."""
    B, N = masks[0].shape[:2]
    label = np.arange(B * N).reshape(B, N)
    nxt = B * N
    shares, relive, nothing = [], False, False
    for m in masks:
        z = (m[..., 0] == 0).numpy()
        shares.append(float(z.mean()))
        for b in range(B):
            live = ~z[b]
            if live.all():
                nothing = True
            counts = {l: int((label[b] == l).sum()) for l in set(label[b][live].tolist())}
            if any(c > 1 for c in counts.values()):
                relive = True
            if z[b].any():
                label[b][z[b]] = nxt
                nxt += 1
    return shares, relive, nothing


def compare(dense, packed):
    """Worst relative L2 over the loss, the logits and every parameter gradient (a gradient that is None on one side counts as zeros)."""
    ld, gd, _, grads_d = dense
    lp, gp, _, grads_p = packed[:4]
    errs = {"loss": abs(float(lp) - float(ld)) / abs(float(ld)), "logits": R.rel_l2(gp.numpy(), gd.numpy())}
    assert set(grads_d) == set(grads_p)
    for k, g in grads_d.items():
        a = grads_p[k]
        if g is None and a is None:
            continue
        g = torch.zeros_like(a) if g is None else g
        a = torch.zeros_like(g) if a is None else a
        if float(g.norm()) == 0.0:
            assert float(a.norm()) == 0.0, k
            continue
        errs[k] = R.rel_l2(a.numpy(), g.numpy())
    return errs


@pytest.mark.parametrize("name", list(CASES))
def test_packed_training_step_equals_the_dense_composite_in_fp64(name):
    torch.set_num_threads(min(8, torch.get_num_threads()))
    cfg, model, x, y, budgets = build(name)
    dense = dense_step(model, x, y)
    shares, relive, nothing = mask_facts(dense[2])
    print(f"\n{name}: masked share per block {['%.2f' % s for s in shares]}, a merged class live again: {relive}, an image that masks nothing: {nothing}")
    # the case's own preconditions (dense side), so that the comparison cannot pass vacuously
    assert any(0.2 <= s <= 0.8 for s in shares)
    if name == "micro":
        assert relive, "no class row with multiplicity > 1 comes live again in a later block"
        assert nothing, "no image masks nothing in some block"
    packed = packed_step(model, cfg, x, y, budgets)
    assert packed[5] > 0, "the mask loss is zero: its gradient would not be exercised"
    S = synth.seq_length(cfg) + 1
    assert sum(packed[4]) < len(packed[4]) * x.shape[0] * S
    for md, mp in zip(dense[2], packed[2]):
        assert torch.equal(md == 0, mp == 0) and float((md - mp).abs().max()) < 1e-12
    errs = compare(dense, packed)
    worst = max(errs, key=errs.get)
    print(f"{name}: loss {errs['loss']:.3g}, logits {errs['logits']:.3g}, worst gradient {worst} {errs[worst]:.3g} over {len(errs) - 2} tensors, "
          f"rows share {sum(packed[4]) / (len(packed[4]) * x.shape[0] * S):.3f}")
    assert errs[worst] < LIMIT, (worst, errs[worst])
    # every parameter that the dense step gives a gradient got compared, the gate and budget-gate ones among them
    for k in ("encoder.layers.0.residual_gate.projection.weight", "encoder.layers.1.budget_token_gate.weight", "learnable_budget_token_1",
              "conv_proj.weight", "encoder.pos_embedding"):
        assert k in errs, k


def test_gates_that_mask_nothing_give_the_dense_gradients():
    torch.set_num_threads(min(8, torch.get_num_threads()))
    cfg, model, x, y, budgets = build("micro", gate_bias=10.0, gain=1.0)          # the stock gates: sigmoid(. + 10) is above every threshold
    dense = dense_step(model, x, y)
    assert all(bool((m > 0).all()) for m in dense[2])
    packed = packed_step(model, cfg, x, y, budgets)
    S = synth.seq_length(cfg) + 1
    assert sum(packed[4]) == len(packed[4]) * x.shape[0] * S                      # every row runs
    errs = compare(dense, packed)
    worst = max(errs, key=errs.get)
    print(f"\nnothing masked: loss {errs['loss']:.3g}, logits {errs['logits']:.3g}, worst gradient {worst} {errs[worst]:.3g}")
    assert errs[worst] < LIMIT, (worst, errs[worst])


def test_differentiable_pack_step_is_the_inference_restatement():
    """pack_step_train_ref against pack_step_ref (the checker of the inference kernels): same tables, same values."""
    g = torch.Generator().manual_seed(3)
    D, lens = 16, [6, 2, 9, 4]
    seg = np.concatenate([[0], np.cumsum(lens)])
    x = torch.randn(seg[-1], D, generator=g, dtype=torch.float64)
    mult = np.ones(seg[-1], dtype=np.int64)
    mult[2], mult[10] = 5, 3
    N = 12
    tok_row = np.stack([np.sort(np.random.RandomState(b).randint(1, max(l - 1, 2), size=N)) if l > 2 else np.zeros(N, dtype=np.int64)
                        for b, l in enumerate(lens)])
    wg, wb = torch.randn(D, generator=g, dtype=torch.float64), torch.randn(D, generator=g, dtype=torch.float64) * 0.1
    a = R.pack_step_ref(x, seg, mult, tok_row, wg, 0.1, wb, -0.2, 1.0, 0.0)
    b = T.pack_step_train_ref(x, seg, mult, tok_row, wg, 0.1, wb, -0.2, 1.0, 0.0)
    for k in ("x_next", "row_scale_next", "log_mult_next", "mask_out", "thr_out", "margin"):
        assert torch.equal(a[k], b[k]), k
    for k in ("mult_next", "seg_next", "tok_row_next"):
        assert np.array_equal(a[k], b[k]), k
    assert a["totals"] == b["totals"] and bool((b["src"] < 0).any())


# ---- include/peekvit_hip_sparse_train.h: every declared entry point is exported, bound, wrapped and has a test that calls it directly ----
LEDGER = {
    "pv_attention_varlen_w_lse_bf16": ["test_hip_residual_sparse_train.py::test_ragged_weighted_attention_forward_and_backward_against_fp64"],
    "pv_attention_varlen_w_bwd16_bf16": ["test_hip_residual_sparse_train.py::test_ragged_weighted_attention_forward_and_backward_against_fp64"],
    "pv_residual_pack_step_train": ["test_hip_residual_sparse_train.py::test_pack_step_train_and_its_backward_against_fp64_autograd"],
    "pv_residual_pack_step_bwd": ["test_hip_residual_sparse_train.py::test_pack_step_train_and_its_backward_against_fp64_autograd"],
}
WRAPPERS = {"pv_attention_varlen_w_lse_bf16": "attention_varlen_w_lse", "pv_attention_varlen_w_bwd16_bf16": "attention_varlen_w_bwd16",
            "pv_residual_pack_step_train": "residual_pack_step_train", "pv_residual_pack_step_bwd": "residual_pack_step_bwd"}


def test_ledger_names_a_direct_test_for_every_declared_entry_point():
    import os
    import re
    from conftest import REPO
    from peekvit_amd import _build, _lib
    header = open(os.path.join(REPO, "include", "peekvit_hip_sparse_train.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pv_\w+)\s*\(", src, flags=re.M))
    assert "peekvit_hip_sparse_train.h" in _build.HEADERS and "-fno-slp-vectorize" in _build.FILE_FLAGS["pv_sparse_train.hip"]
    assert set(LEDGER) == declared == set(_lib.SIGNATURES_SPARSE_TRAIN) == set(WRAPPERS), declared ^ set(LEDGER)
    ops_src = open(os.path.join(REPO, "peekvit_amd", "ops.py")).read()
    for name, (_, args) in _lib.SIGNATURES_SPARSE_TRAIN.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == len(args), name
        assert hasattr(_lib.load(), name) and hasattr(_lib.load("f16"), name)                      # exported by both libraries
        assert re.search(rf"def {WRAPPERS[name]}\(", ops_src) and f"{name}(" in ops_src
        for tid in LEDGER[name]:
            fname, _, test = tid.partition("::")
            body = open(os.path.join(REPO, "tests", fname)).read()
            assert f"def {test}(" in body and f"ops.{WRAPPERS[name]}(" in body, tid
    assert _lib.load().pv_version() == 10 and _lib.load("f16").pv_version() == 10                  # ABI unchanged
    # no atomics in the new source: every sum has one owner
    text = open(os.path.join(_build.CSRC, "pv_sparse_train.hip")).read()
    assert "atomic" not in text


def check_attention_argument_validation():
    """Every refusal below happens before a launch: the pointers are never dereferenced."""
    import ctypes as C
    from peekvit_amd import _lib
    p, q, null, odd16, odd4 = C.c_void_p(256), C.c_void_p(1 << 30), C.c_void_p(0), C.c_void_p(264), C.c_void_p(258)
    for op in ("bf16", "f16"):
        lib = _lib.load(op)

        def fwd(qkv=p, out=q, lse=p, seg=p, lm=p, B=4, max_len=198, H=12, dh=64, flag=null):
            return lib.pv_attention_varlen_w_lse_bf16(qkv, out, lse, seg, lm, B, max_len, H, dh, flag, null)
        for k in ("qkv", "out", "lse", "seg", "lm"):
            assert fwd(**{k: null}) == -1, k
        assert fwd(B=0) == -1 and fwd(H=0) == -1 and fwd(max_len=0) == -1
        assert fwd(qkv=odd16) == -1 and fwd(out=odd16) == -1 and fwd(lse=odd4) == -1 and fwd(lm=odd4) == -1 and fwd(seg=odd4) == -1 and fwd(flag=odd4) == -1
        assert fwd(dh=32) == -2 and fwd(dh=128) == -2 and fwd(max_len=209) == -2 and fwd(B=1 << 31, H=2) == -2

        def bwd(qkv=p, dout=p, out=p, lse=p, seg=p, lm=p, g=q, part=p, delta=p, B=4, max_len=198, H=12, dh=64):
            return lib.pv_attention_varlen_w_bwd16_bf16(qkv, dout, out, lse, seg, lm, g, part, delta, B, max_len, H, dh, 0.125, null)
        for k in ("qkv", "dout", "out", "lse", "seg", "lm", "g", "delta"):
            assert bwd(**{k: null}) == -1, k
        assert bwd(B=0) == -1 and bwd(H=0) == -1 and bwd(max_len=0) == -1
        for k in ("qkv", "dout", "out", "g"):
            assert bwd(**{k: odd16}) == -1, k
        for k in ("lse", "seg", "lm", "part", "delta"):
            assert bwd(**{k: odd4}) == -1, k
        assert bwd(dh=32) == -2 and bwd(max_len=209) == -2 and bwd(B=1 << 30, H=2) == -2


def check_pack_step_argument_validation():
    import ctypes as C
    from peekvit_amd import _lib
    p, q, r, null = C.c_void_p(256), C.c_void_p(1 << 30), C.c_void_p(1 << 31), C.c_void_p(0)
    for op in ("bf16", "f16"):
        lib = _lib.load(op)

        def pack(x=p, seg=p, mult=p, tok=p, B=4, N=196, D=768, wg=p, bg=p, wb=p, bb=p, temp=1.0, mrow=p, xn=q, rs=p, mn=p, lm=p, sn=p, tn=p,
                 mo=p, th=p, tot=p, g=null, b=null, ln=null, ga=p, src=p):
            return lib.pv_residual_pack_step_train(x, seg, mult, tok, B, N, D, wg, bg, wb, bb, temp, 0.0, mrow, xn, rs, mn, lm, sn, tn, mo, th, tot,
                                                   g, b, 1e-6, ln, ga, src, null)
        for k in ("x", "seg", "mult", "tok", "wg", "bg", "wb", "bb", "mrow", "xn", "rs", "mn", "lm", "sn", "tn", "mo", "th", "tot", "ga", "src"):
            assert pack(**{k: null}) == -1, k
        assert pack(B=0) == -1 and pack(D=0) == -1 and pack(N=-1) == -1 and pack(temp=0.0) == -1 and pack(xn=p) == -1
        assert pack(D=770) == -2 and pack(D=8192) == -2 and pack(N=207) == -2 and pack(x=C.c_void_p(260)) == -2

        def bwd(x=p, seg=p, tok=p, mrow=p, ga=p, thr=p, sn=p, src=p, g=q, drs=p, dm=p, B=4, N=196, D=768, wg=p, wb=p, temp=1.0, dx=r, dmr=p, dwg=p,
                dwb=p, scal=p):
            return lib.pv_residual_pack_step_bwd(x, seg, tok, mrow, ga, thr, sn, src, g, drs, dm, B, N, D, wg, wb, temp, dx, dmr, dwg, dwb, scal, null)
        for k in ("x", "seg", "tok", "mrow", "ga", "thr", "sn", "src", "g", "drs", "wg", "wb", "dx", "dmr", "dwg", "dwb", "scal"):
            assert bwd(**{k: null}) == -1, k                                     # a null pointer (dm alone may be null)
        assert bwd(B=0) == -1 and bwd(D=0) == -1 and bwd(N=-1) == -1 and bwd(temp=0.0) == -1
        for k in ("x", "g", "dx", "wg", "wb", "dwg", "dwb", "scal"):
            assert bwd(**{k: C.c_void_p(264)}) == -1, k                          # a misaligned pointer
        assert bwd(dx=p) == -1 and bwd(dx=q) == -1                               # in place
        assert bwd(N=207) == -2 and bwd(D=770) == -2 and bwd(D=8192) == -2       # a segment over 208 rows; widths the row kernels do not take


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    check_attention_argument_validation()
    check_pack_step_argument_validation()


# ---- the public switch ----
def test_switch_exists_is_off_by_default_and_a_cpu_step_takes_the_dense_path():
    import inspect
    from peekvit_amd import engine
    from peekvit_amd.models.residualvit import ResidualVisionTransformer as cls
    cfg, m, x, y, _ = build("micro")
    assert m.compact_training is False and m.set_compact_training() is m and m.compact_training is True
    with pytest.raises(AttributeError):
        m.compact_training = False                                  # read-only
    params = [k for k in inspect.signature(cls.__init__).parameters if k != "self"]
    assert not any("compact" in k for k in params) and not any("compact" in k for k in m.state_dict())
    assert m.token_compaction is False                              # the inference switch is another one
    n0, d0, r0 = engine.sparse_train_dense_forwards, engine.sparse_dense_forwards, engine.sparse_rows
    on = dense_step(m, x, y)                                        # a CPU tensor: today's path, counted
    assert engine.sparse_train_dense_forwards == n0 + 1 and engine.sparse_dense_forwards == d0 and engine.sparse_rows == r0
    off = dense_step(m.set_compact_training(False), x, y)
    assert engine.sparse_train_dense_forwards == n0 + 1
    assert torch.equal(on[1], off[1]) and all(torch.equal(on[3][k], off[3][k]) for k in on[3] if on[3][k] is not None)
    m.eval().set_compact_training(True)
    m.set_budget(0.5)
    with torch.no_grad():
        m(x)                                                        # eval: not the new switch's business
    assert engine.sparse_train_dense_forwards == n0 + 1


def test_the_reference_stays_under_the_knee_cap_of_the_gpu_step_test():
    """tests/test_hip_residual_sparse_train.py excludes tokens within 1e-3 of the relu's knee from its mask comparison and caps them at 5 %: the fp64
    composite itself stays under that cap for the chosen seeds."""
    for name in CASES:
        cfg, m, x, y, _ = build(name)
        share, hooks, out = 0.0, [], []
        def pre(blk, inp):
            t = inp[0]
            thr = torch.sigmoid(blk.budget_token_gate(t[:, -1:]))
            sig = torch.sigmoid(blk.residual_gate.projection(t[:, 1:-1]) / blk.residual_gate.temp + blk.residual_gate.sigmoid_bias)
            out.append((sig - thr).abs().reshape(-1).detach())
        for blk in m.encoder.layers:
            hooks.append(blk.register_forward_pre_hook(pre))
        with torch.no_grad():
            m(x)
        for h in hooks:
            h.remove()
        share = float((torch.cat(out) < 1e-3).double().mean())
        print(f"\n{name}: tokens within 1e-3 of the knee {share:.4f}")
        assert share <= 0.05


def test_harness_key_parses_and_switches_the_model_on():
    from peekvit_amd.harness import config, train as htrain
    assert config.load_config("train_config", ["model=residualvit_b_16"])["training"]["compact_tokens"] is False
    assert config.load_config("train_config", ["model=residualvit_b_16", "training.compact_tokens=true"])["training"]["compact_tokens"] is True
    with pytest.raises(ValueError, match="set_compact_training"):
        htrain.main(["model=vit_tiny", "training.compact_tokens=true", "device=cpu", "dataset.image_size=32", "dataset.num_classes=10", "dataset.train_size=8",
                     "dataset.val_size=8", "model.image_size=32", "model.num_classes=10", "training.train_batch_size=8", "training.eval_batch_size=8"])
