"""A-ViT training on the MI355X: the halting step's two kernels (pv_avit_act_fwd / pv_avit_act_bwd, through
train_engine.ActStepFn) against an fp64 restatement and its autograd, train_engine.avit_block_forward_train against the fp64 block, and the whole fused training
pass (`set_fused_training`) against an fp64 composite that replays the fused pass's halting decisions."""
import copy
import json
import os

import pytest
import torch

import avit_train_ref as ref
from conftest import GOLDEN, rel_l2
from peekvit_amd import synth

pytestmark = pytest.mark.gpu

META = json.load(open(os.path.join(GOLDEN, "avit_meta.json")))
THR = float(torch.tensor(1 - 0.01, dtype=torch.float32))
U = 2.0 ** -24          # half an fp32 ulp of 1: the rounding of one fp32 operation, relative
GS, GC = 10.0, 30.0


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


# ---- the halting step ----------------------------------------------------------------------------------------------------------------------------
STEP_SHAPES = [(3, 17, 128, 1), (2, 20, 128, 2), (1, 17, 128, 1), (3, 197, 192, 1), (2, 208, 384, 1)]


def _step_inputs(B, S, D, n_cls, last, seed):
    """fp32 inputs of one step (CPU).  Channel 0 of y puts the gate's argument in [-4, 4]; c is built from the fp64 h so that every c' lies in
    [0.2, 0.98] or [1.0, 1.8] - at least 1e-3 from the threshold 0.99, so fp32 and fp64 decide alike; masks mix running and halted tokens and the
    last image (when there is more than one) has every token halted."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(B, S, D, generator=g)
    z = torch.rand(B, S, generator=g) * 8 - 4
    y[:, :, 0] = (z + GC) / GS
    h = torch.sigmoid(y[:, :, 0].double() * GS - GC)
    hh = torch.ones_like(h) if last else h
    below = torch.rand(B, S, generator=g) < 0.6
    target = torch.where(below, 0.2 + 0.78 * torch.rand(B, S, generator=g), 1.0 + 0.8 * torch.rand(B, S, generator=g)).double()
    c = (target - hh).float()
    c1 = c.double() + hh
    assert ((c1 - THR).abs() > 1e-3).all()
    m = (torch.rand(B, S, generator=g) < 0.7).float()
    if B > 1:
        m[-1] = 0.0
    R = torch.rand(B, S, generator=g)
    rho = torch.rand(B, S, generator=g) * 3
    counter = torch.randint(1, 6, (B, S), generator=g).float()
    acc = torch.randn(B, n_cls, D, generator=g)
    return y, c, R, rho, counter, m, acc


def _h_err(y0, h):
    """Absolute error bound of the kernel's h = 1 / (1 + expf(-(y0 * gate_scale - gate_center))): the product y0 * gate_scale is rounded once before
    the centre is subtracted - an absolute error U |y0 gate_scale| of the argument, times sigmoid' = h (1 - h) - then expf (2 ulp allowed), an add and
    a divide (half an ulp each): 6 U h."""
    return U * (y0 * GS).abs() * h * (1 - h) + 6 * U * h


@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("B,S,D,n_cls", STEP_SHAPES)
def test_act_step_forward_against_fp64(B, S, D, n_cls, last):
    """pv_avit_act_fwd (train_engine.ActStepFn.forward): counter', m' and the zeroed rows exact, every other output within a bound made of the
    kernel's own operations."""
    from peekvit_amd import train_engine
    dev = _dev()
    y, c, R, rho, counter, m, acc = _step_inputs(B, S, D, n_cls, last, seed=B * 1000 + S + last)
    x64, c64, R64, rho64, cnt64, m64, acc64, score64, h64 = ref.act_step(*(t.double() for t in (y, c, R, rho, counter, m, acc)), GS, GC, THR, bool(last),
                                                                         n_cls)
    yg = y.to(dev).clone()
    out = train_engine.act_step_train(yg, *(t.to(dev) for t in (c, R, rho, counter, m, acc)), GS, GC, THR, bool(last))
    torch.cuda.synchronize()
    xn, c1, R1, rho1, cnt1, m1, acc1, score = (t.detach().cpu() for t in out)
    assert out[0].data_ptr() == yg.data_ptr()          # x_next IS y, edited in place
    assert torch.equal(cnt1.double(), cnt64) and torch.equal(m1.double(), m64)
    halted = m64 == 0
    assert torch.equal(xn[halted], torch.zeros_like(xn[halted])) and torch.equal(xn[~halted], y[~halted])
    h_err = _h_err(y[:, :, 0].double(), h64)
    hh_err = torch.zeros_like(h_err) if last else h_err                                # |hh - hh64|
    assert ((c1.double() - c64).abs() <= hh_err + 2 * U * c64.abs()).all()
    assert ((R1.double() - R64).abs() <= hh_err + 2 * U * (R.double().abs() + 1)).all()
    assert ((rho1.double() - rho64).abs() <= 4 * U * rho64.abs()).all()
    hh64 = torch.ones_like(h64) if last else h64
    w64 = m.double() * (R.double() * ((c64 > THR).double() * m.double()) + hh64 * m64)          # (m' = nr)
    w_err = hh_err + 4 * U * w64.abs()
    yc = y[:, :n_cls].double()
    acc_tol = yc.abs() * w_err[:, :n_cls, None] + 3 * U * (acc.double().abs() + (yc * w64[:, :n_cls, None]).abs())
    assert ((acc1.double() - acc64).abs() <= acc_tol + 1e-30).all()
    if B == 1:
        assert torch.isnan(score)
    else:
        # a sum of (B - 1) S terms in a fixed order: at most that many roundings of a partial sum no larger than the sum of the terms
        tol = (h_err[1:].sum() + (B - 1) * S * U * h64[1:].sum()) / ((B - 1) * S) + 2 * U * score64.abs()
        assert abs(score.double() - score64) <= tol, (float(score), float(score64), float(tol))


@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("B,S,D,n_cls", STEP_SHAPES)
def test_act_step_backward_against_fp64_autograd(B, S, D, n_cls, last):
    """pv_avit_act_bwd (train_engine.ActStepFn.backward) with random gradients on all five differentiable outputs against fp64 autograd of the
    restatement: the gradient of x_next passes through every row - halted ones included - bit for bit outside channel 0 and the class rows."""
    from peekvit_amd import train_engine
    dev = _dev()
    y, c, R, rho, counter, m, acc = _step_inputs(B, S, D, n_cls, last, seed=B * 2000 + S + last)
    g = torch.Generator().manual_seed(7 + S)
    gx, gR, grho, gacc, gs = (torch.randn(B, S, D, generator=g), torch.randn(B, S, generator=g), torch.randn(B, S, generator=g),
                              torch.randn(B, n_cls, D, generator=g), torch.randn((), generator=g) * 50)
    y64, R64, rho64, acc64 = (t.double().requires_grad_(True) for t in (y, R, rho, acc))
    o = ref.act_step(y64, c.double(), R64, rho64, counter.double(), m.double(), acc64, GS, GC, THR, bool(last), n_cls)
    outs, grads = [o[0], o[2], o[3], o[6]], [gx.double(), gR.double(), grho.double(), gacc.double()]
    if B > 1:
        outs.append(o[7]); grads.append(gs.double())
    dy64, dR64, drho64, dacc64 = torch.autograd.grad(outs, [y64, R64, rho64, acc64], grads)
    h64, nr64 = o[8].detach(), o[5].detach()

    yl, Rl, rhol, accl = (t.to(dev).requires_grad_(True) for t in (y, R, rho, acc))
    og = train_engine.act_step_train(yl.clone(), c.to(dev), Rl, rhol, counter.to(dev), m.to(dev), accl, GS, GC, THR, bool(last))
    outs_g, grads_g = [og[0], og[2], og[3], og[6]], [gx.to(dev), gR.to(dev), grho.to(dev), gacc.to(dev)]
    if B > 1:                       # at B = 1 the score is NaN and has no gradient
        outs_g.append(og[7]); grads_g.append(gs.to(dev))
    dy, dR, drho, dacc = (t.cpu() for t in torch.autograd.grad(outs_g, [yl, Rl, rhol, accl], grads_g))
    assert torch.equal(grads_g[0].cpu(), gx), "the caller's gradient tensor was edited"
    assert torch.equal(drho, grho) and torch.equal(dacc, gacc)
    # rows outside the class rows: only channel 0 differs from gx
    assert torch.equal(dy[:, n_cls:, 1:], gx[:, n_cls:, 1:])
    h_err = _h_err(y[:, :, 0].double(), h64)
    yc, ga = y[:, :n_cls].double(), gacc.double()
    dot_abs = torch.zeros(B, S, dtype=torch.float64)
    dot_abs[:, :n_cls] = (ga * yc).abs().sum(-1)
    dot_err = D * U * dot_abs                                                         # a D-term sum: D roundings of partial sums <= the sum of |terms|
    hh64 = torch.ones_like(h64) if last else h64
    reached = ((c.double() + hh64) > THR).double() * m.double()
    live_nr = 0.0 if last else nr64
    assert ((dR.double() - dR64).abs() <= reached * dot_err + 4 * U * (gR.double().abs() + grho.double().abs() + dot_abs)).all()
    coef = torch.zeros(B, 1, dtype=torch.float64)
    if B > 1:
        coef[1:] = gs.double().abs() / ((B - 1) * S)
    dh_abs = coef + live_nr * (gR.double().abs() + m.double() * dot_abs)
    gate = GS * h64 * (1 - h64)
    gate_err = GS * ((1 - 2 * h64).abs() * h_err + 3 * U * h64 * (1 - h64))           # h (1 - h) from the rounded h: the error of h, not of 1 - h, is small
    tol_d0 = gate_err * dh_abs + gate * (live_nr * m.double() * dot_err + 4 * U * dh_abs)
    w64 = m.double() * (R.double() * reached + hh64 * nr64)
    w_err = (0.0 if last else 1.0) * m.double() * nr64 * h_err + 4 * U * w64.abs()    # w is the forward kernel's, h inside
    tol = 2 * U * dy64.abs() + 1e-30
    tol[:, :n_cls] += ga.abs() * w_err[:, :n_cls, None] + 2 * U * ga.abs() * w64[:, :n_cls, None].abs()
    tol[:, :, 0] += tol_d0
    assert ((dy.double() - dy64).abs() <= tol).all(), float(((dy.double() - dy64).abs() - tol).max())


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("B,S,D,n_cls,last", [(3, 17, 128, 1, 0), (2, 20, 128, 2, 0), (2, 208, 384, 1, 1)])
def test_act_step_backward_rewrites_the_16_bit_copy_in_place(B, S, D, n_cls, last, mode):
    """ops.avit_act_bwd (pv_avit_act_bwd) called directly with dy16, the hand-off form ActStepFn.backward uses behind a block: dy is edited in place,
    equals the result without a copy bit for bit, and dy16 holds the rounded new value wherever dy changed and its old bits everywhere else."""
    from peekvit_amd import _lib, engine, ops
    dev = _dev()
    y, c, R, rho, counter, m, acc = (t.to(dev) for t in _step_inputs(B, S, D, n_cls, last, seed=B * 3000 + S + last))
    g = torch.Generator().manual_seed(11 + S)
    gx, gR, grho, gacc, gs = (t.to(dev) for t in (torch.randn(B, S, D, generator=g), torch.randn(B, S, generator=g), torch.randn(B, S, generator=g),
                                                   torch.randn(B, n_cls, D, generator=g), torch.randn(1, generator=g) * 50))
    with engine.precision(mode):
        dt = _lib.operand_dtype()
        _, _, _, sv, ycls = ops.avit_act_fwd(y.clone(), c, R, rho, counter, m, acc, GS, GC, THR, bool(last))
        plain = gx.clone()
        dR_plain = ops.avit_act_bwd(plain, None, gR, grho, gacc, gs, sv, ycls, GS, bool(last))
        dy, dy16 = gx.clone(), gx.to(dt)
        ptr = dy.data_ptr()
        dR = ops.avit_act_bwd(dy, dy16, gR, grho, gacc, gs, sv, ycls, GS, bool(last))
        torch.cuda.synchronize()
    assert dy.data_ptr() == ptr and torch.equal(dy, plain) and torch.equal(dR, dR_plain)
    changed = dy != gx
    assert changed[:, :, 0].any() and not changed[:, n_cls:, 1:].any()
    assert torch.equal(dy16, dy.to(dt)), "dy16 is not the rounded dy"          # (unchanged elements: the rounding of gx, which is what it held)
    assert torch.equal(dy16[:, n_cls:, 1:], gx.to(dt)[:, n_cls:, 1:])


# ---- the block ---------------------------------------------------------------------------------------------------------------------------------
def _micro_block(D, H, dev, seed=0):
    from peekvit_amd.models.adavit import AViTBlock
    torch.manual_seed(seed)
    blk = AViTBlock(H, D, 2 * D, 0.0, 0.0)
    with torch.no_grad():
        for n, p in blk.named_parameters():
            if p.dim() == 1 and "ln" in n and "weight" in n:
                p.copy_(1 + 0.2 * torch.randn_like(p))
            elif p.dim() == 1:
                p.copy_(0.1 * torch.randn_like(p))
            p.copy_(p.to(torch.bfloat16).float())
    return blk


@pytest.mark.parametrize("halt", ["none", "some", "all_but_class"])
@pytest.mark.parametrize("B,S,D,H", [(2, 17, 128, 2), (2, 197, 192, 3)])
def test_avit_block_against_fp64(B, S, D, H, halt):
    """train_engine.avit_block_forward_train (bf16 operands, as every block function called on its own) against the fp64 block: the output per row - halted rows,
    whose input is zero and whose output is real, included - dx and all twelve parameter gradients.  Bounds: the ones tests/test_hip_backward.py
    applies to the bf16-operand training blocks (3e-2 relative for gradients), 1.2e-2 for the forward rows."""
    from peekvit_amd import ops, train_engine
    dev = _dev()
    blk = _micro_block(D, H, dev, seed=S)
    blk64 = copy.deepcopy(blk).double()
    blk = blk.to(dev)
    g = torch.Generator().manual_seed(S + D)
    m = torch.ones(B, S)
    if halt == "some":
        m = (torch.rand(B, S, generator=g) < 0.6).float()
        m[:, 0] = 1
    elif halt == "all_but_class":
        m[:, 1:] = 0
    x = (torch.randn(B, S, D, generator=g) * m[:, :, None]).to(torch.bfloat16).float()      # a halted row's input is zero
    dout = torch.randn(B, S, D, generator=g)
    x64 = x.double().requires_grad_(True)
    out64 = ref.block(blk64, x64, m.double())
    out64.backward(dout.double())
    xg = x.to(dev).requires_grad_(True)
    n0 = ops.launch_count
    out = train_engine.avit_block_forward_train(blk, xg, m.to(dev))
    out.backward(dout.to(dev))
    torch.cuda.synchronize()
    assert ops.launch_count - n0 > 20, "the HIP block did not run"
    o, o64 = out.detach().cpu().double(), out64.detach()
    row_err = (o - o64).norm(dim=-1) / o64.norm(dim=-1)
    assert row_err.max() < 1.2e-2, (float(row_err.max()), int(row_err.argmax()))
    assert rel_l2(xg.grad, x64.grad) < 3e-2, rel_l2(xg.grad, x64.grad)
    names = [n for n, _ in blk.named_parameters()]
    assert len(names) == 12
    for (n, p), (_, p64) in zip(blk.named_parameters(), blk64.named_parameters()):
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        assert rel_l2(p.grad, p64.grad) < 3e-2, (n, rel_l2(p.grad, p64.grad))


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------
def _model(name, dev=None):
    from peekvit_amd.models.adavit import AdaptiveVisionTransformer
    case = META["cases"][name]
    model = AdaptiveVisionTransformer(**case["kwargs"]).train()
    sd = {k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(case["synth_cfg"], seed=0).items()}
    model.load_state_dict(sd, strict=True)
    return model.to(dev) if dev is not None else model


def _batch(name, seed, B=6):
    size = META["cases"][name]["kwargs"]["image_size"]
    x = torch.from_numpy(synth.synth_images(B, size, seed=seed, name="avit"))
    return x, torch.arange(B) % META["cases"][name]["kwargs"]["num_classes"]


_free64 = {}


def _free_running(name, seed):
    """counter_token of the free-running fp64 composite (computed once per case and seed, on the CPU).  The image seed must be one at which the fp32
    composite itself decides every token as fp64 does: only then does the 3 % budget of the fused pass measure the fused pass."""
    if (name, seed) not in _free64:
        x = _batch(name, seed)[0]
        m32 = _model(name)
        with torch.no_grad():
            m32(x)
            free = ref.model_forward(_model(name).double(), x)[3]
        differing = int((m32.encoder.counter_token.double() != free).sum())
        assert differing == 0, f"{name}, image seed {seed}: the fp32 composite differs from the fp64 one on {differing} tokens - pick another seed"
        _free64[(name, seed)] = free
    return _free64[(name, seed)]


def fused_case(name, mode, kind, seed=0):
    """One fused training step of loss `kind` in precision mode `mode` and its fp64 replay.  Returns the figures the tests assert on (and
    the measurement behind their bounds prints): logits / rho / score errors, the loss values, the relative L2 of the COMPLETE gradient (all
    parameters as one vector), the worst single parameter and the share of tokens whose depth differs from the free-running fp64 composite."""
    from peekvit_amd import engine, train_engine
    dev = _dev()
    x, labels = _batch(name, seed)
    model = _model(name, dev)
    model.set_fused_training(True)
    with engine.precision(mode):
        logits = model(x.to(dev))
        enc = model.encoder
        loss = ref.loss_terms(kind, logits, labels.to(dev), enc.rho_token, enc.halting_score_layer)
        loss.backward()
        skipped, operand = train_engine.last_step_skipped(model), train_engine.pass_operand(model)
    counter = enc.counter_token.detach().cpu()
    m64 = _model(name).double()
    lg64, rho64, sc64, cnt64, _ = ref.model_forward(m64, x, counter=counter)
    assert torch.equal(cnt64, counter.double())
    loss64 = ref.loss_terms(kind, lg64, labels, rho64, sc64)
    loss64.backward()
    gp = dict(model.named_parameters())
    names = [n for n, p in m64.named_parameters() if p.grad is not None]
    missing = [n for n in names if gp[n].grad is None]
    assert not missing, missing
    got = torch.cat([gp[n].grad.detach().cpu().double().reshape(-1) for n in names])
    want = torch.cat([p.grad.reshape(-1) for n, p in m64.named_parameters() if p.grad is not None])
    ref_grads = dict(m64.named_parameters())
    per = {n: rel_l2(gp[n].grad, ref_grads[n].grad) for n in names if float(ref_grads[n].grad.norm()) > 1e-3 * float(want.norm())}
    worst = max(per, key=per.get) if per else None          # (avit_allhalt under the ponder term alone: rho is the constant 2, every gradient zero)
    return {"logits": rel_l2(logits, lg64), "rho": rel_l2(enc.rho_token, rho64), "scores": rel_l2(torch.stack(enc.halting_score_layer), torch.stack(sc64)),
            "loss": float(loss.detach()), "loss64": float(loss64.detach()), "grad": float((got - want).norm() / max(float(want.norm()), 1e-30)), "worst": (worst, per.get(worst)),
            "finite": bool(torch.isfinite(got).all()), "skipped": skipped, "operand": operand,
            "flipped": float((counter.double() != _free_running(name, seed)).double().mean())}


# Bounds against the fp64 replay.  Mode "auto" (fp16 operands) takes the project's contract for the ViT's kernel chain on cross-entropy alone: logits
# within 1e-3, complete gradient within 2e-3.  bf16 operands round every operand to 2^-9 = 2e-3 and cannot meet those two figures (measured 6.4e-3 and
# 9.1e-3); they are held to what was measured instead.  Everything else - the complete gradient under the three losses that reach the parameters
# through the gate (whose gate_scale h (1 - h) <= 2.5 amplifies the block error), bf16's cross-entropy gradient and logits, rho_token, the layer scores
# and the loss value in both modes - is asserted at twice the worst value MEASURED on the MI355X over image seeds 0, 1, 2 and both models (48 runs;
# the project's seed-to-seed spread is about a factor of two).  Gradient bounds have a ceiling of 1e-2 - five times the 2e-3 contract: beyond it an
# error is a defect, not a tolerance - and nothing is asserted looser than mode "auto"'s contract allows where that contract applies.
# In those 48 runs no token's depth differed from the free-running fp64 composite.
MEASURED = {
    "auto": {"logits": 7.60e-4, "rho": 7.49e-5, "scores": 1.08e-4, "loss": 6.55e-4, "ce": 1.17e-3, "ponder": 5.82e-4, "prior": 7.47e-4, "yaml": 1.12e-3},
    "bf16": {"logits": 6.43e-3, "rho": 5.55e-4, "scores": 7.36e-4, "loss": 2.33e-3, "ce": 9.13e-3, "ponder": 5.01e-3, "prior": 5.31e-3, "yaml": 9.20e-3},
}
CEILING = 1e-2


def _bound(mode, what):
    """what: 'logits' | 'rho' | 'scores' | 'loss' (relative) | a loss kind (complete-gradient relative L2)."""
    if mode == "auto" and what in ("logits", "ce"):
        return 1e-3 if what == "logits" else 2e-3          # the contract
    twice = 2 * MEASURED[mode][what]
    if what in ("ce", "ponder", "prior", "yaml"):
        return min(twice, CEILING)
    return min(twice, 1e-3) if mode == "auto" else twice


def _grad_bound(mode, kind):
    return _bound(mode, kind)


@pytest.mark.parametrize("kind", ["ce", "ponder", "prior", "yaml"])
@pytest.mark.parametrize("mode", ["auto", "bf16"])
@pytest.mark.parametrize("name", ["avit_micro", "avit_cls2_reg2"])
def test_fused_training_step_against_fp64_replay(name, mode, kind):
    r = fused_case(name, mode, kind)
    print(name, mode, kind, r)
    assert r["finite"] and not r["skipped"] and r["operand"] == ("f16" if mode == "auto" else "bf16")
    assert r["flipped"] <= 0.03, r["flipped"]          # replay must not hide a broken halting kernel
    assert r["logits"] < _bound(mode, "logits"), r["logits"]
    assert r["rho"] < _bound(mode, "rho") and r["scores"] < _bound(mode, "scores"), (r["rho"], r["scores"])
    assert abs(r["loss"] - r["loss64"]) < _bound(mode, "loss") * abs(r["loss64"]), (r["loss"], r["loss64"])
    assert r["grad"] < _grad_bound(mode, kind), (r["grad"], r["worst"])


def test_every_token_halting_after_the_first_layer():
    """avit_allhalt: every token halts after layer 1, so layers 2.. run on zero rows only; gradients stay finite and match the fp64 replay."""
    r = fused_case("avit_allhalt", "auto", "yaml")
    print(r)
    assert r["finite"] and not r["skipped"] and r["flipped"] == 0.0
    assert r["logits"] < _bound("auto", "logits") and r["grad"] < _grad_bound("auto", "yaml"), r


def test_switch_off_is_bit_identical_to_a_model_that_never_had_it():
    dev = _dev()
    x, labels = _batch("avit_micro", 0)
    a, b = _model("avit_micro", dev), _model("avit_micro", dev)
    a.set_fused_training(True)
    torch.nn.functional.cross_entropy(a(x.to(dev)), labels.to(dev)).backward()          # the fused pass leaves its state behind ...
    a.zero_grad(set_to_none=True)
    a.set_fused_training(False)                                                         # ... and the switch goes off again
    la, lb = a(x.to(dev)), b(x.to(dev))
    torch.nn.functional.cross_entropy(la, labels.to(dev)).backward()
    torch.nn.functional.cross_entropy(lb, labels.to(dev)).backward()
    assert torch.equal(la, lb)
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p.grad, q.grad), n
    assert torch.equal(a.encoder.rho_token, b.encoder.rho_token) and torch.equal(a.encoder.counter_token, b.encoder.counter_token)


def test_fused_pass_launches_the_two_halting_kernels_once_per_layer(monkeypatch):
    """ops.KernelTimer around a fused forward + backward: pv_avit_act_fwd and pv_avit_act_bwd once per layer.  With the composite they never run."""
    from peekvit_amd import ops
    dev = _dev()
    x, labels = _batch("avit_micro", 0)
    model = _model("avit_micro", dev)
    L = len(model.encoder.layers)
    with ops.KernelTimer() as kt:
        torch.nn.functional.cross_entropy(model(x.to(dev)), labels.to(dev)).backward()
    torch.cuda.synchronize()
    assert "pv_avit_act_fwd" not in kt.summary() and "pv_avit_act_bwd" not in kt.summary()          # switch off: the composite
    model.set_fused_training(True)
    handed, real = [], ops.avit_act_bwd
    monkeypatch.setattr(ops, "avit_act_bwd", lambda dy, dy16, *a, **k: (handed.append(dy16 is not None), real(dy, dy16, *a, **k))[1])
    with ops.KernelTimer() as kt:
        loss = ref.loss_terms("yaml", model(x.to(dev)), labels.to(dev), model.encoder.rho_token, model.encoder.halting_score_layer)
        loss.backward()
    torch.cuda.synchronize()
    s = kt.summary()
    # behind every block but the last the gradient arrives with the block's 16-bit copy and is edited in place (no copy, no second cast)
    assert handed == [False] + [True] * (L - 1), handed
    assert s["pv_avit_act_fwd"]["launches"] == L and s["pv_avit_act_bwd"]["launches"] == L, {k: v["launches"] for k, v in s.items()}
    assert s["pv_layernorm_bwd"]["launches"] == 2 * L and s["pv_attention_bf16"]["launches"] == L, {k: v["launches"] for k, v in s.items()}


def test_two_optimizer_steps_under_the_fp16_loss_scale():
    from peekvit_amd import train_engine
    dev = _dev()
    x, labels = _batch("avit_micro", 0)
    model = _model("avit_micro", dev)
    model.set_fused_training(True)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    before = model.encoder.layers[0].mlp.fc1.weight.detach().clone()
    for _ in range(2):
        opt.zero_grad()
        loss = ref.loss_terms("yaml", model(x.to(dev)), labels.to(dev), model.encoder.rho_token, model.encoder.halting_score_layer)
        loss.backward()
        opt.step()
        assert train_engine.pass_operand(model) == "f16" and not train_engine.last_step_skipped(model)
        assert torch.isfinite(loss)
    assert train_engine.train_state(model).scale > 1.0
    assert not torch.equal(before, model.encoder.layers[0].mlp.fc1.weight)
