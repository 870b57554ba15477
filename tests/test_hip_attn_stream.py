"""Streaming attention for training (include/peekvit_hip_attn_stream.h) on the GPU: the forward with row statistics and the two-launch backward
against fp64 on the same 16-bit values, at the smallest shapes that reach every block edge of the kernels; the autograd function
(pct_train.StreamAttention); and the opt-in switch of the point-cloud models (set_fused_attention).

The level of the backward's error is set by a stock-op restatement with the kernels' rounding points (`_restated`), not by the code under test."""
import copy
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attn_backward_ref as R
from conftest import GOLDEN, rel_l2
from peekvit_amd import ops, pct_train, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
META = json.load(open(os.path.join(GOLDEN, "pct_meta.json")))

SHAPES = [
    (2, 1, 2, 32),        # one key
    (2, 64, 2, 32),       # exactly one block
    (2, 65, 3, 48),       # a second block of one row; dh padded to 64
    (2, 130, 2, 64),      # three blocks, the last holding two rows
    (3, 200, 4, 32),      # the pct heads; a half-filled 16-row tile
    (2, 417, 2, 32),      # the shortest length the inference kernel streams
    (1, 449, 2, 64),      # seven blocks plus one row
]
MODES = ["bf16", "f16"]
CAP = {"bf16": 1e-2, "f16": 1.5e-3}          # the project's bounds for 16-bit attention gradients (test_hip_backward.py)


def _bf(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, generator=g, device="cuda") * scale).to(torch.bfloat16)


def _inputs(B, S, H, dh, dt):
    D = H * dh
    qkv = _bf(B, S, 3 * D, seed=S).float()
    qkv[..., :D] *= dh ** -0.5
    return qkv.to(dt), _bf(B, S, D, seed=S + 1, scale=0.1).to(dt)


_heads, _rows = R.heads, R.rows          # (test_hip_rank_train.py imports them from here)
_fp64 = R.fp64          # fp64 autograd on the same 16-bit values: out, lse (log2), dqkv


def _restated(qkv, dout, B, S, H, dh, qscale):
    """The backward on stock ops in fp32 with the kernels' rounding points (attn_backward_ref.restated, shared with the per-row tests): fp32 scores and
    softmax, P rounded to the operand type for dV (and for the forward's output), delta from the 16-bit output, dS = P o (dP - delta) rounded to the
    operand type for dQ and dK, fp32 results.  p_shift = 0: P rounded at its own magnitude, the level these tests have always had."""
    return R.restated(qkv, dout, B, S, H, dh, qscale, "out", store16=False, p_shift=0)


_CACHE = {}


def _run(shape, mode):
    """One forward and two backward launches of a shape in a mode, with its references (computed once, read by both tests)."""
    key = (shape, mode)
    if key in _CACHE:
        return _CACHE[key]
    from peekvit_amd import _lib, engine
    B, S, H, dh = shape
    D, qscale = H * dh, dh ** -0.5
    nan = float("nan")
    with engine.precision(mode):
        dt = _lib.operand_dtype()
        qkv, dout = _inputs(B, S, H, dh, dt)
        # one extra trailing row each (an extra head-row for lse), NaN before the launch
        out_p = torch.full((B * S + 1, D), nan, dtype=dt, device=DEV)
        lse_p = torch.full((B * H + 1, S), nan, device=DEV)
        out, lse = out_p[:B * S].view(B, S, D), lse_p[:B * H].view(B, H, S)
        n0 = ops.launch_count
        ops.attention_stream(qkv, out, lse, B, S, H, dh)
        inf_out = None
        if S > 416:
            inf_out = torch.empty((B, S, D), dtype=dt, device=DEV)
            ops.attention(qkv, inf_out, B, S, H, dh)
        grads, deltas = [], []
        for _ in range(2):
            g_p = torch.full((B * S + 1, 3 * D), nan, device=DEV)
            dl = torch.full((B * H + 1, S), nan, device=DEV)
            ops.attention_stream_bwd(qkv, dout, out, lse, g_p[:B * S].view(B, S, 3 * D), B, S, H, dh, qscale, delta_ws=dl[:B * H].view(B, H, S))
            grads.append(g_p)
            deltas.append(dl)
        two_pass = None
        if S <= 208 or (dh == 32 and S <= 416):
            two_pass = torch.empty((B, S, 3 * D), dtype=dt, device=DEV)
            ops.attention_bwd(qkv, dout, two_pass, B, S, H, dh, qscale)
        torch.cuda.synchronize()
        launches = ops.launch_count - n0
    ref_out, ref_lse, ref_g = _fp64(qkv, dout, B, S, H, dh, qscale)
    r = dict(qkv=qkv, dout=dout, out_p=out_p, lse_p=lse_p, inf_out=inf_out, grads=grads, deltas=deltas, two_pass=two_pass, ref_out=ref_out, ref_lse=ref_lse,
             ref_g=ref_g, restated=_restated(qkv, dout, B, S, H, dh, qscale), launches=launches)
    _CACHE[key] = r
    return r


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stream_forward_with_row_statistics(shape, mode):
    B, S, H, dh = shape
    r = _run(shape, mode)
    out, lse = r["out_p"][:B * S], r["lse_p"][:B * H]
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    assert torch.isnan(r["out_p"][B * S:].float()).all() and torch.isnan(r["lse_p"][B * H:]).all()          # nothing is stored past the last row
    assert r["launches"] >= 3                                  # the kernels ran (no eager path)
    if S > 416:                                                # the LSE = false instantiation is what pv_attention_bf16 streams with: same bits
        assert torch.equal(out.view(B, S, H * dh), r["inf_out"])
    e_lse = float((lse.view(B, H, S).double() - r["ref_lse"]).abs().max())
    e_out = rel_l2(out.view(B, S, H * dh).float(), r["ref_out"])
    print(f"forward {shape} {mode}: |lse - fp64| max {e_lse:.3g}, out rel L2 {e_out:.3g}")
    assert e_lse < 1e-4                                        # test_attention_backward_from_the_forward_statistics' bound on the same quantity
    assert e_out < 6e-3                                        # test_hip_ops.py::test_attention's bound against fp64


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stream_backward_against_fp64(shape, mode):
    B, S, H, dh = shape
    D = H * dh
    r = _run(shape, mode)
    g0, g1 = r["grads"]
    assert torch.equal(g0[:B * S], g1[:B * S]) and torch.equal(r["deltas"][0][:B * H], r["deltas"][1][:B * H])          # two launches: identical bits
    assert torch.isfinite(g0[:B * S]).all() and torch.isnan(g0[B * S:]).all()
    assert torch.isfinite(r["deltas"][0][:B * H]).all() and torch.isnan(r["deltas"][0][B * H:]).all()
    got = g0[:B * S].view(B, S, 3 * D)
    for i, name in enumerate("qkv"):
        sl = slice(i * D, (i + 1) * D)
        err, base = rel_l2(got[..., sl], r["ref_g"][..., sl]), rel_l2(r["restated"][..., sl], r["ref_g"][..., sl])
        line = f"backward {shape} {mode} d{name}: rel L2 {err:.3g} (restated on stock ops {base:.3g}"
        if r["two_pass"] is not None:
            res = rel_l2(r["two_pass"][..., sl].float(), r["ref_g"][..., sl])
            line += f", resident two-pass kernel {res:.3g}"
        print(line + ")")
        assert err <= 2.0 * base + 1e-5, (name, err, base)          # the restatement sets the level; 2 x covers exp2 / P-shift / summation order
        assert err < CAP[mode], (name, err)
        if r["two_pass"] is not None:
            assert err <= 2.0 * res + 1e-4, (name, err, res)
    # delta = sum_d dO O of the stored 16-bit output
    out = r["out_p"][:B * S].view(B, S, H, dh)
    delta64 = (r["dout"].view(B, S, H, dh).double() * out.double()).sum(-1).permute(0, 2, 1)
    assert rel_l2(r["deltas"][0][:B * H].view(B, H, S), delta64) < 1e-5


@pytest.mark.parametrize("mode", MODES)
def test_stream_attention_function(mode):
    from peekvit_amd import _lib, engine
    B, S, H, dh = 2, 130, 2, 32
    D = H * dh
    with engine.precision(mode):
        dt = _lib.operand_dtype()
        qkv16, g16 = _inputs(B, S, H, dh, dt)
        qkv = qkv16.float().requires_grad_(True)
        g = g16.float()
        n0, b0, l0 = pct_train.attn_passes, pct_train.attn_backwards, ops.launch_count
        out = pct_train.StreamAttention.apply(qkv, H)
        assert out.dtype == torch.float32 and out.shape == (B, S, D) and "StreamAttention" in type(out.grad_fn).__name__
        held = sum(t.numel() * t.element_size() for t in out.grad_fn.saved_tensors)
        print(f"saved by StreamAttention: {held} bytes; B S (8 D + 4 H) = {B * S * (8 * D + 4 * H)}; one [B, H, S, S] fp32 matrix: {4 * B * H * S * S}")
        assert held <= B * S * (8 * D + 4 * H) + 256
        (dq,) = torch.autograd.grad(out, qkv, g, retain_graph=True)
        (dq_small,) = torch.autograd.grad(out, qkv, g * 2.0 ** -20, retain_graph=True)
        (dq_zero,) = torch.autograd.grad(out, qkv, torch.zeros_like(g), retain_graph=True)
        torch.cuda.synchronize()
        assert (pct_train.attn_passes - n0, pct_train.attn_backwards - b0) == (1, 3) and ops.launch_count - l0 == 4
    assert dq.dtype == torch.float32 and torch.isfinite(dq).all()
    assert torch.equal(dq_small, dq * 2.0 ** -20)              # the normalisation is exact: the result does not depend on the loss scale
    assert torch.equal(dq_zero, torch.zeros_like(dq))          # (and a zero gradient gives zeros, not 0 / 0)
    ref_out, _, ref_g = _fp64(qkv16, g16, B, S, H, dh, 1.0)
    restated = _restated(qkv16, g16, B, S, H, dh, 1.0)
    assert rel_l2(out, ref_out) < 6e-3
    for i, name in enumerate("qkv"):
        sl = slice(i * D, (i + 1) * D)
        err, base = rel_l2(dq[..., sl], ref_g[..., sl]), rel_l2(restated[..., sl], ref_g[..., sl])
        print(f"StreamAttention {mode} d{name}: rel L2 {err:.3g} (restated on stock ops {base:.3g})")
        assert err <= 2.0 * base + 1e-5 and err < CAP[mode], (name, err, base)


# ---------------------------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------------------------
ZERO_GRAD = ("embedder.lin1.bias", "embedder.lin2.bias", "head.lin1.bias")          # biases in front of a batch-statistics BatchNorm: exactly zero


def _model(cname, kw, dtype):
    """test_hip_pct_train.py::_model."""
    from peekvit_amd.models import pct
    m = getattr(pct, cname)(**kw)
    sd = synth.pct_state_dict({k: v for k, v in kw.items() if k in ("num_points", "num_layers", "num_heads", "hidden_dim", "mlp_dim", "num_classes",
                                                                     "num_registers", "num_class_tokens")}, 0)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    with torch.no_grad():
        m.embedder.bn1.weight.mul_(torch.tensor([1., -1., 1., 1., -1., 1.]))
    m.head.dp.p = 0.0
    if cname == "RankPointCloudTransformer":
        m.enable_ranking(True)
        m.set_budget(0.5)
    return m.to(DEV, dtype).train()


def _step(m, x, target):
    n0, b0 = pct_train.attn_passes, pct_train.attn_backwards
    m.zero_grad(set_to_none=True)
    loss = F.cross_entropy(m(x), target)
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    return loss.detach(), grads, (pct_train.attn_passes - n0, pct_train.attn_backwards - b0)


SEED = 3


@pytest.mark.parametrize("cname", ["PointCloudTransformer", "RankPointCloudTransformer"])
def test_one_training_step_with_fused_attention(cname, monkeypatch):
    from peekvit_amd import engine
    from peekvit_amd.models import pct
    monkeypatch.setenv("PEEKVIT_AMD_TRAIN", "hip")
    monkeypatch.delenv("PEEKVIT_AMD_BACKEND", raising=False)
    kw = dict(META["cases"]["pct_n128"]["kwargs"])
    B, N, L = 16, kw["num_points"], kw["num_layers"]
    x = torch.from_numpy(synth.synth_points(B, N, seed=SEED)).to(DEV)
    target = (torch.arange(B, device=DEV) * 7 + 1) % kw["num_classes"]
    zero_grad = ZERO_GRAD + (f"encoder.layers.{L - 1}.mlp.fc2.bias",)
    kept = {}
    order0 = pct.RankingPCTBlock.sort_order

    def recording(tag):
        def sort_order(inp):
            order = order0(inp)
            keep = 1 + math.ceil((inp.shape[1] - 1) * 0.5)
            kept.setdefault(tag, []).append(torch.sort(order[:, :keep], dim=-1).values)
            return order
        return staticmethod(sort_order)

    fused, never, f64 = _model(cname, kw, torch.float32), _model(cname, kw, torch.float32), _model(cname, kw, torch.float64)
    assert not any(blk.fused_attention for blk in fused.encoder.layers)          # off by default
    keys0 = list(fused.state_dict())
    eval_model = copy.deepcopy(fused).eval()
    with torch.no_grad():
        logits0 = eval_model(x).clone()

    # the switch off again: bit-identical to a model that never had it
    fused.set_fused_attention(True)
    fused.set_fused_attention(False)
    loss_a, grads_a, cnt_a = _step(fused, x, target)
    loss_b, grads_b, cnt_b = _step(never, x, target)
    assert cnt_a == (0, 0) and cnt_b == (0, 0)
    assert torch.equal(loss_a, loss_b) and set(grads_a) == set(grads_b) and all(torch.equal(grads_a[n], grads_b[n]) for n in grads_a)

    fused.set_fused_attention(True)
    assert all(blk.fused_attention for blk in fused.encoder.layers) and list(fused.state_dict()) == keys0
    monkeypatch.setattr(pct.RankingPCTBlock, "sort_order", recording("f64"))
    loss64, grads64, cnt64 = _step(f64, x.double(), target)
    assert cnt64 == (0, 0)                                    # (an fp64 tensor takes the composite)
    monkeypatch.setattr(pct.RankingPCTBlock, "sort_order", recording("f16"))
    with engine.precision("f16"):
        loss, grads, cnt = _step(fused, x, target)
    monkeypatch.setattr(pct.RankingPCTBlock, "sort_order", staticmethod(order0))
    assert cnt == (L, L)                                      # every block's attention ran on the kernels, forward and backward
    if cname == "RankPointCloudTransformer":
        assert len(kept["f16"]) == L and all(torch.equal(a, b) for a, b in zip(kept["f16"], kept["f64"])), "the two runs mask other tokens: choose another seed"
    assert set(grads) == set(grads64) and "class_tokens" not in grads
    for n in sorted(grads):
        if n in zero_grad:
            print(f"{cname} f16 {n}: max abs {float(grads[n].abs().max()):.3g} (exactly zero in fp64)")
        else:
            print(f"{cname} f16 {n}: rel L2 {rel_l2(grads[n], grads64[n]):.3g}")
    names = [n for n in sorted(grads) if n not in zero_grad]
    e_loss = abs(float(loss) - float(loss64)) / abs(float(loss64))
    e_grad = rel_l2(torch.cat([grads[n].flatten() for n in names]), torch.cat([grads64[n].flatten() for n in names]))
    print(f"{cname} f16: loss {float(loss):.6f} against {float(loss64):.6f} (relative {e_loss:.3g}); all gradients rel L2 {e_grad:.3g}")
    # README's training contract for fp16 operands (borrowed bounds: DESIGN.md section 21 has the measured values)
    assert e_loss < 1e-3
    assert e_grad < 2e-3

    with engine.precision("bf16"):
        loss_bf, grads_bf, cnt_bf = _step(fused, x, target)
    assert cnt_bf == (L, L)
    assert bool(torch.isfinite(loss_bf)) and all(bool(torch.isfinite(g).all()) for g in grads_bf.values())
    e_bf = rel_l2(torch.cat([grads_bf[n].flatten() for n in names]), torch.cat([grads64[n].flatten() for n in names]))
    print(f"{cname} bf16: loss {float(loss_bf):.6f} (relative {abs(float(loss_bf) - float(loss64)) / abs(float(loss64)):.3g}); all gradients rel L2 {e_bf:.3g}")

    # every no_grad forward is what it was
    with torch.no_grad():
        assert torch.equal(eval_model(x), logits0)
        eval_model.set_fused_attention(True)
        assert torch.equal(eval_model(x), logits0)


def test_fused_attention_fallbacks_take_the_composite(monkeypatch):
    from peekvit_amd import engine
    from peekvit_amd.models.pct import PointCloudTransformer
    monkeypatch.setenv("PEEKVIT_AMD_TRAIN", "hip")
    monkeypatch.delenv("PEEKVIT_AMD_BACKEND", raising=False)
    kw = dict(num_points=32, num_layers=2, num_heads=2, hidden_dim=64, mlp_dim=128, num_classes=5)
    torch.manual_seed(0)
    m = PointCloudTransformer(**kw).to(DEV).train()
    m.set_fused_attention(True)
    x = torch.from_numpy(synth.synth_points(4, 32, 1)).to(DEV)

    def ran(model, inp):
        n0 = pct_train.attn_passes
        model(inp)
        return pct_train.attn_passes - n0

    assert ran(m, x) == 2                                      # eligible: both blocks
    assert ran(copy.deepcopy(m).cpu(), x.cpu()) == 0           # CPU tensors
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert ran(m, x) == 0
    with torch.no_grad():
        assert ran(m, x) == 0
    monkeypatch.setenv("PEEKVIT_AMD_TRAIN", "torch")
    assert ran(m, x) == 0
    monkeypatch.setenv("PEEKVIT_AMD_TRAIN", "hip")
    monkeypatch.setenv("PEEKVIT_AMD_BACKEND", "torch")
    assert ran(m, x) == 0
    monkeypatch.delenv("PEEKVIT_AMD_BACKEND")
    with engine.precision("bf16x3"):
        assert ran(m, x) == 0
    torch.manual_seed(0)
    d = PointCloudTransformer(attention_dropout=0.1, **kw).to(DEV).train()
    d.set_fused_attention(True)
    assert ran(d, x) == 0                                      # active attention dropout
    assert ran(d.eval(), x) == 2                               # ... inactive in eval mode (grads on: fine-tuning)
    assert ran(m, x) == 2
