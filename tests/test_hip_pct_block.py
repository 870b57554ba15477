"""The point-cloud encoder block on the training kernels (include/peekvit_hip_pct_block.h, pct_train.PCTBlockFn, set_fused_blocks) on the GPU: the
LayerNorm backward of a summed gradient and the 16-bit streaming attention backward against fp64 and against the entry points they extend, one block
and one model step against the same block / model in fp64 on stock ops, and the fallbacks.  DESIGN.md section 22 has the measured values.

Every output has one extra NaN-filled trailing row that must still be NaN afterwards."""
import copy
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, rel_l2
from peekvit_amd import ops, pct_train, synth
from test_hip_attn_stream import SHAPES, _inputs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
META = json.load(open(os.path.join(GOLDEN, "pct_meta.json")))
MODES = ["bf16", "f16"]
NAN = float("nan")

# ---------------------------------------------------------------------------------------------------------------------------------
# 1. pv_layernorm_bwd_sum
# ---------------------------------------------------------------------------------------------------------------------------------
# one row; a partly filled group of four rows; past one 256-row block; past the 1024-partial-row grid sweep; the widest bucket
LN_SHAPES = [(1, 64), (5, 128), (257, 128), (4101, 64), (130, 1024)]
EPS = 1e-6


def _guarded(rows, cols, dtype, fill=NAN):
    """(rows + 1, cols) filled with NaN, and the view of its first `rows` rows the kernels write."""
    full = torch.full((rows + 1, cols), fill, dtype=dtype, device=DEV)
    return full, full[:rows]


def _ln_sum(x, dy16, dy32, gamma, dt, want32=True, want16=True, accumulate_into=None):
    rows, D = x.shape
    dx_p, dx = _guarded(rows, D, torch.float32)
    dx16_p, dx16 = _guarded(rows, D, dt)
    if accumulate_into is None:
        dgb_p, dgb = _guarded(3, D, torch.float32)
    else:
        dgb_p, dgb = accumulate_into
    ops.layernorm_bwd_sum(x, dy16, dy32, gamma, dx if want32 else None, dx16 if want16 else None, dgb, EPS, accumulate=accumulate_into is not None)
    torch.cuda.synchronize()
    assert torch.isnan(dx_p[rows:]).all() and torch.isnan(dx16_p[rows:].float()).all() and torch.isnan(dgb_p[3:]).all()      # nothing past the last row
    return dx, dx16, dgb, (dgb_p, dgb)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rows,D", LN_SHAPES)
def test_layernorm_backward_of_a_sum(rows, D, mode):
    from peekvit_amd import _lib, engine
    g = torch.Generator(device="cuda").manual_seed(rows)
    x = torch.randn(rows, D, generator=g, device="cuda") * 2 + 0.5
    gamma = torch.randn(D, generator=g, device="cuda") * 0.3 + 1
    beta = torch.randn(D, generator=g, device="cuda") * 0.1
    dy32 = torch.randn(rows, D, generator=g, device="cuda") * 0.05
    with engine.precision(mode):
        dt = _lib.operand_dtype()
        dy16 = (torch.randn(rows, D, generator=g, device="cuda") * 0.05).to(dt)
        n0 = ops.launch_count
        dx, dx16, dgb, _ = _ln_sum(x, dy16, dy32, gamma, dt)
        assert ops.launch_count - n0 == 1
        # fp64 on the same inputs: dy = float(dy16) + dy32, never rounded
        xr, gr, br = (t.double().requires_grad_(True) for t in (x, gamma, beta))
        F.layer_norm(xr, (D,), gr, br, EPS).backward(dy16.double() + dy32.double())
        errs = dict(dx=rel_l2(dx, xr.grad), dgamma=rel_l2(dgb[0], gr.grad), dbeta=rel_l2(dgb[1], br.grad), colsum=rel_l2(dgb[2], dx16.double().sum(0)))
        print(f"layernorm_bwd_sum ({rows}, {D}) {mode}: " + ", ".join(f"{k} {v:.3g}" for k, v in errs.items()))
        assert torch.equal(dx16, dx.to(dt))                        # the 16-bit copy is the fp32 result rounded once
        assert all(v < 5e-6 for v in errs.values()), errs          # test_hip_backward.py::test_layernorm_backward's bounds
        # only one of the two results asked for: the same bits, and the third plane is the column sums of what was stored
        dx_a, _, dgb_a, _ = _ln_sum(x, dy16, dy32, gamma, dt, want16=False)
        _, dx16_b, dgb_b, _ = _ln_sum(x, dy16, dy32, gamma, dt, want32=False)
        assert torch.equal(dx_a, dx) and torch.equal(dx16_b, dx16) and torch.equal(dgb_a[:2], dgb[:2]) and torch.equal(dgb_b, dgb)
        assert rel_l2(dgb_a[2], dx.double().sum(0)) < 5e-6
        # identity 1: a zero fp32 term is pv_layernorm_bwd without a residual gradient
        ref = (torch.empty_like(dx), torch.empty_like(dx16), torch.empty(3, D, device=DEV))
        ops.layernorm_bwd(x, dy16, gamma, None, ref[0], ref[2], EPS, dx_bf16=ref[1])
        got = _ln_sum(x, dy16, torch.zeros_like(dy32), gamma, dt)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])
        # identity 2: no 16-bit term and an fp32 term that holds 16-bit values is the same call again
        got = _ln_sum(x, None, dy16.float(), gamma, dt)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])
        if (rows, D) == (257, 128):                                 # accumulate: a second call onto the first is twice a single call, exactly
            once = _ln_sum(x, dy16, dy32, gamma, dt)
            twice = _ln_sum(x, dy16, dy32, gamma, dt, accumulate_into=once[3])
            assert torch.equal(twice[2], 2.0 * dgb) and torch.equal(twice[0], dx)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. pv_attention_stream_bwd16_bf16
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stream_backward_in_16_bits_with_bias_partials(shape, mode):
    from peekvit_amd import _lib, engine
    B, S, H, dh = shape
    D, qscale, nb = H * dh, dh ** -0.5, (S + 63) // 64
    with engine.precision(mode):
        dt = _lib.operand_dtype()
        qkv, dout = _inputs(B, S, H, dh, dt)
        out = torch.empty((B, S, D), dtype=dt, device=DEV)
        lse = torch.empty((B, H, S), device=DEV)
        ops.attention_stream(qkv, out, lse, B, S, H, dh)
        g32 = torch.empty((B, S, 3 * D), device=DEV)
        delta32 = torch.empty((B, H, S), device=DEV)
        ops.attention_stream_bwd(qkv, dout, out, lse, g32, B, S, H, dh, qscale, delta_ws=delta32)
        runs = []
        for with_bias in (True, True, False):
            g_p, g16 = _guarded(B * S, 3 * D, dt)
            p_p, part = _guarded(B * nb, 3 * D, torch.float32)
            d_p, delta = _guarded(B * H, S, torch.float32)
            n0 = ops.launch_count
            ops.attention_stream_bwd16(qkv, dout, out, lse, g16.view(B, S, 3 * D), B, S, H, dh, qscale,
                                       dbias_partial=part.view(B, nb, 3 * D) if with_bias else None, delta_ws=delta.view(B, H, S))
            assert ops.launch_count - n0 == 1
            runs.append((g_p, p_p, d_p))
        dbias = ops.colsum(runs[0][1][:B * nb], torch.empty(3 * D, device=DEV))
        torch.cuda.synchronize()
    (g_p, p_p, d_p), second, no_bias = runs
    assert torch.isnan(g_p[B * S:].float()).all() and torch.isnan(p_p[B * nb:]).all() and torch.isnan(d_p[B * H:]).all()
    g16, part, delta = g_p[:B * S], p_p[:B * nb], d_p[:B * H]
    assert torch.equal(g16.view(B, S, 3 * D), g32.to(dt))          # the fp32 entry point's value, rounded once
    assert torch.equal(delta.view(B, H, S), delta32)
    assert all(torch.equal(a[:-1], b[:-1]) for a, b in zip(runs[0], second))   # two runs: identical bits (the last row is the NaN guard)
    assert torch.equal(no_bias[0][:-1], g16) and torch.isnan(no_bias[1]).all()  # without the partial rows: the same dqkv, nothing written to them
    # every element of the partial rows was written (none is still NaN), and row (b, j) is the sum of the STORED values over rows 64 j .. of image b
    assert part.shape == (B * nb, 3 * D) and torch.isfinite(part).all()
    v = g16.view(B, S, 3 * D).double()
    pad = torch.zeros((B, nb * 64 - S, 3 * D), dtype=torch.float64, device=DEV)
    blocks = torch.cat([v, pad], dim=1).view(B, nb, 64, 3 * D)
    assert ((part.view(B, nb, 3 * D).double() - blocks.sum(2)).abs() <= 64 * 2.0 ** -24 * blocks.abs().sum(2)).all()
    # ... and pv_colsum_f32 over them ends the bias gradient: the sequential fp32 summation bound over n = B S values
    n = B * S
    err, bound = (dbias.double() - v.sum((0, 1))).abs(), n * 2.0 ** -24 * v.abs().sum((0, 1))
    print(f"bwd16 {shape} {mode}: bias column sums, worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3g}")
    assert (err <= bound).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. PCTBlockFn on one block
# ---------------------------------------------------------------------------------------------------------------------------------
BLOCKS = [("PCTBlock", 128, 4, 256), ("PCTBlock", 192, 4, 192), ("RankingPCTBlock", 128, 4, 256)]          # (192, 4): dh = 48


def _block(cname, D, H, Mh):
    from peekvit_amd.models import pct
    blk = getattr(pct, cname)(num_heads=H, hidden_dim=D, mlp_dim=Mh, dropout=0.0, attention_dropout=0.0)
    sd = synth.pct_state_dict(dict(num_points=128, num_layers=1, num_heads=H, hidden_dim=D, mlp_dim=Mh, num_classes=10), 0)
    prefix = "encoder.layers.0."
    blk.load_state_dict({k[len(prefix):]: torch.from_numpy(np.array(v)) for k, v in sd.items() if k.startswith(prefix)}, strict=True)
    return blk.to(DEV).train()


def _block_grads(blk, x, g, mode):
    """One forward of `blk` on the kernels in `mode` and the gradients of <out, g>: (out, {name: gradient}, out.grad_fn, the tensors differentiated)."""
    from peekvit_amd import engine
    names = ["x"] + [n for n, p in blk.named_parameters() if p.requires_grad]
    with engine.precision(mode):
        xg = x.clone().requires_grad_(True)
        n0, b0 = pct_train.block_passes, pct_train.block_backwards
        out = blk(xg)
        wrt = [xg] + [p for p in blk.parameters() if p.requires_grad]
        grads = torch.autograd.grad(out, wrt, g, retain_graph=True)
        torch.cuda.synchronize()
        assert (pct_train.block_passes - n0, pct_train.block_backwards - b0) == (1, 1)
    return out.detach(), dict(zip(names, grads)), out, wrt


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cname,D,H,Mh", BLOCKS)
def test_block_function_against_fp64(cname, D, H, Mh, mode, monkeypatch):
    from peekvit_amd import engine
    monkeypatch.setenv("PEEKVIT_AMD_TRAIN", "hip")
    monkeypatch.delenv("PEEKVIT_AMD_BACKEND", raising=False)
    B, S = 2, 130
    gen = torch.Generator(device="cuda").manual_seed(D + S)
    x = torch.randn(B, S, D, generator=gen, device="cuda")
    g = torch.randn(B, S, D, generator=gen, device="cuda") * 0.1
    blk = _block(cname, D, H, Mh)
    # the same block in fp64 on stock ops
    b64 = copy.deepcopy(blk).double()
    x64 = x.double().requires_grad_(True)
    out64 = b64(x64)
    ref = dict(zip(["x"] + [n for n, _ in b64.named_parameters()], torch.autograd.grad(out64, [x64] + list(b64.parameters()), g.double())))

    blk.fused_block = True
    assert pct_train.block_eligible(blk, x)
    l0 = ops.launch_count
    out, grads, node, wrt = _block_grads(blk, x, g, mode)
    assert ops.launch_count - l0 >= 20 and "PCTBlockFn" in type(node.grad_fn).__name__          # the kernels ran (no eager path)
    assert set(grads) == set(ref) and all(torch.isfinite(t).all() for t in grads.values()) and torch.isfinite(out).all()
    for n in grads:
        print(f"{cname} D {D} {mode} d{n}: rel L2 {rel_l2(grads[n], ref[n]):.3g}")
    e_out = rel_l2(out, out64.detach())
    e_grad = rel_l2(torch.cat([grads[n].flatten() for n in sorted(grads)]), torch.cat([ref[n].flatten() for n in sorted(grads)]))
    print(f"{cname} D {D} {mode}: out rel L2 {e_out:.3g}; dx and all parameter gradients rel L2 {e_grad:.3g}")
    if mode == "f16":              # README's training contract for fp16 operands; bf16 has no fixed bound (DESIGN.md section 22 has the values)
        assert e_out < 1e-3
        assert e_grad < 2e-3

    # saved for the backward: x, v in fp32; u, att, w, qkv and the GELU pair in 16 bits; lse - nothing of size S^2, no fp32 copy of u or w
    held = sum(t.numel() * t.element_size() for t in node.grad_fn.saved_tensors)
    formula = B * S * pct_train.block_saved_bytes_per_row(D, H, Mh)
    print(f"saved by PCTBlockFn: {held} bytes; B S (20 D + 4 Mh + 4 H) = {formula}")
    assert formula == B * S * (20 * D + 4 * Mh + 4 * H) and held <= formula + 256

    # the normalisation is exact: the result does not depend on the scale of the incoming gradient
    with engine.precision(mode):
        for f in (2.0 ** -20, 2.0 ** 20):
            scaled = torch.autograd.grad(node, wrt, g * f, retain_graph=True)
            assert all(torch.equal(a, b * f) for a, b in zip(scaled, grads.values())), f
        zero = torch.autograd.grad(node, wrt, torch.zeros_like(g), retain_graph=True)
        assert all(torch.equal(a, torch.zeros_like(a)) for a in zero)          # (and a zero gradient gives zeros, not 0 / 0)

    # a frozen parameter gets no gradient (its weight-gradient GEMM is skipped); the others keep their bits
    mha = blk.self_attention.self_attention
    for frozen, p in (("mlp.fc1.weight", blk.mlp.fc1.weight), ("self_attention.self_attention.in_proj_weight", mha.in_proj_weight), ("ln_1.weight", blk.ln_1.weight)):
        p.requires_grad_(False)
        _, part, _, _ = _block_grads(blk, x, g, mode)
        p.requires_grad_(True)
        assert set(part) == set(grads) - {frozen} and all(torch.equal(part[n], grads[n]) for n in part), frozen
    xg = x.clone().requires_grad_(True)
    with engine.precision(mode):
        blk(xg).backward(g)
    assert all(torch.equal(p.grad, grads[n]) for n, p in blk.named_parameters()) and torch.equal(xg.grad, grads["x"])
    p.requires_grad_(False)
    blk.zero_grad(set_to_none=True)
    with engine.precision(mode):
        blk(x.clone().requires_grad_(True)).backward(g)
    assert p.grad is None                                       # None, not zeros


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. one model step
# ---------------------------------------------------------------------------------------------------------------------------------
ZERO_GRAD = ("embedder.lin1.bias", "embedder.lin2.bias", "head.lin1.bias")          # biases in front of a batch-statistics BatchNorm: exactly zero
SEED = 3


def _model(cname, kw, dtype, ranking=False):
    """test_hip_attn_stream.py::_model, with the ranking of RankPointCloudTransformer off unless asked for."""
    from peekvit_amd.models import pct
    m = getattr(pct, cname)(**kw)
    sd = synth.pct_state_dict({k: v for k, v in kw.items() if k in ("num_points", "num_layers", "num_heads", "hidden_dim", "mlp_dim", "num_classes",
                                                                     "num_registers", "num_class_tokens")}, 0)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    with torch.no_grad():
        m.embedder.bn1.weight.mul_(torch.tensor([1., -1., 1., 1., -1., 1.]))
    m.head.dp.p = 0.0
    if ranking:
        m.enable_ranking(True)
        m.set_budget(0.5)
    return m.to(DEV, dtype).train()


def _step(m, x, target):
    n0, b0 = pct_train.block_passes, pct_train.block_backwards
    m.zero_grad(set_to_none=True)
    loss = F.cross_entropy(m(x), target)
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    return loss.detach(), grads, (pct_train.block_passes - n0, pct_train.block_backwards - b0)


def _same(a, b):
    return torch.equal(a[0], b[0]) and set(a[1]) == set(b[1]) and all(torch.equal(a[1][n], b[1][n]) for n in a[1])


@pytest.mark.parametrize("cname", ["PointCloudTransformer", "RankPointCloudTransformer"])
def test_one_training_step_with_fused_blocks(cname, monkeypatch):
    from peekvit_amd import engine
    monkeypatch.setenv("PEEKVIT_AMD_TRAIN", "hip")
    monkeypatch.delenv("PEEKVIT_AMD_BACKEND", raising=False)
    kw = dict(META["cases"]["pct_n128"]["kwargs"])
    B, N, L = 16, kw["num_points"], kw["num_layers"]
    x = torch.from_numpy(synth.synth_points(B, N, seed=SEED)).to(DEV)
    target = (torch.arange(B, device=DEV) * 7 + 1) % kw["num_classes"]
    zero_grad = ZERO_GRAD + (f"encoder.layers.{L - 1}.mlp.fc2.bias",)

    fused, never, f64 = _model(cname, kw, torch.float32), _model(cname, kw, torch.float32), _model(cname, kw, torch.float64)
    assert not any(blk.fused_block for blk in fused.encoder.layers)             # off by default
    keys0 = list(fused.state_dict())
    eval_model = copy.deepcopy(fused).eval()
    with torch.no_grad():
        logits0 = eval_model(x).clone()

    # the switch off again: bit-identical to a model that never had it
    fused.set_fused_blocks(True)
    fused.set_fused_blocks(False)
    step_a, step_b = _step(fused, x, target), _step(never, x, target)
    assert step_a[2] == (0, 0) and step_b[2] == (0, 0) and _same(step_a, step_b)

    fused.set_fused_blocks(True)
    assert all(blk.fused_block for blk in fused.encoder.layers) and list(fused.state_dict()) == keys0
    loss64, grads64, cnt64 = _step(f64, x.double(), target)
    assert cnt64 == (0, 0)                                    # (an fp64 tensor takes the composite)
    with engine.precision("f16"):
        loss, grads, cnt = _step(fused, x, target)
    assert cnt == (L, L)                                      # every block ran on the kernels, forward and backward
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
    # README's training contract for fp16 operands (borrowed bounds: DESIGN.md section 22 has the measured values)
    assert e_loss < 1e-3
    assert e_grad < 2e-3

    with engine.precision("bf16"):
        loss_bf, grads_bf, cnt_bf = _step(fused, x, target)
    assert cnt_bf == (L, L)
    assert bool(torch.isfinite(loss_bf)) and all(bool(torch.isfinite(t).all()) for t in grads_bf.values())
    e_bf = rel_l2(torch.cat([grads_bf[n].flatten() for n in names]), torch.cat([grads64[n].flatten() for n in names]))
    print(f"{cname} bf16: loss {float(loss_bf):.6f} (relative {abs(float(loss_bf) - float(loss64)) / abs(float(loss64)):.3g}); all gradients rel L2 {e_bf:.3g}")

    # every no_grad forward is what it was
    with torch.no_grad():
        assert torch.equal(eval_model(x), logits0)
        eval_model.set_fused_blocks(True)
        assert torch.equal(eval_model(x), logits0)


def test_a_sorting_block_keeps_the_path_it_has(monkeypatch):
    monkeypatch.setenv("PEEKVIT_AMD_TRAIN", "hip")
    monkeypatch.delenv("PEEKVIT_AMD_BACKEND", raising=False)
    kw = dict(META["cases"]["pct_n128"]["kwargs"])
    B, L = 16, kw["num_layers"]
    x = torch.from_numpy(synth.synth_points(B, kw["num_points"], seed=SEED)).to(DEV)
    target = (torch.arange(B, device=DEV) * 7 + 1) % kw["num_classes"]
    ranked = _model("RankPointCloudTransformer", kw, torch.float32, ranking=True)
    never = _model("RankPointCloudTransformer", kw, torch.float32, ranking=True)
    ranked.set_fused_blocks(True)
    assert not any(pct_train.block_eligible(blk, torch.zeros(B, kw["num_points"], kw["hidden_dim"], device=DEV)) for blk in ranked.encoder.layers)
    step_a, step_b = _step(ranked, x, target), _step(never, x, target)
    assert step_a[2] == (0, 0) and _same(step_a, step_b)      # fused attention off as well: the stock path, bit for bit
    ranked.set_fused_attention(True)                           # ... and with it on, the attention core is where it was before this switch existed
    a0 = pct_train.attn_passes
    assert _step(ranked, x, target)[2] == (0, 0) and pct_train.attn_passes - a0 == L


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. fallbacks
# ---------------------------------------------------------------------------------------------------------------------------------
def test_fused_block_fallbacks_take_the_composite(monkeypatch):
    from peekvit_amd import engine
    from peekvit_amd.models.pct import PointCloudTransformer
    monkeypatch.setenv("PEEKVIT_AMD_TRAIN", "hip")
    monkeypatch.delenv("PEEKVIT_AMD_BACKEND", raising=False)
    kw = dict(num_points=32, num_layers=2, num_heads=2, hidden_dim=64, mlp_dim=128, num_classes=5)
    torch.manual_seed(0)
    m = PointCloudTransformer(**kw).to(DEV).train()
    m.set_fused_blocks(True)
    x = torch.from_numpy(synth.synth_points(4, 32, 1)).to(DEV)

    def ran(model, inp):
        n0 = pct_train.block_passes
        model(inp)
        return pct_train.block_passes - n0

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
    d.set_fused_blocks(True)
    assert ran(d, x) == 0                                      # active attention dropout
    assert ran(d.eval(), x) == 2                               # ... inactive in eval mode (grads on: fine-tuning)
    torch.manual_seed(0)
    w = PointCloudTransformer(**dict(kw, hidden_dim=96)).to(DEV).train()
    w.set_fused_blocks(True)
    assert ran(w, x) == 0                                      # hidden_dim 96: not a multiple of 64
    assert ran(m, x) == 2
