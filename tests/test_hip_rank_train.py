"""A sorting point-cloud block in train mode on the HIP kernels (include/peekvit_hip_rank_train.h, pct_train.RankedPCTBlockFn, set_fused_ranking) on the
GPU: the four row movers against index ops, the masked LayerNorms and the weighted streaming attention against the entry points they extend and against
fp64, one block and one model step against the model's own RankingPCTBlock in fp64 on stock ops, and the fallbacks.  DESIGN.md section 23 has the
measured values.

Every output has one extra NaN-filled trailing row that must still be NaN afterwards."""
import copy
import math

import pytest
import torch

from conftest import rel_l2
from peekvit_amd import ops, pct_train, synth
from test_hip_attn_stream import CAP, _heads, _inputs, _rows
from test_hip_pct_block import META, SEED, ZERO_GRAD, _block, _model, _same, _step

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = ["bf16", "f16"]
NAN = float("nan")
EPS = 1e-6


def _guarded(rows, cols, dtype=torch.float32):
    """(rows + 1, cols) filled with NaN, and the view of its first `rows` rows the kernels write."""
    full = torch.full((rows + 1, cols), NAN, dtype=dtype, device=DEV)
    return full, full[:rows]


def _untouched(full):
    return bool(torch.isnan(full[-1:].float()).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. pack / expand / unpack_grad / reduce
# ---------------------------------------------------------------------------------------------------------------------------------
def _keeps(S):
    return sorted({1, max(1, S - 2), S - 1})


@pytest.mark.parametrize("D", [64, 192, 1024])
@pytest.mark.parametrize("S", [2, 13, 130])
def test_pack_expand_unpack_against_index_ops(S, D):
    B = 2
    gen = torch.Generator(device="cuda").manual_seed(S * D)
    x = torch.randn(B, S, D, generator=gen, device="cuda")
    for k in _keeps(S):
        keep = torch.stack([torch.randperm(S - 1, generator=gen, device="cuda")[:k] for _ in range(B)]).to(torch.int32)
        L, m = k + 1, S - 1 - k
        Sc = L + (1 if m else 0)
        rows = torch.cat([torch.zeros(B, 1, dtype=torch.int64, device=DEV), keep.long() + 1], dim=1)
        # pack: a gather and a zero tail row
        full, xc = _guarded(B * Sc, D)
        n0 = ops.launch_count
        ops.rank_pack(x, keep, xc.view(B, Sc, D))
        assert ops.launch_count - n0 == 1
        want = torch.gather(x, 1, rows[:, :, None].expand(-1, -1, D))
        if m:
            want = torch.cat([want, torch.zeros(B, 1, D, device=DEV)], dim=1)
        assert torch.equal(xc.view(B, Sc, D), want) and _untouched(full), (S, D, k)
        # unpack_grad: the scatter back, zeros elsewhere, the tail row dropped
        dxc = torch.randn(B, Sc, D, generator=gen, device="cuda")
        full, dx = _guarded(B * S, D)
        ops.rank_unpack_grad(dxc, keep, S, dx.view(B, S, D))
        want = torch.zeros(B, S, D, device=DEV).scatter_(1, rows[:, :, None].expand(-1, -1, D), dxc[:, :L])
        assert torch.equal(dx.view(B, S, D), want) and _untouched(full), (S, D, k)
        if m:
            # expand: the tail row into every row L .. S - 1
            full, y = _guarded(B * S, D)
            ops.rank_expand(dxc, S, y.view(B, S, D))
            want = torch.cat([dxc[:, :L], dxc[:, L:].expand(-1, m, -1)], dim=1)
            assert torch.equal(y.view(B, S, D), want) and _untouched(full), (S, D, k)


@pytest.mark.parametrize("m,D", [(1, 64), (2, 192), (65, 64), (65, 1024), (1000, 192)])
def test_reduce_copies_the_live_rows_and_sums_the_tail_in_a_fixed_order(m, D):
    B, L = 2, 3
    S = L + m
    gen = torch.Generator(device="cuda").manual_seed(m + D)
    g = torch.randn(B, S, D, generator=gen, device="cuda")
    runs = []
    for _ in range(2):
        full, gc = _guarded(B * (L + 1), D)
        n0 = ops.launch_count
        ops.rank_reduce(g, L, gc.view(B, L + 1, D))
        assert ops.launch_count - n0 == 1
        runs.append((full, gc.view(B, L + 1, D)))
    torch.cuda.synchronize()
    (full, gc), (full2, gc2) = runs
    assert _untouched(full) and torch.equal(gc, gc2)                     # two runs: identical bits
    assert torch.equal(gc[:, :L], g[:, :L])
    tail = g[:, L:].double()
    err, bound = (gc[:, L].double() - tail.sum(1)).abs(), m * 2.0 ** -24 * tail.abs().sum(1)
    print(f"rank_reduce m {m} D {D}: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3g}")
    assert (err <= bound).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the masked LayerNorms
# ---------------------------------------------------------------------------------------------------------------------------------
LN_SHAPES = [(5, 64), (257, 128), (130, 1024)]


def _mask(rows):
    msk = torch.ones(rows, device=DEV)
    msk[::3] = 0.0
    msk[rows - 1] = 0.0
    return msk


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rows,D", LN_SHAPES)
def test_masked_layernorm_forward(rows, D, mode):
    from peekvit_amd import _lib, engine
    gen = torch.Generator(device="cuda").manual_seed(rows)
    x = torch.randn(rows, D, generator=gen, device="cuda") * 2 + 0.5
    gamma = torch.randn(D, generator=gen, device="cuda") * 0.3 + 1
    beta = torch.randn(D, generator=gen, device="cuda") * 0.1
    with engine.precision(mode):
        dt = _lib.operand_dtype()
        ref16, ref32 = torch.empty(rows, D, dtype=dt, device=DEV), torch.empty(rows, D, device=DEV)
        ops.layernorm_f32_bf16(x, gamma, beta, EPS, ref16, ref32)
        for msk in (torch.ones(rows, device=DEV), _mask(rows)):
            f16, o16 = _guarded(rows, D, dt)
            f32, o32 = _guarded(rows, D)
            n0 = ops.launch_count
            ops.layernorm_f32_bf16_masked(x, gamma, beta, msk, EPS, o16, o32)
            assert ops.launch_count - n0 == 1
            torch.cuda.synchronize()
            assert _untouched(f16) and _untouched(f32)
            live = msk > 0
            assert torch.equal(o16[live], ref16[live]) and torch.equal(o32[live], ref32[live])          # a scale of 1 changes no bit
            assert (o16[~live].float() == 0).all() and (o32[~live] == 0).all()                           # a scale of 0: zeros in both planes


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rows,D", LN_SHAPES)
def test_masked_layernorm_backward_of_a_sum(rows, D, mode):
    from peekvit_amd import _lib, engine
    gen = torch.Generator(device="cuda").manual_seed(rows + 1)
    x = torch.randn(rows, D, generator=gen, device="cuda") * 2 + 0.5
    gamma = torch.randn(D, generator=gen, device="cuda") * 0.3 + 1
    dy32 = torch.randn(rows, D, generator=gen, device="cuda") * 0.05
    with engine.precision(mode):
        dt = _lib.operand_dtype()
        dy16 = (torch.randn(rows, D, generator=gen, device="cuda") * 0.05).to(dt)

        def plain(a16, a32):
            dx, dgb = torch.empty(rows, D, device=DEV), torch.empty(3, D, device=DEV)
            ops.layernorm_bwd_sum(x, a16, a32, gamma, dx, None, dgb, EPS)
            return dx, dgb

        def masked(msk):
            fx, dx = _guarded(rows, D)
            fg, dgb = _guarded(3, D)
            n0 = ops.launch_count
            ops.layernorm_bwd_sum_masked(x, dy16, dy32, gamma, msk, dx, None, dgb, EPS)
            assert ops.launch_count - n0 == 1
            torch.cuda.synchronize()
            assert _untouched(fx) and _untouched(fg)
            return dx, dgb

        dx, dgb = masked(torch.ones(rows, device=DEV))
        rx, rgb = plain(dy16, dy32)
        assert torch.equal(dx, rx) and torch.equal(dgb, rgb)                # row_scale = 1: pv_layernorm_bwd_sum's bits
        msk = _mask(rows)
        dx, dgb = masked(msk)
        rx, rgb = plain(dy16 * msk[:, None].to(dt), dy32 * msk[:, None])    # ... and with a mask: that entry point on dy whose masked rows are zero
        assert torch.equal(dx, rx) and torch.equal(dgb, rgb)
        assert (dx[msk == 0] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the weighted streaming attention
# ---------------------------------------------------------------------------------------------------------------------------------
W_SHAPES = [(2, S, 2, dh) for S in (2, 64, 65, 130) for dh in (32, 48, 64)]          # S = 64 / 65: the tail key last in a 64-key block / alone in one


def _weighted(qkv, out, lse, dout, B, S, H, dh, qscale, t, dt):
    nb, D = (S + 63) // 64, H * dh
    fo, o = _guarded(B * S, D, dt)
    fl, l = _guarded(B * H, S)
    fg, g16 = _guarded(B * S, 3 * D, dt)
    fp, part = _guarded(B * nb, 3 * D)
    fd, delta = _guarded(B * H, S)
    n0 = ops.launch_count
    ops.attention_stream_w(qkv, o.view(B, S, D), l.view(B, H, S), B, S, H, dh, t)
    ops.attention_stream_bwd16_w(qkv, dout, o.view(B, S, D), l.view(B, H, S), g16.view(B, S, 3 * D), B, S, H, dh, qscale, t,
                                 dbias_partial=part.view(B, nb, 3 * D), delta_ws=delta.view(B, H, S))
    assert ops.launch_count - n0 == 2
    torch.cuda.synchronize()
    assert all(_untouched(f) for f in (fo, fl, fg, fp, fd))
    return o.view(B, S, D), l.view(B, H, S), g16.view(B, S, 3 * D), part.view(B, nb, 3 * D), delta.view(B, H, S)


def _fp64_weighted(qkv, dout, B, S, H, dh, qscale, m, repeat):
    """fp64 attention on the same 16-bit q | k | v where key S - 1 counts m times: physically repeated (`repeat`: the definition; the shared row's
    gradient is the sum over its copies) or as + ln m on its score.  out [B, S, D], lse (log2) [B, H, S], dqkv [B, S, 3 D]."""
    D = H * dh
    t = qkv.double().reshape(B, S, 3, H, dh).permute(2, 0, 3, 1, 4).contiguous().requires_grad_(True)
    if repeat:
        idx = torch.cat([torch.arange(S, device=DEV), torch.full((m - 1,), S - 1, device=DEV)])
        k, v = t[1].index_select(2, idx), t[2].index_select(2, idx)
        s = t[0] @ k.transpose(-1, -2)
    else:
        bias = torch.zeros(S, dtype=torch.float64, device=DEV)
        bias[S - 1] = math.log(m)
        s, v = t[0] @ t[1].transpose(-1, -2) + bias, t[2]
    out = _rows(torch.softmax(s, dim=-1) @ v, B, S, H, dh)
    (out * dout.double()).sum().backward()
    g = t.grad.clone()
    g[0] *= qscale
    return out.detach(), (torch.logsumexp(s, -1) / math.log(2.0)).detach(), g.permute(1, 3, 0, 2, 4).reshape(B, S, 3 * D)


def _restated_weighted(qkv, dout, B, S, H, dh, qscale, m):
    """test_hip_attn_stream._restated with the bias and the weighted kernels' delta: the backward on stock ops in fp32 with the kernels' rounding points,
    its result rounded to 16 bits."""
    dt, D = qkv.dtype, H * dh
    q, k, v = (_heads(t, B, S, H, dh) for t in qkv.float().split(D, dim=-1))
    do = _heads(dout.float(), B, S, H, dh)
    bias = torch.zeros(S, device=DEV)
    bias[S - 1] = math.log(m)
    P = torch.softmax(q @ k.transpose(-1, -2) + bias, dim=-1)
    P16 = P.to(dt).float()
    dv = P16.transpose(-1, -2) @ do
    dP = do @ v.transpose(-1, -2)
    delta = (P * dP).sum(-1, keepdim=True)          # with a weight the kernels form delta from p and dP in fp32, not from the stored 16-bit output
    dS = (P * (dP - delta)).to(dt).float()
    dq, dk = (dS @ k) * qscale, dS.transpose(-1, -2) @ q
    return torch.cat([_rows(t, B, S, H, dh) for t in (dq, dk, dv)], dim=-1).to(dt).float()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", W_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_weighted_stream_attention_without_a_weight_is_the_unweighted_one(shape, mode):
    from peekvit_amd import _lib, engine
    B, S, H, dh = shape
    D, qscale, nb = H * dh, dh ** -0.5, (S + 63) // 64
    with engine.precision(mode):
        dt = _lib.operand_dtype()
        qkv, dout = _inputs(B, S, H, dh, dt)
        # tail_log_mult = 0: the unweighted entry points, bit for bit
        out0, lse0 = torch.empty((B, S, D), dtype=dt, device=DEV), torch.empty((B, H, S), device=DEV)
        g0, part0, delta0 = torch.empty((B, S, 3 * D), dtype=dt, device=DEV), torch.empty((B, nb, 3 * D), device=DEV), torch.empty((B, H, S), device=DEV)
        ops.attention_stream(qkv, out0, lse0, B, S, H, dh)
        ops.attention_stream_bwd16(qkv, dout, out0, lse0, g0, B, S, H, dh, qscale, dbias_partial=part0, delta_ws=delta0)
        got = _weighted(qkv, out0, lse0, dout, B, S, H, dh, qscale, 0.0, dt)
        assert all(torch.equal(a, b) for a, b in zip(got, (out0, lse0, g0, part0, delta0)))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m", [3, 500])
@pytest.mark.parametrize("shape", W_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_weighted_stream_attention(shape, m, mode):
    """out, lse and the 16-bit dqkv of the weighted entry points against fp64 dense attention on the same 16-bit q | k | v, with the bounds the
    unweighted kernels' tests assert (forward: |lse| 1e-4, out 6e-3; backward: twice the stock-op restatement with the kernels' rounding points, and
    CAP = 1e-2 bf16 / 1.5e-3 f16).  S = 2 with m = 500 is the case that needs the weighted backward's own delta (sum_k p dP in fp32): one other key
    against a key that holds p = 0.998, where a delta formed from the stored 16-bit output left dq and dk 8 - 30 % (bf16) and 1 - 3 % (f16) off."""
    from peekvit_amd import _lib, engine
    B, S, H, dh = shape
    D, qscale, nb = H * dh, dh ** -0.5, (S + 63) // 64
    with engine.precision(mode):
        dt = _lib.operand_dtype()
        qkv, dout = _inputs(B, S, H, dh, dt)
        out, lse, g16, part, _ = _weighted(qkv, None, None, dout, B, S, H, dh, qscale, math.log(m), dt)
        again = _weighted(qkv, None, None, dout, B, S, H, dh, qscale, math.log(m), dt)
        assert torch.equal(again[2], g16) and torch.equal(again[3], part) and torch.equal(again[0], out)          # two runs: identical bits
        ref_out, ref_lse, ref_g = _fp64_weighted(qkv, dout, B, S, H, dh, qscale, m, repeat=S == 65)
        e_lse, e_out = float((lse.double() - ref_lse).abs().max()), rel_l2(out.float(), ref_out)
        print(f"weighted forward {shape} {mode} m {m}: |lse - fp64| max {e_lse:.3g}, out rel L2 {e_out:.3g}")
        assert e_lse < 1e-4                        # test_hip_attn_stream.py::test_stream_forward_with_row_statistics' bounds
        assert e_out < 6e-3
        restated = _restated_weighted(qkv, dout, B, S, H, dh, qscale, m)
        errs = {}
        for i, name in enumerate("qkv"):
            sl = slice(i * D, (i + 1) * D)
            errs[name] = err, base = rel_l2(g16[..., sl].float(), ref_g[..., sl]), rel_l2(restated[..., sl], ref_g[..., sl])
            print(f"weighted backward {shape} {mode} m {m} d{name}: rel L2 {err:.3g} (restated on stock ops {base:.3g})")
        for name, (err, base) in errs.items():
            assert err <= 2.0 * base + 1e-5, (name, err, base)          # test_hip_attn_stream.py::test_stream_backward_against_fp64's bounds
            assert err < CAP[mode], (name, err)
        # the bias partial rows: the column sums of the STORED values per block of 64 rows (test_hip_pct_block.py's bound)
        v = g16.double()
        pad = torch.zeros((B, nb * 64 - S, 3 * D), dtype=torch.float64, device=DEV)
        blocks = torch.cat([v, pad], dim=1).view(B, nb, 64, 3 * D)
        assert ((part.double() - blocks.sum(2)).abs() <= 64 * 2.0 ** -24 * blocks.abs().sum(2)).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. RankedPCTBlockFn on one block
# ---------------------------------------------------------------------------------------------------------------------------------
def _ranked_input(B, S, D, gen):
    """Rows whose norms differ by >= 1e-2 relative from one rank to the next (asserted): rounding in the norm cannot flip the order."""
    x = torch.randn(B, S, D, generator=gen, device="cuda")
    x = x / x.norm(dim=-1, keepdim=True)
    expo = torch.stack([torch.randperm(S, generator=gen, device="cuda") for _ in range(B)]).float()
    x = x * (0.3 * math.sqrt(D) * 1.02 ** expo)[:, :, None]
    n = torch.sort(x[:, 1:].double().norm(dim=-1), dim=-1, descending=True).values
    assert ((n[:, :-1] - n[:, 1:]) / n[:, :-1] >= 1e-2).all()
    return x


def _ranked_grads(blk, x, g, mode):
    from peekvit_amd import engine
    names = ["x"] + [n for n, p in blk.named_parameters() if p.requires_grad]
    with engine.precision(mode):
        xg = x.clone().requires_grad_(True)
        n0, b0, p0 = pct_train.ranked_passes, pct_train.ranked_backwards, pct_train.block_passes
        out = blk(xg)
        wrt = [xg] + [p for p in blk.parameters() if p.requires_grad]
        grads = torch.autograd.grad(out, wrt, g, retain_graph=True)
        torch.cuda.synchronize()
        assert (pct_train.ranked_passes - n0, pct_train.ranked_backwards - b0, pct_train.block_passes - p0) == (1, 1, 0)
    return out.detach(), dict(zip(names, grads)), out, wrt


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("keep", [33, 65, 128, 129])
@pytest.mark.parametrize("D,H,Mh", [(128, 4, 256), (192, 4, 192)])
def test_ranked_block_function_against_fp64(D, H, Mh, keep, mode, monkeypatch):
    from peekvit_amd import engine
    monkeypatch.setenv("PEEKVIT_AMD_TRAIN", "hip")
    monkeypatch.delenv("PEEKVIT_AMD_BACKEND", raising=False)
    B, S = 2, 130
    gen = torch.Generator(device="cuda").manual_seed(D + keep)
    x = _ranked_input(B, S, D, gen)
    g = torch.randn(B, S, D, generator=gen, device="cuda") * 0.1
    blk = _block("RankingPCTBlock", D, H, Mh)
    blk.sort = True
    blk.set_budget(1.0 if keep == S - 1 else (keep - 0.5) / (S - 1))
    assert math.ceil((S - 1) * blk.current_budget) == keep
    # the model's own block in fp64 on stock ops (train mode, sort on)
    b64 = copy.deepcopy(blk).double()
    x64 = x.double().requires_grad_(True)
    out64 = b64(x64)
    ref = dict(zip(["x"] + [n for n, _ in b64.named_parameters()], torch.autograd.grad(out64, [x64] + list(b64.parameters()), g.double())))

    assert blk.fused_ranking is False and blk.last_train_keep is None and not pct_train.ranked_block_eligible(blk, x)
    blk.fused_ranking = True
    assert pct_train.ranked_block_eligible(blk, x) and not pct_train.block_eligible(blk, x)
    l0 = ops.launch_count
    out, grads, node, wrt = _ranked_grads(blk, x, g, mode)
    assert ops.launch_count - l0 >= 22 and "RankedPCTBlockFn" in type(node.grad_fn).__name__
    assert out.shape == (B, S, D) and set(grads) == set(ref) and all(torch.isfinite(t).all() for t in grads.values()) and torch.isfinite(out).all()
    # the rows it kept: row 0, then the stable descending order of ops.token_norm's own output
    order = torch.argsort(ops.token_norm(x), dim=-1, descending=True, stable=True)[:, :keep] + 1
    want = torch.cat([torch.zeros_like(order[:, :1]), order], dim=1)
    assert blk.last_train_keep.dtype == torch.int64 and torch.equal(blk.last_train_keep, want)
    assert torch.equal(want, b64.sort_order(x.double())[:, :keep + 1])               # (the fp64 block kept the same rows: the norms are well apart)
    m = S - 1 - keep
    if m > 1:
        assert torch.equal(out[:, keep + 1:], out[:, keep + 1:keep + 2].expand(-1, m, -1))          # m copies of the tail row
    for n in grads:
        print(f"ranked D {D} keep {keep} {mode} d{n}: rel L2 {rel_l2(grads[n], ref[n]):.3g}")
    e_out = rel_l2(out, out64.detach())
    e_grad = rel_l2(torch.cat([grads[n].flatten() for n in sorted(grads)]), torch.cat([ref[n].flatten() for n in sorted(grads)]))
    print(f"ranked D {D} keep {keep} {mode}: out rel L2 {e_out:.3g}; dx and all parameter gradients rel L2 {e_grad:.3g}")
    if mode == "f16":              # test_hip_pct_block.py::test_block_function_against_fp64's bounds; bf16 has no fixed bound
        assert e_out < 1e-3
        assert e_grad < 2e-3

    # saved for the backward: PCTBlockFn's bytes per COMPACT row, plus keep as int32
    Sc = keep + 1 + (1 if m else 0)
    held = sum(t.numel() * t.element_size() for t in node.grad_fn.saved_tensors)
    formula = B * Sc * pct_train.block_saved_bytes_per_row(D, H, Mh) + 4 * B * keep
    print(f"saved by RankedPCTBlockFn: {held} bytes; B Sc (20 D + 4 Mh + 4 H) + 4 B keep = {formula}; the dense block: {B * S * pct_train.block_saved_bytes_per_row(D, H, Mh)}")
    assert held <= formula + 256

    with engine.precision(mode):
        # the normalisation is exact: the result does not depend on the scale of the incoming gradient
        for f in (2.0 ** -20, 2.0 ** 20):
            scaled = torch.autograd.grad(node, wrt, g * f, retain_graph=True)
            assert all(torch.equal(a, b * f) for a, b in zip(scaled, grads.values())), f
        zero = torch.autograd.grad(node, wrt, torch.zeros_like(g), retain_graph=True)
        assert all(torch.equal(a, torch.zeros_like(a)) for a in zero)
        again = torch.autograd.grad(node, wrt, g, retain_graph=True)
        assert all(torch.equal(a, b) for a, b in zip(again, grads.values()))          # two backwards: identical bits

    if m == 0:                     # no tail row, no masks, no bias: PCTBlockFn applied to the gathered rows, bit for bit
        plain = copy.deepcopy(blk)
        plain.sort, plain.fused_ranking, plain.fused_block = False, False, True
        rows = want[:, :, None].expand(-1, -1, D)
        with engine.precision(mode):
            xs = torch.gather(x, 1, rows).requires_grad_(True)
            p0 = pct_train.block_passes
            o2 = plain(xs)
            assert pct_train.block_passes - p0 == 1
            g2 = torch.autograd.grad(o2, [xs] + list(plain.parameters()), g)
        assert torch.equal(o2.detach(), out)
        assert torch.equal(torch.zeros_like(x).scatter_(1, rows, g2[0]), grads["x"])
        assert all(torch.equal(a, grads[n]) for a, (n, _) in zip(g2[1:], plain.named_parameters()))

    # a frozen parameter gets no gradient; the others keep their bits
    mha = blk.self_attention.self_attention
    for frozen, p in (("mlp.fc1.weight", blk.mlp.fc1.weight), ("self_attention.self_attention.in_proj_bias", mha.in_proj_bias), ("ln_1.weight", blk.ln_1.weight)):
        p.requires_grad_(False)
        _, part, _, _ = _ranked_grads(blk, x, g, mode)
        p.requires_grad_(True)
        assert set(part) == set(grads) - {frozen} and all(torch.equal(part[n], grads[n]) for n in part), frozen
    p.requires_grad_(False)
    blk.zero_grad(set_to_none=True)
    with engine.precision(mode):
        blk(x.clone().requires_grad_(True)).backward(g)
    assert p.grad is None                                       # None, not zeros


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. one model step
# ---------------------------------------------------------------------------------------------------------------------------------
def _ranked_step(m, x, target):
    n0, b0 = pct_train.ranked_passes, pct_train.ranked_backwards
    loss, grads, blocks = _step(m, x, target)
    return loss, grads, blocks, (pct_train.ranked_passes - n0, pct_train.ranked_backwards - b0)


def test_one_training_step_with_fused_ranking(monkeypatch):
    from peekvit_amd import engine
    from peekvit_amd.models.pct import RankingPCTBlock
    monkeypatch.setenv("PEEKVIT_AMD_TRAIN", "hip")
    monkeypatch.delenv("PEEKVIT_AMD_BACKEND", raising=False)
    cname = "RankPointCloudTransformer"
    kw = dict(META["cases"]["pct_n128"]["kwargs"])
    B, N, L = 16, kw["num_points"], kw["num_layers"]
    x = torch.from_numpy(synth.synth_points(B, N, seed=SEED)).to(DEV)
    target = (torch.arange(B, device=DEV) * 7 + 1) % kw["num_classes"]
    zero_grad = ZERO_GRAD + (f"encoder.layers.{L - 1}.mlp.fc2.bias",)
    fused, never, f64 = (_model(cname, kw, dt, ranking=True) for dt in (torch.float32, torch.float32, torch.float64))
    assert not any(blk.fused_ranking for blk in fused.encoder.layers) and all(blk.last_train_keep is None for blk in fused.encoder.layers)
    keys0, nparam, nbuf = list(fused.state_dict()), len(list(fused.parameters())), len(list(fused.buffers()))
    eval_model = copy.deepcopy(fused).eval()
    with torch.no_grad():
        logits0, train0 = eval_model(x).clone(), fused(x).clone()

    # the fused run first, in mode f16, with every block's fp32 input captured
    fused.set_fused_ranking(True)
    assert all(blk.fused_ranking for blk in fused.encoder.layers) and not any(blk.fused_block or blk.fused_attention for blk in fused.encoder.layers)
    assert list(fused.state_dict()) == keys0 and len(list(fused.parameters())) == nparam and len(list(fused.buffers())) == nbuf
    seen = []
    hooks = [blk.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().clone(memory_format=torch.contiguous_format)))
             for blk in fused.encoder.layers]
    with engine.precision("f16"):
        loss, grads, blocks, ranked = _ranked_step(fused, x, target)
    for h in hooks:
        h.remove()
    assert ranked == (L, L) and blocks == (0, 0) and len(seen) == L
    S = seen[0].shape[1]
    keep = math.ceil((S - 1) * 0.5)
    recorded = [blk.last_train_keep.clone() for blk in fused.encoder.layers]
    for inp, rec in zip(seen, recorded):          # exactly the top-keep of ops.token_norm of the block's own input
        order = torch.argsort(ops.token_norm(inp), dim=-1, descending=True, stable=True)[:, :keep] + 1
        assert torch.equal(rec, torch.cat([torch.zeros_like(order[:, :1]), order], dim=1))

    # the fp64 model replays each layer's recorded rows (the remaining indices follow in ascending order): both mask the same tokens by construction
    calls = []

    def replay(inp):
        rec = recorded[len(calls)]
        rest = torch.ones((B, S), dtype=torch.bool, device=DEV).scatter_(1, rec, False)
        rest = torch.arange(S, device=DEV).expand(B, -1)[rest].view(B, S - rec.shape[1])
        n = inp.detach().double().norm(dim=-1)
        kept, dropped = torch.gather(n, 1, rec[:, 1:]).min(1).values, torch.gather(n, 1, rest).max(1).values
        calls.append(float(((dropped - kept) / kept).clamp_min(0).max()))
        return torch.cat([rec, rest], dim=1)

    stock_order = RankingPCTBlock.__dict__["sort_order"]
    monkeypatch.setattr(RankingPCTBlock, "sort_order", staticmethod(replay))
    loss64, grads64, blocks64, ranked64 = _ranked_step(f64, x.double(), target)
    monkeypatch.setattr(RankingPCTBlock, "sort_order", stock_order)
    assert len(calls) == L and blocks64 == (0, 0) and ranked64 == (0, 0)
    print("replayed order against the fp64 norms at the keep boundary, worst relative inversion per layer: " + ", ".join(f"{c:.3g}" for c in calls))
    assert set(grads) == set(grads64)
    for n in sorted(grads):
        if n in zero_grad:
            print(f"ranked f16 {n}: max abs {float(grads[n].abs().max()):.3g} (exactly zero in fp64)")
        else:
            print(f"ranked f16 {n}: rel L2 {rel_l2(grads[n], grads64[n]):.3g}")
    names = [n for n in sorted(grads) if n not in zero_grad]
    e_loss = abs(float(loss) - float(loss64)) / abs(float(loss64))
    e_grad = rel_l2(torch.cat([grads[n].flatten() for n in names]), torch.cat([grads64[n].flatten() for n in names]))
    print(f"ranked f16: loss {float(loss):.6f} against {float(loss64):.6f} (relative {e_loss:.3g}); all gradients rel L2 {e_grad:.3g}")
    assert e_loss < 1e-3               # README's training contract for fp16 operands
    assert e_grad < 2e-3

    # blocks that do not sort keep the path the other switches give them
    mixed = _model(cname, dict(kw, num_layers=4), torch.float32, ranking=True)
    mixed.enable_ranking([False, True, False, True])
    mixed.set_fused_blocks(True)
    mixed.set_fused_ranking(True)
    with engine.precision("f16"):
        _, _, blocks_m, ranked_m = _ranked_step(mixed, x, target)
    assert ranked_m == (2, 2) and blocks_m == (2, 2)

    # the switch off again: bit-identical to a model that never had it; every no_grad forward is what it was
    fused.set_fused_ranking(False)
    step_a, step_b = _ranked_step(fused, x, target), _ranked_step(never, x, target)
    assert step_a[3] == (0, 0) and step_a[2] == (0, 0) and _same(step_a, step_b)
    fused.set_fused_ranking(True)
    eval_model.set_fused_ranking(True)
    with torch.no_grad():
        assert torch.equal(eval_model(x), logits0)
        r0 = pct_train.ranked_passes
        assert torch.equal(fused(x), train0) and pct_train.ranked_passes == r0


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. fallbacks
# ---------------------------------------------------------------------------------------------------------------------------------
def test_fused_ranking_fallbacks_take_the_path_they_had(monkeypatch):
    from peekvit_amd import engine
    from peekvit_amd.models.pct import RankPointCloudTransformer
    monkeypatch.setenv("PEEKVIT_AMD_TRAIN", "hip")
    monkeypatch.delenv("PEEKVIT_AMD_BACKEND", raising=False)
    kw = dict(num_points=32, num_layers=2, num_heads=2, hidden_dim=64, mlp_dim=128, num_classes=5)

    def make(**extra):
        torch.manual_seed(0)
        m = RankPointCloudTransformer(**dict(kw, **extra)).to(DEV).train()
        m.enable_ranking(True)
        m.set_budget(0.5)
        m.set_fused_ranking(True)
        return m

    m = make()
    x = torch.from_numpy(synth.synth_points(4, 32, 1)).to(DEV)

    def ran(model, inp):
        n0 = pct_train.ranked_passes
        model(inp)
        return pct_train.ranked_passes - n0

    assert ran(m, x) == 2                                      # eligible: both blocks
    assert ran(copy.deepcopy(m).eval(), x) == 0                # eval mode with grads: rows are dropped, not masked
    m.set_budget(0.0)
    assert ran(m, x) == 0                                      # keep = 0
    m.set_budget(0.5)
    assert ran(copy.deepcopy(m).cpu(), x.cpu()) == 0           # CPU tensors
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert ran(m, x) == 0
    with torch.no_grad():
        assert ran(m, x) == 0
    monkeypatch.setenv("PEEKVIT_AMD_TRAIN", "torch")
    assert ran(m, x) == 0
    monkeypatch.setenv("PEEKVIT_AMD_TRAIN", "hip")
    with engine.precision("bf16x3"):
        assert ran(m, x) == 0
    assert ran(make(attention_dropout=0.1), x) == 0            # active attention dropout
    assert ran(make(hidden_dim=96), x) == 0                    # hidden_dim 96: not a multiple of 64
    m.enable_ranking(False)
    assert ran(m, x) == 0                                      # `sort` off
    m.enable_ranking(True)
    assert ran(m, x) == 2
