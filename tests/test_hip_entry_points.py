"""Direct tests of the C-ABI entry points that model-level forwards reach but no op-level test called by name, and of the code paths
(dispatch buckets, second kernels, ragged edges) the op-level tests never reach.  Each kernel runs through its peekvit_amd.ops wrapper on
seeded inputs and is compared with a float64 restatement written here in plain torch ops, or, where include/peekvit_hip.h or a kernel
comment promises bit identity, with the kernel it names.

Tolerances:
  16-bit outputs    every element within one 16-bit ulp of the fp64 value.  For LayerNorm outputs the fp32 arithmetic the kernel is
                    documented to use adds its own bound, e32 below: no fp32 LayerNorm (torch's own included) rounds every element of
                    a row to within one 16-bit ulp of fp64 where x - mean or y - beta cancels.
  fp32 sums         bit-exact against the same fp32 additions in the documented order.
  other fp32        relative L2 < 1e-6 against fp64.
"""
import ctypes as C
import math

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = ("bf16", "f16")
LN_DS = (4, 12, 192, 260, 1280, 1536, 2052, 4096)      # every PV_DISPATCH_NCH bucket (NCH 1, 1, 1, 2, 8 partly, 8 partly, 16 partly, 16)


@pytest.fixture(scope="module")
def ops():
    from peekvit_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _ops


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _dt(mode):
    return torch.float16 if mode == "f16" else torch.bfloat16


def _ulp16(a, mode):
    """Spacing of the 16-bit format at |a| (float64 magnitudes); the subnormal spacing below the smallest normal."""
    mant, emin = (10, -14) if mode == "f16" else (7, -126)
    return torch.pow(2.0, torch.floor(torch.log2(a.clamp_min(2.0 ** emin))) - mant)


def _ulp32(a):
    return torch.pow(2.0, torch.floor(torch.log2(a.clamp_min(2.0 ** -126))) - 23)


def _assert_within_ulp16(got, ref, mode, extra=0.0, what=""):
    got = got.double().cpu()
    err = (got - ref).abs()
    bound = _ulp16(ref.abs(), mode) + extra
    bad = ~(err <= bound)
    if bad.any():
        i = int(torch.nonzero(bad.flatten())[0])
        pytest.fail(f"{what} [{mode}]: {int(bad.sum())} of {bad.numel()} elements beyond one 16-bit ulp of fp64; first at flat index {i}: "
                    f"got {got.flatten()[i].item()!r}, fp64 {ref.flatten()[i].item()!r}")


def _ln_fp64(x, gamma, beta, eps, row_scale=None):
    """fp64 LayerNorm of fp32 rows, and e32: 16 fp32 roundings of the terms the kernel's arithmetic sums (mean from a sum of |x|,
    x - mean, the product chain, + beta), i.e. how far its fp32 result may sit from fp64 before the 16-bit rounding."""
    x = x.double()
    g, b = gamma.double(), beta.double()
    mu = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + float(torch.tensor(eps, dtype=torch.float32)))
    y = (x - mu) * rstd * g + b
    e32 = 2.0 ** -20 * (g.abs() * rstd * ((x - mu).abs() + x.abs().mean(-1, keepdim=True)) + b.abs())
    if row_scale is not None:
        s = row_scale.double()[:, None]
        y, e32 = y * s, e32 * s.abs()
    return y, e32


def _ln_inputs(rows, D, seed, shift=0.3, scale=2.0):
    g = _g(seed)
    x = torch.randn(rows, D, generator=g) * scale + shift
    x += torch.randn(rows, 1, generator=g) * scale * 0.5              # rows of different means
    gamma = torch.randn(D, generator=g) * 0.5 + 1.0
    beta = torch.randn(D, generator=g) * 0.5
    rs = torch.rand(rows, generator=g)
    rs[0::3] = 0.0
    rs[1::3] = 0.3
    return x.float(), gamma.float(), beta.float(), rs.float()


# ---- pv_token_prologue --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("D", [64, 192, 768])
def test_token_prologue(ops, B, D):
    SENT = -777.25
    for n_special in (0, 1, 2, 5):
        for budget in (None, 0.0, 0.37, 1.0):
            g = _g(1000 * n_special + D)
            S = n_special + 7 + (budget is not None)
            special = torch.randn(max(n_special, 1), D, generator=g)
            pos = torch.randn(S, D, generator=g)
            btok = torch.randn(D, generator=g)
            tokens = torch.full((B, S, D), SENT, device=DEV)
            ops.token_prologue(tokens, special.to(DEV), pos.to(DEV), None if budget is None else btok.to(DEV),
                               0.0 if budget is None else budget, n_special)
            torch.cuda.synchronize()
            exp = torch.full((B, S, D), SENT)
            exp[:, :n_special] = special[:n_special] + pos[:n_special]                     # fp32 adds
            if budget is not None:
                exp[:, S - 1] = btok * torch.tensor(budget, dtype=torch.float32)           # fp32 product
            assert torch.equal(tokens.cpu(), exp), (n_special, budget)


# ---- pv_im2col_u8_bf16 --------------------------------------------------------------------------------------------------------
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
# channel 0 of this set tells x / 255 from x * (1 / 255): the two round one byte value to different 16-bit values, in both formats
OTHER_NORM = ((0.2, 0.62, 0.1), (0.331, 0.21, 0.45))


@pytest.mark.parametrize("B,H,W,P", [(2, 224, 224, 16), (3, 32, 48, 8), (1, 64, 64, 32), (5, 16, 16, 16)])
@pytest.mark.parametrize("mode", MODES)
def test_im2col_u8_equals_im2col_of_normalised_image(ops, B, H, W, P, mode):
    from peekvit_amd import engine
    x = torch.randint(0, 256, (B, H, W, 3), generator=_g(H * W + P), dtype=torch.uint8)
    x[0].view(-1, 3)[:256, 0] = torch.arange(256, dtype=torch.uint8)     # every byte value, 0 and 255 among them
    x[-1, -1, -4:] = 255
    K, M = 3 * P * P, B * (H // P) * (W // P)
    for mean, std in (IMAGENET, OTHER_NORM):
        # ToTensor + Normalize in fp32, this op order, every operand a full tensor (true division, no reciprocal)
        xf = x.permute(0, 3, 1, 2).contiguous().float()
        m = torch.tensor(mean, dtype=torch.float32)[None, :, None, None].expand_as(xf).contiguous()
        s = torch.tensor(std, dtype=torch.float32)[None, :, None, None].expand_as(xf).contiguous()
        norm = (xf / torch.full_like(xf, 255.0) - m) / s
        with engine.precision(mode):
            got = torch.empty((M, K), dtype=_dt(mode), device=DEV)
            ops.im2col_u8(x.to(DEV), P, got, mean, std)
            ref = torch.empty((M, K), dtype=_dt(mode), device=DEV)
            ops.im2col(norm.to(DEV), P, ref)
            torch.cuda.synchronize()
        assert torch.equal(got, ref), (mean, std)
        # and ops.im2col itself is the RNE rounding of the unfolded fp32 image
        unf = torch.nn.functional.unfold(norm, kernel_size=P, stride=P).transpose(1, 2).reshape(M, K)
        assert torch.equal(ref.cpu(), unf.to(_dt(mode)))


# ---- split-mode packers (bf16 library: precision mode "bf16x3") -----------------------------------------------------------------
def _planes(out, K):
    o = out.cpu()
    return o[:, :K], o[:, K:2 * K], o[:, 2 * K:]


@pytest.mark.parametrize("B,Cc,H,W,P", [(2, 3, 32, 48, 8), (1, 3, 224, 224, 16), (3, 2, 64, 64, 32)])
def test_im2col_split_planes(ops, B, Cc, H, W, P):
    x = torch.randn(B, Cc, H, W, generator=_g(H + P)) * 3.0
    x[0, 0, 0, :8] = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 65504.0, 3e38, 1.0 + 2 ** -8, 1.0 + 2 ** -9])
    K, M = Cc * P * P, B * (H // P) * (W // P)
    out = torch.empty((M, 3 * K), dtype=torch.bfloat16, device=DEV)
    ops.im2col_split(x.to(DEV), P, out)
    v = torch.nn.functional.unfold(x, kernel_size=P, stride=P).transpose(1, 2).reshape(M, K)
    hi, lo, hi2 = _planes(out, K)
    assert torch.equal(hi2, hi)
    assert torch.equal(hi, v.to(torch.bfloat16))                                   # RNE of the fp32 value
    assert torch.equal(lo, (v - hi.float()).to(torch.bfloat16))                    # (v - hi is exact in fp32)
    rec = hi.double() + lo.double()
    assert ((rec - v.double()).abs() <= 2.0 ** -16 * v.double().abs()).all()


def _check_ln_split(out_split, out_plain, x, gamma, beta, eps, rs, what):
    D = x.shape[1]
    hi, lo, hi2 = _planes(out_split, D)
    assert torch.equal(hi2, hi), what
    assert torch.equal(hi, out_plain.cpu()), what               # hi = pv_layernorm_bf16's RNE rounding of the same fp32 value
    ref, e32 = _ln_fp64(x, gamma, beta, eps, rs)
    hd, ld_ = hi.double(), lo.double()
    assert (ld_.abs() <= 0.5 * _ulp16(hd.abs(), "bf16")).all(), what        # hi is the nearest 16-bit value: |v - hi| <= half an ulp
    err = (hd + ld_ - ref).abs()
    bad = ~(err <= 2.0 ** -16 * ref.abs() + e32)
    assert not bad.any(), f"{what}: hi + lo off the fp64 LayerNorm in {int(bad.sum())} elements (max {float(err.max()):.3g})"


# ---- LayerNorm: every PV_DISPATCH_NCH bucket, both libraries, the split form ----------------------------------------------------
@pytest.mark.parametrize("rows", [1, 5, 4099])
@pytest.mark.parametrize("D", LN_DS)
def test_layernorm_every_bucket(ops, D, rows):
    from peekvit_amd import engine
    x, gamma, beta, rs = _ln_inputs(rows, D, seed=D + rows)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    for eps, scale in ((1e-5, None), (1e-6, rs)):
        sd = None if scale is None else scale.to(DEV)
        ref, e32 = _ln_fp64(x, gamma, beta, eps, scale)
        plain = {}
        for mode in MODES:
            with engine.precision(mode):
                out = torch.empty((rows, D), dtype=_dt(mode), device=DEV)
                ops.layernorm_bf16(xd, gd, bd, eps, out, sd)
                torch.cuda.synchronize()
            _assert_within_ulp16(out, ref, mode, e32, f"layernorm D={D} rows={rows} eps={eps} row_scale={scale is not None}")
            plain[mode] = out
        if scale is not None:
            z = scale == 0
            assert (plain["bf16"].cpu()[z].float() == 0).all() and (plain["f16"].cpu()[z].float() == 0).all()
        with engine.precision("bf16"):
            split = torch.empty((rows, 3 * D), dtype=torch.bfloat16, device=DEV)
            ops.layernorm_split(xd, gd, bd, eps, split, sd)
            torch.cuda.synchronize()
        _check_ln_split(split, plain["bf16"], x, gamma, beta, eps, scale, f"layernorm_split D={D} rows={rows} eps={eps}")


@pytest.mark.parametrize("D", [192, 1280, 4096])
def test_layernorm_two_pass_variance(ops, D):
    """Rows whose |mean| is ~100x their spread: E[x^2] - mean^2 in fp32 would lose the variance; the two-pass form must not."""
    from peekvit_amd import engine
    rows = 257
    x, gamma, beta, rs = _ln_inputs(rows, D, seed=7 * D, shift=0.0, scale=1.0)
    sign = torch.where(torch.arange(rows) % 2 == 0, 1.0, -1.0)[:, None]
    x = (x - x.mean(-1, keepdim=True) + 100.0 * sign * x.std(-1, keepdim=True)).float()
    ref, e32 = _ln_fp64(x, gamma, beta, 1e-6, None)
    for mode in MODES:
        with engine.precision(mode):
            out = torch.empty((rows, D), dtype=_dt(mode), device=DEV)
            ops.layernorm_bf16(x.to(DEV), gamma.to(DEV), beta.to(DEV), 1e-6, out)
            torch.cuda.synchronize()
        _assert_within_ulp16(out, ref, mode, e32, f"layernorm |mean| = 100 std, D={D}")
        if mode == "bf16":
            with engine.precision(mode):
                split = torch.empty((rows, 3 * D), dtype=torch.bfloat16, device=DEV)
                ops.layernorm_split(x.to(DEV), gamma.to(DEV), beta.to(DEV), 1e-6, split)
                torch.cuda.synchronize()
            _check_ln_split(split, out, x, gamma, beta, 1e-6, None, f"layernorm_split |mean| = 100 std, D={D}")


@pytest.mark.parametrize("D", [12, 260, 2052])
def test_layernorm_strided_input(ops, D):
    """ldx > D through the C entry itself (the wrapper always passes ldx = D): the same bits as the contiguous rows."""
    from peekvit_amd import _lib, engine
    rows, ldx = 37, D + 12
    x, gamma, beta, rs = _ln_inputs(rows, ldx, seed=D)
    gamma, beta = gamma[:D].contiguous(), beta[:D].contiguous()
    xs, xc = x.to(DEV), x[:, :D].contiguous()
    gd, bd, rd = gamma.to(DEV), beta.to(DEV), rs.to(DEV)
    ref, e32 = _ln_fp64(xc, gamma, beta, 1e-5, rs)
    for mode in MODES:
        for fn, width, wrapper in (("pv_layernorm_bf16", D, ops.layernorm_bf16), ("pv_layernorm_split_bf16", 3 * D, ops.layernorm_split)):
            if width != D and mode != "bf16":
                continue
            with engine.precision(mode):
                got = torch.full((rows, width), float("nan"), dtype=_dt(mode), device=DEV)
                exp = torch.empty((rows, width), dtype=_dt(mode), device=DEV)
                rc = getattr(_lib.load(), fn)(C.c_void_p(xs.data_ptr()), ldx, C.c_void_p(gd.data_ptr()), C.c_void_p(bd.data_ptr()),
                                              C.c_void_p(rd.data_ptr()), C.c_void_p(got.data_ptr()), rows, D, 1e-5, C.c_void_p(ops.raw_stream(0)))
                assert rc == 0
                wrapper(xc.to(DEV), gd, bd, 1e-5, exp, rd)
                torch.cuda.synchronize()
            assert torch.equal(got, exp), (fn, mode)
            _assert_within_ulp16(got[:, :D], ref, mode, e32, f"{fn} strided D={D}")


# ---- split-K finishes ---------------------------------------------------------------------------------------------------------
def _fp32_slice_sum(base, parts):
    out = base.clone()
    for t in range(parts.shape[0]):
        out += parts[t]                  # fp32, slice by slice
    return out


@pytest.mark.parametrize("n", [4, 5 * 768, 197 * 384])
@pytest.mark.parametrize("slices", [1, 2, 3, 6, 16])
def test_sum_slices_add(ops, n, slices):
    g = _g(n + slices)
    parts = torch.randn(slices, n, generator=g) * torch.logspace(-3, 3, slices)[:, None]
    base = torch.randn(n, generator=g) * 10
    exp = _fp32_slice_sum(base, parts)
    pd = parts.to(DEV)
    out = torch.full((n,), float("nan"), device=DEV)
    ops.sum_slices(pd, out, base=base.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), exp)
    inplace = base.to(DEV)                                           # base aliasing out
    ops.sum_slices(pd, inplace, base=inplace)
    torch.cuda.synchronize()
    assert torch.equal(inplace.cpu(), exp)


@pytest.mark.parametrize("D", LN_DS)
@pytest.mark.parametrize("mode", MODES)
def test_sum_slices_add_ln(ops, D, mode):
    from peekvit_amd import engine
    rows = 37
    g = _g(3 * D)
    gamma, beta = (torch.randn(D, generator=g) * 0.5 + 1.0), torch.randn(D, generator=g) * 0.5
    gd, bd = gamma.to(DEV), beta.to(DEV)
    for slices, alias in ((1, False), (3, True), (6, False), (16, True)):
        parts = torch.randn(slices, rows, D, generator=g)
        base = torch.randn(rows, D, generator=g) * 4 + 1
        exp = _fp32_slice_sum(base, parts)
        with engine.precision(mode):
            ln_out = torch.empty((rows, D), dtype=_dt(mode), device=DEV)
            out = base.to(DEV) if alias else torch.full((rows, D), float("nan"), device=DEV)
            ops.sum_slices(parts.to(DEV), out, base=out if alias else base.to(DEV), ln=(gd, bd, 1e-6, ln_out))
            sep = torch.empty_like(ln_out)
            ops.layernorm_bf16(out, gd, bd, 1e-6, sep)
            torch.cuda.synchronize()
        assert torch.equal(out.cpu(), exp), (slices, alias)
        assert torch.equal(ln_out, sep), (slices, alias)               # the header: bit-identical to pv_layernorm_bf16 on `out`
        ref, e32 = _ln_fp64(exp, gamma, beta, 1e-6)
        _assert_within_ulp16(ln_out, ref, mode, e32, f"sum_slices_add_ln D={D}")


def _gelu64(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


@pytest.mark.parametrize("M,N,slices", [(5, 768, 3), (197, 1536, 2), (64, 2304, 6), (1400, 3072, 2)])
@pytest.mark.parametrize("mode", MODES)
def test_sum_slices_act(ops, M, N, slices, mode):
    """gelu = 1: the fp64 erf GELU of the fp32 slice sum, within one 16-bit ulp + the A&S GELU's 1e-6; gelu = 0: the q pre-scale of the
    first qcols columns (an exact power of two) - the RNE rounding of the scaled fp32 sum, bit for bit.  1400 x 3072 wraps the grid-stride loop."""
    from peekvit_amd import engine
    g = _g(M + N + slices)
    parts = torch.randn(slices, M, N, generator=g) * 1.5
    s32 = parts[0].clone()
    for t in range(1, slices):
        s32 += parts[t]
    pd = parts.to(DEV)
    with engine.precision(mode):
        out = torch.empty((M, N), dtype=_dt(mode), device=DEV)
        ops.sum_slices_act(pd, out, gelu=True)
        torch.cuda.synchronize()
        _assert_within_ulp16(out, _gelu64(s32), mode, 1e-6, f"sum_slices_act gelu M={M} N={N}")
        for qcols in (0, (N // 3) // 4 * 4, N):
            out = torch.empty((M, N), dtype=_dt(mode), device=DEV)
            ops.sum_slices_act(pd, out, gelu=False, qcols=qcols, qscale=0.125)
            torch.cuda.synchronize()
            exp = s32.clone()
            exp[:, :qcols] *= 0.125
            assert torch.equal(out.cpu(), exp.to(_dt(mode))), qcols


@pytest.mark.parametrize("gelu", [True, False])
def test_sum_slices_act_range_flag(ops, gelu):
    """f16 library: the operand-range flag goes up when one finished value is above 65504 and stays down otherwise; bf16: never written."""
    from peekvit_amd import engine
    M, N, slices = 33, 512, 2
    parts = torch.randn(slices, M, N, generator=_g(5)) * 100.0
    big = parts.clone()
    big[0, 17, 300], big[1, 17, 300] = 40000.0, 30000.0                  # 70000 after the sum
    SENT = 256
    try:
        for mode in MODES:
            for p, over in ((parts, False), (big, True)):
                flag = torch.full((1,), SENT, dtype=torch.int32, device=DEV)
                ops.set_range_flag(flag)
                with engine.precision(mode):
                    out = torch.empty((M, N), dtype=_dt(mode), device=DEV)
                    ops.sum_slices_act(p.to(DEV), out, gelu=gelu, qcols=N, qscale=1.0)
                torch.cuda.synchronize()
                expect = SENT | 1 if (mode == "f16" and over) else SENT
                assert int(flag.item()) == expect, (mode, over)
    finally:
        ops.set_range_flag(None)


# ---- pv_masked_residual --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 591])
@pytest.mark.parametrize("D", [4, 384, 768])
@pytest.mark.parametrize("mode", MODES)
def test_masked_residual(ops, rows, D, mode):
    from peekvit_amd import engine
    g = _g(rows * D)
    x = torch.randn(rows, D, generator=g) * 3
    u = (torch.randn(rows, D, generator=g) * 2).to(_dt(mode))
    rs = torch.rand(rows, generator=g)
    rs[0::3] = 0.0
    rs[1::3] = 1.0
    rs[2::3] = 0.37
    with engine.precision(mode):
        out = torch.full((rows, D), float("nan"), device=DEV)
        ops.masked_residual(x.to(DEV), u.to(DEV), rs.to(DEV), out)
        torch.cuda.synchronize()
    got = out.cpu()
    ref = x.double() + rs.double()[:, None] * u.double()
    assert ((got.double() - ref).abs() <= _ulp32(ref.abs())).all()
    z = rs == 0
    assert torch.equal(got[z], x[z])


# ---- pv_cls_pool / pv_head_f32 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 192, 384, 1280, 4096])
def test_cls_pool(ops, D):
    B = 6
    g = _g(D)
    gamma, beta = torch.randn(D, generator=g) * 0.5 + 1.0, torch.randn(D, generator=g) * 0.5
    for S in (1, 17, 197):
        x = (torch.randn(B, S, D, generator=g) * 2 + 0.5).float()
        for nc in sorted({n for n in (1, 2, 16, S) if n <= S}):
            pooled = ops.cls_pool(x.to(DEV), gamma.to(DEV), beta.to(DEV), 1e-6, nc)
            torch.cuda.synchronize()
            ref = _ln_fp64(x[:, :nc].reshape(-1, D), gamma, beta, 1e-6)[0].reshape(B, nc, D).sum(1)
            err = rel_l2(pooled.cpu(), ref)
            assert err < 1e-6, f"cls_pool D={D} S={S} nc={nc}: rel L2 {err:.3g}"


@pytest.mark.parametrize("D", [4, 36, 100, 192, 768])
def test_head_both_kernels(ops, D):
    """B <= 16 runs pv_head_small_kernel, B > 16 the tiled pv_head_kernel (D % 32 != 0: a ragged last K step; C % 64 != 0: ragged columns).
    Inputs share a positive component so every logit is far from 0 and the per-row bound measures the kernel, not the conditioning."""
    g = _g(D)
    for C_ in (1, 10, 63, 65, 1000):
        w = (torch.randn(C_, D, generator=g) * 0.1 + 0.2).float()
        bias = torch.randn(C_, generator=g).float()
        a_all = (torch.randn(517, D, generator=g) + 2.0).float()
        for bi, B in enumerate((1, 16, 17, 33, 517)):
            b_ = bias if bi % 2 == 0 else None
            a = a_all[:B].contiguous()
            logits = ops.head(a.to(DEV), w.to(DEV), None if b_ is None else b_.to(DEV))
            torch.cuda.synchronize()
            ref = a.double() @ w.double().t() + (0.0 if b_ is None else b_.double())
            got = logits.cpu().double()
            row_err = (got - ref).norm(dim=1) / ref.norm(dim=1)
            assert float(row_err.max()) < 1e-6, f"head B={B} C={C_} D={D}: worst row rel L2 {float(row_err.max()):.3g}"
        # the kernel comment's claim: an image's logits do not depend on which kernel its batch selects
        wd, bd = w.to(DEV), bias.to(DEV)
        alone = ops.head(a_all[:16].contiguous().to(DEV), wd, bd)
        in17 = ops.head(a_all[:17].contiguous().to(DEV), wd, bd)
        in517 = ops.head(a_all.to(DEV), wd, bd)
        torch.cuda.synchronize()
        assert torch.equal(alone, in17[:16]) and torch.equal(alone, in517[:16]), (C_, D)


# ---- pv_rank_topk / pv_rank_topk_partials (the forms without the gap output) -----------------------------------------------------
def test_rank_topk_without_gap(ops):
    """The two plain rankings give the same keep lists as their _gap forms (what ops calls) and as a stable descending sort."""
    from peekvit_amd import _lib
    lib = _lib.load()
    g = _g(11)
    B, S, k, tiles = 7, 197, 98, 3
    rowsq = torch.rand(tiles, B * S, generator=g)
    rowsq[:, 5:9] = rowsq[:, 5:6]                                          # ties: lowest index first
    norms = rowsq.double().sum(0).sqrt().float().reshape(B, S)[:, 1:].contiguous()
    ref = torch.sort(-norms, dim=1, stable=True).indices[:, :k].int()
    nd, rd = norms.to(DEV), rowsq.to(DEV)
    stream = C.c_void_p(ops.raw_stream(0))
    keep = torch.full((B, k), -1, dtype=torch.int32, device=DEV)
    assert lib.pv_rank_topk(C.c_void_p(nd.data_ptr()), C.c_void_p(keep.data_ptr()), B, S - 1, k, stream) == 0
    keep_p = torch.full((B, k), -1, dtype=torch.int32, device=DEV)
    assert lib.pv_rank_topk_partials(C.c_void_p(rd.data_ptr()), tiles, C.c_void_p(keep_p.data_ptr()), B, S, k, stream) == 0
    gap_form = ops.rank_topk(nd, k)
    gap_form_p = ops.rank_topk_partials(rd, B, S, k)
    torch.cuda.synchronize()
    assert torch.equal(keep, gap_form) and torch.equal(keep.cpu(), ref)
    assert torch.equal(keep_p, gap_form_p)
