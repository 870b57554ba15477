"""GPU parity, op level: every C-ABI kernel against the CPU oracle on the same seeded inputs.
Inputs are bf16-representable, so bf16-operand kernels differ from the oracle's bf16 mode only by fp32
summation order (and by 1-ulp bf16 rounding flips on bf16 outputs)."""
import math

import numpy as np
import pytest
import torch

from conftest import rel_l2
from oracle import vit_oracle as O
from peekvit_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from peekvit_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _ops


def T(name, shape, kind="normal", scale=1.0, shift=0.0, bf16=True):
    return torch.from_numpy(synth.tensor("t/" + name, shape, kind, scale, shift, seed=1, bf16=bf16))


def bf(x):   # fp32 tensor holding bf16-representable values -> bf16 GPU tensor
    return x.to(torch.bfloat16).to(DEV)


def test_cast_and_im2col_bit_exact(ops):
    x = T("img", (3, 3, 32, 48))
    cols = torch.empty((3 * 4 * 6, 3 * 64), dtype=torch.bfloat16, device=DEV)
    ops.im2col(x.to(DEV), 8, cols)
    ref = torch.nn.functional.unfold(x, kernel_size=8, stride=8).transpose(1, 2).reshape(-1, 192)
    assert torch.equal(cols.float().cpu(), ref)
    # non-vector path (P not a multiple of 8)
    x2 = T("img2", (2, 3, 12, 12))
    cols2 = torch.empty((2 * 4, 3 * 36), dtype=torch.bfloat16, device=DEV)
    ops.im2col(x2.to(DEV), 6, cols2)
    ref2 = torch.nn.functional.unfold(x2, kernel_size=6, stride=6).transpose(1, 2).reshape(-1, 108)
    assert torch.equal(cols2.float().cpu(), ref2)
    v = T("cast", (1037,), bf16=False)
    assert torch.equal(ops.cast_bf16(v.to(DEV)).cpu(), v.to(torch.bfloat16))


@pytest.mark.parametrize("rows,D", [(7, 64), (197 * 3, 768), (50, 256), (33, 384), (5, 1024), (3, 2048)])
def test_layernorm(ops, rows, D):
    x = T(f"ln{D}", (rows, D), scale=2.0, shift=0.3, bf16=False)
    g, b = T(f"lng{D}", (D,), "uniform", 0.2, 1.0), T(f"lnb{D}", (D,), "uniform", 0.1)
    rs = T(f"lnrs{D}", (rows,), "uniform", 0.5, 0.5, bf16=False)
    for eps, scale in ((1e-5, None), (1e-6, rs)):
        out = torch.empty((rows, D), dtype=torch.bfloat16, device=DEV)
        ops.layernorm_bf16(x.to(DEV), g.to(DEV), b.to(DEV), eps, out, None if scale is None else scale.to(DEV))
        ref = O.layer_norm(x, g, b, eps)
        if scale is not None:
            ref = ref * scale[:, None]
        got = out.float().cpu()
        assert rel_l2(got, ref) < 3e-3                      # bf16 output rounding
        assert (got - ref).abs().max() <= 2.0 ** -7 * ref.abs().max()


# the last four shapes (M >= 2048, N % 256 == 0, K % 128 == 0) run the 256x256 deep-pipelined kernel, incl. a ragged M edge
GEMM_SHAPES = [(100, 128, 64), (256, 256, 128), (300, 384, 192), (197 * 2, 2304, 768), (130, 768, 3072), (77, 1000, 256),
               (2048, 256, 128), (2304 + 37, 768, 768), (2048, 2304, 256), (2100, 768, 3072),
               (2048, 768, 768), (4096 + 128, 2304, 768), (2048 + 384, 768, 3072), (2560, 3072, 768), (66 * 128, 256, 1536),
               # N % 256 == 128: ragged last column tile of the 256^2 kernel (vit_small: 384, 1152)
               (2048 + 77, 384, 384), (2304, 1152, 384), (2048, 640, 256)]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_epilogues(ops, M, N, K):
    from peekvit_amd._lib import PV_EPI_BIAS_BF16, PV_EPI_BIAS_GELU_BF16, PV_EPI_BIAS_RES_F32
    a, w = T(f"ga{M}{K}", (M, K)), T(f"gw{N}{K}", (N, K), "uniform", 1.0 / math.sqrt(K))
    bias = T(f"gb{N}", (N,), "uniform", 0.1, bf16=False)
    res = T(f"gr{M}{N}", (M, N), bf16=False)
    rs = T(f"gs{M}", (M,), "uniform", 0.5, 0.5, bf16=False)
    ref = a.double() @ w.double().t() + bias.double()
    A, W, Bv = bf(a), bf(w), bias.to(DEV)
    # bias (+ q scaling on the first qcols columns), bf16 out
    out = torch.empty((M, N), dtype=torch.bfloat16, device=DEV)
    qcols = (N // 3) // 4 * 4
    ops.gemm(A, W, Bv, out, PV_EPI_BIAS_BF16, qcols=qcols, qscale=0.125)
    r = ref.clone()
    r[:, :qcols] *= 0.125
    assert rel_l2(out.float().cpu(), r) < 3e-3
    # bias + exact GELU, bf16 out
    ops.gemm(A, W, Bv, out, PV_EPI_BIAS_GELU_BF16)
    assert rel_l2(out.float().cpu(), torch.nn.functional.gelu(ref)) < 3e-3
    # bias + residual (+ row scale), fp32 out
    o32 = torch.empty((M, N), dtype=torch.float32, device=DEV)
    ops.gemm(A, W, Bv, o32, PV_EPI_BIAS_RES_F32, res=res.to(DEV))
    assert rel_l2(o32.cpu(), ref + res.double()) < 2e-6
    ops.gemm(A, W, Bv, o32, PV_EPI_BIAS_RES_F32, res=res.to(DEV), row_scale=rs.to(DEV))
    assert rel_l2(o32.cpu(), rs.double()[:, None] * ref + res.double()) < 2e-6
    # in-place residual (out aliases res)
    inpl = res.to(DEV).clone()
    ops.gemm(A, W, Bv, inpl, PV_EPI_BIAS_RES_F32, res=inpl)
    assert rel_l2(inpl.cpu(), ref + res.double()) < 2e-6


def test_gemm_patch_embed_epilogue(ops):
    from peekvit_amd._lib import PV_EPI_BIAS_POS_F32
    B, Np, S, D, K, off = 3, 16, 19, 128, 192, 2
    a, w = T("pa", (B * Np, K)), T("pw", (D, K), "uniform", 0.07)
    bias, pos = T("pb", (D,), "uniform", 0.1), T("pp", (S, D), scale=0.02)
    out = torch.full((B, S, D), 7.0, dtype=torch.float32, device=DEV)
    ops.gemm(bf(a), bf(w), bias.to(DEV), out.view(B * S, D), PV_EPI_BIAS_POS_F32, pos=pos.to(DEV),
             rows_per_img_in=Np, rows_per_img_out=S, row_off=off)
    ref = (a.double() @ w.double().t() + bias.double()).view(B, Np, D) + pos.double()[off:off + Np]
    got = out.cpu()
    assert rel_l2(got[:, off:off + Np], ref) < 2e-6
    assert torch.all(got[:, :off] == 7.0) and torch.all(got[:, off + Np:] == 7.0)   # untouched rows


def test_gemm_patch_embed_epilogue_big_kernel(ops):
    """Same epilogue at a shape the 256^2 kernel takes (M = B*Np >= 2048, K = 768), row remap across images."""
    from peekvit_amd._lib import PV_EPI_BIAS_POS_F32
    B, Np, S, D, K, off = 32, 196, 199, 256, 768, 2
    a, w = T("ppa", (B * Np, K)), T("ppw", (D, K), "uniform", 0.04)
    bias, pos = T("ppb", (D,), "uniform", 0.1), T("ppp", (S, D), scale=0.02)
    out = torch.full((B, S, D), 7.0, dtype=torch.float32, device=DEV)
    ops.gemm(bf(a), bf(w), bias.to(DEV), out.view(B * S, D), PV_EPI_BIAS_POS_F32, pos=pos.to(DEV),
             rows_per_img_in=Np, rows_per_img_out=S, row_off=off)
    ref = (a.double() @ w.double().t() + bias.double()).view(B, Np, D) + pos.double()[off:off + Np]
    got = out.cpu()
    assert rel_l2(got[:, off:off + Np], ref) < 2e-6
    assert torch.all(got[:, :off] == 7.0) and torch.all(got[:, off + Np:] == 7.0)


@pytest.mark.parametrize("M,N,K", [(41 * 256 + 37, 13 * 256 - 128, 256), (64 * 256, 9 * 256, 768), (43 * 256 + 200, 3 * 256 * 5 - 128, 384)])
def test_gemm_persistent_launch_is_bit_identical(ops, M, N, K):
    """Shapes with >= 2 x CUs tiles run the prefetching persistent launch (pv_gemm256_pf_kernel: the next tile's first K-tile and bias are
    staged under the epilogue).  A tile's arithmetic is the one-tile kernel's: every epilogue must reproduce it bit for bit, ragged bottom
    row tile and ragged last column tile included; pv_debug_set_gemm_pf(0) = one tile per workgroup."""
    from peekvit_amd import _lib
    from peekvit_amd._lib import (PV_EPI_BIAS_BF16, PV_EPI_BIAS_F32, PV_EPI_BIAS_GELU_BF16, PV_EPI_BIAS_GELU_PAIR_BF16, PV_EPI_BIAS_POS_F32,
                                  PV_EPI_BIAS_RES_F32, PV_EPI_GELU_GRAD_BF16)
    lib = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(M + N)
    A = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
    W = (torch.randn(N, K, generator=g, device=DEV) * K ** -0.5).to(torch.bfloat16)
    bias = torch.randn(N, generator=g, device=DEV) * 0.1
    res = torch.randn(M, N, generator=g, device=DEV)
    pre = torch.randn(M, N, generator=g, device=DEV).to(torch.bfloat16)
    rs = torch.rand(M, generator=g, device=DEV) + 0.5
    stat = torch.stack([torch.randn(M, generator=g, device=DEV) * 0.05, 1.0 + 0.1 * torch.rand(M, generator=g, device=DEV)], 1).contiguous()
    c1 = W.float().sum(1).contiguous()
    rpi = 197
    B = (M + rpi - 2) // (rpi - 1)
    pos = torch.randn(rpi, N, generator=g, device=DEV) * 0.02

    def run_all():
        r = {}
        o16 = lambda: torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
        o32 = lambda: torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
        r["bias"] = ops.gemm(A, W, bias, o16(), PV_EPI_BIAS_BF16, qcols=(N // 3) // 8 * 8, qscale=0.125)
        r["bias_fold"] = ops.gemm(A, W, None, o16(), PV_EPI_BIAS_BF16, fold=(stat, c1, bias))
        r["gelu"] = ops.gemm(A, W, bias, o16(), PV_EPI_BIAS_GELU_BF16)
        r["gelu_fold"] = ops.gemm(A, W, None, o16(), PV_EPI_BIAS_GELU_BF16, fold=(stat, c1, bias))
        pair = torch.full((M, 2 * N), float("nan"), dtype=torch.bfloat16, device=DEV)      # training fc1: [gelu(h) | h]
        r["pair"] = ops.gemm(A, W, bias, pair, PV_EPI_BIAS_GELU_PAIR_BF16)
        r["f32"] = ops.gemm(A, W, bias, o32(), PV_EPI_BIAS_F32)
        r["res"] = ops.gemm(A, W, bias, o32(), PV_EPI_BIAS_RES_F32, res=res, row_scale=rs)
        x16, part = o16(), torch.full(((N + 255) // 256, M, 2), float("nan"), device=DEV)
        r["res_fold"] = ops.gemm(A, W, bias, o32(), PV_EPI_BIAS_RES_F32, res=res, x16_out=x16, rowstat_out=part)
        r["res_fold_x16"], r["res_fold_stat"] = x16, part
        sq = torch.full(((N + 255) // 256, M), float("nan"), device=DEV)
        r["res_rowsq"] = ops.gemm(A, W, bias, o32(), PV_EPI_BIAS_RES_F32, res=res, rowsq_out=sq)
        r["rowsq"] = sq
        cs = torch.zeros(N, device=DEV)
        r["gelu_grad"] = ops.gemm(A, W, None, o16(), PV_EPI_GELU_GRAD_BF16, res=pre, colsum_out=cs)
        r["gelu_grad_colsum"] = cs
        outp = torch.full((B * rpi, N), 7.0, device=DEV)
        Mp = B * (rpi - 1)
        if Mp <= M:
            r["pos"] = ops.gemm(A[:Mp], W, bias, outp, PV_EPI_BIAS_POS_F32, pos=pos, rows_per_img_in=rpi - 1, rows_per_img_out=rpi, row_off=1)
        torch.cuda.synchronize()
        return r

    lib.pv_debug_set_gemm_pf(0)
    try:
        one = run_all()
        lib.pv_debug_set_gemm_pf(1)
        pf = run_all()
        again = run_all()
    finally:
        lib.pv_debug_set_gemm_pf(-1)
    for k in one:
        assert not torch.isnan(one[k].float()).any(), k
        assert torch.equal(one[k], pf[k]), k
        assert torch.equal(pf[k], again[k]), k


def test_gemm_kernels_agree_bitwise(ops, tmp_path):
    """An output element is rounded identically by the 128^2 and 256^2 kernels (batch invariance relies on it)."""
    import os, subprocess, sys
    code = (
        "import sys, torch; sys.path.insert(0, %r); from peekvit_amd import ops, synth\n"
        "from peekvit_amd._lib import PV_EPI_BIAS_GELU_BF16, PV_EPI_BIAS_RES_F32\n"
        "g = torch.Generator(device='cuda').manual_seed(5)\n"
        "a = torch.randn(2048, 768, generator=g, device='cuda').bfloat16(); w = (torch.randn(768, 768, generator=g, device='cuda') / 28).bfloat16()\n"
        "b = torch.randn(768, generator=g, device='cuda'); r = torch.randn(2048, 768, generator=g, device='cuda')\n"
        "o1 = torch.empty(2048, 768, device='cuda'); ops.gemm(a, w, b, o1, PV_EPI_BIAS_RES_F32, res=r)\n"
        "o2 = torch.empty(2048, 768, dtype=torch.bfloat16, device='cuda'); ops.gemm(a, w, b, o2, PV_EPI_BIAS_GELU_BF16)\n"
        "torch.save((o1.cpu(), o2.cpu()), sys.argv[1])\n") % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for tile in ("128", "256"):
        path = str(tmp_path / f"pv_gemm_tile_{tile}.pt")
        subprocess.check_call([sys.executable, "-c", code, path], env=dict(os.environ, PV_GEMM_TILE=tile))
        outs.append(torch.load(path))
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])


@pytest.mark.parametrize("M,N,K", [(300, 256, 128), (2048 + 77, 768, 768), (1000, 768, 3072), (520, 1024, 256),
                                   (3000, 384, 384), (1001, 384, 1536), (2100, 256, 768), (700, 512, 512), (128 * 97 + 5, 384, 64), (50, 512, 1536),
                                   # more than one round of 128-row tiles on 256 CUs with a remainder of at most half a round: the split remainder
                                   # (whole rounds of 128-row tiles + one round of 64-row tiles, ragged last tile) of the full-row kernel; and
                                   # a remainder beyond half a round (plain 128-row tiles)
                                   (256 * 128 + 5003, 384, 384), (2 * 256 * 128 + 64 * 256 - 1, 256, 128), (256 * 128 + 20000, 512, 128),
                                   # round 4, the deep-pipelined K loop of the full-row kernel (K % 128 == 0; K = 64 and 192 keep the plain loop): 2, 3, 5, 8 and
                                   # 16 K-tile pairs at every width, 64-row tail tiles, fewer rows than one tile
                                   (5000, 384, 640), (777, 256, 1024), (4097, 512, 256), (130, 384, 2048), (63, 256, 256), (3 * 128 + 1, 384, 192),
                                   (256 * 128 + 64 * 40 + 3, 384, 768),
                                   # round 6, a LAST ROUND of 160-row tiles (N <= 384, deep-pipelined loop, remainder of the last whole round <= 32 rows per CU):
                                   # vit_small's own shapes at batch 512 (two rounds of 128-row tiles + 221 tiles of 160 rows), one round of 160-row tiles only,
                                   # N = 256, the remainder at the rule's boundary and one row beyond it (-> 64-row tiles), a ragged last 160-row tile
                                   (512 * 197, 384, 384), (512 * 197, 384, 1536), (256 * 128 + 8000, 256, 256), (256 * 128 + 8192, 384, 128),
                                   (256 * 128 + 8193, 384, 128), (2 * 256 * 128 + 161, 256, 768)])
def test_gemm_fused_layernorm_bit_identical_to_separate_kernels(ops, M, N, K):
    """GEMM with fused LayerNorm (full-row tile for N = 256 / 384 / 512, row-block kernel otherwise) == plain GEMM followed by
    pv_layernorm_bf16, bit for bit (with and without row scale); N = 384 ... also cover the full-row kernel WITHOUT LayerNorm against the
    128^2 / 256^2 kernels (PV_GEMM_FULLROW-independent: an element rounds identically in every kernel)."""
    from peekvit_amd._lib import PV_EPI_BIAS_RES_F32
    a, w = bf(T(f"fa{M}{K}", (M, K))), bf(T(f"fw{N}{K}", (N, K), "uniform", 1.0 / math.sqrt(K)))
    bias, res = T(f"fb{N}", (N,), "uniform", 0.1).to(DEV), T(f"fr{M}{N}", (M, N), bf16=False).to(DEV)
    g, b = T(f"fg{N}", (N,), "uniform", 0.2, 1.0).to(DEV), T(f"fbeta{N}", (N,), "uniform", 0.1).to(DEV)
    rs = T(f"frs{M}", (M,), "uniform", 0.5, 0.5, bf16=False).to(DEV)
    for scale in (None, rs):
        o1 = torch.empty((M, N), dtype=torch.float32, device=DEV)
        ops.gemm(a, w, bias, o1, PV_EPI_BIAS_RES_F32, res=res, row_scale=scale)
        h1 = torch.empty((M, N), dtype=torch.bfloat16, device=DEV)
        ops.layernorm_bf16(o1, g, b, 1e-5, h1, scale)
        o2 = torch.empty((M, N), dtype=torch.float32, device=DEV)
        h2 = torch.full((M, N), 7.0, dtype=torch.bfloat16, device=DEV)
        ops.gemm(a, w, bias, o2, PV_EPI_BIAS_RES_F32, res=res, row_scale=scale, ln=(g, b, 1e-5, h2, scale))
        assert torch.equal(o1, o2)
        assert torch.equal(h1, h2)
    if N in (256, 384, 512) and K % 128 == 0:
        # without a bias (the deep-pipelined full-row loop takes its bias through LDS: the accumulators then start from zero)
        o1 = torch.empty((M, N), dtype=torch.float32, device=DEV)
        ops.gemm(a, w, None, o1, PV_EPI_BIAS_RES_F32, res=res)
        h1 = torch.empty((M, N), dtype=torch.bfloat16, device=DEV)
        ops.layernorm_bf16(o1, g, b, 1e-5, h1, None)
        o2 = torch.empty((M, N), dtype=torch.float32, device=DEV)
        h2 = torch.full((M, N), 7.0, dtype=torch.bfloat16, device=DEV)
        ops.gemm(a, w, None, o2, PV_EPI_BIAS_RES_F32, res=res, ln=(g, b, 1e-5, h2, None))
        assert torch.equal(o1, o2) and torch.equal(h1, h2)
        ref = a.float() @ w.float().t() + res
        assert rel_l2(o2, ref) < 2e-5


def test_gemm_rejects_bad_shapes(ops):
    from peekvit_amd._lib import PV_EPI_BIAS_BF16, PeekvitHipError
    a, w = bf(T("ba", (8, 96))), bf(T("bw", (16, 96)))
    with pytest.raises(PeekvitHipError):
        ops.gemm(a, w, None, torch.empty((8, 16), dtype=torch.bfloat16, device=DEV), PV_EPI_BIAS_BF16)   # K % 64 != 0


@pytest.mark.parametrize("B,S,H,dh", [(2, 197, 12, 64), (3, 17, 2, 64), (2, 401, 8, 32), (2, 197, 8, 48), (2, 99, 3, 64),
                                      (1, 50, 4, 64), (2, 26, 12, 64), (1, 5, 2, 32), (1, 1, 1, 64), (2, 64, 2, 32)])
def test_attention(ops, B, S, H, dh):
    D = H * dh
    qkv = T(f"qkv{S}{H}{dh}", (B, S, 3 * D), scale=1.0)
    qkv[..., :D] *= dh ** -0.5            # q arrives pre-scaled from the in-proj epilogue
    qkv = qkv.to(torch.bfloat16).float()
    out = torch.empty((B, S, D), dtype=torch.bfloat16, device=DEV)
    ops.attention(qkv.to(torch.bfloat16).to(DEV), out, B, S, H, dh)
    q, k, v = (t.reshape(B, S, H, dh).transpose(1, 2) for t in qkv.split(D, dim=-1))
    ref = O.attention_core(q, k, v, "bf16").transpose(1, 2).reshape(B, S, D)
    assert rel_l2(out.float().cpu(), ref) < 3e-3
    exact = torch.softmax(q.double() @ k.double().transpose(-1, -2), -1) @ v.double()
    assert rel_l2(out.float().cpu(), exact.transpose(1, 2).reshape(B, S, D)) < 6e-3


@pytest.mark.parametrize("B,S,H,dh", [(1, 417, 2, 64), (2, 577, 12, 64), (1, 785, 3, 32), (1, 1025, 2, 48), (1, 2000, 1, 64),
                                      (2, 257, 4, 80), (1, 197, 2, 128), (1, 50, 3, 96)])
def test_attention_long_sequences(ops, B, S, H, dh):
    """S > 416 (e.g. 384x384 images at patch 16: S = 577): the streaming kernel with the online softmax."""
    D = H * dh
    qkv = T(f"lqkv{S}{H}{dh}", (B, S, 3 * D), scale=1.0)
    qkv[..., :D] *= dh ** -0.5
    qkv[0, 5, :dh] = 3.0                   # one query with a few dominant keys: exercises the running-max rescale across blocks
    qkv[0, S - 3, D:D + dh] = 3.0
    qkv = qkv.to(torch.bfloat16).float()
    out = torch.full((B, S, D), float("nan"), dtype=torch.bfloat16, device=DEV)
    ops.attention(qkv.to(torch.bfloat16).to(DEV), out, B, S, H, dh)
    q, k, v = (t.reshape(B, S, H, dh).transpose(1, 2) for t in qkv.split(D, dim=-1))
    exact = (torch.softmax(q.double() @ k.double().transpose(-1, -2), -1) @ v.double()).transpose(1, 2).reshape(B, S, D)
    assert torch.isfinite(out.float()).all()
    assert rel_l2(out.float().cpu(), exact) < 6e-3


def test_attention_spiked_scores(ops):
    """One key dominates a query row (softmax ~ one-hot) and one row has huge negative scores."""
    B, S, H, dh = 1, 197, 1, 64
    qkv = T("spk", (B, S, 3 * dh), scale=0.5)
    qkv[0, 3, :dh] = 6.0
    qkv[0, 100, dh:2 * dh] = 6.0
    qkv[0, 7, :dh] = -6.0
    qkv = qkv.to(torch.bfloat16).float()
    out = torch.empty((B, S, dh), dtype=torch.bfloat16, device=DEV)
    ops.attention(qkv.to(torch.bfloat16).to(DEV), out, B, S, H, dh)
    q, k, v = (t.reshape(B, S, H, dh).transpose(1, 2) for t in qkv.split(dh, dim=-1))
    ref = O.attention_core(q, k, v, "bf16").transpose(1, 2).reshape(B, S, dh)
    assert torch.isfinite(out.float()).all()
    assert rel_l2(out.float().cpu(), ref) < 3e-3


@pytest.mark.parametrize("B,S,H,dh,nq", [(3, 197, 12, 64, 1), (2, 197, 3, 64, 2), (2, 26, 12, 64, 1), (1, 1, 1, 64, 1), (2, 5, 2, 32, 1),
                                         (2, 401, 8, 32, 3), (2, 99, 8, 48, 1), (1, 577, 2, 128, 1), (2, 50, 3, 96, 2), (1, 7, 4, 80, 1)])
def test_attention_rows(ops, B, S, H, dh, nq):
    """Attention for the first nq rows of every image only (the last encoder block): k | v of all tokens in a [B*S, 2D] buffer,
    q of the wanted rows in its own; softmax weights stay fp32, so the only rounding is the 16-bit output."""
    D = H * dh
    qkv = T(f"rqkv{S}{H}{dh}", (B, S, 3 * D), scale=1.0)
    qkv[..., :D] *= dh ** -0.5
    qkv[0, 0, :dh] = 3.0                   # a query with a few dominant keys (running-max rescale inside and across the lane groups)
    qkv[0, S - 1, D:D + dh] = 3.0
    qkv = qkv.to(torch.bfloat16).float()
    q = qkv[:, :nq, :D].reshape(B * nq, D).contiguous()
    wide = torch.zeros((B * S, 2 * D + 64), dtype=torch.bfloat16, device=DEV)      # row stride wider than 2D: a view into a larger buffer
    wide[:, :2 * D] = qkv[..., D:].reshape(B * S, 2 * D).to(torch.bfloat16).to(DEV)
    out = torch.full((B * nq, D), float("nan"), dtype=torch.bfloat16, device=DEV)
    ops.attention_rows(bf(q), wide[:, :2 * D], out, B, S, nq, H, dh)
    qh, kh, vh = (t.reshape(B, S, H, dh).transpose(1, 2).double() for t in qkv.split(D, dim=-1))
    exact = (torch.softmax(qh[:, :, :nq] @ kh.transpose(-1, -2), -1) @ vh).transpose(1, 2).reshape(B * nq, D)
    assert torch.isfinite(out.float()).all()
    assert rel_l2(out.float().cpu(), exact) < 3e-3
    # the full kernel's rows agree (it rounds the softmax weights to 16 bits, this one does not)
    full = torch.empty((B, S, D), dtype=torch.bfloat16, device=DEV)
    ops.attention(qkv.to(torch.bfloat16).to(DEV), full, B, S, H, dh)
    assert rel_l2(out.float().cpu(), full[:, :nq].reshape(B * nq, D).float().cpu()) < 8e-3


def test_attention_rows_rejects_bad_arguments(ops):
    from peekvit_amd._lib import PeekvitHipError
    q = torch.zeros((2, 64), dtype=torch.bfloat16, device=DEV)
    kv = torch.zeros((10, 128), dtype=torch.bfloat16, device=DEV)
    out = torch.zeros((2, 64), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(PeekvitHipError):
        ops.attention_rows(q, kv[:, :64], out, 2, 5, 1, 1, 64)          # no room for v
    with pytest.raises(PeekvitHipError):
        ops.attention_rows(q, kv, out, 2, 4, 1, 1, 64)                  # B*S rows expected
    with pytest.raises(PeekvitHipError):
        ops.attention_rows(q.float(), kv, out, 2, 5, 1, 1, 64)          # operand type
    with pytest.raises(PeekvitHipError):
        ops.attention_rows(q, kv, out, 2, 5, 1, 1, 40)                  # head width not built


def test_cls_pool_and_head(ops):
    B, S, D, C = 5, 9, 256, 1000
    x = T("cp", (B, S, D), scale=1.5, bf16=False)
    g, b = T("cpg", (D,), "uniform", 0.2, 1.0), T("cpb", (D,), "uniform", 0.1)
    for nc in (1, 3):
        pooled = ops.cls_pool(x.to(DEV), g.to(DEV), b.to(DEV), 1e-5, nc)
        ref = O.layer_norm(x[:, :nc], g, b, 1e-5).sum(1)
        assert rel_l2(pooled.cpu(), ref) < 1e-6
    w, hb = T("hw", (C, D), scale=0.02), T("hb", (C,), "uniform", 0.02)
    logits = ops.head(pooled, w.to(DEV), hb.to(DEV))
    assert rel_l2(logits.cpu(), pooled.cpu().double() @ w.double().t() + hb.double()) < 1e-6
    assert logits.shape == (B, C)


def test_rank_path_bit_exact_vs_reference_golden(ops, golden):
    """token_norm -> rank_topk -> gather against indices/outputs the REAL reference produced."""
    from oracle.make_golden import sorted_gap_tokens
    g = golden("sort_and_drop")
    for N in (196, 400):
        x = torch.from_numpy(sorted_gap_tokens(2, N, 64, seed=0))
        xd = x.to(DEV)
        norms = ops.token_norm(xd)
        assert rel_l2(norms.cpu(), torch.norm(x[:, 1:], dim=-1)) < 1e-6
        for b in (0.1, 0.25, 0.5, 0.75, 0.99):
            k = math.ceil(N * b)
            keep = ops.rank_topk(norms, k)
            assert np.array_equal(keep.cpu().numpy().astype(np.int64), g[f"N{N}_b{b}_idx"])      # bit-exact indices
            out = ops.gather_tokens(xd, keep)
            assert np.array_equal(out.cpu().numpy(), g[f"N{N}_b{b}_out"])                        # bit-exact rows


def test_rank_ties_lowest_index_first_and_edges(ops):
    norms = torch.tensor([[1.0, 3.0, 3.0, 0.5, 3.0, 2.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]], device=DEV)
    keep = ops.rank_topk(norms, 6).cpu()
    assert keep[0].tolist() == [1, 2, 4, 5, 0, 3] and keep[1].tolist() == [0, 1, 2, 3, 4, 5]
    assert ops.rank_topk(norms, 1).cpu()[:, 0].tolist() == [1, 0]
    x = T("g1", (2, 7, 64), bf16=False).to(DEV)
    out = ops.gather_tokens(x, keep[:, :1].to(DEV).contiguous())       # k = 1
    assert torch.equal(out[:, 0], x[:, 0]) and torch.equal(out[0, 1], x[0, 2]) and torch.equal(out[1, 1], x[1, 1])


def test_residual_gate(ops):
    B, S, D = 3, 19, 128
    x = T("rg", (B, S, D), bf16=False)
    wg, bg = T("rgw", (1, D), "uniform", 0.3), T("rgb", (1,), "uniform", 0.1)
    wb, bb = T("rbw", (1, D), "uniform", 0.1), T("rbb", (1,), "uniform", 0.1)
    for sbias in (10.0, 0.0):
        xo = torch.empty_like(x, device=DEV)
        mask, rs = ops.residual_gate(x.to(DEV), xo, wg.to(DEV), bg.to(DEV), wb.to(DEV), bb.to(DEV), 1.0, sbias)
        thr = torch.sigmoid(torch.nn.functional.linear(x[:, -1:], wb, bb))
        ref = O.residual_gate(x[:, 1:-1], wg, bg, 1.0, sbias, thr)
        assert (mask.cpu() - ref).abs().max() < 1e-6
        if sbias == 0.0:
            assert (ref == 0).any() and torch.equal(mask.cpu() == 0, ref == 0)
        m = mask.cpu()
        exp = torch.cat([x[:, :1], m * x[:, 1:-1], x[:, -1:]], dim=1)
        assert torch.equal(xo.cpu(), exp)
        assert torch.equal(rs.cpu(), torch.cat([torch.ones(B, 1), m[..., 0], torch.ones(B, 1)], dim=1))


@pytest.mark.parametrize("M,D,N,epi", [(2304, 768, 2304, 0), (4096, 768, 3072, 1), (2050, 384, 1152, 0)])
def test_layernorm_folded_into_gemms(ops, M, D, N, epi):
    """LayerNorm folding: the producer GEMM (residual epilogue) also writes the 16-bit copy of its rows + per-tile (sum, sumsq);
    pv_rowstat_finalize turns them into (mean, rstd); the consumer GEMM on that copy with gamma (.) W finishes
    rstd * (acc - mean * c1) + c2.  Checked against the same formula in fp64 and against LayerNorm -> Linear."""
    from peekvit_amd._lib import PV_EPI_BIAS_RES_F32
    K0 = 256
    a, w0 = T(f"fa{M}", (M, K0)).to(torch.bfloat16), T(f"fw{D}", (D, K0), "uniform", K0 ** -0.5).to(torch.bfloat16)
    b0, res = T(f"fb{D}", (D,), "uniform", 0.1), T(f"fr{M}{D}", (M, D), scale=2.0, shift=0.3, bf16=False)
    x = torch.empty((M, D), dtype=torch.float32, device=DEV)
    x16 = torch.full((M, D), float("nan"), dtype=torch.bfloat16, device=DEV)
    part = torch.full(((D + 255) // 256, M, 2), float("nan"), device=DEV)
    ops.gemm(a.to(DEV), w0.to(DEV), b0.to(DEV), x, PV_EPI_BIAS_RES_F32, res=res.to(DEV), x16_out=x16, rowstat_out=part)
    xr = (a.double() @ w0.double().t() + b0.double() + res.double())
    assert rel_l2(x.cpu(), xr) < 2e-6 and torch.equal(x16.cpu(), x.cpu().to(torch.bfloat16))
    stat = ops.rowstat_finalize(part, D, 1e-5).cpu().double()
    assert rel_l2(stat[:, 0], xr.mean(1)) < 1e-5 and rel_l2(stat[:, 1], (xr.var(1, unbiased=False) + 1e-5).rsqrt()) < 1e-5
    # consumer
    gamma, beta = T(f"fg{D}", (D,), "uniform", 0.3, 1.0, bf16=False), T(f"fbeta{D}", (D,), "uniform", 0.1, bf16=False)
    w, b = T(f"fw2{N}{D}", (N, D), "uniform", D ** -0.5, bf16=False), T(f"fb2{N}", (N,), "uniform", 0.1, bf16=False)
    wg = (w * gamma).to(torch.bfloat16)
    c1, c2 = wg.float().sum(1), (w @ beta + b)
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    st_dev = ops.rowstat_finalize(part, D, 1e-5)
    ops.gemm(x16, wg.to(DEV), None, out, epi, fold=(st_dev, c1.to(DEV).contiguous(), c2.to(DEV).contiguous()))
    x16d = x16.cpu().double()
    exact = stat[:, 1:2] * (x16d @ wg.double().t() - stat[:, 0:1] * c1.double()) + c2.double()
    ln_lin = torch.nn.functional.layer_norm(xr, (D,), gamma.double(), beta.double(), 1e-5) @ w.double().t() + b.double()
    if epi == 1:
        exact, ln_lin = torch.nn.functional.gelu(exact), torch.nn.functional.gelu(ln_lin)
    assert rel_l2(out.float().cpu(), exact) < 3e-3            # 16-bit output rounding
    assert rel_l2(out.float().cpu(), ln_lin) < 8e-3           # + operand rounding of the raw (un-normalised) row copy


def test_attention_at_the_headline_batch_is_finite_deterministic_and_close_to_fp64(ops):
    """The LDS-resident kernel at BASELINE's size (2048 x 12 heads, S = 197, fp16 operands, wide scores): every output finite, every
    relaunch bit-identical, a sample within fp16 rounding of fp64 softmax(q k^T) v.  (Round 3 screen: a build whose score guard carried a
    running maximum through the query-tile loop produced non-finite rows in 0.4 % of the (image, head, tile) triples - invisible to small
    shapes and to a 4-image error sample; profiles/r03_attention_ab.json.)"""
    from peekvit_amd import engine
    B, S, H, dh = 2048, 197, 12, 64
    g = torch.Generator(device=DEV).manual_seed(3)
    with engine.precision("f16"):
        qkv = (torch.randn(B, S, 3 * H * dh, generator=g, device=DEV) * 0.7).to(torch.float16)
        out = torch.empty(B, S, H * dh, dtype=torch.float16, device=DEV)
        ops.attention(qkv, out, B, S, H, dh)
        first = out.clone()
        assert bool(torch.isfinite(first).all())
        for _ in range(4):
            out.zero_()
            ops.attention(qkv, out, B, S, H, dh)
            assert torch.equal(out, first)
    idx = [0, 777, 2047]
    q, k, v = (qkv[idx].double().view(3, S, 3, H, dh).permute(2, 0, 3, 1, 4)[i] for i in range(3))
    ref = (torch.softmax(q @ k.transpose(-1, -2), -1) @ v).permute(0, 2, 1, 3).reshape(3, S, H * dh)
    assert rel_l2(first[idx].double().cpu(), ref.cpu()) < 4e-4


def test_attention_streaming_kernel_fp16_keeps_small_probabilities(ops):
    """Round 3 ADVICE: the LDS-resident kernel packs its probabilities as p * 2^k in the fp16 build (the fp16 MFMA flushes subnormal
    operands: up to 0.7 % of a row's mass vanished from P.V while still counted in l), the streaming kernel (S > 416, wide heads) did
    not.  Both do now (2^10): fp16 operands, scores spread over ~17 units, S = 577 and a 128-wide head (both streamed) against fp64, at the
    bound the resident kernel is held to at the headline batch."""
    from peekvit_amd import engine
    g = torch.Generator(device=DEV).manual_seed(11)
    for (B, S, H, dh) in [(2, 577, 4, 64), (1, 300, 2, 128)]:
        with engine.precision("f16"):
            qkv = torch.randn(B, S, 3 * H * dh, generator=g, device=DEV)
            qkv[..., :H * dh] *= 2.2 * dh ** -0.5          # scores ~ N(0, 2.2^2): row spread ~ 17 units
            qkv = qkv.to(torch.float16)
            out = torch.full((B, S, H * dh), float("nan"), dtype=torch.float16, device=DEV)
            ops.attention(qkv, out, B, S, H, dh)
        q, k, v = (qkv.double().view(B, S, 3, H, dh).permute(2, 0, 3, 1, 4)[i] for i in range(3))
        ref = (torch.softmax(q @ k.transpose(-1, -2), -1) @ v).permute(0, 2, 1, 3).reshape(B, S, H * dh)
        assert bool(torch.isfinite(out).all())
        assert rel_l2(out.double().cpu(), ref.cpu()) < 4e-4


@pytest.mark.parametrize("M,N,K,tile", [(2560, 3072, 768, 128), (2560, 3072 + 64, 768, 128), (16384, 3072, 768, 256), (8192, 3072, 768, 256)])
def test_gemm_gelu_is_elementwise_exact_on_both_tile_kernels(ops, M, N, K, tile):
    """Round 3 ADVICE / round 4 finding: the GELU epilogue ELEMENT BY ELEMENT against fp64 gelu(A W^T + b) at the fc1 shape, three launches
    each - a norm cannot see a polynomial that is wrong for one value in 1e5 (the 128^2 kernel's packed form with an op_sel bit was:
    DESIGN.md section 11, tests/test_isa_audit.py).  2560 rows take the 128^2 kernel (table gathered from global memory; N = 3136 its
    ragged column tile), the others the 256^2 kernel (table in LDS; 16384 rows = the prefetching persistent launch, 8192 = one tile per workgroup).  16-bit operands are exact in the reference, so what
    is left is fp32 accumulation order, the table's 8e-7 and the 16-bit output rounding (2^-9 relative)."""
    from peekvit_amd._lib import PV_EPI_BIAS_GELU_BF16
    assert ops.gemm_tile_rows(M, N, K, PV_EPI_BIAS_GELU_BF16) == tile
    g = torch.Generator(device=DEV).manual_seed(M + N)
    a = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
    w = ((torch.rand(N, K, generator=g, device=DEV) * 2 - 1) / math.sqrt(K) * 3).to(torch.bfloat16)      # pre-activations ~ N(0, 3): every table interval
    bias = (torch.rand(N, generator=g, device=DEV) * 2 - 1) * 0.1
    ref = torch.nn.functional.gelu(a.double() @ w.double().t() + bias.double())
    for _ in range(3):
        out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
        ops.gemm(a, w, bias, out, PV_EPI_BIAS_GELU_BF16)
        err = (out.double() - ref).abs()
        bad = err > 0.006 * ref.abs() + 2e-5
        assert int(bad.sum()) == 0, f"{int(bad.sum())} of {M * N} elements off: worst {float(err.max()):.3e}"


@pytest.mark.parametrize("B,S,H,dh,amp", [(2, 197, 12, 64, 1.0), (3, 197, 4, 64, 6.0), (2, 50, 3, 64, 10.0), (2, 99, 8, 32, 6.0), (1, 26, 2, 48, 8.0), (2, 5, 2, 64, 4.0)])
def test_attention_split_scores(B, S, H, dh, amp):
    """pv_attention_split_bf16 (the LOCAL fallback of the score guard): fp32 q|k|v in, scores from split operands.  Against fp64 softmax(q k^T) v
    on the same fp32 inputs with scores up to several hundred (`amp` scales q and k): the split kernel stays at the 16-bit rounding of p and v
    (~3e-4), while the ordinary fp16-operand kernel on the rounded q, k loses accuracy with the score (the reason for the guard)."""
    from peekvit_amd import _lib, ops
    D = H * dh
    g = torch.Generator(device="cuda").manual_seed(S * 7 + dh)
    qkv = torch.randn(B, S, 3 * D, generator=g, device="cuda")
    qkv[..., :2 * D] *= amp
    qkv[..., :D] *= dh ** -0.5                                     # (q arrives pre-scaled)
    q, k, v = (t.reshape(B, S, H, dh).permute(0, 2, 1, 3).double() for t in qkv.split(D, dim=-1))
    scores = q @ k.transpose(-1, -2)
    ref = (torch.softmax(scores, -1) @ v).permute(0, 2, 1, 3).reshape(B * S, D)
    old = _lib.set_operand("f16")
    try:
        out = torch.empty(B * S, D, device="cuda", dtype=torch.float16)
        ops.attention_split(qkv.view(B * S, 3 * D), out, B, S, H, dh)
        plain = torch.empty_like(out)
        ops.attention(qkv.view(B * S, 3 * D).half(), plain, B, S, H, dh)
    finally:
        _lib.set_operand(old)
    e_split, e_plain = rel_l2(out, ref), rel_l2(plain, ref)
    print(f"max |score| {float(scores.abs().max()):.0f}: split {e_split:.2e}, plain fp16 {e_plain:.2e}")
    assert torch.isfinite(out).all() and e_split < 4e-4, e_split
    if float(scores.abs().max()) > 100:
        assert torch.isfinite(plain).all() and e_plain > 2 * e_split
    # the bf16 library's build of the same kernel (bf16 halves: 16 mantissa bits in the scores) is held to bf16's output rounding
    outb = torch.empty(B * S, D, device="cuda", dtype=torch.bfloat16)
    ops.attention_split(qkv.view(B * S, 3 * D), outb, B, S, H, dh)
    assert rel_l2(outb, ref) < 6e-3


@pytest.mark.parametrize("B,S,H,dh", [(2, 99, 8, 32), (2, 80, 4, 64), (2, 48, 4, 48), (2, 96, 4, 48), (1, 272, 2, 64), (2, 197, 8, 32), (2, 197, 12, 64)])
@pytest.mark.parametrize("operand", ["f16", "bf16"])
def test_attention_row_maximum_is_taken_from_finished_scores(B, S, H, dh, operand):
    """Round 5 regression (tests/test_isa_audit.py has the static form): pv_attn_kernel's inline-asm row maxima ran 0 - 2 instructions behind the
    MFMAs that write the scores in 16 instantiations (these sequence lengths / head sizes among them), i.e. on stale registers; with scores
    spread over tens of units exp2(s - m) then overflowed the 16-bit probabilities: non-finite output rows (4 of 198 rows on N(0,1) scores, 70 at
    scores ~50: scripts/dbg/attn_nonfinite.py).  Every row must be finite and match fp64 softmax(q k^T) v on the same 16-bit inputs."""
    from peekvit_amd import _lib, ops
    D = H * dh
    dt = torch.float16 if operand == "f16" else torch.bfloat16
    for amp in (1.0, 6.0):
        g = torch.Generator(device="cuda").manual_seed(S + dh)
        qkv = torch.randn(B, S, 3 * D, generator=g, device="cuda")
        qkv[..., :2 * D] *= amp
        qkv[..., :D] *= dh ** -0.5
        q16 = qkv.view(B * S, 3 * D).to(dt)
        q, k, v = (t.reshape(B, S, H, dh).permute(0, 2, 1, 3).double() for t in q16.view(B, S, 3 * D).split(D, dim=-1))
        ref = (torch.softmax(q @ k.transpose(-1, -2), -1) @ v).permute(0, 2, 1, 3).reshape(B * S, D)
        old = _lib.set_operand(operand)
        try:
            out = torch.empty(B * S, D, device="cuda", dtype=dt)
            ops.attention(q16, out, B, S, H, dh)
        finally:
            _lib.set_operand(old)
        assert torch.isfinite(out.float()).all(), (amp, int((~torch.isfinite(out.float())).any(1).sum()))
        assert rel_l2(out, ref) < (2e-3 if operand == "f16" else 1.2e-2), (amp, rel_l2(out, ref))


@pytest.mark.parametrize("B,R,P,D,S,row_off", [(3, 224, 16, 384, 197, 1), (5, 160, 8, 256, 401, 1), (2, 224, 16, 512, 200, 4), (9, 64, 16, 128, 17, 1), (1, 32, 8, 64, 17, 1)])
def test_patch_embed_without_a_patch_matrix_is_bit_identical_to_im2col_plus_gemm(ops, B, R, P, D, S, row_off):
    """pv_patch_embed_f32 (round 6): the patch embedding with the patches gathered inside the GEMM's operand staging - same bits as pv_im2col_bf16 followed
    by pv_gemm_bf16(PV_EPI_BIAS_POS_F32), rows outside [row_off, row_off + Np) of every image untouched; ragged row and column tiles; P = 8 and 16."""
    from peekvit_amd import _lib
    from peekvit_amd._lib import PV_EPI_BIAS_POS_F32
    Np, K = (R // P) ** 2, 3 * P * P
    assert row_off + Np <= S
    x = T(f"pe_x{B}{R}", (B, 3, R, R), bf16=False).to(DEV)
    w = bf(T(f"pe_w{D}{K}", (D, K), "uniform", 1.0 / math.sqrt(K)))
    bias, pos = T(f"pe_b{D}", (D,), "uniform", 0.1, bf16=False).to(DEV), T(f"pe_p{S}{D}", (S, D), "uniform", 0.02, bf16=False).to(DEV)
    cols = torch.empty((B * Np, K), dtype=_lib.operand_dtype(), device=DEV)
    ops.im2col(x, P, cols)
    want = torch.full((B, S, D), 7.0, device=DEV)
    ops.gemm(cols, w, bias, want.view(B * S, D), PV_EPI_BIAS_POS_F32, M=B * Np, pos=pos, rows_per_img_in=Np, rows_per_img_out=S, row_off=row_off)
    got = torch.full((B, S, D), 7.0, device=DEV)
    ops.patch_embed(x, w, bias, pos, got, P, row_off)
    assert torch.equal(got, want)
    ref = (torch.nn.functional.unfold(x.to(w.dtype).float(), P, stride=P).transpose(1, 2) @ w.float().t() + bias + pos[row_off:row_off + Np])
    assert rel_l2(got[:, row_off:row_off + Np], ref) < 2e-5
    # without a bias
    got2, want2 = torch.zeros((B, S, D), device=DEV), torch.zeros((B, S, D), device=DEV)
    ops.gemm(cols, w, None, want2.view(B * S, D), PV_EPI_BIAS_POS_F32, M=B * Np, pos=pos, rows_per_img_in=Np, rows_per_img_out=S, row_off=row_off)
    ops.patch_embed(x, w, None, pos, got2, P, row_off)
    assert torch.equal(got2, want2)
