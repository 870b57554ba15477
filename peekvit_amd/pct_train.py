"""Training path of the point-cloud stem's pair stage (ARPE: k-NN -> lin1 -> bn1 -> ELU -> max over the neighbours) on the kernels of
include/peekvit_hip_pct_train.h, as one autograd function: points [B, N, 3] -> y [B, N, 6].  DESIGN.md section 20 derives the arithmetic.

Pairs are p = (b, q, j), j one of the k nearest neighbours of q; M = B N k; f_p = [x_q, x_q - x_j]; z_p = W1 f_p + b1.  BatchNorm 1 is
y = s z + t per channel with s = gamma / sigma, t = beta - mu s, sigma = sqrt(v + eps); mu, v are the batch statistics of z over all pairs
(bn1 in train mode) or the running statistics (bn1 in eval mode: frozen).  ELU is monotone and BatchNorm affine, so the max over the
neighbours moves in front of both: y = elu(s z* + t), z* the z of the neighbour that maximises sign(s) z.

Batch statistics of z are a function of the weights and of 27 moments of the pair features, F = sum f and G = sum f f^T, which do not depend
on the weights: mu = W1 F / M + b1, v = diag(W1 cov(f) W1^T).  The backward needs three sums over the B N query points (A = sum g',
Z = sum g' z*, C = sum g' f*, with g' = dL/dy * elu'(y)) and, for batch statistics, F and X = sum_p zhat_p f_p = (W1 G + (b1 - mu) F) / sigma.
So the function saves the points, y, the winning neighbour of every (query, channel) and a handful of 6-vectors and 6 x 6 matrices - about 36
bytes a point, nothing that scales with k.

The kernels leave every sum over the batch as one fp32 partial row per 64 query points; the rows are added in fp64 in a fixed order
(`.double().sum(0)`), and everything that is a 6-vector or a 6 x 6 matrix is fp64 on the device: no atomics, two runs give identical bits.
"""
from __future__ import annotations

import contextlib
import math
import os

import torch
from torch.autograd.function import once_differentiable

from . import _lib, engine, ops
from ._lib import PV_EPI_BIAS_BF16, PV_EPI_BIAS_GELU_PAIR_BF16, PV_EPI_BIAS_RES_F32
from .engine import _f32, bf16_weight, workspace
from .train_engine import BLOCK_PARAMS, attn_backward, block_params, mlp_backward

ARPE_MIN_N, ARPE_MAX_N = 16, 4096          # include/peekvit_hip_pct.h PV_ARPE_MIN_N / PV_ARPE_MAX_N

# forwards / backwards of the pair stage that ran on the kernels (tests and scripts/bench_pct_train.py read them to see which path ran)
stem_passes = 0
stem_backwards = 0
# ... and of the encoder's attention core on the streaming kernels (StreamAttention; off unless a model's set_fused_attention switched it on)
attn_passes = 0
attn_backwards = 0

_TRIU = {}


def _triu(dev):
    iu = _TRIU.get(dev)
    if iu is None:
        iu = _TRIU[dev] = torch.triu_indices(6, 6, device=dev)
    return iu


def finalize_moments(partial: torch.Tensor, shift: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, M: int):
    """Batch statistics of z from the partial moment rows of ops.arpe_pair_moments, in fp64: (mu [6], v [6] biased, F [6], XS [6, 6]) with
    F = sum f about the ORIGIN and XS = W1 G' + (b1' - mu) F' = sigma * sum_p zhat_p f_p, where the primed quantities are taken about `shift`
    (b1' = b1 + W1[:, :3] shift).  A covariance does not depend on the point about which its moments are taken, and sum zhat = 0, so the shift
    drops out of v and XS exactly; it is added back to F."""
    S = partial.double().sum(0)
    Fp = S[:6]
    iu = _triu(partial.device)
    U = torch.zeros((6, 6), dtype=torch.float64, device=partial.device)
    U[iu[0], iu[1]] = S[6:27]
    Gp = U + U.T - torch.diag(torch.diagonal(U))
    W = w1.double()
    c6 = torch.cat([shift.double(), torch.zeros(3, dtype=torch.float64, device=partial.device)])
    bp = b1.double() + W @ c6
    mf = Fp / M
    cov = Gp / M - torch.outer(mf, mf)
    mu = W @ mf + bp
    v = ((W @ cov) * W).sum(1).clamp_min(0.0)
    XS = W @ Gp + torch.outer(bp - mu, Fp)
    return mu, v, Fp + M * c6, XS


class PairStage(torch.autograd.Function):
    """y = max over the neighbours of elu(bn1(lin1([x, x - neighbour]))).  Inputs: points, lin1.weight, lin1.bias, bn1.weight, bn1.bias; `bn`
    (the BatchNorm1d module: its mode chooses batch or running statistics, its running statistics are updated in train mode as
    nn.BatchNorm1d updates them) and k are not tensors.  The points get no gradient."""

    @staticmethod
    def forward(ctx, points, w1, b1, gamma, beta, bn, k):
        global stem_passes
        B, N, _ = points.shape
        M = B * N * k
        points = points.contiguous()
        w1c, b1c = w1.detach().contiguous(), b1.detach().contiguous()
        idx = ops.arpe_knn(points, k)                    # workspace: not saved
        batch_stats = bn.training
        if batch_stats:
            shift = points.mean(dim=(0, 1))
            mu, v, F, XS = finalize_moments(ops.arpe_pair_moments(points, idx, shift), shift, w1c, b1c, M)
            bn.num_batches_tracked += 1
            m = 1.0 / bn.num_batches_tracked.double() if bn.momentum is None else bn.momentum
            bn.running_mean.copy_((1.0 - m) * bn.running_mean.double() + m * mu)                           # (fp64, rounded once)
            bn.running_var.copy_((1.0 - m) * bn.running_var.double() + m * v * (M / (M - 1.0)))
        else:
            mu, v = bn.running_mean.double(), bn.running_var.double()
        sigma = torch.sqrt(v + bn.eps)
        s = gamma.detach().double() / sigma
        # y = s (z* - mu) + beta with mu folded into the bias the kernel adds (the winner does not depend on a bias): s z* + (beta - mu s) would
        # cancel in fp32 wherever |mu| is large against sigma
        y, arg = ops.arpe_pair_max(points, idx, w1c, (b1c.double() - mu).float(), s.float(), beta.detach().float().contiguous())
        stats = torch.stack([mu, sigma, s] + ([F] if batch_stats else []))              # fp64 [3 or 4, 6]
        ctx.save_for_backward(points, y, arg, w1c, b1c, stats, XS / sigma[:, None] if batch_stats else stats.new_empty(0))
        ctx.batch_stats, ctx.M = batch_stats, M
        stem_passes += 1
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        global stem_backwards
        points, y, arg, w1, b1, stats, X = ctx.saved_tensors
        P = ops.arpe_pair_bwd(points, arg, y, g.contiguous(), w1, b1).double().sum(0)
        A, Z, Cm = P[:6], P[6:12], P[12:].view(6, 6)
        mu, sigma, s = stats[0], stats[1], stats[2]
        dgamma = (Z - mu * A) / sigma
        if ctx.batch_stats:
            m1, m2 = A / ctx.M, dgamma / ctx.M
            dw = s[:, None] * (Cm - m1[:, None] * stats[3][None, :] - m2[:, None] * X)
            db = torch.zeros_like(A)                  # BatchNorm removes the bias: the gradient is 0 exactly
        else:
            dw, db = s[:, None] * Cm, s * A
        need = ctx.needs_input_grad
        stem_backwards += 1
        return (None, dw.float() if need[1] else None, db.float() if need[2] else None, dgamma.float() if need[3] else None,
                A.float() if need[4] else None, None, None)


def eligible(arpe, x: torch.Tensor) -> bool:
    """Whether ARPE.forward runs its pair stage on the kernels: an fp32 GPU tensor that does not require grad, under autograd, without
    autocast, a 6 -> 6 lin1, an affine bn1 with running statistics, fp32 parameters, N and k within the kernels' limits, and the training
    knobs of train_engine.train_eligible (read per call)."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.numel() > 0 and x.dim() == 3 and x.shape[2] == 3):
        return False
    if not torch.is_grad_enabled() or x.requires_grad or torch.is_autocast_enabled():
        return False
    if os.environ.get("PEEKVIT_AMD_BACKEND", "") == "torch" or os.environ.get("PEEKVIT_AMD_TRAIN", "hip") != "hip":
        return False
    lin, bn = arpe.lin1, arpe.bn1
    if tuple(lin.weight.shape) != (6, 6) or lin.bias is None or not bn.affine or not bn.track_running_stats or bn.running_mean is None:
        return False
    tensors = (lin.weight, lin.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)
    if any(t.dtype != torch.float32 or t.device != x.device for t in tensors):
        return False
    return ARPE_MIN_N <= x.shape[1] <= ARPE_MAX_N and 1 <= arpe.k <= x.shape[1]


def pair_stage(arpe, x: torch.Tensor) -> torch.Tensor:
    """The pair stage of `arpe` on x [B, N, 3] under autograd: y [B, N, 6].  The caller has checked `eligible`."""
    with torch.cuda.device(x.device):
        return PairStage.apply(x, arpe.lin1.weight, arpe.lin1.bias, arpe.bn1.weight, arpe.bn1.bias, arpe.bn1, arpe.k)


# ---- the encoder's attention core on the streaming kernels (include/peekvit_hip_attn_stream.h) ----------------------------
ATTN_HEAD_DIMS = (32, 48, 64)


def _grad_exponent(g: torch.Tensor) -> torch.Tensor:
    """Integer e with max|g| = m 2^e, m in [1/2, 1), clamped to [-126, 126]; 0 where the maximum is 0 or not finite.  On the device, no host read."""
    a = g.abs().amax()
    e = torch.frexp(a).exponent.clamp(-126, 126)
    return torch.where(torch.isfinite(a) & (a > 0), e, torch.zeros_like(e))


@contextlib.contextmanager
def _saved_operand(t16: torch.Tensor):
    """Autograd runs a backward on its own thread, where the precision mode is the default: the library is the one of the saved operands."""
    old = _lib.set_operand("f16" if t16.dtype == torch.float16 else "bf16")
    try:
        yield
    finally:
        _lib.set_operand(old)


class StreamAttention(torch.autograd.Function):
    """out = softmax(q k^T) v per head.  qkv fp32 [B, S, 3 D], packed q | k | v with q ALREADY scaled; H heads; out fp32 [B, S, D].  The operands
    are rounded to the 16-bit type of the current precision mode once; the forward saves those, its 16-bit output and the rows' log-sum-exp -
    B S (8 D + 4 H) bytes, nothing that scales with S^2.  The input is fp32 so that autograd hands the backward an fp32 gradient.

    The backward normalises the incoming gradient by a power of two c with max|g| c in [1/2, 1) (computed on the device, no host read; 1 where
    the maximum is 0 or not finite), rounds it to 16 bits, and multiplies the kernels' fp32 result by 1 / c: both factors are exact, so the
    result does not depend on the loss scale and the path needs no loss-scale state of its own."""

    @staticmethod
    def forward(ctx, qkv, H):
        global attn_passes
        B, S, D3 = qkv.shape
        D = D3 // 3
        dh = D // H
        dt = _lib.operand_dtype()
        q16 = qkv.detach().to(dt).contiguous()
        out = torch.empty((B, S, D), dtype=dt, device=qkv.device)
        lse = torch.empty((B, H, S), dtype=torch.float32, device=qkv.device)
        ops.attention_stream(q16, out, lse, B, S, H, dh)
        ctx.save_for_backward(q16, out, lse)
        ctx.H = H
        attn_passes += 1
        return out.float()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        global attn_backwards
        q16, out, lse = ctx.saved_tensors
        B, S, D = out.shape
        H = ctx.H
        e = _grad_exponent(g)
        one = torch.ones_like(e, dtype=g.dtype)
        dout = (g * torch.ldexp(one, -e)).to(q16.dtype).contiguous()
        dqkv = torch.empty((B, S, 3 * D), dtype=torch.float32, device=g.device)
        with _saved_operand(q16):
            ops.attention_stream_bwd(q16, dout, out, lse, dqkv, B, S, H, D // H, 1.0)       # qscale = 1: the input is the scaled q
        attn_backwards += 1
        return dqkv.mul_(torch.ldexp(one, e)), None


_QSCALE = {}


def _qscale_row(dev, D: int, dh: int) -> torch.Tensor:
    """fp32 [3 D]: dh^-0.5 over the q third, 1 over k | v."""
    v = _QSCALE.get((dev, D, dh))
    if v is None:
        v = torch.ones(3 * D, dtype=torch.float32, device=dev)
        v[:D] = dh ** -0.5
        _QSCALE[(dev, D, dh)] = v
    return v


def attention_eligible(block, x: torch.Tensor) -> bool:
    """Whether a PCT block runs its attention core in StreamAttention: the block's `fused_attention` switch is on (set_fused_attention: off by
    default - a 16-bit attention core is not the stock fp32 ops' arithmetic), an fp32 GPU tensor [B, S, D] under autograd without autocast, the
    training knobs of `eligible` (read per call), a precision mode with 16-bit operands, dh in 32 / 48 / 64, an fp32 nn.MultiheadAttention with a
    packed in-projection and biases, and no active attention dropout."""
    return bool(getattr(block, "fused_attention", False)) and _attention_conditions(block, x)


def _attention_conditions(block, x: torch.Tensor) -> bool:
    """Everything attention_eligible asks for but the switch (block_eligible asks for the same, behind its own switch)."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.numel() > 0):
        return False
    if not torch.is_grad_enabled() or torch.is_autocast_enabled():
        return False
    if os.environ.get("PEEKVIT_AMD_BACKEND", "") == "torch" or os.environ.get("PEEKVIT_AMD_TRAIN", "hip") != "hip":
        return False
    if engine._mode() == "bf16x3":
        return False
    mha = block.self_attention.self_attention
    D, H = x.shape[2], mha.num_heads
    if mha.embed_dim != D or D % H or D // H not in ATTN_HEAD_DIMS:
        return False
    if not mha._qkv_same_embed_dim or mha.in_proj_weight is None or mha.in_proj_bias is None or mha.out_proj.bias is None:
        return False
    if mha.bias_k is not None or mha.bias_v is not None or mha.add_zero_attn or not mha.batch_first:
        return False
    if any(t.dtype != torch.float32 or t.device != x.device for t in (mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias)):
        return False
    return mha.dropout == 0.0 or not mha.training


def attention(mha, x: torch.Tensor) -> torch.Tensor:
    """nn.MultiheadAttention(x, x, x) without weights on x fp32 [B, S, D] under autograd: the projections are stock ops, the core is
    StreamAttention.  The caller has checked `attention_eligible`."""
    D, H = x.shape[2], mha.num_heads
    with torch.cuda.device(x.device):
        qkv = torch.nn.functional.linear(x, mha.in_proj_weight, mha.in_proj_bias) * _qscale_row(x.device, D, D // H)
        out = StreamAttention.apply(qkv, H)
    return torch.nn.functional.linear(out, mha.out_proj.weight, mha.out_proj.bias)


# ---- a whole encoder block on the training kernels (include/peekvit_hip_pct_block.h) --------------------------------------
# forwards / backwards of PCTBlockFn (off unless a model's set_fused_blocks switched it on)
block_passes = 0
block_backwards = 0


def _pow2(e: torch.Tensor) -> torch.Tensor:
    """fp32 2^e for an integer tensor e in [-126, 126], built from its bits: exact for every e (a device pow need not be)."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def block_saved_bytes_per_row(D: int, H: int, Mh: int) -> int:
    """Bytes PCTBlockFn keeps per row of x for its backward: x and v in fp32 (8 D), u, att, w in 16 bits (6 D), qkv (6 D), the GELU pair (4 Mh) and the
    rows' log-sum-exp (4 H)."""
    return 20 * D + 4 * Mh + 4 * H


class PCTBlockFn(torch.autograd.Function):
    """One PCTBlock - u = ln_1(x), v = attn(u) + u, out = mlp(ln_2(v)) + v - forward and backward on the kernels.  x fp32 [B, S, D]; the
    parameters are arguments so that autograd routes their gradients, the kernels read them through the block.  16-bit operands of the current
    precision mode, fp32 residual stream.  Saved: x, u16, qkv16, att16, lse, v32, w16 = ln_2(v) and the GELU pair (block_saved_bytes_per_row): no
    fp32 copy of u or w, nothing of size S^2.

    The backward calls the stage functions train_engine's block functions call (mlp_backward, attn_backward) between LayerNorm backwards of its own.
    The FIRST residual is LayerNorm 1's OUTPUT, so its gradient does not bypass that LayerNorm: it is the fp32 term of the LayerNorm's own dy
    (ops.layernorm_bwd_sum), the 16-bit term being the data gradient of the in-projection.  (The second residual is v, LayerNorm 2's INPUT: there the
    residual gradient bypasses the LayerNorm as in a pre-LN block - ops.layernorm_bwd with dres_in.)  The attention backward handed to attn_backward is
    the streaming one with a 16-bit dqkv and the bias partial rows (ops.attention_stream_bwd16).

    fp16 range: the incoming gradient is multiplied by the power of two c with max|dout| c in [1/2, 1) (on the device, no host read; 1 for a zero
    or non-finite maximum) and every returned gradient by 1 / c - both exact, so the result does not depend on a loss scale and the function
    carries no loss-scale state."""

    @staticmethod
    def forward(ctx, blk, x, ln1w, ln1b, inw, inb, ow, ob, ln2w, ln2b, w1, b1, w2, b2):
        global block_passes
        x = x.detach()
        x = x if x.is_contiguous() else x.contiguous()
        out, saved, ctx.dims = PCTBlockFn._fw(blk, x, ln1w, ln1b, inb, ob, ln2w, ln2b, b1, b2)
        ctx.blk = blk
        ctx.save_for_backward(*saved)
        block_passes += 1
        return out

    @staticmethod
    def _fw(blk, x, ln1w, ln1b, inb, ob, ln2w, ln2b, b1, b2, row_scale=None, tail_log_mult=0.0):
        """The forward's launches on x fp32 [B, S, D] contiguous: (out, the saved tensors, dims).  row_scale (fp32 [B * S], RankedPCTBlockFn's compact rows)
        multiplies both LayerNorm outputs per row and tail_log_mult goes on the score of key S - 1; without it the launches are PCTBlockFn's own."""
        B, S, D = x.shape
        mha, mlp = blk.self_attention.self_attention, blk.mlp
        H = mha.num_heads
        dh, Mh, R, dev, dt = D // H, mlp.fc1.out_features, B * S, x.device, _lib.operand_dtype()
        qscale = float(dh) ** -0.5
        u16 = torch.empty((R, D), dtype=dt, device=dev)
        qkv = torch.empty((R, 3 * D), dtype=dt, device=dev)
        att = torch.empty((R, D), dtype=dt, device=dev)
        lse = torch.empty((B, H, S), dtype=torch.float32, device=dev)
        v32 = torch.empty((R, D), dtype=torch.float32, device=dev)
        w16 = torch.empty((R, D), dtype=dt, device=dev)
        pair = torch.empty((R, 2 * Mh), dtype=dt, device=dev)            # [gelu(pre) | gelu'(pre)]
        out = torch.empty((B, S, D), dtype=torch.float32, device=dev)
        u32 = workspace.get("pb_u32", (R, D), torch.float32, dev)        # u in fp32: the residual term of the out-projection, not kept
        with engine.no_param_checks():
            if row_scale is None:
                ops.layernorm_f32_bf16(x.view(R, D), _f32(ln1w), _f32(ln1b), blk.ln_1.eps, u16, u32)
            else:
                ops.layernorm_f32_bf16_masked(x.view(R, D), _f32(ln1w), _f32(ln1b), row_scale, blk.ln_1.eps, u16, u32)
            ops.gemm(u16, bf16_weight(mha.in_proj_weight), _f32(inb), qkv, PV_EPI_BIAS_BF16, M=R, qcols=D, qscale=qscale)
            if row_scale is None:
                ops.attention_stream(qkv, att, lse, B, S, H, dh)
            else:
                ops.attention_stream_w(qkv, att, lse, B, S, H, dh, tail_log_mult)
            ops.gemm(att, bf16_weight(mha.out_proj.weight), _f32(ob), v32, PV_EPI_BIAS_RES_F32, M=R, res=u32)
            ops.layernorm_bf16(v32, _f32(ln2w), _f32(ln2b), blk.ln_2.eps, w16, row_scale=row_scale)
            ops.gemm(w16, bf16_weight(mlp.fc1.weight), _f32(b1), pair, PV_EPI_BIAS_GELU_PAIR_BF16, M=R)
            ops.gemm(pair[:, :Mh], bf16_weight(mlp.fc2.weight), _f32(b2), out.view(R, D), PV_EPI_BIAS_RES_F32, M=R, res=v32)
        return out, (x, u16, qkv, att, lse, v32, w16, pair), (B, S, D, H, dh, Mh, qscale)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        u16 = ctx.saved_tensors[1]
        with _saved_operand(u16), torch.cuda.device(u16.device), engine.no_param_checks():
            return PCTBlockFn._bw(ctx, g)

    @staticmethod
    def _bw(ctx, g):
        global block_backwards
        need = dict(zip(BLOCK_PARAMS, ctx.needs_input_grad[2:14]))
        g = g.float() if g.dtype != torch.float32 else g
        g = g if g.is_contiguous() else g.contiguous()
        dx, grads = PCTBlockFn._bw_core(ctx.blk, ctx.saved_tensors[:8], ctx.dims, need, g)
        block_backwards += 1
        return (None, dx if ctx.needs_input_grad[1] else None) + grads

    @staticmethod
    def _bw_core(blk, saved, dims, need, g, row_scale=None, tail_log_mult=0.0):
        """The backward's launches for g fp32 [B, S, D] contiguous: (dx, the twelve parameter gradients in BLOCK_PARAMS' order, None where not needed).
        row_scale / tail_log_mult as in _fw (the masked LayerNorm backwards and the weighted attention backward); without them PCTBlockFn's own launches."""
        ws = workspace
        x, u16, qkv, att, lse, v32, w16, pair = saved
        B, S, D, H, dh, Mh, qscale = dims
        R, dev, dt = B * S, x.device, u16.dtype
        g = g.view(R, D)
        # ---- the exact normalisation: everything below works on c * dout (scratch pb_*: never shared with train_engine's bw_*) -----------------------
        e = _grad_exponent(g)
        gs = torch.mul(g, _pow2(-e), out=ws.get("pb_g", (R, D), torch.float32, dev))
        # ---- MLP branch: out = fc2(gelu(fc1(w))) + v, w = ln_2(v) -------------------------------------------
        d2 = ops.cast_bf16(gs, ws.get("pb_d2", (R, D), dt, dev))
        dpre, dhid = ws.get("pb_dpre", (R, Mh), dt, dev), ws.get("pb_dh", (R, D), dt, dev)
        # (db2_always off: a gradient nobody needs is returned as None here, so fc2's bias sums are taken only where b2 needs them)
        dw2, db2, dw1, db1 = mlp_backward(blk, d2, pair, w16, need, dpre, dhid, db2_always=False)
        # v feeds ln_2 AND the second residual: dv = dout + LN2'(v)^T dhid
        dv = ws.get("pb_dv", (R, D), torch.float32, dev)
        d1 = ws.get("pb_d1", (R, D), dt, dev)
        dgb2 = torch.empty((3, D), dtype=torch.float32, device=dev)
        if row_scale is None:
            ops.layernorm_bwd(v32, dhid, _f32(blk.ln_2.weight), gs, dv, dgb2, blk.ln_2.eps, dx_bf16=d1)
        else:          # w = row_scale * ln_2(v): dy times row_scale (the per-row dmask it also forms is not a gradient anyone asks for)
            ops.layernorm_bwd_masked(v32, dhid, _f32(blk.ln_2.weight), _f32(blk.ln_2.bias), row_scale, gs, None, dv, d1, False, dgb2,
                                     ws.get("pb_dmask", (R,), torch.float32, dev), False, blk.ln_2.eps)
        # ---- attention branch: v = out_proj(attn(in_proj(u))) + u -------------------------------------------
        datt, dqkv = ws.get("pb_datt", (R, D), dt, dev), ws.get("pb_dqkv", (R, 3 * D), dt, dev)
        dbp = ws.get("pb_dbp", (B * ((S + 63) // 64), 3 * D), torch.float32, dev) if need["inb"] else None          # one row per 64 query rows
        if row_scale is None:
            def attention_bwd(datt, dqkv, dbp):
                ops.attention_stream_bwd16(qkv, datt, att, lse, dqkv, B, S, H, dh, qscale, dbias_partial=dbp)
        else:
            def attention_bwd(datt, dqkv, dbp):
                ops.attention_stream_bwd16_w(qkv, datt, att, lse, dqkv, B, S, H, dh, qscale, tail_log_mult, dbias_partial=dbp)
        dwo, dwin, dbin = attn_backward(blk, d1, att, u16, need, datt, dqkv, dhid, dbp, attention_bwd)
        # u = ln_1(x) feeds the in-projection AND the first residual: du = dv + dhid, formed in fp32 inside the kernel and never rounded
        dx = torch.empty((B, S, D), dtype=torch.float32, device=dev)
        dgb1 = torch.empty((3, D), dtype=torch.float32, device=dev)
        if row_scale is None:
            ops.layernorm_bwd_sum(x.view(R, D), dhid, dv, _f32(blk.ln_1.weight), dx.view(R, D), None, dgb1, blk.ln_1.eps)
        else:
            ops.layernorm_bwd_sum_masked(x.view(R, D), dhid, dv, _f32(blk.ln_1.weight), row_scale, dx.view(R, D), None, dgb1, blk.ln_1.eps)
        # ---- the gradients leave the normalised chain (dgb2[2] = the column sums of d1 = the out-projection's bias gradient) -----------------------
        torch._foreach_mul_([t for t in (dx, dgb1, dgb2, dwin, dbin, dwo, dw1, db1, dw2, db2) if t is not None], _pow2(e))
        grads = (dgb1[0], dgb1[1], dwin, dbin, dwo, dgb2[2], dgb2[0], dgb2[1], dw1, db1, dw2, db2)
        return dx, tuple(t if need[n] else None for n, t in zip(BLOCK_PARAMS, grads))


def block_eligible(block, x: torch.Tensor) -> bool:
    """Whether a PCT block runs whole in PCTBlockFn: the block's `fused_block` switch is on (set_fused_blocks: off by default - 16-bit operands are
    not the stock fp32 ops' arithmetic), attention_eligible's conditions on x, the knobs and the attention module (read per call), D and the MLP width
    multiples of 64, D <= 1024, fp32 LayerNorms with affine parameters and fp32 MLP linears with biases on x's device, and - RankingPCTBlock - `sort`
    off: a sorting block zeroes rows after both LayerNorms in training and stays on the path it has without this switch."""
    if not getattr(block, "fused_block", False) or getattr(block, "sort", False):
        return False
    return _block_conditions(block, x)


def _block_conditions(block, x: torch.Tensor) -> bool:
    """Everything block_eligible asks for but its switch and `sort` (ranked_block_eligible asks for the same, behind its own switch)."""
    if not _attention_conditions(block, x):
        return False
    D = x.shape[2]
    ln1, ln2, fc1, fc2 = block.ln_1, block.ln_2, block.mlp.fc1, block.mlp.fc2
    if not all(isinstance(ln, torch.nn.LayerNorm) and tuple(ln.normalized_shape) == (D,) and ln.weight is not None and ln.bias is not None for ln in (ln1, ln2)):
        return False
    if not all(isinstance(fc, torch.nn.Linear) and fc.bias is not None for fc in (fc1, fc2)):
        return False
    Mh = fc1.out_features
    if fc1.in_features != D or fc2.in_features != Mh or fc2.out_features != D or D % 64 or Mh % 64 or D > 1024:
        return False
    tensors = (ln1.weight, ln1.bias, ln2.weight, ln2.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias)
    return not any(t.dtype != torch.float32 or t.device != x.device for t in tensors)


def block(blk, x: torch.Tensor) -> torch.Tensor:
    """`blk` on x fp32 [B, S, D] under autograd, whole, in PCTBlockFn.  The caller has checked `block_eligible`."""
    with torch.cuda.device(x.device):
        return PCTBlockFn.apply(blk, x, *block_params(blk))


# ---- a SORTING block in train mode on the same kernels, on its live rows only (include/peekvit_hip_rank_train.h) ----------------
# forwards / backwards of RankedPCTBlockFn (off unless a model's set_fused_ranking switched it on); block_passes / block_backwards do not count them
ranked_passes = 0
ranked_backwards = 0
RANK_MAX_N = 4096                          # rows 1.. of an image: pv_rank_topk's limit
_ROW_SCALE = {}


def _tail_row_scale(dev, B: int, Sc: int) -> torch.Tensor:
    """fp32 [B * Sc]: 1 on the live rows, 0 on the last (tail) row of every image."""
    v = _ROW_SCALE.get((dev, B, Sc))
    if v is None:
        v = torch.ones((B, Sc), dtype=torch.float32, device=dev)
        v[:, Sc - 1] = 0.0
        v = _ROW_SCALE[(dev, B, Sc)] = v.view(-1)
    return v


def ranked_keep(blk, S: int) -> int:
    """Rows 1.. a sorting block leaves unmasked in train mode: RankingPCTBlock.mask_tokens' ceil((S - 1) * budget), at most S - 1."""
    return min(S - 1, math.ceil((S - 1) * blk.current_budget))


class RankedPCTBlockFn(torch.autograd.Function):
    """A RankingPCTBlock with `sort` on, in train mode, whole: rows 1.. ranked by descending norm (ops.token_norm, ops.rank_topk: ties to the lowest
    index), all but the first `keep` zeroed at the input and after both LayerNorms.  The m = S - 1 - keep masked rows of an image are identical, so the
    block runs on L = 1 + keep live rows plus ONE tail row per image - x = 0, both LayerNorm outputs times 0, its key weighted by m (+ ln m on the score
    in fp32) - through PCTBlockFn's own launches (_fw / _bw_core: same rounding, block_saved_bytes_per_row bytes per COMPACT row, plus keep), and the
    tail row's output is written to rows L .. S - 1.  The output is the sorted sequence [B, S, D], as the composite returns it.

    Backward: the tail row's incoming gradient is the sum of dout over rows L .. S - 1 (ops.rank_reduce: fixed order, no atomics); everything after it is
    linear in that sum, so PCTBlockFn's backward on the compact rows - with its exact power-of-two normalisation taken of the REDUCED gradient - gives
    every parameter gradient, and dx is scattered back to the input's row order with zeros at the masked rows.  m = 0 (keep = S - 1): no tail row, no
    masks, no bias - PCTBlockFn applied to the gathered rows, bit for bit."""

    @staticmethod
    def forward(ctx, blk, x, ln1w, ln1b, inw, inb, ow, ob, ln2w, ln2b, w1, b1, w2, b2):
        global ranked_passes
        x = x.detach()
        x = x if x.is_contiguous() else x.contiguous()
        B, S, D = x.shape
        k = ranked_keep(blk, S)
        m = S - 1 - k
        keep = ops.rank_topk(ops.token_norm(x), k)                       # int32 [B, k], indices into rows 1..
        xc = ops.rank_pack(x, keep)                                       # [B, Sc, D], saved as the block's input
        Sc = xc.shape[1]
        row_scale = _tail_row_scale(x.device, B, Sc) if m else None
        tlm = math.log(m) if m else 0.0
        yc, saved, dims = PCTBlockFn._fw(blk, xc, ln1w, ln1b, inb, ob, ln2w, ln2b, b1, b2, row_scale, tlm)
        out = ops.rank_expand(yc, S) if m else yc
        ctx.blk, ctx.dims, ctx.rank = blk, dims, (S, k, m, tlm)
        ctx.save_for_backward(*saved, keep)
        blk.last_train_keep = torch.cat([keep.new_zeros((B, 1)), keep + 1], dim=1).to(torch.int64)
        ranked_passes += 1
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        global ranked_backwards
        u16 = ctx.saved_tensors[1]
        with _saved_operand(u16), torch.cuda.device(u16.device), engine.no_param_checks():
            keep = ctx.saved_tensors[8]
            S, k, m, tlm = ctx.rank
            B, Sc = ctx.dims[0], ctx.dims[1]
            need = dict(zip(BLOCK_PARAMS, ctx.needs_input_grad[2:14]))
            g = g.float() if g.dtype != torch.float32 else g
            g = g if g.is_contiguous() else g.contiguous()
            gc = ops.rank_reduce(g, k + 1, workspace.get("rb_gc", (B, Sc, g.shape[2]), torch.float32, g.device)) if m else g
            row_scale = _tail_row_scale(g.device, B, Sc) if m else None
            dxc, grads = PCTBlockFn._bw_core(ctx.blk, ctx.saved_tensors[:8], ctx.dims, need, gc, row_scale, tlm)
            dx = ops.rank_unpack_grad(dxc, keep, S) if ctx.needs_input_grad[1] else None
            ranked_backwards += 1
            return (None, dx) + grads


def ranked_block_eligible(block, x: torch.Tensor) -> bool:
    """Whether a RankingPCTBlock runs whole in RankedPCTBlockFn: `sort` and the block's `fused_ranking` switch on (set_fused_ranking: off by default, for
    the reason set_fused_blocks is), train mode (eval drops rows instead of masking them: the path it has), everything block_eligible asks of x, the
    knobs and the modules, 2 <= S with S - 1 <= RANK_MAX_N, and at least one row of rows 1.. kept."""
    if not (getattr(block, "sort", False) and getattr(block, "fused_ranking", False) and block.training and hasattr(block, "current_budget")):
        return False
    if not _block_conditions(block, x):
        return False
    S = x.shape[1]
    return 2 <= S and S - 1 <= RANK_MAX_N and ranked_keep(block, S) >= 1


def ranked_block(blk, x: torch.Tensor) -> torch.Tensor:
    """`blk` on x fp32 [B, S, D] under autograd, whole, in RankedPCTBlockFn.  The caller has checked `ranked_block_eligible`."""
    with torch.cuda.device(x.device):
        return RankedPCTBlockFn.apply(blk, x, *block_params(blk))
