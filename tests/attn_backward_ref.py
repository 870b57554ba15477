"""References for the attention backward kernels, in plain torch on whatever device the inputs live on (no GPU needed): fp64 autograd on the
same 16-bit values, the backward restated on stock fp32 ops with a kernel's rounding points, and a per-row error measure.

Layouts: qkv [B, S, 3 D] (q pre-scaled by qscale, as the forward stores it), dout [B, S, D], dqkv [B, S, 3 D] with the q third times qscale
(the gradient of the in-projection output BEFORE the pre-scale).  D = H dh.

Rounding points of the kernels, as read from their sources (csrc = peekvit_amd/csrc).  `P` is the fp32 softmax, dP = dO V^T,
dS = P o (dP - delta), "16" = rounded to the operand type (bf16 or fp16):

  kernel (entry point)                                      P for dV   dS for dQ / dK   result   delta_from
  pv_attn_bwd2_kernel  (pv_attention_bwd_bf16, 1 .. 13      16 *       16              16       "pdp"   pv_attention.hip:1418-1427 dd = sum fma(P, dP) in fp32,
                        tiles of 16 rows, dh 32 / 48 / 64)                                              :1437 and :1531 pack dS, :1530 packs P, :1459 / :1581 / :1585 pack the result
  pv_attn_bwd_kernel   (pv_attention_bwd_bf16, dh 32 at     16 *       16              16       "pdp"   pv_attention.hip:1086-1095 the same dd, :1104 and :1196 pack dS, :1195 packs P,
                        14 .. 26 tiles)                                                                 :1126 / :1242 / :1246 pack the result
  pv_attn_bwd5_kernel  (pv_attention_bwd_lse_bf16)          16 *       16              16       "out"   pv_attention.hip:1835-1847 D = rowsum(dO o O) of the forward's stored 16-bit
                                                                                                        output, p = exp2(s log2 e - lse) from the forward's fp32 lse; :1876 and :2018 pack dS,
                                                                                                        :2017 packs P, :1924 / :2082 / :2083 pack the result
  pv_attn_stream_dq / dkv_kernel (pv_attention_stream_bwd_bf16)   16 *   16            fp32     "out"   pv_attention_stream.hip:5 delta[q] = sum_d dO O of the stored output (the dQ
                                                                                                        kernel's prologue, left in delta_ws); :25-29 packed P and dS, fp32 results
  pv_attn_rows_bwd_kernel (pv_attention_rows_bwd_bf16)      fp32       fp32            16       "out"   pv_attention.hip:2386 delta = dout . out of the stored 16-bit output; no MFMA, p and
                                                                                                        ds stay fp32 (:2439-2440), :2445 / :2446 / :2467 pack the result (`restated_rows`)

  * fp16 build: P is packed as p 2^10 (PV_P_SHIFT, pv_attn.h:15-27) and the exact factor is taken out of dV where it is stored; `restated` does the same.
    dS is packed at its own magnitude.  In pass 1 of the three resident kernels and in the streaming dQ kernel the UNROUNDED fp32 P enters dS, in
    every kernel dS is formed in fp32 and rounded once.

The 16-bit output the "out" variants read is restated as the forward forms it: P rounded to the operand type (times 2^10 in the fp16 build), P V
accumulated in fp32, the row rounded once (pv_attn_kernel; the class-row forward keeps P in fp32, pv_attention.hip:2245)."""
import math

import torch

P_SHIFT_F16 = 10                        # pv_attn.h: PV_P_SHIFT of the fp16 build (0 in the bf16 build)
CAP = {"bf16": 1e-2, "f16": 1.5e-3}     # the project's whole-tensor bounds for 16-bit attention gradients (test_hip_backward.py)
DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16}
THIRDS = "qkv"


def heads(t, B, S, H, dh):
    return t.reshape(B, S, H, dh).permute(0, 2, 1, 3)


def rows(t, B, S, H, dh):
    return t.permute(0, 2, 1, 3).reshape(B, S, H * dh)


def randn16(*shape, seed=0, scale=1.0, device="cpu"):
    """The existing tests' `_bf`: Gaussian values rounded to bf16 (a CPU generator off the GPU: other values, the same distribution)."""
    g = torch.Generator(device=device).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=device) * scale).to(torch.bfloat16)


def inputs(B, S, H, dh, dt, family="gaussian", device="cpu", seed=None):
    """qkv [B, S, 3 D] and dout [B, S, D] in the operand type `dt`.  gaussian: `_bf(seed = S)` with q pre-scaled, dout = `_bf(seed = S + 1)` / 10 - what
    the existing attention-backward tests use.  peaked: the same with the q rows 0, 5, 10, ... times 12 before the rounding to the operand type: those
    rows put their probability on one key, as class and register tokens of a trained ViT do."""
    assert family in ("gaussian", "peaked")
    D = H * dh
    seed = S if seed is None else seed
    qkv = randn16(B, S, 3 * D, seed=seed, device=device).float()
    qkv[..., :D] *= dh ** -0.5
    if family == "peaked":
        qkv[:, 0::5, :D] *= 12.0
    return qkv.to(dt), randn16(B, S, D, seed=seed + 1, scale=0.1, device=device).to(dt)


def fp64(qkv, dout, B, S, H, dh, qscale):
    """fp64 autograd through softmax(q' k^T) v on the same 16-bit values: out [B, S, D], lse [B, H, S] (log2), dqkv [B, S, 3 D]."""
    D = H * dh
    t = qkv.double().reshape(B, S, 3, H, dh).permute(2, 0, 3, 1, 4).contiguous().requires_grad_(True)
    s = t[0] @ t[1].transpose(-1, -2)
    out = rows(torch.softmax(s, dim=-1) @ t[2], B, S, H, dh)
    (out * dout.double()).sum().backward()
    g = t.grad.clone()
    g[0] *= qscale
    return out.detach(), (torch.logsumexp(s, -1) / math.log(2.0)).detach(), g.permute(1, 3, 0, 2, 4).reshape(B, S, 3 * D)


def restated(qkv, dout, B, S, H, dh, qscale, delta_from, store16=True, p_shift=None):
    """The backward on stock fp32 ops with a kernel's rounding points (the table above): fp32 scores and softmax, P rounded to the operand type for dV
    (and for the forward's output), dS = P o (dP - delta) from the fp32 P rounded to the operand type for dQ and dK, the result rounded to the operand
    type when `store16`.  delta_from: "pdp" = rowsum(P o dP) in fp32, "out" = rowsum(dO o O) of the 16-bit output.  p_shift: P is rounded as
    P 2^p_shift (default: the build's PV_P_SHIFT for qkv's type; 0 = test_hip_attn_stream's original restatement, bit for bit).  fp32 [B, S, 3 D]."""
    assert delta_from in ("pdp", "out")
    dt, D = qkv.dtype, H * dh
    if p_shift is None:
        p_shift = P_SHIFT_F16 if dt == torch.float16 else 0
    q, k, v = (heads(t, B, S, H, dh) for t in qkv.float().split(D, dim=-1))
    do = heads(dout.float(), B, S, H, dh)
    P = torch.softmax(q @ k.transpose(-1, -2), dim=-1)
    P16 = P.to(dt).float() if p_shift == 0 else (P * 2.0 ** p_shift).to(dt).float() * 2.0 ** -p_shift
    dv = P16.transpose(-1, -2) @ do
    dP = do @ v.transpose(-1, -2)
    if delta_from == "out":
        o16 = (P16 @ v).to(dt).float()
        delta = (do * o16).sum(-1, keepdim=True)
    else:
        delta = (P * dP).sum(-1, keepdim=True)
    dS = (P * (dP - delta)).to(dt).float()
    dq, dk = (dS @ k) * qscale, dS.transpose(-1, -2) @ q
    g = torch.cat([rows(t, B, S, H, dh) for t in (dq, dk, dv)], dim=-1)
    return g.to(dt).float() if store16 else g


# ---- the class-row backward: one query row per image, q [B, D] (pre-scaled), kv [B S, 2 D] (k | v), dout [B, D] ----
def rows_inputs(B, S, H, dh, dt, peaked=False, device="cpu"):
    """test_attention_rows_backward's inputs; peaked: the one query row times 12 before the rounding."""
    D = H * dh
    q = randn16(B, D, seed=S, device=device).float() * dh ** -0.5 * (12.0 if peaked else 1.0)
    return q.to(dt), randn16(B * S, 2 * D, seed=S + 1, device=device).to(dt), randn16(B, D, seed=S + 2, scale=0.1, device=device).to(dt)


def _rows_split(q, kv, dout, B, S, H, dh, ft):
    D = H * dh
    qh = q.to(ft).view(B, H, 1, dh)
    kh = kv[:, :D].to(ft).reshape(B, S, H, dh).transpose(1, 2)
    vh = kv[:, D:2 * D].to(ft).reshape(B, S, H, dh).transpose(1, 2)
    return qh, kh, vh, dout.to(ft).view(B, H, 1, dh)


def fp64_rows(q, kv, dout, B, S, H, dh, qscale):
    """fp64 autograd of the class-row attention: out [B, D], dq [B, D] (times qscale), dk, dv [B S, D]."""
    D = H * dh
    qh, kh, vh, do = (t.contiguous().requires_grad_(True) for t in _rows_split(q, kv, dout, B, S, H, dh, torch.float64))
    out = torch.softmax(qh @ kh.transpose(-1, -2), -1) @ vh
    (out * do.detach()).sum().backward()
    return (out.detach().reshape(B, D), qh.grad.reshape(B, D) * qscale, kh.grad.transpose(1, 2).reshape(B * S, D), vh.grad.transpose(1, 2).reshape(B * S, D))


def restated_rows(q, kv, dout, B, S, H, dh, qscale, delta_from="out"):
    """pv_attn_rows_bwd_kernel on stock fp32 ops: everything fp32 (no operand is rounded), delta from the forward's stored 16-bit output (or, for
    comparison, "pdp"), dq, dk, dv rounded to the operand type where they are stored.  fp32 dq [B, D], dk, dv [B S, D]."""
    dt, D = q.dtype, H * dh
    qh, kh, vh, do = _rows_split(q, kv, dout, B, S, H, dh, torch.float32)
    P = torch.softmax(qh @ kh.transpose(-1, -2), -1)                    # [B, H, 1, S]
    dP = do @ vh.transpose(-1, -2)
    if delta_from == "out":
        delta = (do * (P @ vh).to(dt).float()).sum(-1, keepdim=True)
    else:
        delta = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dq = (dS @ kh).reshape(B, D) * qscale
    dk = (dS.transpose(-1, -2) * qh).transpose(1, 2).reshape(B * S, D)
    dv = (P.transpose(-1, -2) * do).transpose(1, 2).reshape(B * S, D)
    return tuple(t.to(dt).float() for t in (dq, dk, dv))


# ---- the per-row measure ----
def row_err(got, ref):
    """e[..., r] = ||got_r - ref_r|| / max(||ref_r||, rms / 8) over the last dimension of [..., R, dh] tensors, rms = the root mean square row norm of
    `ref` over the R rows.  The floor keeps rows whose true gradient is nearly 0 (the dq rows of peaked queries) from dividing by noise; a Gaussian
    row never reaches it from S = 13 on."""
    got, ref = got.double(), ref.double()
    n = ref.norm(dim=-1)
    rms = n.square().mean(-1, keepdim=True).sqrt()
    return (got - ref).norm(dim=-1) / torch.maximum(n, rms / 8).clamp_min(1e-300)


def row_errors(got, ref, B, S, H, dh):
    """{third: e [B, H, S]} of a [B, S, 3 D] gradient against its reference, per (image, head, row)."""
    D = H * dh
    return {name: row_err(heads(got[..., i * D:(i + 1) * D], B, S, H, dh), heads(ref[..., i * D:(i + 1) * D], B, S, H, dh)) for i, name in enumerate(THIRDS)}


def worst(e):
    """(max, its index tuple) of an error tensor."""
    flat = int(e.reshape(-1).argmax())
    idx = []
    for n in reversed(e.shape):
        idx.append(flat % n)
        flat //= n
    return float(e.max()), tuple(reversed(idx))


def row_condition(label, e_kernel, e_restated, what="(image, head, row)"):
    """THE row condition: max over rows of e(kernel) <= 2 x max over rows of e(restated) + 1e-5.  The restatement sets the level, never the kernel;
    2 x and the floor are test_hip_attn_stream's margin for exp2, the P shift and the summation order.  Prints both maxima; returns the failures."""
    bad = []
    for name in e_kernel:
        ek, at = worst(e_kernel[name])
        er, _ = worst(e_restated[name])
        print(f"{label} d{name}: worst row kernel {ek:.3g} at {what} {at}, restated {er:.3g}, ratio {ek / max(er, 1e-30):.3g}")
        if not ek <= 2.0 * er + 1e-5:
            bad.append((label, "d" + name, at, ek, er))
    return bad
