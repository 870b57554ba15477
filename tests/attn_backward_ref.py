"""References for the attention backward kernels - and, further down, the forward kernels - in plain torch on whatever device the inputs live on
(no GPU needed): fp64 on the same 16-bit values, the kernels restated on stock fp32 ops with their rounding points, and a per-row error measure.

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


The FORWARD kernels (restated_forward and its relatives below).  s = fp32 scores from the 16-bit q (pre-scaled) and k, m = the row maximum, p = exp(s - m)
NOT normalised, l = the sum of the UNROUNDED p, O = (p16 V) / l accumulated in fp32 and rounded once, lse = m log2(e) + log2(l) in fp32:

  kernel (entry point)                                   p for P V                         l                 result        lines (pv_attention.hip)
  pv_attn_kernel (pv_attention_bf16 / _lse_bf16,         16 *, relative to the ROW         fp32, unrounded   16            :284-293 p = exp2(fma(s, log2 e, -m log2 e + shift)) and l += p,
    S <= 416, dh 32 / 48 / 64)                           maximum                           p                               :318-320 and :331 pack p, :340-347 o (1 / l) packed once, :301 lse
  pv_attn_stream_kernel (pv_attention_bf16 past 416      16 *, at the SAME point (behind   fp32: l alpha +   16            :551-570 the block's maximum joins the running one, alpha =
    and at dh 80 / 96 / 128; pv_attention_stream_lse     the exponent, unnormalised) but   the block's                     exp2((m - mn) log2 e), p = exp2(fma(s, log2 e, -mn log2 e + shift)),
    [_w]_bf16 at every S)                                relative to the RUNNING maximum   unrounded p                     l = fma(l, alpha, sum p); :573 o alpha in fp32; :576 packs p;
                                                         of the 64-key blocks so far                                       :601 lse, :602-611 o (1 / l) packed once; W: :539-544 key S - 1's
                                                         (`block=64`)                                                      score + tail_log_mult in fp32 before the maximum
  pv_attn_rows_kernel (pv_attention_rows_bf16)           fp32 (`p16=False`)                fp32              16            :2284-2298 fp32 dot product, online softmax and p v per key, nothing
                                                                                                                           rounded (the comment at :2245); :2314-2318 o (1 / l) packed once
  pv_attn_f32_kernel (pv_attention_f32_split)            fp32                              fp32              hi | lo | hi  :671 fp32 MFMA scores from the fp32 q, k; :687 expf(s - m); :702 fp32
                                                                                                                           P V; :708-711 hi = 16(o / l), lo = 16(o / l - hi) (pv_split2, pv_common.h:101)
  pv_attn_split_kernel (pv_attention_split_bf16)         16 *, relative to the row         fp32, unrounded   16            :767-775 x = hi + lo, hi = 16(x), lo = 16((x - hi) 2^11) (2^0 in the
                                                         maximum                           p                               bf16 build); :856-861 s = k_hi.q_hi + (k_hi.q_lo + k_lo.q_hi) 2^-11;
                                                                                                                           :803 v rounded once; :873-882 p and l; :890 and :903 pack p; :911-918 store

  * p is packed as p 2^10 in the fp16 build, as in the backward; the exact factor rides in l and cancels in o / l; lse is m log2(e) + (log2(l 2^10) - 10),
    :301 and :601 - log2 is rounded at the magnitude of log2(l) + 10, which at S = 2 is four ulps of the lse itself.
  The existing `restated` rounds the NORMALISED P instead (the backward kernels recompute P from the statistics); `restated_forward(normalised=True)` is
  that second legitimate restatement for the forward, used by tests/test_attn_forward_ref_host.py to show that the level does not hang on the choice.

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


def inputs(B, S, H, dh, dt, family="gaussian", device="cpu", seed=None, first_of_last=None):
    """qkv [B, S, 3 D] and dout [B, S, D] in the operand type `dt`.  gaussian: `_bf(seed = S)` with q pre-scaled, dout = `_bf(seed = S + 1)` / 10 - what
    the existing attention-backward tests use.  peaked: the same with the q rows 0, 5, 10, ... times 12 before the rounding to the operand type: those
    rows put their probability on one key, as class and register tokens of a trained ViT do.  spread (forward): the q and k thirds times 6 before the
    rounding - scores over tens of units, the data that exposed the stale row maximum of round 5.  edge (forward): the k rows of key S - 1 and of key
    `first_of_last` (the first key of the last tile or block; default 16 (ceil(S / 16) - 1)) times 3 before the rounding, so that a masking slip at the
    ragged edge moves many rows and not only the few whose probability happens to sit there."""
    assert family in ("gaussian", "peaked", "spread", "edge")
    D = H * dh
    seed = S if seed is None else seed
    qkv = randn16(B, S, 3 * D, seed=seed, device=device).float()
    qkv[..., :D] *= dh ** -0.5
    if family == "peaked":
        qkv[:, 0::5, :D] *= 12.0
    elif family == "spread":
        qkv[..., :2 * D] *= 6.0
    elif family == "edge":
        first_of_last = 16 * ((S + 15) // 16 - 1) if first_of_last is None else first_of_last
        for key in sorted({S - 1, first_of_last}):
            qkv[:, key, D:2 * D] *= 3.0
    return qkv.to(dt), randn16(B, S, D, seed=seed + 1, scale=0.1, device=device).to(dt)


def inputs32(B, S, H, dh, amp=1.0, device="cpu", seed=None):
    """fp32 qkv [B, S, 3 D] for the fp32-input kernels: Gaussian values that no 16-bit type holds, q and k times `amp`, q pre-scaled."""
    D = H * dh
    g = torch.Generator(device=device).manual_seed(S if seed is None else seed)
    qkv = torch.randn(B, S, 3 * D, generator=g, device=device)
    qkv[..., :2 * D] *= amp
    qkv[..., :D] *= dh ** -0.5
    return qkv


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


# ---- the forward kernels: out [B, S, D] and lse [B, H, S] = log2 sum_k exp(s[q, k]) ----
LOG2E = 1.0 / math.log(2.0)
LO_SHIFT_F16 = 11                       # pv_attention.hip: PV_LO_SCALE of the fp16 build, 2^11 (1 in the bf16 build)


def _round16(t, dt, shift=0):
    """t rounded to the 16-bit type `dt` as t 2^shift, the exact factor taken out again (fp32)."""
    return t.to(dt).float() if shift == 0 else (t * 2.0 ** shift).to(dt).float() * 2.0 ** -shift


def attend_restated(s, v, dt, p16=True, block=None, normalised=False):
    """What every 16-bit forward kernel does behind its fp32 scores `s` [..., Q, S], on stock fp32 ops: (o [..., Q, dh] BEFORE the store, lse [..., Q]).
    v [..., S, dh] fp32 values.  p16: p = exp(s - m), not normalised, rounded to `dt` (times 2^10 in fp16) for P V; l sums the unrounded p.  block:
    the streaming kernel - the maximum runs over blocks of `block` keys, p is rounded relative to the running maximum, o and l are rescaled in fp32.
    normalised: the other legitimate restatement, which rounds softmax(s) itself (what `restated` does)."""
    shift = P_SHIFT_F16 if dt == torch.float16 else 0
    S = s.shape[-1]
    pack = (lambda p: _round16(p, dt, shift)) if p16 else (lambda p: p)
    if normalised:
        P = torch.softmax(s, dim=-1)
        return pack(P) @ v, torch.logsumexp(s, -1) * LOG2E
    m = torch.full_like(s[..., :1], -math.inf)
    l = torch.zeros_like(m)
    o = torch.zeros(s.shape[:-1] + v.shape[-1:], dtype=s.dtype, device=s.device)
    step = S if block is None else block
    for k0 in range(0, S, step):
        sb = s[..., k0:k0 + step]
        mn = torch.maximum(m, sb.amax(-1, keepdim=True))
        alpha = torch.exp(m - mn)                         # 0 in the first block (m = -inf)
        p = torch.exp(sb - mn)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + pack(p) @ v[..., k0:k0 + step, :]
        m = mn
    # the kernels' l carries 2^shift (it sums the p 2^shift they pack), so log2 is rounded at the magnitude of log2(l) + shift and the exact shift is
    # taken out behind it: m log2(e) + (log2(l 2^shift) - shift), pv_attention.hip:301 and :601 (S = 2 in the fp16 build: an ulp at 10 is four at 2)
    return o / l, (m * LOG2E + (torch.log2(l * 2.0 ** shift) - shift)).squeeze(-1)


def restated_forward(qkv, B, S, H, dh, p16=True, tail_log_mult=0.0, block=None, normalised=False):
    """pv_attn_kernel on stock fp32 ops with its rounding points (the forward table above): (out fp32 [B, S, D] of values the operand type holds, lse fp32
    [B, H, S]).  p16=False: pv_attn_rows_kernel (p stays fp32).  tail_log_mult: added to key S - 1's score in fp32 before the maximum (the W
    instantiation of the streaming kernel).  block=64: pv_attn_stream_kernel.  normalised: see attend_restated."""
    dt, D = qkv.dtype, H * dh
    q, k, v = (heads(t, B, S, H, dh) for t in qkv.float().split(D, dim=-1))
    s = q @ k.transpose(-1, -2)
    if tail_log_mult:
        s[..., S - 1] += tail_log_mult
    o, lse = attend_restated(s, v, dt, p16, block, normalised)
    return rows(o, B, S, H, dh).to(dt).float(), lse


def restated_forward_f32(qkv32, B, S, H, dh, dt=torch.bfloat16):
    """pv_attn_f32_kernel: fp32 attention on stock ops, stored as the [hi | lo | hi] planes of pv_attention_f32_split - hi = the value rounded to the
    library's 16-bit type (bf16 in the bf16 build), lo = the remainder rounded to it.  fp32 [B, S, 3 D]."""
    D = H * dh
    q, k, v = (heads(t, B, S, H, dh) for t in qkv32.float().split(D, dim=-1))
    o = rows(torch.softmax(q @ k.transpose(-1, -2), dim=-1) @ v, B, S, H, dh)
    hi = o.to(dt).float()
    lo = (o - hi).to(dt).float()
    return torch.cat([hi, lo, hi], dim=-1)


def restated_forward_split(qkv32, B, S, H, dh, dt):
    """pv_attn_split_kernel: q = q_hi + q_lo and k = k_hi + k_lo in two 16-bit halves (the lo halves times 2^11 in the fp16 build), s = k_hi.q_hi +
    (k_hi.q_lo + k_lo.q_hi) 2^-11 in fp32, v rounded once, everything behind the scores as restated_forward.  fp32 out [B, S, D]."""
    D = H * dh
    lo_shift = LO_SHIFT_F16 if dt == torch.float16 else 0
    q, k, v = (heads(t, B, S, H, dh) for t in qkv32.float().split(D, dim=-1))
    qh, kh = q.to(dt).float(), k.to(dt).float()
    ql, kl = ((q - qh) * 2.0 ** lo_shift).to(dt).float(), ((k - kh) * 2.0 ** lo_shift).to(dt).float()
    s = (qh @ kl.transpose(-1, -2) + ql @ kh.transpose(-1, -2)) * 2.0 ** -lo_shift + qh @ kh.transpose(-1, -2)
    o, _ = attend_restated(s, v.to(dt).float(), dt)
    return rows(o, B, S, H, dh).to(dt).float()


def fp64_forward(qkv, B, S, H, dh, tail_log_mult=0.0):
    """softmax(q' k^T [+ tail_log_mult on key S - 1]) v in fp64 on the same input values: out [B, S, D], lse [B, H, S] (log2)."""
    D = H * dh
    q, k, v = (heads(t, B, S, H, dh) for t in qkv.double().split(D, dim=-1))
    s = q @ k.transpose(-1, -2)
    if tail_log_mult:
        s[..., S - 1] += tail_log_mult
    return rows(torch.softmax(s, dim=-1) @ v, B, S, H, dh), torch.logsumexp(s, -1) * LOG2E


def forward_row_errors(out, ref, B, S, H, dh):
    """{"out": e [B, H, S]}: the per-row measure of a forward output [B, S, D] against its reference, in row_condition's form."""
    return {"out": row_err(heads(out.float(), B, S, H, dh), heads(ref, B, S, H, dh))}


def lse_condition(label, lse_kernel, lse_restated, lse_ref):
    """THE lse condition: max |lse - fp64| <= 2 x max |lse_restated - fp64| + 2 fp32 ulps at the largest |lse| of the case (one ulp each for the
    hardware exp2 and log2, which the restatement does not have).  Prints the figures; returns the failures."""
    ek = float((lse_kernel.double() - lse_ref).abs().max())
    er = float((lse_restated.double() - lse_ref).abs().max())
    top = float(lse_ref.abs().max())
    ulp = 2.0 ** (math.floor(math.log2(top)) - 23) if top > 0.0 else 2.0 ** -149
    print(f"{label} lse: kernel {ek:.3g}, restated {er:.3g}, ulp at {top:.3g} = {ulp:.3g}")
    return [] if ek <= 2.0 * er + 2.0 * ulp else [(label, "lse", ek, er, ulp)]


# ---- the class-row backward: one query row per image, q [B, D] (pre-scaled), kv [B S, 2 D] (k | v), dout [B, D] ----
def rows_inputs(B, S, H, dh, dt, peaked=False, device="cpu", nq=1):
    """test_attention_rows_backward's inputs; peaked: the one query row times 12 before the rounding.  nq (forward): query rows per image, q [B nq, D]."""
    D = H * dh
    q = randn16(B * nq, D, seed=S, device=device).float() * dh ** -0.5 * (12.0 if peaked else 1.0)
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


def row_condition(label, e_kernel, e_restated, what="(image, head, row)", prefix="d", floor=1e-5):
    """THE row condition: max over rows of e(kernel) <= 2 x max over rows of e(restated) + 1e-5.  The restatement sets the level, never the kernel;
    2 x and the floor are test_hip_attn_stream's margin for exp2, the P shift and the summation order.  Prints both maxima; returns the failures.
    (prefix names the tensors in the report: "d" + third for gradients, "" for the forward's "out"; floor: 2^-20 for the fp32 forward kernel, whose
    summation-order term sqrt(416) 2^-24 is all the error it has.)"""
    bad = []
    for name in e_kernel:
        ek, at = worst(e_kernel[name])
        er, _ = worst(e_restated[name])
        print(f"{label} {prefix}{name}: worst row kernel {ek:.3g} at {what} {at}, restated {er:.3g}, ratio {ek / max(er, 1e-30):.3g}")
        if not ek <= 2.0 * er + floor:
            bad.append((label, prefix + name, at, ek, er))
    return bad
