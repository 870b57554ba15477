"""References for dropout on the training path (include/peekvit_hip_dropout.h), no GPU needed:

  * the mask generator of peekvit_amd/csrc/pv_dropout.h in numpy uint64 / uint32 arithmetic, bit for bit;
  * attention with an explicit mask in fp64: by autograd, and by the hand-written backward the kernels run (the delta identity);
  * `restated_*`: the streaming kernels' DROP instantiations on stock fp32 ops with their rounding points, built on attn_backward_ref;
  * an fp64 composite of a whole VisionTransformer / RankVisionTransformer that replays a `dropout_record`.

Rounding points of the DROP instantiations (csrc/pv_attention.hip pv_attn_stream_kernel, csrc/pv_attention_stream.hip):
  forward   the running maximum, l = the sum of ALL unrounded p and lse are those of the dropout-free kernel; a dropped p is 0 where p is rounded to the
            operand type (times 2^10 in the fp16 build) for V^T P^T; out = o / (l (1 - p)) rounded once
  backward  delta = rowsum(dO o O) of the stored output; dS = P o (M o dP / (1 - p) - delta) in fp32 from the unrounded P, rounded once; dV from
            round16(P o M) with 1 / (1 - p) (and the fp16 build's exact 2^-10) applied where dV is stored; results rounded once."""
import math

import numpy as np
import torch

import attn_backward_ref as R


# ---- the generator (pv_dropout.h) ----
def sm64(z):
    """splitmix64's finaliser on uint64 arrays (wrap-around arithmetic)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def lowbias32(x):
    x = np.asarray(x, dtype=np.uint32)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x7feb352d)
        x = x ^ (x >> np.uint32(15))
        x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def threshold(p):
    """floor(p 2^32) of the fp32 value of p (the product is exact in fp64)."""
    return np.uint32(int(math.floor(float(np.float32(p)) * 4294967296.0)))


def scale(p):
    """The fp32 value 1 / (1 - p) survivors are multiplied by, as a Python float."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def words(key, site, rows, cols, row0=0):
    """The 32-bit word of every element of rows [row0, row0 + rows) x cols of a site: uint32 [rows, cols]."""
    base = sm64(np.uint64(key) ^ sm64(np.uint64(site)))
    with np.errstate(over="ignore"):
        r = np.arange(row0, row0 + rows, dtype=np.uint64) * np.uint64(0xD1B54A32D192ED03)
        rk = sm64(base ^ r)
        lo, hi = (rk & np.uint64(0xFFFFFFFF)).astype(np.uint32), (rk >> np.uint64(32)).astype(np.uint32)
        c = np.arange(cols, dtype=np.uint32) * np.uint32(0x9E3779B1)
        return lowbias32((lo[:, None] + c[None, :]) ^ hi[:, None])


def keep_mask(key, site, rows, cols, p, row0=0):
    """uint8 [rows, cols]: 1 = kept."""
    return (words(key, site, rows, cols, row0) >= threshold(p)).astype(np.uint8)


def keep_tensor(key, site, shape, p, device="cpu", dtype=torch.float64):
    """The mask of a site of any shape [..., cols] (rows = everything in front, row-major), as a 0 / 1 tensor."""
    cols = int(shape[-1])
    rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
    return torch.from_numpy(keep_mask(key, site, rows, cols, p)).to(device=device, dtype=dtype).reshape(tuple(shape))


# ---- attention with an explicit mask, fp64 ----
def _split(qkv, B, S, H, dh, ft):
    D = H * dh
    return tuple(R.heads(t, B, S, H, dh) for t in qkv.to(ft).split(D, dim=-1))


def fp64_attention(qkv, dout, mask, p, B, S, H, dh, qscale):
    """fp64 AUTOGRAD through (softmax(q' k^T) o mask / (1 - p)) v on the given values: out [B, S, D], lse [B, H, S] (log2, of all keys), dqkv [B, S, 3 D]
    with the q third times qscale.  mask [B, H, S, S] of 0 / 1."""
    D = H * dh
    t = qkv.double().reshape(B, S, 3, H, dh).permute(2, 0, 3, 1, 4).contiguous().requires_grad_(True)
    s = t[0] @ t[1].transpose(-1, -2)
    P = torch.softmax(s, dim=-1) * (mask.double() * scale(p))
    out = R.rows(P @ t[2], B, S, H, dh)
    (out * dout.double()).sum().backward()
    g = t.grad.clone()
    g[0] *= qscale
    return out.detach(), (torch.logsumexp(s, -1) / math.log(2.0)).detach(), g.permute(1, 3, 0, 2, 4).reshape(B, S, 3 * D)


def fp64_attention_manual(qkv, dout, mask, p, B, S, H, dh, qscale):
    """The same in fp64 by the hand-written backward the kernels run: delta = rowsum(dO o O), dS = P o (M o dP / (1 - p) - delta), dV = (P o M)^T dO / (1 - p)."""
    q, k, v = _split(qkv, B, S, H, dh, torch.float64)
    do = R.heads(dout.double(), B, S, H, dh)
    M, sc = mask.double(), scale(p)
    P = torch.softmax(q @ k.transpose(-1, -2), dim=-1)
    O = (P * M * sc) @ v
    delta = (do * O).sum(-1, keepdim=True)
    dP = do @ v.transpose(-1, -2)
    dS = P * (M * dP * sc - delta)
    dq, dk, dv = (dS @ k) * qscale, dS.transpose(-1, -2) @ q, (P * M).transpose(-1, -2) @ do * sc
    return R.rows(O, B, S, H, dh), torch.cat([R.rows(t, B, S, H, dh) for t in (dq, dk, dv)], dim=-1)


# ---- the DROP instantiations on stock fp32 ops ----
def restated_forward(qkv, mask, p, B, S, H, dh, block=64):
    """pv_attn_stream_kernel<DH, true, false, true>: attn_backward_ref.attend_restated's streaming loop with the mask applied where p is packed.
    (out fp32 [B, S, D] of values the operand type holds, lse fp32 [B, H, S])."""
    dt = qkv.dtype
    shift = R.P_SHIFT_F16 if dt == torch.float16 else 0
    q, k, v = _split(qkv, B, S, H, dh, torch.float32)
    Mf = mask.float()
    s = q @ k.transpose(-1, -2)
    m = torch.full_like(s[..., :1], -math.inf)
    l = torch.zeros_like(m)
    o = torch.zeros(s.shape[:-1] + v.shape[-1:], dtype=s.dtype, device=s.device)
    for k0 in range(0, S, block):
        sb = s[..., k0:k0 + block]
        mn = torch.maximum(m, sb.amax(-1, keepdim=True))
        alpha = torch.exp(m - mn)
        pe = torch.exp(sb - mn)
        l = l * alpha + pe.sum(-1, keepdim=True)                       # every key
        o = o * alpha + R._round16(pe * Mf[..., k0:k0 + block], dt, shift) @ v[..., k0:k0 + block, :]
        m = mn
    omp = float(np.float32(1.0) - np.float32(p))
    out = o * (1.0 / (l * omp))
    lse = (m * R.LOG2E + (torch.log2(l * 2.0 ** shift) - shift)).squeeze(-1)
    return R.rows(out, B, S, H, dh).to(dt).float(), lse


def restated_backward(qkv, dout, mask, p, B, S, H, dh, qscale):
    """pv_attn_stream_dq / dkv_kernel<DH, true, false, true> on stock fp32 ops (attn_backward_ref.restated with delta_from = "out", the mask and
    1 / (1 - p) at the kernels' places): fp32 [B, S, 3 D] of values the operand type holds."""
    dt = qkv.dtype
    shift = R.P_SHIFT_F16 if dt == torch.float16 else 0
    sc = scale(p)
    q, k, v = _split(qkv, B, S, H, dh, torch.float32)
    do = R.heads(dout.float(), B, S, H, dh)
    Mf = mask.float()
    P = torch.softmax(q @ k.transpose(-1, -2), dim=-1)
    P16 = R._round16(P * Mf, dt, shift)
    dv = (P16.transpose(-1, -2) @ do) * sc
    dP = do @ v.transpose(-1, -2)
    o16 = R.heads(restated_forward(qkv, mask, p, B, S, H, dh)[0], B, S, H, dh)
    delta = (do * o16).sum(-1, keepdim=True)
    dS = (P * (Mf * dP * sc - delta)).to(dt).float()
    dq, dk = (dS @ k) * qscale, dS.transpose(-1, -2) @ q
    return torch.cat([R.rows(t, B, S, H, dh) for t in (dq, dk, dv)], dim=-1).to(dt).float()


def attention_mask(key, site, B, H, S, p, device="cpu"):
    """bool [B, H, S, S]: row (b H + h) S + q, column k of the attention site."""
    return torch.from_numpy(keep_mask(key, site, B * H * S, S, p).astype(bool)).to(device).view(B, H, S, S)


# an attention site at S = 3, p = 0.9 that holds fully dropped rows next to rows that are not (the host and the GPU test assert both)
FULL_DROP = dict(key=1234, site=7, B=2, H=2, S=3, dh=32, p=0.9)


# ---- a whole model in fp64, replaying a dropout_record ----
def model_composite_fp64(model, x, record, keeps=None):
    """Logits of a VisionTransformer / RankVisionTransformer `model` (an fp64 copy, any device) on x, with the masks of `record` = (key, [(kind, site, p,
    shape), ...]) - train_engine.train_state(m).dropout_record of the HIP pass - applied at the three dropout sites in call order; record None: no
    dropout.  keeps: per ranked block (in layer order) the int [B, k] indices the HIP pass kept (blk.last_keep), replayed instead of a ranking."""
    key, sites = record if record is not None else (0, [])
    it = iter(sites)
    keeps = iter(keeps or [])
    dev = x.device

    def mask(kind, shape, p_live):
        if record is None or p_live <= 0.0:
            return None
        k, site, p, shp = next(it)
        assert k == kind and tuple(shp) == tuple(shape) and abs(p - p_live) < 1e-12, (k, kind, shp, shape, p, p_live)
        return keep_tensor(key, site, shape, p, dev) * scale(p)

    enc = model.encoder
    t = model._composite_tokens(x.double()) + enc.pos_embedding
    mk = mask("input", t.shape, float(enc.dropout.p))
    if mk is not None:
        t = t * mk
    for blk in enc.layers:
        if getattr(blk, "current_budget", 1) != 1:
            keep = next(keeps).long()
            rest = t[:, 1:]
            t = torch.cat([t[:, :1], torch.gather(rest, 1, keep.unsqueeze(-1).expand(-1, -1, rest.shape[-1]))], dim=1)
        B, S, D = t.shape
        mha = blk.self_attention.self_attention
        H = mha.num_heads
        dh = D // H
        h1 = blk.ln_1(t)
        q, k, v = (R.heads(u, B, S, H, dh) for u in torch.nn.functional.linear(h1, mha.in_proj_weight, mha.in_proj_bias).split(D, dim=-1))
        P = torch.softmax((q * dh ** -0.5) @ k.transpose(-1, -2), dim=-1)
        mk = mask("attention", (B, H, S, S), float(mha.dropout))
        if mk is not None:
            P = P * mk
        br = mha.out_proj(R.rows(P @ v, B, S, H, dh))
        mk = mask("branch", (B * S, D), float(blk.dropout.p))
        if mk is not None:
            br = br * mk.view(B, S, D)
        x1 = t + br
        t = x1 + blk.mlp(blk.ln_2(x1))
    assert next(it, None) is None, "the record holds more sites than the composite met"
    return model._composite_head(enc.ln(t))
