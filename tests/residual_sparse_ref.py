"""Torch restatements of ResidualViT's exact token compaction, shared by tests/test_residual_sparse_host.py (which
validates them against oracle.vit_oracle's dense forward in fp64) and tests/test_hip_residual_sparse.py (which checks the kernels and the
packed engine forward against them).  Test infrastructure, not product code: the package never imports this module.

  pack_step_ref      one gate + compaction step on a packed row matrix (what pv_residual_pack_step computes), any float dtype / device
  attention_w_ref    ragged attention with a per-key log-multiplicity (what pv_attention_varlen_w_bf16 computes)
  packed_forward     the whole compacting forward built from the two, in the dtype of its inputs
  dense_forward      oracle.vit_oracle's dense ResidualViT forward, op by op, in the dtype of its inputs (the oracle's own
                     residualvit_forward casts the image and every parameter to fp32; its building blocks do not)
"""
import contextlib
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vit_oracle as O


def pack_step_ref(x, seg, mult, tok_row, wg, bg, wb, bb, temp, sigmoid_bias):
    """x [R, D]; seg int [B + 1]; mult int [R]; tok_row int [B, N]; wg / wb [D]; bg / bb scalars (tensors or floats).  Returns a dict with
    x_next, row_scale_next, mult_next, log_mult_next, seg_next, tok_row_next, mask_out [B, N], thr_out [B], totals (R', longest segment), and
    `margin` [R]: |sigmoid - threshold| of every input row (inf on class and budget rows)."""
    seg = np.asarray(torch.as_tensor(seg).cpu()).astype(np.int64)
    mult = np.asarray(torch.as_tensor(mult).cpu()).astype(np.int64)
    tok_row = np.asarray(torch.as_tensor(tok_row).cpu()).astype(np.int64)
    B = len(seg) - 1
    lens = np.diff(seg)
    dev, dt = x.device, x.dtype
    img = torch.from_numpy(np.repeat(np.arange(B), lens)).to(dev)
    first, last = torch.from_numpy(seg[:-1]).to(dev), torch.from_numpy(seg[1:] - 1).to(dev)
    wg, wb = wg.reshape(-1).to(dt), wb.reshape(-1).to(dt)
    thr = torch.sigmoid(x[last] @ wb + float(bb))                                  # residualvit.py:212
    sig = torch.sigmoid((x @ wg + float(bg)) / temp + sigmoid_bias)                # blocks.py:69
    m = F.relu(sig - thr[img])                                                      # residualvit.py:66
    margin = (sig - thr[img]).abs()
    m[first], m[last] = 1.0, 1.0
    margin[first], margin[last] = float("inf"), float("inf")
    mh = m.detach().cpu().numpy()
    src, scale_idx, mult_next, seg_next, tok_next, mask_out = [], [], [], [0], np.empty_like(tok_row), []
    for b in range(B):
        s0, L = seg[b], lens[b]
        mid = np.arange(1, L - 1)
        live = mid[mh[s0 + mid] > 0]
        dead = mid[~(mh[s0 + mid] > 0)]
        new = np.full(L, -1, dtype=np.int64)
        rows = [0] + live.tolist()
        new[rows] = np.arange(len(rows))
        s, mu = [s0 + r for r in rows], [int(mult[s0 + r]) for r in rows]
        if len(dead):
            new[dead] = len(rows)
            s.append(-1)
            mu.append(int(mult[s0 + dead].sum()))
        new[L - 1] = len(s)
        s.append(s0 + L - 1)
        mu.append(int(mult[s0 + L - 1]))
        src += s
        mult_next += mu
        seg_next.append(seg_next[-1] + len(s))
        tok_next[b] = new[tok_row[b]]
        mask_out.append(m[torch.from_numpy(s0 + tok_row[b]).to(dev)])
    src_t = torch.tensor(src, dtype=torch.int64, device=dev)
    zero = src_t < 0
    scale = torch.where(zero, torch.zeros((), dtype=dt, device=dev), m[src_t.clamp(min=0)])
    x_next = x[src_t.clamp(min=0)] * scale[:, None]
    x_next[zero] = 0
    mult_next = np.asarray(mult_next, dtype=np.int64)
    seg_next = np.asarray(seg_next, dtype=np.int64)
    return {"x_next": x_next, "row_scale_next": scale, "mult_next": mult_next,
            "log_mult_next": torch.log(torch.from_numpy(mult_next).to(dev).to(dt)), "seg_next": seg_next, "tok_row_next": tok_next,
            "mask_out": torch.stack(mask_out), "thr_out": thr, "totals": (int(seg_next[-1]), int(np.diff(seg_next).max())), "margin": margin}


def attention_w_ref(qkv, seg, log_mult, H):
    """qkv [R, 3 * H * dh] (q pre-scaled), seg int [B + 1], log_mult [R] -> [R, H * dh]: per segment and head softmax(q k^T + log_mult) v."""
    seg = np.asarray(torch.as_tensor(seg).cpu()).astype(np.int64)
    R, D = qkv.shape[0], qkv.shape[1] // 3
    dh = D // H
    out = torch.empty((R, D), dtype=qkv.dtype, device=qkv.device)
    for b in range(len(seg) - 1):
        s0, s1 = int(seg[b]), int(seg[b + 1])
        q, k, v = (qkv[s0:s1, i * D:(i + 1) * D].reshape(s1 - s0, H, dh).transpose(0, 1) for i in range(3))
        p = torch.softmax(q @ k.transpose(-1, -2) + log_mult[s0:s1][None, None, :], dim=-1)
        out[s0:s1] = (p @ v).transpose(0, 1).reshape(s1 - s0, D)
    return out


def _embed(x, sd, cfg, budget):
    t = O.embed_tokens(x, sd, cfg) + sd["encoder.pos_embedding"]                  # residualvit.py:338-343
    btok = sd["learnable_budget_token_1"].expand(t.shape[0], -1, -1) * torch.tensor(budget, dtype=torch.float32).to(x.dtype)   # :566-568
    return torch.cat([t, btok], dim=1)                                             # :345


def _head(cls_rows, sd):
    t = O.layer_norm(cls_rows, sd["encoder.ln.weight"], sd["encoder.ln.bias"], 1e-5)
    return F.linear(t, sd["head.weight"], sd["head.bias"])


@contextlib.contextmanager
def _oracle_keeps_dtype():
    """oracle.vit_oracle reads every parameter through `_t`, which casts to fp32: inside, it hands the tensors over as they are."""
    old = O._t
    O._t = lambda sd, key: sd[key]
    try:
        yield
    finally:
        O._t = old


def dense_forward(x, sd, cfg, budget):
    """(logits [B, C], masks [L, B, N, 1], thresholds [L, B], margins [L, B, N]) of the dense forward in the dtype of x / sd: the body of
    oracle.vit_oracle.residualvit_forward with the oracle's own embed_tokens / residual_block / layer_norm."""
    H, L = cfg["num_heads"], cfg["num_layers"]
    temp, gb = cfg.get("gate_temp", 1.0), cfg.get("gate_bias", 10.0)
    masks, thrs, margins = [], [], []
    with _oracle_keeps_dtype(), torch.no_grad():
        t = _embed(x, sd, cfg, budget)
        for i in range(L):
            p = f"encoder.layers.{i}."
            thr = torch.sigmoid(F.linear(t[:, -1:], sd[p + "budget_token_gate.weight"], sd[p + "budget_token_gate.bias"]))
            sig = torch.sigmoid(F.linear(t[:, 1:-1], sd[p + "residual_gate.projection.weight"], sd[p + "residual_gate.projection.bias"]) / temp + gb)
            t, mask = O.residual_block(t, sd, p, H, temp, gb)
            masks.append(mask)
            thrs.append(thr.reshape(-1))
            margins.append((sig - thr).abs().squeeze(-1))
        logits = _head(t[:, 0], sd)
    return logits, torch.stack(masks), torch.stack(thrs), torch.stack(margins)


def packed_forward(x, sd, cfg, budget):
    """The compacting forward (engine.residual_forward_packed's algorithm) in the dtype of x / sd.  Returns (logits, masks [L, B, N, 1],
    thresholds [L, B], rows run per layer)."""
    H, L = cfg["num_heads"], cfg["num_layers"]
    temp, gb = cfg.get("gate_temp", 1.0), cfg.get("gate_bias", 10.0)
    with _oracle_keeps_dtype(), torch.no_grad():
        t = _embed(x, sd, cfg, budget)
        B, S, D = t.shape
        N, dh = S - 2, D // H
        xs = t.reshape(B * S, D)
        seg, mult = np.arange(0, (B + 1) * S, S), np.ones(B * S, dtype=np.int64)
        tok_row = np.tile(np.arange(1, S - 1), (B, 1))
        masks, thrs, rows = [], [], []
        for i in range(L):
            p = f"encoder.layers.{i}."
            g = lambda k: sd[p + k]
            st = pack_step_ref(xs, seg, mult, tok_row, g("residual_gate.projection.weight"), g("residual_gate.projection.bias"),
                               g("budget_token_gate.weight"), g("budget_token_gate.bias"), temp, gb)
            masks.append(st["mask_out"].reshape(B, N, 1))
            thrs.append(st["thr_out"])
            xm, rs, seg, mult, tok_row = st["x_next"], st["row_scale_next"][:, None], st["seg_next"], st["mult_next"], st["tok_row_next"]
            rows.append(xm.shape[0])
            h = rs * O.layer_norm(xm, g("ln_1.weight"), g("ln_1.bias"), 1e-6)                          # residualvit.py:251-252
            qkv = F.linear(h, g("self_attention.self_attention.in_proj_weight"), g("self_attention.self_attention.in_proj_bias"))
            qkv = torch.cat([qkv[:, :D] * (float(dh) ** -0.5), qkv[:, D:]], dim=1)
            a = attention_w_ref(qkv, seg, st["log_mult_next"], H)
            a = F.linear(a, g("self_attention.self_attention.out_proj.weight"), g("self_attention.self_attention.out_proj.bias"))
            x1 = rs * a + xm                                                                        # :254-255
            y = rs * O.layer_norm(x1, g("ln_2.weight"), g("ln_2.bias"), 1e-6)                          # :258
            xs = x1 + O.mlp(y, g("mlp.fc1.weight"), g("mlp.fc1.bias"), g("mlp.fc2.weight"), g("mlp.fc2.bias"))
        logits = _head(xs[torch.from_numpy(seg[:-1])], sd)
    return logits, torch.stack(masks), torch.stack(thrs), rows


def sparse_sd(cfg, gate_gain, dtype=torch.float64, seed=0):
    from peekvit_amd import synth
    return {k: torch.from_numpy(v.copy()).to(dtype) for k, v in synth.residual_sparse_state_dict(cfg, gate_gain=gate_gain, seed=seed).items()}


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
