"""Torch restatements of ResidualViT's packed TRAINING forward under autograd, shared by
tests/test_residual_sparse_train_host.py (which validates them against the dense composite model in fp64) and
tests/test_hip_residual_sparse_train.py (which checks the kernels against them).  Test infrastructure, not product code: the package never
imports this module.  tests/residual_sparse_ref.py (the inference restatement, under no_grad) stays as it is; its helpers are used here.

  pack_step_train_ref     pack_step_ref's arithmetic and tables, differentiable in x and the four gate tensors (pack_step_ref itself writes
                          the class and budget rows' mask in place into relu's output, which autograd refuses to differentiate)
  attention_w_train_ref   ragged attention with a per-key log-multiplicity: out and the rows' log2-sum-exp [R, H], differentiable in qkv
  packed_train_forward    embed, per-image budget row, per layer pack step + masked block body on the ragged segments, class-row head

Why plain autograd of the packed forward gives the dense model's parameter gradients: a token whose mask is exactly 0 enters the block as a
zero row, leaves it as the constant fc2(gelu(b1)) + b2 and receives no gradient (relu's slope is 0 there), and the packed forward is an exact
restatement of the dense one (section 17).  A packed row that stands for n identical tokens is used n times (as a key: + ln n on its score;
in the dense mask: through tok_row), so it collects the summed gradient of its n members without any explicit multiplicity factor."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vit_oracle as O
import residual_sparse_ref as R


def pack_step_train_ref(x, seg, mult, tok_row, wg, bg, wb, bb, temp, sigmoid_bias):
    """pack_step_ref with a graph: x [R, D]; wg / wb [D] (or [1, D]); bg / bb tensors of one element (or floats).  Returns pack_step_ref's dict
    plus `src` (int64 [R']: the source packed row of every next row, -1 for a zero row), `sig` [R] (the gate's sigmoid value per row) and
    `mask_row` [R]."""
    seg = np.asarray(torch.as_tensor(seg).cpu()).astype(np.int64)
    mult = np.asarray(torch.as_tensor(mult).cpu()).astype(np.int64)
    tok_row = np.asarray(torch.as_tensor(tok_row).cpu()).astype(np.int64)
    B = len(seg) - 1
    lens = np.diff(seg)
    dev, dt = x.device, x.dtype
    img = torch.from_numpy(np.repeat(np.arange(B), lens)).to(dev)
    first, last = torch.from_numpy(seg[:-1]).to(dev), torch.from_numpy(seg[1:] - 1).to(dev)
    as_t = lambda v: v.reshape(()).to(dt) if torch.is_tensor(v) else torch.tensor(float(v), dtype=dt, device=dev)
    wg, wb, bg, bb = wg.reshape(-1).to(dt), wb.reshape(-1).to(dt), as_t(bg), as_t(bb)
    thr = torch.sigmoid(x[last] @ wb + bb)
    sig = torch.sigmoid((x @ wg + bg) / temp + sigmoid_bias)
    special = torch.zeros(x.shape[0], dtype=torch.bool, device=dev)
    special[first] = True
    special[last] = True
    m = torch.where(special, torch.ones((), dtype=dt, device=dev), F.relu(sig - thr[img]))
    margin = torch.where(special, torch.full((), float("inf"), dtype=dt, device=dev), (sig - thr[img]).abs().detach())
    mh = m.detach().cpu().numpy()
    src, mult_next, seg_next, tok_next, mask_out = [], [], [0], np.empty_like(tok_row), []
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
    x_next = x[src_t.clamp(min=0)] * scale[:, None]          # (a zero row: scale 0 -> value 0 and no gradient to the row it indexes)
    mult_next = np.asarray(mult_next, dtype=np.int64)
    seg_next = np.asarray(seg_next, dtype=np.int64)
    return {"x_next": x_next, "row_scale_next": scale, "mult_next": mult_next,
            "log_mult_next": torch.log(torch.from_numpy(mult_next).to(dev).to(dt)), "seg_next": seg_next, "tok_row_next": tok_next,
            "mask_out": torch.stack(mask_out), "thr_out": thr, "totals": (int(seg_next[-1]), int(np.diff(seg_next).max())), "margin": margin,
            "src": src_t, "sig": sig, "mask_row": m}


def attention_w_train_ref(qkv, seg, log_mult, H):
    """qkv [R, 3 * H * dh] (q pre-scaled), seg int [B + 1], log_mult [R] -> (out [R, H * dh], lse [R, H]): per segment and head
    softmax(q k^T + log_mult) v and log2 sum_k exp(q k^T + log_mult), the bias included (pv_attention_lse_bf16's definition)."""
    seg = np.asarray(torch.as_tensor(seg).cpu()).astype(np.int64)
    D = qkv.shape[1] // 3
    dh = D // H
    outs, lses = [], []
    for b in range(len(seg) - 1):
        s0, s1 = int(seg[b]), int(seg[b + 1])
        q, k, v = (qkv[s0:s1, i * D:(i + 1) * D].reshape(s1 - s0, H, dh).transpose(0, 1) for i in range(3))
        s = q @ k.transpose(-1, -2) + log_mult[s0:s1][None, None, :]
        outs.append((torch.softmax(s, dim=-1) @ v).transpose(0, 1).reshape(s1 - s0, D))
        lses.append((torch.logsumexp(s, dim=-1) / math.log(2.0)).transpose(0, 1))
    return torch.cat(outs), torch.cat(lses)


def packed_train_forward(x, params, cfg, budgets):
    """The packed training forward in the dtype of x / params.  params: state-dict name -> tensor (leaves that require grad, or plain
    tensors); budgets: one float per image.  Returns (logits [B, C], masks: list of L dense [B, N, 1] tensors that carry the graph,
    thresholds: list of L [B] tensors, rows run per layer).  Differentiable in every parameter."""
    H, L = cfg["num_heads"], cfg["num_layers"]
    temp, gb = cfg.get("gate_temp", 1.0), cfg.get("gate_bias", 10.0)
    with R._oracle_keeps_dtype():
        t = O.embed_tokens(x, params, cfg) + params["encoder.pos_embedding"]
        bud = torch.as_tensor(budgets, dtype=x.dtype).reshape(-1, 1, 1)
        t = torch.cat([t, params["learnable_budget_token_1"].expand(t.shape[0], -1, -1) * bud], dim=1)
        B, S, D = t.shape
        N, dh = S - 2, D // H
        xs = t.reshape(B * S, D)
        seg, mult = np.arange(0, (B + 1) * S, S), np.ones(B * S, dtype=np.int64)
        tok_row = np.tile(np.arange(1, S - 1), (B, 1))
        masks, thrs, rows = [], [], []
        for i in range(L):
            p = f"encoder.layers.{i}."
            g = lambda k: params[p + k]
            st = pack_step_train_ref(xs, seg, mult, tok_row, g("residual_gate.projection.weight"), g("residual_gate.projection.bias"),
                                     g("budget_token_gate.weight"), g("budget_token_gate.bias"), temp, gb)
            masks.append(st["mask_out"].reshape(B, N, 1))
            thrs.append(st["thr_out"])
            xm, rs, seg, mult, tok_row = st["x_next"], st["row_scale_next"][:, None], st["seg_next"], st["mult_next"], st["tok_row_next"]
            rows.append(xm.shape[0])
            h = rs * O.layer_norm(xm, g("ln_1.weight"), g("ln_1.bias"), 1e-6)
            qkv = F.linear(h, g("self_attention.self_attention.in_proj_weight"), g("self_attention.self_attention.in_proj_bias"))
            qkv = torch.cat([qkv[:, :D] * (float(dh) ** -0.5), qkv[:, D:]], dim=1)
            a, _ = attention_w_train_ref(qkv, seg, st["log_mult_next"], H)
            a = F.linear(a, g("self_attention.self_attention.out_proj.weight"), g("self_attention.self_attention.out_proj.bias"))
            x1 = rs * a + xm
            y = rs * O.layer_norm(x1, g("ln_2.weight"), g("ln_2.bias"), 1e-6)
            xs = x1 + O.mlp(y, g("mlp.fc1.weight"), g("mlp.fc1.bias"), g("mlp.fc2.weight"), g("mlp.fc2.bias"))
        cls = xs[torch.from_numpy(seg[:-1])]
        logits = F.linear(O.layer_norm(cls, params["encoder.ln.weight"], params["encoder.ln.bias"], 1e-5), params["head.weight"], params["head.bias"])
    return logits, masks, thrs, rows


def budget_mse_ref(masks, budget, strict=False):
    """peekvit_amd.losses.budget_mse (per_layer) on a list of dense masks [B, N, 1]."""
    terms = []
    for m in masks:
        d = m.mean(dim=(1, 2)) - budget
        terms.append(((d if strict else torch.relu(d)) ** 2).sum())
    return (torch.stack(terms) * (2 - budget)).mean()


# ---- ragged weighted attention backward, row by row in fp64 (what the backward kernel pair computes) ----
def attention_w_backward_ref(qkv, dout, seg, log_mult, H, qscale):
    """fp64 reference of the ragged weighted attention backward.  qkv [R, 3 D] holds q PRE-SCALED by qscale (as the kernels read it); the
    result dqkv [R, 3 D] is the gradient with respect to (q UNSCALED | k | v), i. e. the q third carries the factor qscale, as
    pv_attention_stream_bwd16_bf16 returns it.  Also returns delta [R, H] = sum_k p dP."""
    qkv, dout, log_mult = qkv.double(), dout.double(), log_mult.double()
    seg = np.asarray(torch.as_tensor(seg).cpu()).astype(np.int64)
    Rr, D = qkv.shape[0], qkv.shape[1] // 3
    dh = D // H
    dqkv = torch.zeros_like(qkv)
    delta = torch.zeros((Rr, H), dtype=torch.float64)
    for b in range(len(seg) - 1):
        s0, s1 = int(seg[b]), int(seg[b + 1])
        n = s1 - s0
        if n <= 0:
            continue
        q, k, v = (qkv[s0:s1, i * D:(i + 1) * D].reshape(n, H, dh).transpose(0, 1) for i in range(3))
        do = dout[s0:s1].reshape(n, H, dh).transpose(0, 1)
        p = torch.softmax(q @ k.transpose(-1, -2) + log_mult[s0:s1][None, None, :], dim=-1)
        dp = do @ v.transpose(-1, -2)
        dl = (p * dp).sum(-1, keepdim=True)
        ds = p * (dp - dl)
        dqkv[s0:s1, :D] = (ds @ k).transpose(0, 1).reshape(n, D) * qscale
        dqkv[s0:s1, D:2 * D] = (ds.transpose(-1, -2) @ q).transpose(0, 1).reshape(n, D)
        dqkv[s0:s1, 2 * D:] = (p.transpose(-1, -2) @ do).transpose(0, 1).reshape(n, D)
        delta[s0:s1] = dl.squeeze(-1).transpose(0, 1)
    return dqkv, delta
