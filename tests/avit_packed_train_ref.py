"""The packed A-ViT training pass restated in plain torch, shared by tests/test_avit_packed_train_host.py and
tests/test_hip_avit_packed_train.py: the halting step on packed rows with its compaction (`pack_step_fwd`), its hand-written backward with the
per-image scalar G (`pack_step_bwd`), the block on packed rows with ln n key weights (`packed_block`, the one piece differentiated by autograd: it is
row-wise apart from the attention within a segment), and one whole training step built from them (`packed_model_step`).  Everything runs in the dtype
of its inputs (fp64 in the tests), on the CPU, with no project code.

Layout (include/peekvit_hip_avit_pack_train.h): image b is the row segment [seg[b], seg[b+1]) - its live tokens in token order (pos = token index)
and, when nh[b] > 0, one representative row for its nh[b] halted tokens, last (pos = -1, row scale 0, key weight ln nh[b])."""
import math

import torch

import avit_train_ref as dense

REACHED, NOT_REACHED, LIVE, MERGED, REP = 1, 2, 4, 8, 16


def initial_tables(B, S):
    """(seg [B+1], nh [B], pos [B*S], row_scale [B*S], log_mult [B*S]) of the unpacked first layer."""
    return (torch.arange(0, (B + 1) * S, S), torch.zeros(B, dtype=torch.long), torch.arange(S).repeat(B), torch.ones(B * S), torch.zeros(B * S))


def _row_image(seg, R):
    img = torch.zeros(R, dtype=torch.long)
    for b in range(len(seg) - 1):
        img[int(seg[b]):int(seg[b + 1])] = b
    return img


def pack_step_fwd(y, seg, nh, pos, state, acc, gate_scale, gate_center, thr, last, nr_replay=None):
    """One halting step on the packed block output y [R, D].  state = (c, R, rho, counter, m), each [B, S]; acc [B, n_cls, D]; nr_replay: a bool [B, S]
    of `not reached` decisions to use instead of the comparison (reached = m * (1 - nr) then).  Returns a dict: state (the five updated arrays), acc,
    h_part [B], sv [3, R] = (h, w, flags), ycls, and unless `last`: x_next, rs_next, lm_next, pos_next, seg_next, nh_next, src_next, totals."""
    R_rows, D = y.shape
    c, Rr, rho, cnt, m = state
    B, S = c.shape
    n_cls = acc.shape[1]
    seg, nh, pos = torch.as_tensor(seg).long(), torch.as_tensor(nh).long(), torch.as_tensor(pos).long()
    img = _row_image(seg, R_rows)
    live = pos >= 0
    h = torch.sigmoid(y[:, 0] * gate_scale - gate_center)
    hh = torch.ones_like(h) if last else h
    lb, lp = img[live], pos[live]
    c_l, R_l, m_l = c[lb, lp], Rr[lb, lp], m[lb, lp]
    c1 = c_l + hh[live]
    if nr_replay is None:
        reached = (c1 > thr).to(y.dtype) * m_l
        nr = (c1 < thr).to(y.dtype)
    else:
        nr = nr_replay[lb, lp].to(y.dtype)
        reached = m_l * (1 - nr)
    w_l = m_l * (R_l * reached + hh[live] * nr)
    c_o, R_o, rho_o, cnt_o, m_o = c.clone(), Rr.clone(), rho.clone(), cnt.clone(), torch.zeros_like(m)
    c_o[lb, lp] = c1
    rho_o[lb, lp] = (rho[lb, lp] + m_l) + R_l * reached
    R_o[lb, lp] = R_l - nr * hh[live]
    cnt_o[lb, lp] = cnt[lb, lp] + nr
    m_o[lb, lp] = nr
    w = torch.zeros_like(h)
    w[live] = w_l
    flags = torch.zeros(R_rows, dtype=torch.long)
    flags[live] = (reached != 0).long() * REACHED + (nr != 0).long() * NOT_REACHED + (m_l != 0).long() * LIVE + \
        ((nr == 0).long() * MERGED if not last else 0)
    flags[~live] = REP
    h_part = torch.zeros(B, dtype=y.dtype)
    h_part.index_add_(0, lb, h[live])
    h_part.index_add_(0, img[~live], h[~live] * nh[img[~live]].to(y.dtype))
    acc_o, ycls = acc.clone(), torch.zeros_like(acc)
    rows = torch.arange(R_rows)
    is_cls = live & (pos < n_cls)
    acc_o[img[is_cls], pos[is_cls]] = acc[img[is_cls], pos[is_cls]] + y[is_cls] * w[is_cls, None]
    ycls[img[is_cls], pos[is_cls]] = y[is_cls]
    out = {"state": (c_o, R_o, rho_o, cnt_o, m_o), "acc": acc_o, "h_part": h_part, "sv": torch.stack([h, w, flags.to(y.dtype)]), "ycls": ycls,
           "seg": seg, "nh": nh, "pos": pos, "last": bool(last), "S": S, "gate_scale": gate_scale}
    if last:
        return out
    keep = live.clone()
    keep[live] = nr != 0
    x_next, rs, lm, pos_n, src, seg_n, nh_n = [], [], [], [], [], [0], []
    for b in range(B):
        s0 = int(seg[b])
        kept = rows[(img == b) & keep]
        n = S - len(kept)
        x_next.append(y[kept])
        rs += [1.0] * len(kept)
        lm += [0.0] * len(kept)
        pos_n += pos[kept].tolist()
        src += (kept - s0).tolist()
        if n > 0:
            x_next.append(torch.zeros(1, D, dtype=y.dtype))
            rs.append(0.0); lm.append(math.log(n)); pos_n.append(-1); src.append(-1)
        nh_n.append(n)
        seg_n.append(len(rs))
    seg_n = torch.tensor(seg_n)
    out.update(x_next=torch.cat(x_next), rs_next=torch.tensor(rs, dtype=y.dtype), lm_next=torch.tensor(lm, dtype=y.dtype), pos_next=torch.tensor(pos_n),
               src_next=torch.tensor(src), seg_next=seg_n, nh_next=torch.tensor(nh_n), totals=(int(seg_n[-1]), int((seg_n[1:] - seg_n[:-1]).max())))
    return out


def pack_step_bwd(st, g_next, gR, grho, gacc, gh, G):
    """Backward of pack_step_fwd from what it returned (`st`): g_next [R', D] the gradient of x_next (None when last), gR / grho [B, S], gacc
    [B, n_cls, D], gh the gradient of the layer's score mean(h[1:]) (a 0-dim tensor or None), G [B] the per-image sum of the later layers' score terms
    of a halted token.  Returns (dy [R, D], dR [B, S], G_new [B]); the gradients of rho and acc pass through."""
    h, w, fl = st["sv"][0], st["sv"][1], st["sv"][2].long()
    seg, nh, pos, last, S, gscale = st["seg"], st["nh"], st["pos"], st["last"], st["S"], st["gate_scale"]
    R_rows, B, n_cls = h.numel(), len(nh), gacc.shape[1]
    D = gacc.shape[2]
    dt = h.dtype
    img = _row_image(seg, R_rows)
    gs = torch.zeros(B, dtype=dt)
    if gh is not None and B > 1:
        gs[1:] = gh.to(dt) / ((B - 1) * S)
    gate = h * (1 - h) * gscale
    dy = torch.zeros(R_rows, D, dtype=dt)
    dR = gR.clone()
    G_new = G.clone()
    for b in range(B):
        s0, s1 = int(seg[b]), int(seg[b + 1])
        inv = {}
        if not last:
            d0, d1 = int(st["seg_next"][b]), int(st["seg_next"][b + 1])
            for j in range(d0, d1):
                if int(st["src_next"][j]) >= 0:
                    inv[int(st["src_next"][j])] = j
        if int(pos[s1 - 1]) < 0:
            G_new[b] = G[b] + gs[b] * gate[s1 - 1]
            dy[s1 - 1, 0] = nh[b].to(dt) * G_new[b]
        for r in range(s0, s1):
            p = int(pos[r])
            if p < 0:
                continue
            reached, nr = float((fl[r] & REACHED) != 0), float((fl[r] & NOT_REACHED) != 0)
            if not last and (r - s0) in inv:
                dy[r] = g_next[inv[r - s0]]
            elif not last:
                dy[r, 0] = G[b]
            dot = dy.new_zeros(())
            if p < n_cls:
                dot = (gacc[b, p] * st["ycls"][b, p]).sum()
                dy[r] = dy[r] + gacc[b, p] * w[r]
            dh = gs[b] + (0.0 if last else nr * (dot - gR[b, p]))
            dy[r, 0] = dy[r, 0] + dh * gate[r]
            dR[b, p] = gR[b, p] + grho[b, p] * reached + reached * dot
    return dy, dR, G_new


def packed_block(blk, x, m, seg, log_mult):
    """An AViTBlock on packed rows x [R, D]: x1 = x + MHA(m * LN1(x)) with the keys of a segment weighted by exp(log_mult), out = x1 + MLP(m * LN2(x1))."""
    mha = blk.self_attention.self_attention
    H = mha.num_heads
    R, D = x.shape
    dh = D // H
    h1 = blk.ln_1(x) * m[:, None]
    q, k, v = torch.nn.functional.linear(h1, mha.in_proj_weight, mha.in_proj_bias).view(R, 3, H, dh).unbind(1)
    att = []
    for b in range(len(seg) - 1):
        s0, s1 = int(seg[b]), int(seg[b + 1])
        s = torch.einsum("qhd,khd->hqk", q[s0:s1], k[s0:s1]) * dh ** -0.5 + log_mult[s0:s1][None, None, :]
        att.append(torch.einsum("hqk,khd->qhd", torch.softmax(s, dim=-1), v[s0:s1]).reshape(s1 - s0, D))
    x1 = x + torch.nn.functional.linear(torch.cat(att), mha.out_proj.weight, mha.out_proj.bias)
    return x1 + blk.mlp(blk.ln_2(x1) * m[:, None])


def packed_model_step(model, x, labels, kind, counter=None):
    """One training step of the A-ViT `model` on packed rows, free-running or replaying the decisions of `counter` (dense.model_forward's convention):
    forward layer by layer, the loss on leaves (accumulated class rows, rho, layer scores), then the backward walked by hand from the last layer to the
    first - pack_step_bwd, autograd through packed_block only.  Returns (logits, rho, [scores], counter_token, {parameter name: gradient or None}, rows
    per layer)."""
    enc = model.encoder
    dt = enc.pos_embedding.dtype
    tok = model._composite_tokens(x.to(dt)) + enc.pos_embedding
    B, S, D = tok.shape
    n_cls, L = model.num_class_tokens, len(enc.layers)
    thr = float(torch.tensor(1 - enc.eps, dtype=torch.float32))
    seg, nh, pos, rs, lm = initial_tables(B, S)
    rs, lm = rs.to(dt), lm.to(dt)
    state = (tok.new_zeros(B, S), tok.new_ones(B, S), tok.new_zeros(B, S), tok.new_ones(B, S), tok.new_ones(B, S))
    acc = tok.new_zeros(B, n_cls, D)
    xs = tok.detach().reshape(B * S, D).clone().requires_grad_(True)
    layers, rows = [], []
    for i, blk in enumerate(enc.layers):
        y = packed_block(blk, xs, rs, seg, lm)
        replay = None if counter is None else (counter.to(dt) - 1 > i)
        st = pack_step_fwd(y.detach(), seg, nh, pos, state, acc, blk.gate_scale, blk.gate_center, thr, i == L - 1, replay)
        layers.append((blk, xs, y, st))
        rows.append(xs.shape[0])
        state, acc = st["state"], st["acc"]
        if i < L - 1:
            seg, nh, pos, rs, lm = st["seg_next"], st["nh_next"], st["pos_next"], st["rs_next"], st["lm_next"]
            xs = st["x_next"].clone().requires_grad_(True)
    acc_l, rho_l = acc.clone().requires_grad_(True), state[2].clone().requires_grad_(True)
    scores = [(st["h_part"][1:].sum() / ((B - 1) * S) if B > 1 else tok.new_full((), float("nan"))).clone().requires_grad_(True) for *_, st in layers]
    logits = model.head(enc.ln(acc_l).sum(dim=1))
    loss = dense.loss_terms(kind, logits, labels, rho_l, scores)
    params = dict(model.named_parameters())
    grads = {n: None for n in params}

    def add(names, gs_):
        for n, g in zip(names, gs_):
            if g is not None:
                grads[n] = g if grads[n] is None else grads[n] + g

    tail = [n for n in params if n.startswith("head.") or n.startswith("encoder.ln.")]
    got = torch.autograd.grad(loss, [acc_l, rho_l, *scores] + [params[n] for n in tail], allow_unused=True)
    gacc = got[0] if got[0] is not None else torch.zeros_like(acc_l)
    grho = got[1] if got[1] is not None else torch.zeros_like(rho_l)
    gsc = got[2:2 + L]
    add(tail, got[2 + L:])
    gR, G, g_next = torch.zeros_like(rho_l), tok.new_zeros(B), None
    for i in range(L - 1, -1, -1):
        blk, xs, y, st = layers[i]
        dy, gR, G = pack_step_bwd(st, g_next, gR, grho, gacc, gsc[i], G)
        names = [f"encoder.layers.{i}.{n}" for n, _ in blk.named_parameters()]
        got = torch.autograd.grad(y, [xs] + [params[n] for n in names], dy, allow_unused=True)
        g_next = got[0]
        add(names, got[1:])
    stem = [n for n in params if not n.startswith("encoder.layers.") and n not in tail]
    add(stem, torch.autograd.grad(tok, [params[n] for n in stem], g_next.view(B, S, D), allow_unused=True))
    return logits.detach(), state[2], [s.detach() for s in scores], state[3], grads, rows
