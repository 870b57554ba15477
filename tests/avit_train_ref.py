"""fp64 restatements shared by tests/test_avit_train_host.py and tests/test_hip_avit_train.py: A-ViT's halting step (reference models/adavit.py:170-217)
as one differentiable function, the whole composite forward with optional REPLAY of recorded halting decisions, and the literal formulas of the two
A-ViT regularisers (reference utils/losses.py: avit_ponder_loss, avit_distr_prior_loss).  Plain torch, any device, no project code."""
import math

import torch


def act_step(y, c, R, rho, counter, m, acc, gate_scale, gate_center, thr, last, n_cls, nr_replay=None):
    """(x_next, c', R', rho', counter', m', acc', score, h) in the dtype of y.  x_next = y * m' in DATA only (gradient: identity on every row).
    nr_replay: the `not reached` decisions to use instead of the comparison (reached = m * (1 - nr) then)."""
    B, S, _D = y.shape
    h = torch.sigmoid(y[:, :, 0] * gate_scale - gate_center)
    hh = torch.ones_like(h) if last else h
    c1 = c + hh
    if nr_replay is None:
        reached = (c1 > thr).to(y.dtype) * m
        nr = (c1 < thr).to(y.dtype)
    else:
        nr = nr_replay.to(y.dtype)
        reached = m * (1 - nr)
    rho1 = rho + m + R * reached
    R1 = R - nr * hh
    w = m * (R * reached + hh * nr)
    acc1 = acc + y[:, :n_cls] * w[:, :n_cls, None]
    score = h[1:].mean() if B > 1 else h.new_full((), float("nan"))
    x_next = y + (y.detach() * nr[:, :, None] - y.detach())
    return x_next, c1.detach(), R1, rho1, counter + nr, nr, acc1, score, h


def block(blk, x, m):
    """An AViTBlock under the 0/1 mask m [B,S] (1 = running) with stock ops in the block's own dtype."""
    mm = m[:, :, None]
    x = x + blk.self_attention(blk.ln_1(x * mm) * mm)
    return x + blk.mlp(blk.ln_2(x * mm) * mm)


def model_forward(model, x, counter=None):
    """The A-ViT composite in the model's dtype (fp64 after model.double()), free-running or - with `counter`, a [B,S] counter_token - replaying its
    decisions: at layer i  nr = counter - 1 > i,  reached = m * (1 - nr).  Returns (logits, rho_token, [layer scores], counter_token, margin) with
    margin = the smallest |c' - thr| any running token had (free-running: how far the decisions were from flipping)."""
    enc = model.encoder
    dt = enc.pos_embedding.dtype
    tok = model._composite_tokens(x.to(dt)) + enc.pos_embedding
    B, S, D = tok.shape
    n_cls, L = model.num_class_tokens, len(enc.layers)
    thr = float(torch.tensor(1 - enc.eps, dtype=torch.float32))
    c, rho = tok.new_zeros(B, S), tok.new_zeros(B, S)
    R, cnt, m = tok.new_ones(B, S), tok.new_ones(B, S), tok.new_ones(B, S)
    acc = tok.new_zeros(B, n_cls, D)
    scores, margin = [], float("inf")
    for i, blk in enumerate(enc.layers):
        y = block(blk, tok, m)
        replay = None if counter is None else (counter.to(dt) - 1 > i)
        m_in = m
        tok, c, R, rho, cnt, m, acc, score, _h = act_step(y, c, R, rho, cnt, m, acc, blk.gate_scale, blk.gate_center, thr, i == L - 1, n_cls, replay)
        live = m_in > 0
        if live.any():
            margin = min(margin, float((c - thr).abs()[live].min()))
        scores.append(score)
    logits = model.head(enc.ln(acc).sum(dim=1))
    return logits, rho, scores, cnt, margin


def ponder_loss(rho):
    return rho.mean()


def prior_loss(scores, target_depth):
    """KL(target || normalised layer scores), batchmean over the L layers as the reference's kl_div call reduces it (sum / L)."""
    L = len(scores)
    s = torch.stack(list(scores))
    p = (s / s.sum()).clamp(0.001, 0.999)
    k = torch.arange(1, L + 1, dtype=s.dtype, device=s.device)
    log_t = -0.5 * (k - target_depth) ** 2 - 0.5 * math.log(2 * math.pi)
    return (log_t.exp() * (log_t - p.log())).sum() / L


# The micro models have 4 layers: N(11, 1) - the yaml's target for 12-layer models - puts 1e-11 of its mass on layers 1..4, so "prior alone" at that
# target would be a loss of 1e-10 that tests nothing.  Alone, the term is taken at a target inside the model; the combination keeps the yaml's values.
PRIOR_ALONE_DEPTH = 2


def loss_terms(kind, logits, labels, rho, scores, target_depth=11, w_prior=0.2, w_ponder=0.0005):
    """The four losses of the model-level tests: 'ce', 'ponder', 'prior' (target depth PRIOR_ALONE_DEPTH), 'yaml' (configs/loss/avit_losses.yaml's
    combination, its target depth and weights)."""
    ce = torch.nn.functional.cross_entropy(logits, labels)
    if kind == "ce":
        return ce
    if kind == "ponder":
        return ponder_loss(rho)
    if kind == "prior":
        return prior_loss(scores, PRIOR_ALONE_DEPTH)
    assert kind == "yaml"
    return ce + w_prior * prior_loss(scores, target_depth) + w_ponder * ponder_loss(rho)
