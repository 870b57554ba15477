"""Dropout on the training path on the GPU (include/peekvit_hip_dropout.h), in both operand builds: the mask bits against the
numpy generator, the three row kernels per element, the DROP instantiations of the streaming attention kernels per row against fp64 on the reference
mask (the level set by tests/dropout_ref.py's restatement, never by the kernels), p = 0 bit identity, keying, and one training step of
VisionTransformer / RankVisionTransformer with the switch on against an fp64 composite that replays the pass's `dropout_record`."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attn_backward_ref as R
import dropout_ref as DR
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = ["bf16", "f16"]
KEY, SITE = 0xC3A5C85C97CB3127, 7          # (a key above 2^63: the arguments are unsigned)
NAN = float("nan")


def _mask(key, site, shape, p):
    return DR.keep_tensor(key, site, shape, p, DEV, torch.bool)


# ---------------------------------------------------------------------------------------------------------------------------------
# the mask
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_mask_bits_equal_the_numpy_generator(mode):
    from peekvit_amd import engine, ops
    with engine.precision(mode):
        for rows, cols, p in ((2 * 3 * 77, 77, 0.1), (2 * 197, 197, 0.5), (70, 192, 0.1), (70, 192, 0.9), (5, 7, 0.0)):
            got = ops.dropout_keep(KEY, SITE, rows, cols, p, DEV)
            want = DR.keep_mask(KEY, SITE, rows, cols, p)
            assert got.shape == (rows, cols) and np.array_equal(got.cpu().numpy(), want), (rows, cols, p)
            assert 0 < want.mean() <= 1.0
        assert not torch.equal(ops.dropout_keep(KEY, SITE, 70, 192, 0.5, DEV), ops.dropout_keep(KEY, SITE + 1, 70, 192, 0.5, DEV))
        assert not torch.equal(ops.dropout_keep(KEY, SITE, 70, 192, 0.5, DEV), ops.dropout_keep(KEY + 1, SITE, 70, 192, 0.5, DEV))


# ---------------------------------------------------------------------------------------------------------------------------------
# the row kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("mode", MODES)
def test_row_kernels(mode, p):
    from peekvit_amd import _lib, engine, ops
    sc = DR.scale(p)
    with engine.precision(mode):
        dt = _lib.operand_dtype()
        for rows in (1, 70):
            for D in (64, 192, 1024):
                g = torch.Generator(device="cuda").manual_seed(rows * 10000 + D)
                x = torch.randn(rows, D, generator=g, device=DEV)
                u = torch.randn(rows, D, generator=g, device=DEV).to(dt)
                keep = _mask(KEY, SITE, (rows, D), p)
                kd = keep.double()
                tag = f"{mode} p {p} [{rows}, {D}]"
                # ---- pv_dropout_f32: one extra row behind the result, NaN before the launch ----
                out_p = torch.full((rows + 1, D), NAN, device=DEV)
                ops.dropout_f32(x, out_p[:rows], KEY, SITE, p)
                ref = x.double() * kd * sc
                assert torch.isnan(out_p[rows:]).all(), tag
                assert ((out_p[:rows].double() - ref).abs() <= 2.0 ** -22 * ref.abs()).all(), tag
                assert (out_p[:rows][~keep] == 0).all(), tag
                xa = x.clone()
                ops.dropout_f32(xa, xa, KEY, SITE, p)                                   # in place
                assert torch.equal(xa, out_p[:rows]), tag
                # ---- pv_dropout_residual ----
                res_p = torch.full((rows + 1, D), NAN, device=DEV)
                ops.dropout_residual(x, u, res_p[:rows], KEY, SITE, p)
                ref = x.double() + u.double() * kd * sc
                assert torch.isnan(res_p[rows:]).all(), tag
                assert ((res_p[:rows].double() - ref).abs() <= 2.0 ** -22 * ref.abs()).all(), tag
                assert torch.equal(res_p[:rows][~keep], x[~keep]), tag
                xa = x.clone()
                ops.dropout_residual(xa, u, xa, KEY, SITE, p)
                assert torch.equal(xa, res_p[:rows]), tag
                if p == 0.0:
                    assert torch.equal(out_p[:rows], x) and torch.equal(res_p[:rows], x + u.float()), tag
                # ---- pv_dropout_bwd16: round16 of the fp32 product, exactly; its column sums ----
                du_p = torch.full((rows + 1, D), NAN, dtype=dt, device=DEV)
                ops.dropout_bwd16(u, du_p[:rows], KEY, SITE, p)
                want = torch.where(keep, u.float() * torch.tensor(sc, dtype=torch.float32, device=DEV), torch.zeros((), device=DEV)).to(dt)
                assert torch.isnan(du_p[rows:].float()).all(), tag
                assert torch.equal(du_p[:rows], want), tag
                cs = ops.colsum(du_p[:rows].contiguous(), torch.full((D,), NAN, device=DEV))
                ref = du_p[:rows].double().sum(0)
                assert (cs.double() - ref).abs().max() <= 1e-6 * ref.abs().max() + 1e-30, tag
        with pytest.raises(_lib.PeekvitHipError):
            ops.dropout_bwd16(u, u, KEY, SITE, p)                                       # out of place only
        with pytest.raises(_lib.PeekvitHipError):
            ops.dropout_f32(x, torch.empty_like(x), KEY, SITE, 1.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the attention kernels
# ---------------------------------------------------------------------------------------------------------------------------------
S_LIST = (1, 3, 63, 64, 65, 130, 197)
B_, H_ = 2, 2
_CACHE = {}


def _run(dh, S, p, mode, key=KEY, site=SITE, B=B_, H=H_):
    """One forward and one backward of the DROP entry points with their references (computed once, read by the forward and the backward test)."""
    ck = (dh, S, p, mode, key, site, B, H)
    if ck in _CACHE:
        return _CACHE[ck]
    from peekvit_amd import _lib, engine, ops
    D, qscale, nb = H * dh, dh ** -0.5, (S + 63) // 64
    with engine.precision(mode):
        dt = _lib.operand_dtype()
        qkv, dout = R.inputs(B, S, H, dh, dt, device="cuda", seed=1000 * dh + S)          # distinct data in every (image, head)
        out_p = torch.full((B * S + 1, D), NAN, dtype=dt, device=DEV)
        lse_p = torch.full((B * H + 1, S), NAN, device=DEV)
        out, lse = out_p[:B * S].view(B, S, D), lse_p[:B * H].view(B, H, S)
        ops.attention_stream_drop(qkv, out, lse, B, S, H, dh, p, key, site)
        out0, lse0 = torch.empty_like(out), torch.empty_like(lse)
        ops.attention_stream(qkv, out0, lse0, B, S, H, dh)
        g_p = torch.full((B * S + 1, 3 * D), NAN, dtype=dt, device=DEV)
        dbp_p = torch.full((B * nb + 1, 3 * D), NAN, device=DEV)
        dl_p = torch.full((B * H + 1, S), NAN, device=DEV)
        ops.attention_stream_bwd16_drop(qkv, dout, out, lse, g_p[:B * S].view(B, S, 3 * D), B, S, H, dh, qscale, p, key, site,
                                        dbias_partial=dbp_p[:B * nb].view(B, nb, 3 * D), delta_ws=dl_p[:B * H].view(B, H, S))
        torch.cuda.synchronize()
    mask = DR.attention_mask(key, site, B, H, S, p, DEV)
    ref_out, ref_lse, ref_g = DR.fp64_attention(qkv, dout, mask, p, B, S, H, dh, qscale)
    r = dict(qkv=qkv, dout=dout, mask=mask, out_p=out_p, lse_p=lse_p, out0=out0, lse0=lse0, g_p=g_p, dbp_p=dbp_p, dl_p=dl_p, ref_out=ref_out, ref_lse=ref_lse,
             ref_g=ref_g, rs_out=DR.restated_forward(qkv, mask, p, B, S, H, dh)[0], rs_g=DR.restated_backward(qkv, dout, mask, p, B, S, H, dh, qscale))
    _CACHE[ck] = r
    return r


def _cases(ps):
    return [(S, p) for p in ps for S in S_LIST] + [(3, 0.9)]


@pytest.mark.parametrize("dh", [32, 48, 64])
@pytest.mark.parametrize("mode", MODES)
def test_attention_forward_rows(mode, dh):
    B, H = B_, H_
    bad = []
    for S, p in _cases((0.1, 0.5)):
        r = _run(dh, S, p, mode)
        out, lse = r["out_p"][:B * S].view(B, S, H * dh), r["lse_p"][:B * H].view(B, H, S)
        label = f"forward {mode} dh {dh} S {S} p {p}"
        assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all(), label
        assert torch.isnan(r["out_p"][B * S:].float()).all() and torch.isnan(r["lse_p"][B * H:]).all(), label          # nothing is stored past the last row
        assert torch.equal(lse, r["lse0"]), label                                          # the softmax is of all keys: the dropout-free entry's bits
        dead = ~r["mask"].any(-1)
        assert (R.heads(out, B, S, H, dh)[dead] == 0).all(), label                          # fully dropped rows: exactly 0
        bad += R.row_condition(label, R.forward_row_errors(out, r["ref_out"], B, S, H, dh), R.forward_row_errors(r["rs_out"], r["ref_out"], B, S, H, dh), prefix="")
    assert not bad, bad


def _grad_row_errors(got, ref, B, S, H, dh):
    """attn_backward_ref.row_errors; a third whose fp64 gradient is identically zero (dq and dk at S = 1: one key, dS = 0) has no row norm to be
    relative to, so its rows are measured against the rms row norm of the dv third - the same scale for the kernel and the restatement."""
    D = H * dh
    e = R.row_errors(got, ref, B, S, H, dh)
    for i, name in enumerate(R.THIRDS):
        if float(ref[..., i * D:(i + 1) * D].abs().max()) == 0.0:
            unit = R.heads(ref[..., 2 * D:], B, S, H, dh).norm(dim=-1).square().mean().sqrt().clamp_min(1e-300)
            e[name] = R.heads(got[..., i * D:(i + 1) * D].double(), B, S, H, dh).norm(dim=-1) / unit
    return e


@pytest.mark.parametrize("dh", [32, 48, 64])
@pytest.mark.parametrize("mode", MODES)
def test_attention_backward_rows(mode, dh):
    B, H = B_, H_
    D = H * dh
    bad = []
    for S, p in _cases((0.1, 0.5)):
        r = _run(dh, S, p, mode)
        nb = (S + 63) // 64
        label = f"backward {mode} dh {dh} S {S} p {p}"
        got16 = r["g_p"][:B * S].view(B, S, 3 * D)
        got = got16.float()
        assert torch.isfinite(got).all() and torch.isnan(r["g_p"][B * S:].float()).all(), label
        assert torch.isfinite(r["dbp_p"][:B * nb]).all() and torch.isnan(r["dbp_p"][B * nb:]).all(), label
        assert torch.isfinite(r["dl_p"][:B * H]).all() and torch.isnan(r["dl_p"][B * H:]).all(), label
        dead = ~r["mask"].any(-1)
        assert (R.heads(got[..., :D], B, S, H, dh)[dead] == 0).all(), label                 # a fully dropped row: dS = 0, no NaN
        bad += R.row_condition(label, _grad_row_errors(got, r["ref_g"], B, S, H, dh), _grad_row_errors(r["rs_g"], r["ref_g"], B, S, H, dh))
        whole = rel_l2(got, r["ref_g"])
        print(f"{label}: whole tensor rel L2 {whole:.3g} (restated {rel_l2(r['rs_g'], r['ref_g']):.3g}, cap {R.CAP[mode]})")
        assert whole < R.CAP[mode], (label, whole)
        # the bias partial rows: column sums of the STORED values per block of 64 rows of an image
        pad = torch.zeros((B, nb * 64, 3 * D), dtype=torch.float64, device=DEV)
        pad[:, :S] = got16.double()
        ref = pad.view(B, nb, 64, 3 * D).sum(2)
        assert (r["dbp_p"][:B * nb].view(B, nb, 3 * D).double() - ref).abs().max() <= 1e-6 * ref.abs().max() + 1e-30, label
        # delta = rowsum(dO o O) of the stored output
        out = r["out_p"][:B * S].view(B, S, H, dh)
        delta64 = (r["dout"].view(B, S, H, dh).double() * out.double()).sum(-1).permute(0, 2, 1)
        assert (r["dl_p"][:B * H].view(B, H, S).double() - delta64).abs().max() <= 1e-5 * delta64.abs().max() + 1e-30, label
    assert not bad, bad


@pytest.mark.parametrize("mode", MODES)
def test_the_fully_dropped_fixture_on_the_gpu(mode):
    f = DR.FULL_DROP
    B, H, S, dh, p = f["B"], f["H"], f["S"], f["dh"], f["p"]
    r = _run(dh, S, p, mode, key=f["key"], site=f["site"], B=B, H=H)
    dead = ~r["mask"].any(-1)
    assert dead.any() and (~dead).any()
    out, got = r["out_p"][:B * S].view(B, S, H * dh), r["g_p"][:B * S].view(B, S, 3 * H * dh).float()
    assert torch.isfinite(out.float()).all() and torch.isfinite(got).all()
    assert (R.heads(out, B, S, H, dh)[dead] == 0).all() and (R.heads(got[..., :H * dh], B, S, H, dh)[dead] == 0).all()
    assert (R.heads(out, B, S, H, dh)[~dead] != 0).any()


@pytest.mark.parametrize("shape", [(2, 3, 2, 32), (2, 65, 3, 48), (2, 197, 2, 64)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", MODES)
def test_p_zero_gives_the_dropout_free_bits(mode, shape):
    from peekvit_amd import _lib, engine, ops
    B, S, H, dh = shape
    D, nb, qscale = H * dh, (S + 63) // 64, dh ** -0.5
    with engine.precision(mode):
        dt = _lib.operand_dtype()
        qkv, dout = R.inputs(B, S, H, dh, dt, device="cuda")
        res = []
        for drop in (False, True):
            out, lse = torch.empty((B, S, D), dtype=dt, device=DEV), torch.empty((B, H, S), device=DEV)
            g, dbp, dl = torch.empty((B, S, 3 * D), dtype=dt, device=DEV), torch.empty((B, nb, 3 * D), device=DEV), torch.empty((B, H, S), device=DEV)
            if drop:
                ops.attention_stream_drop(qkv, out, lse, B, S, H, dh, 0.0, KEY, SITE)
                ops.attention_stream_bwd16_drop(qkv, dout, out, lse, g, B, S, H, dh, qscale, 0.0, KEY, SITE, dbias_partial=dbp, delta_ws=dl)
            else:
                ops.attention_stream(qkv, out, lse, B, S, H, dh)
                ops.attention_stream_bwd16(qkv, dout, out, lse, g, B, S, H, dh, qscale, dbias_partial=dbp, delta_ws=dl)
            res.append((out, lse, g, dbp, dl))
    for a, b, name in zip(res[0], res[1], ("out", "lse", "dqkv16", "dbias_partial", "delta")):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("mode", MODES)
def test_determinism_and_keying(mode):
    dh, S, p = 32, 130, 0.5
    a = _run(dh, S, p, mode)
    _CACHE.pop((dh, S, p, mode, KEY, SITE, B_, H_))
    b = _run(dh, S, p, mode)                                   # the same (key, site) again: identical bits
    for name in ("out_p", "lse_p", "g_p", "dbp_p", "dl_p"):
        assert torch.equal(a[name][:-1], b[name][:-1]), name
    for other in (_run(dh, S, p, mode, key=KEY + 1), _run(dh, S, p, mode, site=SITE + 1)):
        assert not torch.equal(a["mask"], other["mask"])
        assert not torch.equal(a["out_p"][:-1], other["out_p"][:-1]) and not torch.equal(a["g_p"][:-1], other["g_p"][:-1])
        assert torch.equal(a["lse_p"][:-1], other["lse_p"][:-1])


# ---------------------------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------------------------
CFG = dict(image_size=32, patch_size=8, num_layers=2, num_heads=2, hidden_dim=64, mlp_dim=128, num_classes=10)
PRECISION = {"bf16": "bf16", "f16": "auto"}                  # a model-level training pass runs on fp16 operands in precision mode "auto"


def _make(kind, dropout, attention_dropout, cfg=CFG, seed=3):
    from peekvit_amd.models.rankvit import RankVisionTransformer
    from peekvit_amd.models.vit import VisionTransformer
    torch.manual_seed(seed)
    if kind == "rank":
        m = RankVisionTransformer(**cfg, dropout=dropout, attention_dropout=attention_dropout, rankvit_layers=[1])
        m.set_budget(0.5)
    else:
        m = VisionTransformer(**cfg, dropout=dropout, attention_dropout=attention_dropout)
    with torch.no_grad():
        torch.nn.init.normal_(m.head.weight, std=0.05)        # (the reference's zero head gives the trunk zero gradients)
        torch.nn.init.normal_(m.class_tokens, std=0.02)
        for blk in m.encoder.layers:
            for b_ in (blk.self_attention.self_attention.in_proj_bias, blk.self_attention.self_attention.out_proj.bias, blk.mlp.fc1.bias, blk.mlp.fc2.bias):
                torch.nn.init.normal_(b_, std=0.02)
    return m


def _batch(cfg=CFG, batch=4):
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(batch, 3, cfg["image_size"], cfg["image_size"], generator=g, device=DEV).to(torch.bfloat16).float()
    return x, torch.randint(0, cfg["num_classes"], (batch,), generator=g, device=DEV)


def _hip_step(m, x, y):
    from peekvit_amd import ops, train_engine
    m.zero_grad(set_to_none=True)
    n0 = ops.launch_count
    logits = m(x)
    F.cross_entropy(logits, y).backward()
    torch.cuda.synchronize()
    assert ops.launch_count - n0 > 40, "the HIP training path did not run"
    assert not train_engine.last_step_skipped(m)
    return logits.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def _fp64_step(kind, m, x, y, record, dropout, attention_dropout):
    twin = _make(kind, dropout, attention_dropout).double().to(DEV)
    twin.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    keeps = [blk.last_keep for blk in m.encoder.layers if getattr(blk, "current_budget", 1) != 1]
    logits = DR.model_composite_fp64(twin, x, record, keeps)
    F.cross_entropy(logits, y).backward()
    return logits.detach(), {n: p.grad for n, p in twin.named_parameters()}


@pytest.mark.parametrize("kind", ["vit", "rank"])
@pytest.mark.parametrize("mode", MODES)
def test_training_step_against_the_fp64_replay(mode, kind):
    """Logits and every parameter gradient of one step with dropout 0.1 / attention_dropout 0.1 and the switch on against the fp64 composite replaying the
    pass's dropout_record.  The yardstick is the EXISTING dropout-free HIP path on the same weights and input against ITS fp64 composite: the dropout
    step may measure up to 2 x that error per quantity plus 1e-5 (one more 16-bit rounding of the branch output, the 1 / (1 - p) gain on survivors)."""
    from peekvit_amd import engine, train_engine
    x, y = _batch()
    with engine.precision(PRECISION[mode]):
        base = _make(kind, 0.0, 0.0).to(DEV).train()
        b_logits, b_grads = _hip_step(base, x, y)
        assert train_engine.train_state(base).dropout_record is None
        r_logits, r_grads = _fp64_step(kind, base, x, y, None, 0.0, 0.0)
        m = _make(kind, 0.1, 0.1).to(DEV).train()
        m.load_state_dict(base.state_dict())
        m.set_fused_dropout(True)
        torch.manual_seed(2024)
        d_logits, d_grads = _hip_step(m, x, y)
        key, sites = train_engine.train_state(m).dropout_record
        assert [s[0] for s in sites] == ["input"] + ["attention", "branch"] * 2 and [s[1] for s in sites] == list(range(5)) and 0 <= key < 1 << 64
        q_logits, q_grads = _fp64_step(kind, m, x, y, (key, sites), 0.1, 0.1)
    assert not torch.equal(d_logits, b_logits)                  # dropout happened
    rows = [("logits", rel_l2(d_logits, q_logits), rel_l2(b_logits, r_logits))]
    rows += [(n, rel_l2(d_grads[n], q_grads[n]), rel_l2(b_grads[n], r_grads[n])) for n in d_grads]
    bad = []
    for n, ed, eb in rows:
        print(f"{kind} {mode} {n}: dropout step {ed:.3g}, dropout-free step {eb:.3g}, ratio {ed / max(eb, 1e-30):.3g}")
        if not ed <= 2.0 * eb + 1e-5:
            bad.append((n, ed, eb))
    print(f"{kind} {mode} worst: dropout step {max(r[1] for r in rows):.3g}, dropout-free step {max(r[2] for r in rows):.3g}")
    assert not bad, bad


def _count_mha(monkeypatch):
    calls = []
    orig = F.multi_head_attention_forward
    monkeypatch.setattr(F, "multi_head_attention_forward", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    return calls


DROP_KERNELS = {"pv_dropout_f32", "pv_dropout_residual", "pv_dropout_bwd16", "pv_attention_stream_lse_drop_bf16", "pv_attention_stream_bwd16_drop_bf16"}


@pytest.mark.parametrize("mode", MODES)
def test_dispatch_of_the_switch(mode, monkeypatch):
    from peekvit_amd import engine, ops, train_engine
    x, y = _batch()
    stock = _count_mha(monkeypatch)
    with engine.precision(PRECISION[mode]):
        m = _make("vit", 0.1, 0.1).to(DEV).train()
        # ---- off: the composite, as today ----
        with ops.KernelTimer() as kt:
            F.cross_entropy(m(x), y).backward()
        torch.cuda.synchronize()
        assert len(stock) == 2 and not DROP_KERNELS & set(kt.summary())
        # ---- on: the dropout kernels, no stock attention ----
        m.set_fused_dropout(True)
        del stock[:]
        with ops.KernelTimer() as kt:
            F.cross_entropy(m(x), y).backward()
        torch.cuda.synchronize()
        names = kt.summary()
        assert not stock and DROP_KERNELS <= set(names), sorted(names)
        assert names["pv_dropout_f32"]["launches"] == 2 and names["pv_dropout_residual"]["launches"] == 2 and names["pv_dropout_bwd16"]["launches"] == 2
        assert names["pv_attention_stream_lse_drop_bf16"]["launches"] == 2 and names["pv_attention_stream_bwd16_drop_bf16"]["launches"] == 2
        assert "pv_attention_bwd_bf16" not in names and "pv_attention_bf16" not in names
        # ---- the same seed twice: identical logits and gradients; another forward draws other masks ----
        runs = []
        for seed in (7, 7, 8):
            torch.manual_seed(seed)
            runs.append(_hip_step(m, x, y))
        assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(runs[0][1][n], runs[1][1][n]) for n in runs[0][1])
        assert not torch.equal(runs[0][0], runs[2][0])
        k1 = train_engine.train_state(m).dropout_record[0]
        _hip_step(m, x, y)
        assert train_engine.train_state(m).dropout_record[0] != k1          # two consecutive forwards: different keys
        # ---- p = 1 somewhere, and PEEKVIT_AMD_TRAIN=torch: the path they have today ----
        m.encoder.layers[0].dropout.p = 1.0
        assert not m._fused_dropout_ok(x)
        m.encoder.layers[0].dropout.p = 0.1
        assert m._fused_dropout_ok(x)
        monkeypatch.setenv("PEEKVIT_AMD_TRAIN", "torch")
        assert not m._fused_dropout_ok(x)
        monkeypatch.delenv("PEEKVIT_AMD_TRAIN")
        # ---- a block called on its own (no pass) keeps the composite under dropout ----
        del stock[:]
        t = torch.randn(2, 17, 64, device=DEV, requires_grad=True)
        m.encoder.layers[0](t)
        assert len(stock) == 1
        # ---- eval mode: the inference path, bit for bit what the switch off gives ----
        m.eval()
        with torch.no_grad():
            on = m(x)
            m.set_fused_dropout(False)
            off = m(x)
        assert torch.equal(on, off)


@pytest.mark.parametrize("mode", MODES)
def test_branch_dropout_alone_keeps_the_persistent_attention_backward(mode, monkeypatch):
    """dropout > 0 with attention_dropout = 0 at S = 197: the resident attention pair, hence pv_attention_bwd_lse_bf16, is still what runs."""
    from peekvit_amd import engine, ops
    cfg = dict(image_size=224, patch_size=16, num_layers=1, num_heads=2, hidden_dim=128, mlp_dim=256, num_classes=10)
    calls = []
    orig = ops.attention_bwd_lse
    monkeypatch.setattr(ops, "attention_bwd_lse", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    x, y = _batch(cfg, batch=2)
    with engine.precision(PRECISION[mode]):
        m = _make("vit", 0.1, 0.0, cfg).to(DEV).train()
        m.set_fused_dropout(True)
        with ops.KernelTimer() as kt:
            F.cross_entropy(m(x), y).backward()
        torch.cuda.synchronize()
    names = set(kt.summary())
    assert len(calls) == 1 and {"pv_dropout_f32", "pv_dropout_residual", "pv_dropout_bwd16"} <= names
    assert not {"pv_attention_stream_lse_drop_bf16", "pv_attention_stream_bwd16_drop_bf16"} & names
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())
