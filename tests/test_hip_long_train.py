"""Dense training past 208 token rows on the GPU, in both operand builds: the plain and the masked encoder block with the
streaming attention pair (train_engine._StreamAttn behind attention_pair) against the fp64 composite of the same block, which kernels a step
launches on either side of the two thresholds, one training step of VisionTransformer / RankVisionTransformer / ResidualVisionTransformer at
226 / 227 / 442 rows against the fp64 composite, the ViT step with fused dropout against the fp64 replay of its masks, and bit identity of two runs.

Bounds.  bf16 operands: the block-level bounds the project applies to the training blocks called on their own (tests/test_hip_avit_train.py,
tests/test_hip_backward.py): 1.2e-2 for the forward, 3e-2 for every gradient.  fp16 operands carry 3 more mantissa bits (2^-11 against 2^-8 per
rounding), so the same quantities are bounded at an eighth of that: 1.5e-3 - the bound tests/test_hip_backward.py puts on the fp16 attention
gradients - and 3.75e-3.  On top of that every long-row error must stay below 2 x the error the RESIDENT pair measures on the same weights at its
longest length (208 rows, 416 at head dim 32) against its own fp64 composite, plus 1e-4 (the yardstick form of
test_attention_backward_from_the_forward_statistics).  Model level: the README's training tolerances in fp16 (logits 1e-3, complete gradient 2e-3);
bf16: 2e-2 for the logits and 3e-2 per parameter gradient, as tests/test_hip_backward.py::test_training_step_gradients."""
import copy

import pytest
import torch
import torch.nn.functional as F

import dropout_ref as DR
import test_hip_block_launches as BL
import test_hip_dropout as TD
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = ["bf16", "f16"]
FWD_BOUND = {"bf16": 1.2e-2, "f16": 1.5e-3}
GRAD_BOUND = {"bf16": 3e-2, "f16": 3.75e-3}
MLP_DIM = 128
# (S, D, H): the first length past the resident backward at dh 64 and at dh 48; resident forward with lse + streaming backward; the first streaming
# forward; dh 32 past its bound; seven key blocks plus one row.  dh 48 runs at D = 192 with 4 heads: the block's GEMMs take K % 64 == 0 only
# (pv_gemm_bf16), so two heads of 48 (D = 96) are no shape of this path at any row count
BLOCK_SHAPES = [(209, 128, 2), (209, 192, 4), (416, 128, 2), (417, 128, 2), (417, 64, 2), (449, 128, 2)]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the block
# ---------------------------------------------------------------------------------------------------------------------------------
def _block(D, H):
    """One block per (D, H) - the long rows and the resident yardstick run on the SAME weights - rounded to bf16 so that both operand types read them exactly."""
    from peekvit_amd.models.vit import ViTBlock
    torch.manual_seed(1000 * D + H)
    blk = ViTBlock(H, D, MLP_DIM, 0.0, 0.0)
    with torch.no_grad():
        for n, p in blk.named_parameters():
            if p.dim() == 1 and "ln" in n and "weight" in n:
                p.copy_(1 + 0.2 * torch.randn_like(p))
            elif p.dim() == 1:
                p.copy_(0.1 * torch.randn_like(p))
            p.copy_(p.to(torch.bfloat16).float())
    return blk


def _composite64(blk64, x, m):
    """The block in fp64 (reference models/vit.py:45-55; with a row scale models/residualvit.py:249-260)."""
    mm = 1.0 if m is None else m[..., None]
    x1 = x + mm * blk64.self_attention(mm * blk64.ln_1(x))
    return x1 + blk64.mlp(mm * blk64.ln_2(x1))


def _block_inputs(variant, B, S, D):
    g = torch.Generator().manual_seed(7 * S + D)
    x = torch.randn(B, S, D, generator=g).to(torch.bfloat16).float()
    dout = torch.randn(B, S, D, generator=g)
    m = None
    if variant == "masked":          # ResidualViT's row scale: relu(sigmoid - threshold) on the patch rows (about a third of them 0), 1 on the class and budget rows
        m = torch.relu(torch.rand(B, S, generator=g) - 0.3)
        m[:, 0], m[:, S - 1] = 1.0, 1.0
    return x, dout, m


def _hip_block(variant, S, D, H, mode, B=2):
    """One forward and one backward of the HIP block: {name: tensor on the CPU} of the output, dx, the mask gradient and the twelve parameter gradients,
    and the names of the kernels launched."""
    from peekvit_amd import engine, ops, train_engine as te
    blk = copy.deepcopy(_block(D, H)).to(DEV)
    x, dout, m = _block_inputs(variant, B, S, D)
    xg = x.to(DEV).requires_grad_(True)
    mg = None if m is None else m.to(DEV).requires_grad_(True)
    with engine.precision(mode):
        n0 = ops.launch_count
        with ops.KernelTimer() as kt:
            out = te.block_forward_train(blk, xg) if m is None else te.masked_block_forward_train(blk, xg, mg)
            n_fw = len(kt.records)
            out.backward(dout.to(DEV))
            torch.cuda.synchronize()
        assert ops.launch_count - n0 == len(kt.records) > 20 and len(kt.records) > n_fw > 0, "the HIP block did not run"
    names = [r[0] for r in kt.records]
    res = {"out": out.detach().cpu(), "dx": xg.grad.cpu()}
    if mg is not None:
        res["dm"] = mg.grad.cpu()
    params = list(blk.named_parameters())
    assert len(params) == 12
    for n, p in params:
        assert p.grad is not None, n
        res[n] = p.grad.cpu()
    assert all(torch.isfinite(v).all() for v in res.values())
    return res, names[:n_fw], names[n_fw:]


_REF, _ERR = {}, {}


def _fp64_block(variant, S, D, H, B=2):
    key = (variant, S, D, H)
    if key not in _REF:
        blk64 = copy.deepcopy(_block(D, H)).double()
        x, dout, m = _block_inputs(variant, B, S, D)
        x64 = x.double().requires_grad_(True)
        m64 = None if m is None else m.double().requires_grad_(True)
        out = _composite64(blk64, x64, m64)
        out.backward(dout.double())
        res = {"out": out.detach(), "dx": x64.grad}
        if m64 is not None:
            res["dm"] = m64.grad
        res.update({n: p.grad for n, p in blk64.named_parameters()})
        _REF[key] = res
    return _REF[key]


def _block_errors(variant, S, D, H, mode):
    """{name: relative L2 error against fp64} of one HIP block step, computed once per case."""
    key = (variant, S, D, H, mode)
    if key not in _ERR:
        got, fw, bw = _hip_block(variant, S, D, H, mode)
        ref = _fp64_block(variant, S, D, H)
        assert set(got) == set(ref)
        _ERR[key] = ({n: rel_l2(got[n], ref[n]) for n in ref}, fw, bw)
    return _ERR[key]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant", ["plain", "masked"])
@pytest.mark.parametrize("S,D,H", BLOCK_SHAPES)
def test_block_against_the_fp64_composite(S, D, H, variant, mode):
    """Measured pairs (long rows / the resident yardstick): DESIGN.md section 32."""
    from peekvit_amd import train_engine as te
    dh = D // H
    assert type(te.attention_pair(2, S, dh)) is te._StreamAttn
    s_res = te.resident_rows(dh)
    errs, _fw, bw = _block_errors(variant, S, D, H, mode)
    base, _fw0, bw0 = _block_errors(variant, s_res, D, H, mode)
    assert "pv_attention_stream_bwd16_bf16" in bw and "pv_attention_bwd_bf16" not in bw
    assert "pv_attention_bwd_bf16" in bw0 and "pv_attention_stream_bwd16_bf16" not in bw0
    assert len(errs) == (15 if variant == "masked" else 14)
    bad = []
    for n, e in errs.items():
        bound = FWD_BOUND[mode] if n == "out" else GRAD_BOUND[mode]
        print(f"{variant} {mode} S {S} D {D} H {H} {n}: {e:.3g} (resident at S {s_res}: {base[n]:.3g}, bound {bound})")
        if not (e < bound and e < 2.0 * base[n] + 1e-4):
            bad.append((n, e, base[n], bound))
    print(f"{variant} {mode} S {S} D {D} H {H} worst: {max(errs.values()):.3g} (resident at S {s_res}: {max(base.values()):.3g})")
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. dispatch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_launches_at_197_rows_are_what_they_were():
    """The launch lists of tests/test_hip_block_launches.py were recorded before the block functions were folded into one body - two commits before the
    streaming pair existed - and that file asserts them on the commit this change starts from; they are taken from there, not from this code."""
    for variant in ("block", "masked"):
        fw, bw, _out, _dx, _dm, _blk = BL.run_case(variant, 2, 197, 192, 3)
        assert fw == BL.EXPECTED[variant][0], fw
        assert bw == BL.EXPECTED[variant][1], bw


@pytest.mark.parametrize("mode", MODES)
def test_kernels_on_either_side_of_the_thresholds(mode):
    names = {S: _block_errors("plain", S, 128, 2, mode)[1:] for S in (208, 209, 416, 417)}
    fw, bw = names[208]
    assert "pv_attention_bf16" in fw and "pv_attention_bwd_bf16" in bw and not any("stream" in n for n in fw + bw)
    fw, bw = names[209]          # the first length past the resident backward: no pv_attention_bwd_bf16, the streaming backward instead
    assert "pv_attention_stream_bwd16_bf16" in bw and "pv_attention_bwd_bf16" not in bw
    assert "pv_attention_bf16" in fw and "pv_attention_stream_lse_bf16" not in fw
    fw, bw = names[416]          # the resident forward still, keeping its row statistics
    assert "pv_attention_bf16" in fw and "pv_attention_stream_lse_bf16" not in fw and "pv_attention_stream_bwd16_bf16" in bw
    fw, bw = names[417]          # the streaming forward
    assert "pv_attention_stream_lse_bf16" in fw and "pv_attention_bf16" not in fw and "pv_attention_stream_bwd16_bf16" in bw
    assert fw.count("pv_attention_stream_lse_bf16") == 1 and bw.count("pv_attention_stream_bwd16_bf16") == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. determinism
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant", ["plain", "masked"])
def test_two_runs_give_identical_bits(variant, mode):
    a, _, _ = _hip_block(variant, 417, 128, 2, mode)
    b, _, _ = _hip_block(variant, 417, 128, 2, mode)
    assert set(a) == set(b)
    for n in a:
        assert torch.equal(a[n], b[n]), n


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the models
# ---------------------------------------------------------------------------------------------------------------------------------
CFG_227 = dict(image_size=120, patch_size=8, num_layers=2, num_heads=2, hidden_dim=128, mlp_dim=256, num_classes=10)          # 226 rows (227 with a budget token)
CFG_RANK3 = dict(CFG_227, num_layers=3)          # a ranked layer 1 of 3: block 0 streams 226 rows, block 1 keeps 114 on the resident pair, block 2 is the class-row block
CFG_442 = dict(image_size=168, patch_size=8, num_layers=2, num_heads=2, hidden_dim=64, mlp_dim=128, num_classes=10)            # head dim 32, 442 rows
MODEL_CASES = {"vit": ("vit", CFG_227), "rank": ("rank", CFG_227), "rank3": ("rank", CFG_RANK3), "vit_dh32": ("vit", CFG_442)}


def _timed_hip_step(m, x, y):
    from peekvit_amd import ops
    with ops.KernelTimer() as kt:
        logits, grads = TD._hip_step(m, x, y)          # (asserts that ops.launch_count rose by more than 40 and that the step was not skipped)
    return logits, grads, kt.summary()


def _fp64_step(kind, cfg, m, x, y, record=None, p=(0.0, 0.0)):
    twin = TD._make(kind, p[0], p[1], cfg).double().to(DEV)
    twin.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    keeps = [blk.last_keep for blk in m.encoder.layers if getattr(blk, "current_budget", 1) != 1]
    logits = DR.model_composite_fp64(twin, x, record, keeps)
    F.cross_entropy(logits, y).backward()
    return logits.detach(), {n: p_.grad for n, p_ in twin.named_parameters()}


def _complete(grads, names):
    return torch.cat([grads[n].double().reshape(-1).cpu() for n in names])


def _check_model(tag, mode, logits, grads, ref_logits, ref_grads):
    names = list(ref_grads)
    assert set(grads) == set(names)
    e_log = rel_l2(logits, ref_logits)
    e_all = rel_l2(_complete(grads, names), _complete(ref_grads, names))
    worst = max((rel_l2(grads[n], ref_grads[n]), n) for n in names)
    print(f"{tag} {mode}: logits {e_log:.3g}, complete gradient {e_all:.3g}, worst parameter gradient {worst[0]:.3g} ({worst[1]})")
    if mode == "f16":
        assert e_log < 1e-3 and e_all < 2e-3, (tag, e_log, e_all)
    else:
        assert e_log < 2e-2 and worst[0] < 3e-2, (tag, e_log, worst)
    return e_log, e_all


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_vit_and_rankvit_training_step_against_the_fp64_composite(case, mode):
    from peekvit_amd import engine, train_engine as te
    kind, cfg = MODEL_CASES[case]
    x, y = TD._batch(cfg, batch=2)
    with engine.precision(TD.PRECISION[mode]):
        m = TD._make(kind, 0.0, 0.0, cfg).to(DEV).train()
        assert not te.resident_rows(cfg["hidden_dim"] // cfg["num_heads"]) >= m.seq_length
        logits, grads, names = _timed_hip_step(m, x, y)
        ref_logits, ref_grads = _fp64_step(kind, cfg, m, x, y)
    L = cfg["num_layers"]
    assert names["pv_attention_rows_bwd_bf16"]["launches"] == 1                          # the last block: the class row only, at any row count
    if case == "rank3":          # 226 rows stream, the 114 kept rows behind the ranked layer take the resident pair
        assert m.encoder.layers[1].last_keep.shape == (2, 113)
        assert names["pv_attention_stream_bwd16_bf16"]["launches"] == 1 and names["pv_attention_bwd_bf16"]["launches"] == 1
    else:
        assert names["pv_attention_stream_bwd16_bf16"]["launches"] == L - 1 and "pv_attention_bwd_bf16" not in names
    assert ("pv_attention_stream_lse_bf16" in names) == (m.seq_length > 416)
    _check_model(case, mode, logits, grads, ref_logits, ref_grads)


# ---- ResidualViT: sigmoid gates, learnable budget token; the fp64 composite is the model itself in double on the CPU ----
RESIDUAL_SEED, RESIDUAL_BUDGETS, KNEE = 2, [0.3, 0.8], 1e-3          # (the seed was picked on the CPU so that no token sits within KNEE of a gate's knee: asserted below)


def _residual_case():
    import residual_sparse_ref as R
    import test_residual_sparse_train_host as host
    from peekvit_amd import synth
    from peekvit_amd.models.residualvit import ResidualVisionTransformer
    cfg = dict(CFG_227, **host.EXTRA, gate_bias=0.0)
    m64 = ResidualVisionTransformer(**cfg).double()
    m64.load_state_dict(R.sparse_sd(cfg, 4.0, torch.float64, seed=RESIDUAL_SEED))
    m64.train()
    bud = torch.tensor(RESIDUAL_BUDGETS, dtype=torch.float64)
    m64._sample_budget = lambda n: bud.clone()
    x = torch.from_numpy(synth.synth_images(2, cfg["image_size"], seed=RESIDUAL_SEED)).double()
    return cfg, m64, x, torch.arange(2) % cfg["num_classes"]


@pytest.mark.parametrize("mode", MODES)
def test_residualvit_training_step_against_the_fp64_composite(mode):
    import test_hip_residual_sparse_train as RT
    import test_residual_sparse_train_host as host
    from peekvit_amd import engine, ops, train_engine as te
    cfg, m64, x, y = _residual_case()
    assert m64.seq_length + 1 == 227
    ref_loss, ref_logits, ref_masks, ref_grads = host.dense_step(m64, x, y)
    ref_grads = {k: (torch.zeros_like(p) if ref_grads[k] is None else ref_grads[k]) for k, p in m64.named_parameters()}
    margins = RT._margins(m64, x)
    assert all(float(mg.min()) >= KNEE for mg in margins), [float(mg.min()) for mg in margins]
    assert all(0.2 < float((mk == 0).double().mean()) < 0.95 for mk in ref_masks)          # the gates mask, and not everything
    with engine.precision(TD.PRECISION[mode]):
        m = RT._gpu_model(cfg, m64, RESIDUAL_BUDGETS)
        n0 = ops.launch_count
        with ops.KernelTimer() as kt:
            loss, logits, masks, _thrs, grads = RT._gpu_step(m, x.float().to(DEV), y.to(DEV))
        assert ops.launch_count - n0 > 40, "the HIP training path did not run"
        assert not te.last_step_skipped(m)
    names = kt.summary()
    assert names["pv_residual_gate"]["launches"] == 2 == names["pv_residual_gate_bwd"]["launches"]
    assert names["pv_attention_stream_bwd16_bf16"]["launches"] == 1 and names["pv_attention_rows_bwd_bf16"]["launches"] == 1 and "pv_attention_bwd_bf16" not in names
    assert "pv_masked_residual" in names
    if mode == "f16":          # (no token within KNEE of a knee: the same tokens are masked; bf16 rows carry more noise than that margin)
        for mk, rk in zip(masks, ref_masks):
            assert torch.equal((mk == 0).cpu(), rk == 0)
    grads = {k: (torch.zeros_like(ref_grads[k], dtype=torch.float32) if g is None else g) for k, g in grads.items()}
    e_loss = abs(loss - float(ref_loss)) / abs(float(ref_loss))
    print(f"residualvit {mode}: loss {e_loss:.3g}")
    assert e_loss < (1e-3 if mode == "f16" else 2e-2)
    _check_model("residualvit", mode, logits, grads, ref_logits, ref_grads)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. dropout
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_vit_dropout_step_at_226_rows_against_the_fp64_replay(mode):
    """set_fused_dropout(True), (dropout, attention_dropout) = (0.1, 0.1), against the fp64 composite replaying the pass's dropout_record; the yardstick
    is test_hip_dropout.py::test_training_step_against_the_fp64_replay's: the dropout-free HIP step on the same weights against ITS fp64 composite,
    2 x that error per quantity plus 1e-5."""
    from peekvit_amd import engine, train_engine as te
    cfg = CFG_227
    x, y = TD._batch(cfg, batch=2)
    with engine.precision(TD.PRECISION[mode]):
        base = TD._make("vit", 0.0, 0.0, cfg).to(DEV).train()
        b_logits, b_grads, _ = _timed_hip_step(base, x, y)
        r_logits, r_grads = _fp64_step("vit", cfg, base, x, y)
        m = TD._make("vit", 0.1, 0.1, cfg).to(DEV).train()
        m.load_state_dict(base.state_dict())
        m.set_fused_dropout(True)
        torch.manual_seed(2024)
        d_logits, d_grads, names = _timed_hip_step(m, x, y)
        key, sites = te.train_state(m).dropout_record
        assert [s[0] for s in sites] == ["input"] + ["attention", "branch"] * 2
        assert (2, 2, 226, 226) in [s[3] for s in sites]
        q_logits, q_grads = _fp64_step("vit", cfg, m, x, y, (key, sites), (0.1, 0.1))
    assert names["pv_attention_stream_bwd16_drop_bf16"]["launches"] == 2 and names["pv_dropout_residual"]["launches"] == 2
    assert not torch.equal(d_logits, b_logits)
    rows = [("logits", rel_l2(d_logits, q_logits), rel_l2(b_logits, r_logits))]
    rows += [(n, rel_l2(d_grads[n], q_grads[n]), rel_l2(b_grads[n], r_grads[n])) for n in d_grads]
    bad = []
    for n, ed, eb in rows:
        print(f"vit 226 rows {mode} {n}: dropout step {ed:.3g}, dropout-free step {eb:.3g}")
        if not ed <= 2.0 * eb + 1e-5:
            bad.append((n, ed, eb))
    assert not bad, bad
