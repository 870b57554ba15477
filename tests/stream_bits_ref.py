"""The cases of tests/golden/stream_attention_bits.json: every instantiation of the streaming attention kernels (pv_attn_stream_kernel,
pv_attn_stream_var_kernel, pv_attn_stream_d{q, kv}_kernel, pv_attn_ragged_d{q, kv}_kernel) at the smallest shapes at which they can go wrong - one
key, one full 64-key block, one block plus a one-row tail, two blocks plus a tail - run through the public ops wrappers on inputs from a CPU
generator with fixed seeds.  The fixture must mean the same on every host, so the inputs are built from the generator's INTEGERS by exact arithmetic
(a sum of three uniform integers over 512: unit variance, every value exact in fp32, one IEEE rounding to the operand type) and the key weights are
math.log in fp64 rounded once to fp32 - no vectorised fp32 transcendental, whose last bit may depend on the CPU, sits between the seed and the bytes
the kernels read.  A case's result is the sha256 of every buffer the call writes.  scripts/make_golden_stream_bits.py records them,
tests/test_hip_stream_bits.py recomputes them: a change to these kernels that is meant to keep the arithmetic keeps every hash."""
import hashlib
import math

import torch

MODES = ("bf16", "f16")                     # the two operand builds (MODES of tests/test_hip_residual_sparse.py)
B, H = 2, 2
DHS = (32, 48, 64)
FWD_S = (1, 64, 65, 130)
BWD_S = (1, 65, 130)
WIDE_DHS, WIDE_S = (80, 96, 128), (1, 65)
INFER_S = 417                               # the first length pv_attention_bf16 streams at dh 32 / 48 / 64
TAIL_LOG_MULT = math.log(5.0)
DROP = dict(p=0.25, key=7, site=3)
RAGGED_FWD_LENS = [1, 64, 65, 209, 130]
RAGGED_BWD_LENS = [1, 64, 65, 130]


def case_ids():
    """The table of the cases, as (kind, variant, dh, S) with S = 0 for the ragged calls (their segments are fixed)."""
    ids = [("fwd", v, dh, S) for v in ("plain", "w", "drop") for dh in DHS for S in FWD_S]
    ids += [("infer", "plain", dh, INFER_S) for dh in DHS]
    ids += [("infer", "plain", dh, S) for dh in WIDE_DHS for S in WIDE_S]
    ids += [("ragged_fwd", v, 64, 0) for v in ("w", "unit")]
    ids += [("bwd", v, dh, S) for v in ("f32", "o16", "o16_w", "o16_drop") for dh in DHS for S in BWD_S]
    ids += [("ragged_bwd", v, 64, 0) for v in ("w", "unit")]
    return ids


N_CASES = 3 * 3 * 4 + 3 + 3 * 2 + 2 + 4 * 3 * 3 + 2          # the rows of the table, per build


def case_name(cid):
    kind, variant, dh, S = cid
    return f"{kind}-{variant}-dh{dh}" + (f"-S{S}" if S else "")


def case_seed(cid):
    kind, variant, dh, S = cid
    if variant == "unit":                   # the same call with log_mult = 0: the same inputs
        cid = (kind, "w", dh, S)
    return 1000 + case_ids().index(cid)


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def _normal(rows, cols, g):
    return torch.randint(-512, 513, (3, rows, cols), generator=g).sum(0).float() / 512.0


def _qkv(rows, D, dh, g, dt, dev):
    qkv = _normal(rows, 3 * D, g)
    qkv[:, :D] *= dh ** -0.5
    return qkv.to(dt).to(dev)


def _mults(lens, seed, hi):                 # _mults of tests/test_hip_residual_sparse.py
    g = torch.Generator().manual_seed(seed)
    mult = torch.randint(1, hi + 1, (sum(lens),), generator=g)
    mult[torch.rand(sum(lens), generator=g) < 0.6] = 1
    return mult


def _seg(lens, dev):
    return torch.tensor([0] + [sum(lens[:i + 1]) for i in range(len(lens))], dtype=torch.int32, device=dev)


def run_case(cid, mode, dev):
    """-> {"shapes": {...}, "sha256": {buffer: hex}} of one case in one operand build."""
    from peekvit_amd import _lib, engine, ops
    kind, variant, dh, S = cid
    D = H * dh
    g = torch.Generator().manual_seed(case_seed(cid))
    flag = torch.zeros(4, dtype=torch.int32, device=dev)
    bufs = {}
    with engine.precision(mode):
        dt = _lib.operand_dtype()
        ops.set_range_flag(flag)
        try:
            if kind in ("fwd", "infer", "bwd"):
                qkv = _qkv(B * S, D, dh, g, dt, dev)
                out = torch.zeros((B * S, D), dtype=dt, device=dev)
                lse = torch.zeros((B, H, S), dtype=torch.float32, device=dev)
                shapes = dict(B=B, S=S, H=H, dh=dh)
                if kind == "infer":
                    ops.attention(qkv, out, B, S, H, dh)
                    bufs = dict(out=out)
                elif variant in ("plain", "f32", "o16"):
                    ops.attention_stream(qkv, out, lse, B, S, H, dh)
                elif variant in ("w", "o16_w"):
                    ops.attention_stream_w(qkv, out, lse, B, S, H, dh, TAIL_LOG_MULT)
                else:
                    ops.attention_stream_drop(qkv, out, lse, B, S, H, dh, DROP["p"], DROP["key"], DROP["site"])
                if kind == "fwd":
                    bufs = dict(out=out, lse=lse)
                if kind == "bwd":
                    dout = _normal(B * S, D, g).to(dt).to(dev)
                    delta = torch.zeros((B, H, S), dtype=torch.float32, device=dev)
                    qscale = dh ** -0.5
                    if variant == "f32":
                        dq = torch.zeros((B * S, 3 * D), dtype=torch.float32, device=dev)
                        ops.attention_stream_bwd(qkv, dout, out, lse, dq, B, S, H, dh, qscale, delta_ws=delta)
                        bufs = dict(dqkv=dq, delta_ws=delta)
                    else:
                        dq = torch.zeros((B * S, 3 * D), dtype=dt, device=dev)
                        dbp = torch.zeros((B, (S + 63) // 64, 3 * D), dtype=torch.float32, device=dev)
                        if variant == "o16":
                            ops.attention_stream_bwd16(qkv, dout, out, lse, dq, B, S, H, dh, qscale, dbias_partial=dbp, delta_ws=delta)
                        elif variant == "o16_w":
                            ops.attention_stream_bwd16_w(qkv, dout, out, lse, dq, B, S, H, dh, qscale, TAIL_LOG_MULT, dbias_partial=dbp, delta_ws=delta)
                        else:
                            ops.attention_stream_bwd16_drop(qkv, dout, out, lse, dq, B, S, H, dh, qscale, DROP["p"], DROP["key"], DROP["site"],
                                                            dbias_partial=dbp, delta_ws=delta)
                        bufs = dict(dqkv16=dq, dbias_partial=dbp, delta_ws=delta)
            else:
                lens = RAGGED_FWD_LENS if kind == "ragged_fwd" else RAGGED_BWD_LENS
                R = sum(lens)
                seg = _seg(lens, dev)
                qkv = _qkv(R, D, dh, g, dt, dev)
                mult = _mults(lens, case_seed(cid), 4096)
                lm = (torch.tensor([math.log(v) for v in mult.tolist()], dtype=torch.float64).float().to(dev) if variant == "w"
                      else torch.zeros(R, device=dev))
                out = torch.zeros((R, D), dtype=dt, device=dev)
                shapes = dict(lens=lens, H=H, dh=dh)
                if kind == "ragged_fwd":
                    ops.attention_varlen_w_stream(qkv, out, seg, lm, max(lens), H, dh)
                    bufs = dict(out=out)
                else:
                    lse = torch.zeros((R, H), dtype=torch.float32, device=dev)
                    ops.attention_varlen_w_lse(qkv, out, lse, seg, lm, max(lens), H, dh)
                    dout = _normal(R, D, g).to(dt).to(dev)
                    dq = torch.zeros((R, 3 * D), dtype=dt, device=dev)
                    dbp = torch.zeros((len(lens) * ((max(lens) + 63) // 64), 3 * D), dtype=torch.float32, device=dev)
                    delta = torch.zeros((R, H), dtype=torch.float32, device=dev)
                    ops.attention_varlen_w_bwd16(qkv, dout, out, lse, seg, lm, dq, max(lens), H, dh, dh ** -0.5, dbias_partial=dbp, delta_ws=delta)
                    bufs = dict(dqkv16=dq, dbias_partial=dbp, delta_ws=delta)
            torch.cuda.synchronize()
        finally:
            ops.set_range_flag(None)
    if kind not in ("bwd", "ragged_bwd"):               # (the backward launches take no range flag)
        bufs["range_flag"] = flag
    return dict(shapes=shapes, seed=case_seed(cid), sha256={k: _sha(v) for k, v in bufs.items()})


def run_all(dev):
    return {mode: {case_name(cid): run_case(cid, mode, dev) for cid in case_ids()} for mode in MODES}
