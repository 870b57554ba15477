"""RankPointCloudTransformer's HIP eval forward without a GPU: the replay hook of the composite (installed: another forward's kept rows; not installed:
inert), the kept lengths the engine computes, include/peekvit_hip_rank_infer.h against both libraries, the argument checks of its two entry points
(every refusal comes before a launch), and the switch on a CPU model (off by default, no state, the composite bit for bit)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
from peekvit_amd import synth

HEADER = os.path.join(REPO, "include", "peekvit_hip_rank_infer.h")
META = json.load(open(os.path.join(GOLDEN, "pct_meta.json")))
SYNTH_KEYS = ("num_points", "num_layers", "num_heads", "hidden_dim", "mlp_dim", "num_classes", "num_registers", "num_class_tokens")


def _load(info):
    from peekvit_amd.models.pct import RankPointCloudTransformer
    kw = info["kwargs"]
    m = RankPointCloudTransformer(**kw).eval()
    cfg = {k: v for k, v in kw.items() if k in SYNTH_KEYS}
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.pct_state_dict(cfg, 0).items()}, strict=True)
    m.enable_ranking(info["ranking"])
    m.set_budget(info["budget"])
    return m


@pytest.mark.parametrize("name", sorted(META["rank_cases"]))
def test_composite_replaying_its_own_rows_reproduces_its_logits(name):
    from peekvit_amd.models.pct import RankingPCTBlock
    info = META["rank_cases"][name]
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    x = torch.from_numpy(z["points"])
    m = _load(info)
    assert all(blk._replay_keep is None for blk in m.encoder.layers)
    with torch.no_grad():
        logits = m(x).clone()
        keeps = [m.encoder.layers[i].last_keep.clone() for i in info["ranked_layers"]]
        calls = []
        stock = RankingPCTBlock.__dict__["sort_order"]
        RankingPCTBlock.sort_order = staticmethod(lambda t: (calls.append(1), stock.__func__(t))[1])
        try:
            with m._replaying(keeps):
                assert all(m.encoder.layers[i]._replay_keep is kp for i, kp in zip(info["ranked_layers"], keeps))
                replayed = m(x).clone()
            assert not calls                                               # a replaying block does not rank
            assert all(blk._replay_keep is None for blk in m.encoder.layers)          # uninstalled on the way out
            again = m(x)
            assert len(calls) == len(info["ranked_layers"])               # and ranks again afterwards
        finally:
            RankingPCTBlock.sort_order = stock
    assert torch.equal(replayed, logits) and torch.equal(again, logits)
    for i, kp in zip(info["ranked_layers"], keeps):
        assert torch.equal(m.encoder.layers[i].last_keep, kp)
    # other rows than its own: another result, and last_keep records the rows it was given
    other = [torch.cat([kp[:, :1], kp[:, 1:].flip(1)], dim=1) for kp in keeps]
    with torch.no_grad(), m._replaying(other):
        flipped = m(x)
    assert all(torch.equal(m.encoder.layers[i].last_keep, kp) for i, kp in zip(info["ranked_layers"], other))
    assert flipped.shape == logits.shape
    # train mode never replays
    m.train()
    with torch.no_grad():
        torch.manual_seed(3)                                               # (the head's dropout)
        stock_train = m(x).clone()
        torch.manual_seed(3)
        with m._replaying(other):
            assert torch.equal(m(x), stock_train)


def test_replayed_order_is_a_permutation_that_starts_with_the_recorded_rows():
    from peekvit_amd.models.pct import RankingPCTBlock
    keep = torch.tensor([[0, 5, 2], [0, 1, 6]])
    order = RankingPCTBlock.replayed_order(keep, 7)
    assert order.tolist() == [[0, 5, 2, 1, 3, 4, 6], [0, 1, 6, 2, 3, 4, 5]]
    assert RankingPCTBlock.replayed_order(torch.arange(4).flip(0)[None], 4).tolist() == [[3, 2, 1, 0]]


def test_kept_lengths():
    from peekvit_amd import engine
    want = {"rankpct_n128": [96, 72], "rankpct_n64r1": [33, 17]}
    for name, info in META["rank_cases"].items():
        m = _load(info)
        S = info["kwargs"]["num_points"] + info["kwargs"].get("num_registers", 0)
        assert engine.rank_pct_lengths(m, S) == want[name]
        assert engine.rank_pct_supported(m) and engine.rank_pct_supported(m, torch.zeros(2, info["kwargs"]["num_points"], 3))
        m.set_budget(1.5)
        assert engine.rank_pct_lengths(m, S) == [S] * len(info["ranked_layers"])          # min(S, .) for a budget > 1
        m.set_budget(1.0)
        assert engine.rank_pct_lengths(m, S) == [S] * len(info["ranked_layers"])
        m.set_budget(0.01)
        assert engine.rank_pct_lengths(m, S) == {"rankpct_n128": [2, 1], "rankpct_n64r1": [1, 1]}[name]
        assert not engine.rank_pct_supported(m, torch.zeros(2, info["kwargs"]["num_points"], 3))          # L < 2: nothing to rank into
        m.enable_ranking(False)
        assert engine.rank_pct_lengths(m, S) == [] and engine.rank_pct_supported(m, torch.zeros(2, info["kwargs"]["num_points"], 3))


def _declared():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pv_\w+)\s*\(", src, flags=re.M))


def test_header_declarations_are_exported_by_both_libraries():
    from peekvit_amd import _build, _lib
    assert "peekvit_hip_rank_infer.h" in _build.HEADERS
    assert os.path.join(_build.CSRC, "pv_rank_infer.hip") in _build.sources()
    declared = _declared()
    assert declared == {"pv_rank_order_gap", "pv_layernorm_gather_f32_bf16"} == set(_lib.SIGNATURES_RANK_INFER)
    others = (_lib.SIGNATURES, _lib.SIGNATURES_MOE, _lib.SIGNATURES_EE, _lib.SIGNATURES_SPARSE, _lib.SIGNATURES_PCT, _lib.SIGNATURES_PCT_TRAIN,
              _lib.SIGNATURES_ATTN_STREAM, _lib.SIGNATURES_PCT_BLOCK, _lib.SIGNATURES_RANK_TRAIN)
    assert not any(set(_lib.SIGNATURES_RANK_INFER) & set(d) for d in others)
    text = open(HEADER).read()
    for name, (_, args) in _lib.SIGNATURES_RANK_INFER.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == len(args), name
        assert hasattr(_lib.load(), name) and hasattr(_lib.load("f16"), name)
    assert _lib.load().pv_version() == 10 and _lib.load("f16").pv_version() == 10          # ABI unchanged
    # call, do not copy: the gathering LayerNorm is an instantiation of the one LayerNorm kernel with both planes, in its source
    pct = open(os.path.join(_build.CSRC, "pv_pct.hip")).read()
    assert 'extern "C" int pv_layernorm_gather_f32_bf16(' in pct and "pv_layernorm_f32_bf16_kernel<N_, false, true>" in pct
    rank = open(os.path.join(_build.CSRC, "pv_rank_infer.hip")).read()
    assert 'extern "C" int pv_rank_order_gap(' in rank and "atomic" not in rank.replace("no atomics", "")


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from peekvit_amd import _lib
    p, q, null = C.c_void_p(256), C.c_void_p(1 << 30), C.c_void_p(0)       # never dereferenced: every call below is refused before a launch
    odd16, odd8, odd4 = C.c_void_p(264), C.c_void_p(260), C.c_void_p(258)
    for op in ("bf16", "f16"):
        lib = _lib.load(op)

        def order(norms=p, keep=q, gap=null, B=2, N=100, k=50):
            return lib.pv_rank_order_gap(norms, keep, gap, B, N, k, null)

        assert order(norms=null) == -1 and order(keep=null) == -1                                  # nulls (gap_min may be null)
        for name in ("norms", "keep", "gap"):
            assert order(**{name: odd4}) == -1, name                                               # 4-byte alignment
        for dim in ("B", "N"):
            assert order(**{dim: 0}) == -1 and order(**{dim: -3}) == -1, dim
        assert order(k=-1) == -1 and order(k=101) == -1 and order(N=1, k=2) == -1                  # k > N
        assert order(N=4097, k=5) == -2 and order(N=1 << 20, k=5) == -2                            # N > 4096
        assert order(B=1 << 31) == -2
        assert order(k=0) == 0 and order(k=0, N=4096) == 0                                         # nothing to keep: PV_OK without a launch

        def lng(x=p, keep=p, gamma=p, beta=p, out16=q, out32=q, B=2, S=13, k=5, D=128):
            return lib.pv_layernorm_gather_f32_bf16(x, keep, gamma, beta, out16, out32, B, S, k, D, 1e-6, null)

        for name in ("x", "keep", "gamma", "beta", "out16", "out32"):
            assert lng(**{name: null}) == -1, name
            assert lng(**{name: odd4}) == -1, name
        for name in ("x", "gamma", "beta", "out32"):
            assert lng(**{name: odd16}) == -1 and lng(**{name: odd8}) == -1, name                  # fp32 arrays: 16-byte aligned
        assert lng(out16=odd8) == -1                                                               # 16-bit rows: 8-byte aligned
        for dim in ("B", "S", "D"):
            assert lng(**{dim: 0}) == -1 and lng(**{dim: -4}) == -1, dim
        assert lng(k=-1) == -1 and lng(k=13) == -1 and lng(S=1, k=1) == -1                         # 0 <= k <= S - 1
        assert lng(D=126) == -2 and lng(D=1028) == -2 and lng(D=2048) == -2                        # D % 4, D > 1024
        assert lng(out32=p) == -1                                                                  # the fp32 rows on the rows being read


def test_switch_on_a_cpu_model_changes_nothing():
    from peekvit_amd import ops
    from peekvit_amd.models.pct import PointCloudTransformer, RankPointCloudTransformer
    info = META["rank_cases"]["rankpct_n64r1"]
    x = torch.from_numpy(np.load(os.path.join(GOLDEN, "rankpct_n64r1.npz"))["points"])
    m = _load(info)
    assert m._fused_inference is False and not hasattr(PointCloudTransformer, "set_fused_inference")
    keys, nparam, nbuf = list(m.state_dict()), len(list(m.parameters())), len(list(m.buffers()))
    with torch.no_grad():
        off = m(x).clone()
    m.set_fused_inference()
    assert m._fused_inference is True
    assert list(m.state_dict()) == keys and len(list(m.parameters())) == nparam and len(list(m.buffers())) == nbuf
    n0 = ops.launch_count
    with torch.no_grad():
        on = m(x).clone()
    assert ops.launch_count == n0 and torch.equal(on, off)
    assert all(blk.last_norms is None for blk in m.encoder.layers)
    m.set_fused_inference(False)
    assert m._fused_inference is False
    with torch.no_grad():
        assert torch.equal(m(x), off)
    assert isinstance(RankPointCloudTransformer._fused_inference, bool) and not RankPointCloudTransformer._fused_inference


def test_harness_config_key_parses_and_the_cpu_sweep_is_the_composite():
    from peekvit_amd.harness import config, test as htest
    assert config.load_config("test_config", ["model=rankpct", "dataset=synthetic_points"])["test"]["ranked_inference"] is False
    assert config.load_config("test_config", ["model=rankpct", "dataset=synthetic_points", "test.ranked_inference=true"])["test"]["ranked_inference"] is True
    micro = ["model=rankpct", "dataset=synthetic_points", "model.num_layers=2", "model.num_heads=2", "model.hidden_dim=64", "model.mlp_dim=128",
             "dataset.num_points=32", "dataset.num_classes=5", "dataset.train_size=8", "dataset.val_size=8", "device=cpu", "test.test_batch_size=4",
             "test.budgets=[0.5,1.0]"]
    on, off = htest.main(micro + ["test.ranked_inference=true"]), htest.main(micro)
    assert [r["budget"] for r in on] == [0.5, 1.0] and all(r["ranked_inference"] is True for r in on) and all("ranked_inference" not in r for r in off)
    assert all(r["flops_per_image"] is None for r in on + off)                          # (the reference's counter is for patch grids)
    # on for the sweep only; the caller's own setting stays
    m = _load(META["rank_cases"]["rankpct_n64r1"])
    x = torch.from_numpy(np.load(os.path.join(GOLDEN, "rankpct_n64r1.npz"))["points"])
    loader = [(x, torch.zeros(3, dtype=torch.int64))]
    r_on, r_off = htest.evaluate(m, loader, "cpu", [0.5], 3, ranked_inference=True)[0], htest.evaluate(m, loader, "cpu", [0.5], 3)[0]
    assert r_on["ranked_inference"] is True and m._fused_inference is False and r_on["accuracy"] == r_off["accuracy"]          # CPU tensors: the composite either way
    m.set_fused_inference(True)
    htest.evaluate(m, loader, "cpu", [0.5], 3, ranked_inference=True)
    assert m._fused_inference is True and "ranked_inference" not in htest.evaluate(m, loader, "cpu", [0.5], 3)[0]
