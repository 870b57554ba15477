"""Generate tests/golden/pct_*.npz, rankpct_*.npz and pct_meta.json by running the REAL reference PointCloudTransformer and
RankPointCloudTransformer (models/pct.py, models/rankpct.py of the reference checkout) on CPU.

Needs the reference checkout (oracle.make_golden.REF_ROOT); no GPU:

    python scripts/make_golden_pct.py

The reference is imported exactly as oracle/make_golden.py does it; a class that does not resolve to a file under the reference checkout is
refused.  The reference does not run as shipped: both modules call pytorch3d's `knn_points`, whose import they have commented out, and
pytorch3d is not installed.  THIS SCRIPT SUPPLIES THE MISSING FUNCTION (`knn_points` below: brute force, squared distances from the coordinate
differences in fp32, a stable sort, so exact ties go to the lowest index; the point itself is a neighbour, as knn_points(x, x) has it) and
assigns it into the two reference modules' namespaces.  Nothing else of the reference is touched.

Weights come from peekvit_amd.synth.pct_state_dict and clouds from synth.synth_points (pure functions of configuration + seed), so a fixture
holds the clouds and the OUTPUTS: the stem's embedding, every query's neighbour set (int16, ascending index), the logits; for the ranking
model the logits and, per ranked layer, the input rows it kept (int16, ascending).

Tie condition, checked in fp64 for every query and REFUSED when violated (the seed is advanced until it holds): the candidates whose fp32
squared distance lies within 32 ulp of the k-th smallest are either one point or copies of one coordinate triple.  Both sides form the same
three differences; the squares and the two additions round at most six times in total; thirty-two is five times that.  `tie` [B, N] marks
the queries where more than one candidate sits at the boundary (copies of one point: the features are identical, a test compares embeddings
only there).
"""
from __future__ import annotations

import hashlib
import inspect
import json
import math
import os
import sys

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np
import torch

from peekvit_amd import synth
from oracle import make_golden as MG

GOLD = os.path.join(REPO, "tests", "golden")
REF_FILES = ("models/pct.py", "models/rankpct.py", "models/blocks.py", "configs/model/pct.yaml", "configs/model/rankpct.yaml",
             "configs/dataset/modelnet40.yaml")
TIE_ULPS = 32

_SMALL = dict(num_layers=2, num_heads=4, hidden_dim=128, mlp_dim=256, num_classes=10)
_YAML = dict(num_layers=4, num_heads=4, hidden_dim=128, mlp_dim=256, num_classes=40)          # configs/model/pct.yaml + modelnet40.yaml

# name -> (model kwargs, batch, share of rows that are copies of row 0)
CASES = {
    "pct_n64r1": (dict(_SMALL, num_points=64, num_registers=1), 3, 0.0),
    "pct_n128": (dict(_SMALL, num_points=128), 3, 0.0),
    "pct_n1024": (dict(_YAML, num_points=1024), 1, 0.0),
    "pct_n128dup": (dict(_SMALL, num_points=128), 2, 0.4),          # data/modelnet40.py random_point_dropout: ~40 % copies of row 0
}
# name -> (model kwargs, batch, enable_ranking argument, budget)
RANK_CASES = {
    "rankpct_n64r1": (dict(_SMALL, num_points=64, num_registers=1), 3, True, 0.5),
    "rankpct_n128": (dict(_SMALL, num_points=128, num_layers=4), 2, [False, True, False, True], 0.75),
}


def knn_points(p1, p2, K, return_nn=True):
    """Stand-in for pytorch3d.ops.knn_points(p1, p2, K=K, return_nn=True) -> (dists, idx, nn), see the module docstring."""
    dx = p1[:, :, None, 0] - p2[:, None, :, 0]
    dy = p1[:, :, None, 1] - p2[:, None, :, 1]
    dz = p1[:, :, None, 2] - p2[:, None, :, 2]
    d = (dx * dx + dy * dy) + dz * dz
    dist, idx = torch.sort(d, dim=-1, stable=True)
    dist, idx = dist[..., :K], idx[..., :K]
    nn = torch.gather(p2.unsqueeze(1).expand(-1, p1.shape[1], -1, -1), 2, idx.unsqueeze(-1).expand(-1, -1, -1, p2.shape[-1]))
    return dist, idx, (nn if return_nn else None)


def import_reference():
    if not os.path.isdir(MG.REF_ROOT):
        raise SystemExit("reference checkout not present: golden vectors can only be made where it is")
    MG.import_reference()
    import peekvit.models.pct as ref_pct
    import peekvit.models.rankpct as ref_rank
    for mod, name in ((ref_pct, "PointCloudTransformer"), (ref_rank, "RankPointCloudTransformer")):
        src = os.path.realpath(inspect.getsourcefile(getattr(mod, name)))
        if not src.startswith(MG.REF_ROOT + "/"):
            raise SystemExit(f"resolved {name} to {src}, not the reference: refusing to write fixtures")
        mod.knn_points = knn_points                       # the function the reference calls and never imports
    return ref_pct.PointCloudTransformer, ref_rank.RankPointCloudTransformer


def tie_report(pts: np.ndarray, k: int):
    """(ok, tie [B, N] bool, smallest relative gap between the k-th and a DIFFERENT point's distance) for clouds pts fp32 [B, N, 3]."""
    B, N, _ = pts.shape
    tie = np.zeros((B, N), dtype=bool)
    ok, min_gap = True, math.inf
    for b in range(B):
        p = pts[b]
        dx = p[:, None, 0] - p[None, :, 0]
        dy = p[:, None, 1] - p[None, :, 1]
        dz = p[:, None, 2] - p[None, :, 2]
        d = ((dx * dx + dy * dy) + dz * dz).astype(np.float32)
        kth = np.sort(d, axis=1)[:, k - 1]
        near = np.abs(d.astype(np.float64) - kth[:, None].astype(np.float64)) <= TIE_ULPS * np.spacing(kth).astype(np.float64)[:, None]
        for q in range(N):
            cand = np.nonzero(near[q])[0]
            tie[b, q] = cand.size > 1
            if cand.size > 1 and not (p[cand] == p[cand[0]]).all():
                ok = False
        other = np.where(near, np.inf, np.abs(d.astype(np.float64) - kth[:, None]))
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = other.min(axis=1) / kth.astype(np.float64)
        rel = rel[np.isfinite(rel)]
        if rel.size:
            min_gap = min(min_gap, float(rel.min()))
    return ok, tie, min_gap


def synth_cfg(kw):
    return {k: kw[k] for k in ("num_points", "num_layers", "num_heads", "hidden_dim", "mlp_dim", "num_classes") + tuple(
        k for k in ("num_registers", "num_class_tokens") if k in kw)}


def load(cls, kw, seed=0):
    torch.manual_seed(0)
    model = cls(**kw).eval()
    sd = {k: torch.from_numpy(np.array(v)) for k, v in synth.pct_state_dict(synth_cfg(kw), seed).items()}
    model.load_state_dict(sd, strict=True)
    return model


def pick_points(batch, n, k, dup):
    for seed in range(64):
        pts = synth.synth_points(batch, n, seed, dup)
        ok, tie, gap = tie_report(pts, k)
        if ok:
            return seed, pts, tie, gap
    raise SystemExit(f"no seed below 64 satisfies the tie condition at N = {n}")


def run_case(cls, kw, batch, dup):
    model = load(cls, kw)
    k = model.embedder.k
    seed, pts, tie, gap = pick_points(batch, kw["num_points"], k, dup)
    x = torch.from_numpy(pts)
    emb = {}
    h = model.embedder.register_forward_hook(lambda m, i, o: emb.__setitem__("e", o.detach().clone()))
    with torch.no_grad():
        logits = model(x)
        idx = knn_points(x, x, k)[1]
    h.remove()
    arrays = {"points": pts, "embedding": emb["e"].numpy(), "neighbours": np.sort(idx.numpy(), axis=-1).astype(np.int16), "tie": tie,
              "logits": logits.numpy()}
    return arrays, {"kwargs": kw, "batch": batch, "dup_frac": dup, "points_seed": seed, "k": k, "min_relative_gap": gap,
                    "tie_queries": int(tie.sum())}


def run_rank_case(cls, kw, batch, ranking, budget):
    model = load(cls, kw)
    model.enable_ranking(ranking)
    model.set_budget(budget)
    seed, pts, _, _ = pick_points(batch, kw["num_points"], model.embedder.k, 0.0)
    kept, gaps = {}, []

    def pre(i):
        def hook(mod, args):
            if not mod.sort:
                return
            x = args[0]
            norms = torch.norm(x[:, 1:, :], dim=-1)
            order = torch.argsort(norms, dim=-1, descending=True) + 1            # (what RankingPCTBlock.sort_tokens computes)
            n_keep = math.ceil(x.shape[1] * mod.current_budget)
            rows = torch.cat([torch.zeros_like(order[:, :1]), order], dim=1)[:, :n_keep]
            kept[i] = np.sort(rows.numpy(), axis=-1).astype(np.int16)
            s = torch.sort(norms, dim=-1, descending=True).values
            if n_keep - 1 < s.shape[1]:
                gaps.append(float(((s[:, n_keep - 2] - s[:, n_keep - 1]) / s[:, n_keep - 2]).min()))
        return hook

    hooks = [blk.register_forward_pre_hook(pre(i)) for i, blk in enumerate(model.encoder.layers)]
    with torch.no_grad():
        logits = model(torch.from_numpy(pts))
    for h in hooks:
        h.remove()
    arrays = {"points": pts, "logits": logits.numpy()}
    for i, rows in kept.items():
        arrays[f"kept_{i}"] = rows
    return arrays, {"kwargs": kw, "batch": batch, "ranking": ranking, "budget": budget, "points_seed": seed, "ranked_layers": sorted(kept),
                    "min_relative_norm_gap": min(gaps) if gaps else None}


def surface(cls, kw):
    sig = inspect.signature(cls.__init__)
    defaults = {k: p.default for k, p in sig.parameters.items() if k != "self" and p.default is not inspect.Parameter.empty}
    return {"constructor_parameters": [k for k in sig.parameters if k != "self"], "constructor_defaults": defaults,
            "state_dict": {k: list(v.shape) for k, v in cls(**kw).state_dict().items()}}


def main():
    pct, rank = import_reference()
    surf_kw = dict(_SMALL, num_points=64, num_registers=1)
    meta = {"torch": torch.__version__,
            "reference_sha256": {f: hashlib.sha256(open(os.path.join(MG.REF_ROOT, f), "rb").read()).hexdigest() for f in REF_FILES},
            "knn_points": "supplied by scripts/make_golden_pct.py (the reference's pytorch3d import is commented out)",
            "weights": "peekvit_amd.synth.pct_state_dict(cfg, seed=0); clouds: synth.synth_points(batch, num_points, points_seed, dup_frac)",
            "tie_ulps": TIE_ULPS, "surface_kwargs": surf_kw,
            "PointCloudTransformer": surface(pct, surf_kw), "RankPointCloudTransformer": surface(rank, surf_kw), "cases": {}, "rank_cases": {}}
    for name, (kw, batch, dup) in CASES.items():
        arrays, info = run_case(pct, kw, batch, dup)
        path = os.path.join(GOLD, name + ".npz")
        np.savez_compressed(path, **arrays)
        meta["cases"][name] = info
        print(f"{name}: batch {batch}, k {info['k']}, seed {info['points_seed']}, min relative gap {info['min_relative_gap']:.3g}, "
              f"{info['tie_queries']} tie queries, {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < (1 << 20)
    for name, (kw, batch, ranking, budget) in RANK_CASES.items():
        arrays, info = run_rank_case(rank, kw, batch, ranking, budget)
        np.savez_compressed(os.path.join(GOLD, name + ".npz"), **arrays)
        meta["rank_cases"][name] = info
        print(f"{name}: batch {batch}, ranked layers {info['ranked_layers']}, min relative norm gap {info['min_relative_norm_gap']:.3g}")
    with open(os.path.join(GOLD, "pct_meta.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
