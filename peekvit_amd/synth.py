"""Deterministic synthetic weights and images for the ViT encoder hot path.

There is no dataset and no pretrained checkpoint reachable (no network), and the
GPU box never sees /root/reference, so every test, the golden-vector script and
bench.py need tensors that can be REGENERATED bit-identically anywhere from a
name and a seed.  This module owns that generator:

    value(name, flat_index) = f(splitmix64(fnv1a(name) ^ seed) + flat_index)

All values are rounded to bf16-representable fp32, so the MI355X path (bf16 MFMA
operands) and the fp32 oracle see *identical* weights/inputs and differences are
due to arithmetic only (SURVEY.md section 7 H1, section 8c golden vectors (2)).

Parameter names/shapes follow the reference state-dict contract (SURVEY.md
section 8b; reference models/vit.py:104-199, models/residualvit.py:390-500).
The reference zero-initialises `head` and `class_tokens` (vit.py:165,186-188)
which makes logits identically zero; like SURVEY appendix A.1 prescribes, the
synthetic state dict re-draws them N(0, 0.02).
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, Optional, Sequence, Tuple

import numpy as np

_MASK64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _fnv1a64(name: str) -> int:
    h = 0xCBF29CE484222325
    for b in name.encode("utf-8"):
        h ^= b
        h = (h * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def _splitmix64(x: np.ndarray) -> np.ndarray:
    """Vectorised splitmix64 finaliser on uint64 arrays (wrap-around arithmetic)."""
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def hash_uniform(name: str, n: int, seed: int = 0, stream: int = 0) -> np.ndarray:
    """n float64 values in [0, 1), a pure function of (name, seed, stream, index)."""
    key = (_fnv1a64(name) ^ (seed * 0x9E3779B97F4A7C15) ^ (stream * 0xD1B54A32D192ED03)) & 0xFFFFFFFFFFFFFFFF
    with np.errstate(over="ignore"):
        idx = np.arange(n, dtype=np.uint64) + np.uint64(key)
    bits = _splitmix64(_splitmix64(idx))
    return (bits >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def hash_normal(name: str, n: int, seed: int = 0) -> np.ndarray:
    """n float64 standard normals (Box-Muller on two hashed uniform streams)."""
    u1 = hash_uniform(name, n, seed, stream=1)
    u2 = hash_uniform(name, n, seed, stream=2)
    u1 = np.maximum(u1, 2.0 ** -53)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * math.pi * u2)


def round_to_bf16(a: np.ndarray) -> np.ndarray:
    """Round fp32 values to the nearest bf16 (ties to even), returned as fp32."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32)
    with np.errstate(over="ignore"):
        r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def tensor(name: str, shape: Sequence[int], kind: str, scale: float = 1.0, shift: float = 0.0,
           seed: int = 0, bf16: bool = True) -> np.ndarray:
    n = int(np.prod(shape)) if len(shape) else 1
    if kind == "normal":
        v = hash_normal(name, n, seed) * scale + shift
    elif kind == "uniform":  # U(-scale, scale) + shift
        v = (hash_uniform(name, n, seed) * 2.0 - 1.0) * scale + shift
    else:
        raise ValueError(kind)
    v = v.astype(np.float32).reshape(tuple(shape))
    return round_to_bf16(v) if bf16 else v


# ----------------------------------------------------------------------------------------------
# model configurations named by BASELINE.json (reference configs/model/*.yaml)
# ----------------------------------------------------------------------------------------------
MODEL_CONFIGS: Dict[str, dict] = {
    # micro model for per-op full-tensor fixtures (widened so D is MFMA friendly)
    "vit_micro": dict(image_size=32, patch_size=8, num_layers=2, num_heads=2, hidden_dim=128, mlp_dim=256,
                      num_classes=10),
    # reference configs/model/vit_tiny.yaml:1-8 on imagenette (configs/dataset/imagenette.yaml: 160, 10)
    "vit_tiny": dict(image_size=160, patch_size=8, num_layers=4, num_heads=8, hidden_dim=256, mlp_dim=768,
                     num_classes=10),
    # reference configs/model/vit_small.yaml:1-8 at 224 / 1000 classes (BASELINE config 2)
    "vit_small": dict(image_size=224, patch_size=16, num_layers=8, num_heads=8, hidden_dim=384, mlp_dim=1536,
                      num_classes=1000),
    # reference configs/model/vit_b_16.yaml:1-9 (BASELINE config 3, the headline)
    "vit_b_16": dict(image_size=224, patch_size=16, num_layers=12, num_heads=12, hidden_dim=768, mlp_dim=3072,
                     num_classes=1000),
}


def seq_length(cfg: dict) -> int:
    return (cfg["image_size"] // cfg["patch_size"]) ** 2 + cfg.get("num_class_tokens", 1) + cfg.get("num_registers", 0)


def state_dict_spec(cfg: dict, variant: str = "vit") -> Iterable[Tuple[str, Tuple[int, ...], str, float, float]]:
    """Yield (name, shape, kind, scale, shift) for every parameter of the reference module tree.

    Scales mimic PyTorch's default initialisers closely enough to give realistic activation
    statistics; exact init parity is irrelevant because tests load these tensors into both sides.
    """
    D, M, L, P = cfg["hidden_dim"], cfg["mlp_dim"], cfg["num_layers"], cfg["patch_size"]
    C = cfg["num_classes"]
    nc, nr = cfg.get("num_class_tokens", 1), cfg.get("num_registers", 0)
    S = seq_length(cfg)
    fan = 3 * P * P
    yield "class_tokens", (1, nc, D), "normal", 0.02, 0.0
    if nr > 0:
        yield "register_tokens", (1, nr, D), "normal", 0.02, 0.0
    if variant == "residualvit" and cfg.get("add_budget_token") == "learnable":
        yield "learnable_budget_token_1", (1, 1, D), "normal", 1.0, 0.0
    yield "conv_proj.weight", (D, 3, P, P), "normal", math.sqrt(1.0 / fan), 0.0
    yield "conv_proj.bias", (D,), "uniform", 0.02, 0.0
    yield "encoder.pos_embedding", (1, S, D), "normal", 0.02, 0.0
    for i in range(L):
        p = f"encoder.layers.{i}."
        if variant == "residualvit":
            skip = (cfg.get("residual_layers") or ["attention+mlp"] * L)[i]
            if skip in ("attention", "mlp", "attention+mlp"):
                yield p + "residual_gate.projection.weight", (1, D), "uniform", 1.0 / math.sqrt(D), 0.0
                yield p + "residual_gate.projection.bias", (1,), "uniform", 1.0 / math.sqrt(D), 0.0
        yield p + "ln_1.weight", (D,), "uniform", 0.1, 1.0
        yield p + "ln_1.bias", (D,), "uniform", 0.05, 0.0
        yield p + "self_attention.self_attention.in_proj_weight", (3 * D, D), "uniform", math.sqrt(6.0 / (4 * D)), 0.0
        yield p + "self_attention.self_attention.in_proj_bias", (3 * D,), "uniform", 0.02, 0.0
        yield p + "self_attention.self_attention.out_proj.weight", (D, D), "uniform", 1.0 / math.sqrt(D), 0.0
        yield p + "self_attention.self_attention.out_proj.bias", (D,), "uniform", 0.02, 0.0
        yield p + "ln_2.weight", (D,), "uniform", 0.1, 1.0
        yield p + "ln_2.bias", (D,), "uniform", 0.05, 0.0
        yield p + "mlp.fc1.weight", (M, D), "uniform", 1.0 / math.sqrt(D), 0.0
        yield p + "mlp.fc1.bias", (M,), "uniform", 1.0 / math.sqrt(D), 0.0
        yield p + "mlp.fc2.weight", (D, M), "uniform", 1.0 / math.sqrt(M), 0.0
        yield p + "mlp.fc2.bias", (D,), "uniform", 1.0 / math.sqrt(M), 0.0
        if variant == "residualvit" and cfg.get("add_budget_token") == "learnable":
            yield p + "budget_token_gate.weight", (1, D), "uniform", 1.0 / math.sqrt(D), 0.0
            yield p + "budget_token_gate.bias", (1,), "uniform", 1.0 / math.sqrt(D), 0.0
    yield "encoder.ln.weight", (D,), "uniform", 0.1, 1.0
    yield "encoder.ln.bias", (D,), "uniform", 0.05, 0.0
    yield "head.weight", (C, D), "normal", 0.02, 0.0
    yield "head.bias", (C,), "uniform", 0.02, 0.0


def synth_state_dict(cfg: dict, variant: str = "vit", seed: int = 0) -> Dict[str, np.ndarray]:
    """bf16-representable fp32 numpy arrays keyed by the reference state-dict names."""
    return {name: tensor(name, shape, kind, scale, shift, seed)
            for name, shape, kind, scale, shift in state_dict_spec(cfg, variant)}


def moe_state_dict(cfg: dict, mlp_moes=None, attn_moes=None, seed: int = 0, dominant: Optional[int] = None) -> Dict[str, np.ndarray]:
    """Synthetic state dict of the reference's VisionTransformerMoE (models/moevit.py) under its key names: the ViT tensors of state_dict_spec
    with every expert's copy drawn under its own name (`...mlp.experts.{e}.fc1.weight`), `class_token` for `class_tokens`, and each half's
    gate `...gating_network.gate.{weight,bias}` ~ U(+-1/sqrt(D)).  `dominant` = e: every gate with more than e experts gets +50 on expert e's
    bias, so that expert takes every token (the other segments stay empty)."""
    L, D = cfg["num_layers"], cfg["hidden_dim"]
    mlp_moes, attn_moes = list(mlp_moes or [1] * L), list(attn_moes or [1] * L)
    out: Dict[str, np.ndarray] = {}

    def put(name, shape, kind, scale, shift):
        out[name] = tensor(name, shape, kind, scale, shift, seed)

    for name, shape, kind, scale, shift in state_dict_spec(cfg):
        if not name.startswith("encoder.layers."):
            put("class_token" if name == "class_tokens" else name, shape, kind, scale, shift)
            continue
        i = int(name.split(".")[2])
        p, rest = f"encoder.layers.{i}.", name[len(f"encoder.layers.{i}."):]
        if rest.startswith("self_attention.self_attention."):
            if rest.endswith("in_proj_weight"):
                E = attn_moes[i]
                put(p + "self_attention.gating_network.gate.weight", (E, D), "uniform", 1.0 / math.sqrt(D), 0.0)
                put(p + "self_attention.gating_network.gate.bias", (E,), "uniform", 1.0 / math.sqrt(D), 0.0)
            for e in range(attn_moes[i]):
                put(p + f"self_attention.experts.{e}." + rest[len("self_attention."):], shape, kind, scale, shift)
        elif rest.startswith("mlp."):
            if rest == "mlp.fc1.weight":
                E = mlp_moes[i]
                put(p + "mlp.gating_network.gate.weight", (E, D), "uniform", 1.0 / math.sqrt(D), 0.0)
                put(p + "mlp.gating_network.gate.bias", (E,), "uniform", 1.0 / math.sqrt(D), 0.0)
            for e in range(mlp_moes[i]):
                put(p + f"mlp.experts.{e}." + rest[len("mlp."):], shape, kind, scale, shift)
        else:
            put(name, shape, kind, scale, shift)
    if dominant is not None:
        for k, v in out.items():
            if k.endswith("gating_network.gate.bias") and v.shape[0] > dominant:
                v[dominant] += 50.0
                out[k] = round_to_bf16(v)
    return out


# E[10^(-12 u)], u ~ U[0, 1): mean square of a log-uniform magnitude over six decades
_LOGU6_MS = (1.0 - 1e-12) / (12.0 * math.log(10.0))


def hostile_state_dict(cfg: dict, seed: int = 0) -> Dict[str, np.ndarray]:
    """The plain-ViT synthetic state dict made numerically HOSTILE to 16-bit operands (round 3, tests/golden/hostile.npz), still a pure
    function of (name, seed) and bf16-representable:
      * every weight MATRIX (conv_proj, in-proj, out-proj, fc1, fc2, head) keeps its signs and its overall RMS but draws its
        magnitudes log-uniformly over six decades, |w| = c * 10^(-6u), u ~ U[0,1): a third of the elements sit below fp16's smallest
        normal number relative to the largest ones;
      * three channels of every LayerNorm gain and four rows of every fc1 are multiplied by 100 (outlier channels);
      * one token is massive: positional-embedding row 5 is multiplied by 5e4 (values ~ N(0, 1e3)), so that token's residual stream
        is three orders of magnitude above its neighbours' through the whole encoder."""
    sd = synth_state_dict(cfg, "vit", seed)
    D = cfg["hidden_dim"]
    out = {}
    for name, w in sd.items():
        v = w.astype(np.float64)
        if w.ndim >= 2 and name not in ("class_tokens", "register_tokens", "encoder.pos_embedding"):
            u = hash_uniform("hostile/" + name, w.size, seed).reshape(w.shape)
            rms = math.sqrt(float(np.mean(v * v)))
            v = np.sign(v) * (10.0 ** (-6.0 * u)) * (rms / math.sqrt(_LOGU6_MS))
            if name.endswith("mlp.fc1.weight"):
                v[[1, 50, 101, v.shape[0] - 3]] *= 100.0
        elif name.endswith(("ln_1.weight", "ln_2.weight", "encoder.ln.weight")):
            v[[3, 77 % D, D - 5]] *= 100.0
        elif name == "encoder.pos_embedding":
            v[0, 5] *= 5e4
        out[name] = round_to_bf16(v.astype(np.float32))
    return out


def hostile_variants(cfg: dict, seed: int = 0) -> Dict[str, Dict[str, np.ndarray]]:
    """name -> state dict: the full hostile set and its ingredients one at a time (tests/golden/hostile.npz holds the reference's outputs)."""
    base = synth_state_dict(cfg, "vit", seed)
    host = hostile_state_dict(cfg, seed)
    is_mat = lambda k, v: v.ndim >= 2 and k not in ("class_tokens", "register_tokens", "encoder.pos_embedding")
    logu = {k: (host[k].copy() if is_mat(k, v) else v) for k, v in base.items()}
    for k in logu:
        if k.endswith("mlp.fc1.weight"):
            rows = [1, 50, 101, logu[k].shape[0] - 3]
            logu[k][rows] = round_to_bf16(logu[k][rows] / 100.0)                 # the magnitudes alone, without the x100 rows
    gains = {k: (host[k] if k.endswith(("ln_1.weight", "ln_2.weight", "encoder.ln.weight")) else v) for k, v in base.items()}
    massive = dict(base, **{"encoder.pos_embedding": host["encoder.pos_embedding"]})
    return {"hostile": host, "loguniform": logu, "ln_gain": gains, "massive_token": massive, "trained_like": trained_like_state_dict(cfg, seed)}


def trained_like_state_dict(cfg: dict, seed: int = 0) -> Dict[str, np.ndarray]:
    """What TRAINED ViTs look like to a 16-bit path, without the x100 gains of the hostile set (round 5): in every third encoder
    layer the q and k rows of the in-projection are scaled up so that the attention logits reach ~40 - 80 (sharp heads), and two channels of the
    residual stream carry massive activations (a constant ~40 x the typical magnitude on every token, through the positional embedding - the
    'massive activation' channels of pretrained ViTs).  Everything else is the benign synthetic model.  bf16-representable like the rest."""
    sd = {k: v.copy() for k, v in synth_state_dict(cfg, "vit", seed).items()}
    D, L = cfg["hidden_dim"], cfg["num_layers"]
    for i in range(L):
        if i % 3 == 1:
            w = sd[f"encoder.layers.{i}.self_attention.self_attention.in_proj_weight"]
            b = sd[f"encoder.layers.{i}.self_attention.self_attention.in_proj_bias"]
            w[:2 * D] = round_to_bf16(w[:2 * D] * 5.0)
            b[:2 * D] = round_to_bf16(b[:2 * D] * 5.0)
    pos = sd["encoder.pos_embedding"]
    for c in (5 % D, (D // 2 + 13) % D):
        pos[:, :, c] = round_to_bf16(pos[:, :, c] + 40.0)               # (the tokens themselves are ~1)
    return sd


def synth_images(batch: int, image_size: int, seed: int = 0, name: str = "images") -> np.ndarray:
    """[B,3,R,R] fp32 ~ N(0,1), bf16-representable (ImageNet-normalised images are ~zero-mean/unit-var)."""
    return tensor(f"{name}/{image_size}", (batch, 3, image_size, image_size), "normal", 1.0, 0.0, seed)


def load_synth_weights(model, cfg: dict, variant: str = "vit", seed: int = 0, strict: bool = True):
    """Load the synthetic state dict into a torch module that follows the reference key contract."""
    import torch
    sd = {k: torch.from_numpy(v.copy()) for k, v in synth_state_dict(cfg, variant, seed).items()}
    return model.load_state_dict(sd, strict=strict)


def fwd_flops_per_image(cfg: dict, seq_per_layer: Optional[Sequence[int]] = None) -> float:
    """GEMM-only forward FLOPs per image: SURVEY.md section 8d / BASELINE.md section 3 formula."""
    D, M, L, P, C = cfg["hidden_dim"], cfg["mlp_dim"], cfg["num_layers"], cfg["patch_size"], cfg["num_classes"]
    Np = (cfg["image_size"] // P) ** 2
    S0 = seq_length(cfg)
    seqs = list(seq_per_layer) if seq_per_layer is not None else [S0] * L
    f = Np * 3 * P * P * D * 2.0
    for S in seqs:
        f += S * D * 3 * D * 2.0 + 2 * S * S * D * 2.0 + S * D * D * 2.0 + 2 * S * D * M * 2.0
    f += D * C * 2.0
    return f


def ee_state_dict(cfg: dict, seed: int = 0) -> Dict[str, np.ndarray]:
    """Synthetic state dict of the reference's EEResidualVisionTransformer (models/eeresidualvit.py) under its key names: the ResidualViT
    tensors of state_dict_spec (cfg may carry residual_layers / add_budget_token / num_class_tokens / num_registers), the second budget token
    the model creates in both learnable modes, and one exit head per layer, `encoder.early_exit_heads.{i}.0` (LayerNorm) and `.1` (Linear).
    The exit Linears are NOT near zero like `head`: their scale grows with depth, (0.6 + 1.6 (i + 1) / L) / sqrt(D), so that the max softmax
    of the exits spreads over roughly 0.2 - 0.99 and images leave at different layers."""
    L, D, C = cfg["num_layers"], cfg["hidden_dim"], cfg["num_classes"]
    out = synth_state_dict(cfg, "residualvit", seed)
    budget = cfg.get("add_budget_token")
    if budget in ("learnable", "learnable_interpolate"):
        for k in ("learnable_budget_token_1", "learnable_budget_token_2"):
            out[k] = tensor(k, (1, 1, D), "normal", 1.0, 0.0, seed)
    for i in range(L):
        p = f"encoder.early_exit_heads.{i}."
        out[p + "0.weight"] = tensor(p + "0.weight", (D,), "uniform", 0.1, 1.0, seed)
        out[p + "0.bias"] = tensor(p + "0.bias", (D,), "uniform", 0.05, 0.0, seed)
        out[p + "1.weight"] = tensor(p + "1.weight", (C, D), "normal", (0.6 + 1.6 * (i + 1) / L) / math.sqrt(D), 0.0, seed)
        out[p + "1.bias"] = tensor(p + "1.bias", (C,), "uniform", 0.02, 0.0, seed)
    return out


def ee_images(batch: int, image_size: int, seed: int = 0) -> np.ndarray:
    """[B,3,R,R] fp32, bf16-representable: a pool of images that DIFFER from each other the way real images do - N(0,1) noise with a per-image
    contrast in [0.3, 1.7), a per-image, per-channel brightness in [-1, 1) and a per-image horizontal / vertical ramp.  Pure noise images give
    nearly the same class token (it averages a few hundred i.i.d. patches), so every image would leave an early-exit model at the same
    layer; with these the exit confidences of one layer spread across images."""
    R = image_size
    base = tensor(f"ee/{R}", (batch, 3, R, R), "normal", 1.0, 0.0, seed, bf16=False)
    u = hash_uniform(f"ee/{R}/style", batch * 8, seed).reshape(batch, 8)
    gain = (0.3 + 1.4 * u[:, 0]).reshape(batch, 1, 1, 1)
    offset = (2.0 * u[:, 1:4] - 1.0).reshape(batch, 3, 1, 1)
    ramp = np.linspace(-1.0, 1.0, R)
    rx = (2.0 * u[:, 4] - 1.0).reshape(batch, 1, 1, 1) * ramp.reshape(1, 1, 1, R)
    ry = (2.0 * u[:, 5] - 1.0).reshape(batch, 1, 1, 1) * ramp.reshape(1, 1, R, 1)
    return round_to_bf16((base * gain + offset + rx + ry).astype(np.float32))


def residual_sparse_state_dict(cfg: dict, gate_gain: float = 4.0, seed: int = 0) -> Dict[str, np.ndarray]:
    """The "residualvit" synthetic state dict with every gate projection weight multiplied by `gate_gain` (bf16-representable like the
    rest).  Meant for `gate_bias=1`: the stock gates (weights ~ U(+-1/sqrt(D)), `gate_bias=10`) mask nothing, these spread the gate
    scores around the budget thresholds, so that roughly half of the tokens of a ViT-B/16 are masked somewhere in the encoder - the
    case ResidualViT's token compaction is built for.  cfg must carry add_budget_token='learnable'."""
    out = synth_state_dict(cfg, "residualvit", seed)
    for k in out:
        if k.endswith("residual_gate.projection.weight"):
            out[k] = round_to_bf16((out[k].astype(np.float64) * gate_gain).astype(np.float32))
    return out


def pct_state_dict(cfg: dict, seed: int = 0) -> Dict[str, np.ndarray]:
    """Synthetic state dict of the reference's PointCloudTransformer / RankPointCloudTransformer (models/pct.py, models/rankpct.py: the same
    keys) for cfg = {num_points, num_layers, num_heads, hidden_dim, mlp_dim, num_classes[, num_registers, num_class_tokens]}.  A pure function
    of (cfg, seed).  Every BatchNorm has non-trivial running statistics (mean ~ N(0, 0.3), variance in [0.5, 1.5]) and an affine part away
    from the identity; the stem's BatchNorm 1 has scales of BOTH signs (+, -, +, +, -, +), so the max over the neighbours becomes a min on two
    channels.  The encoder's matrices are bf16-representable like the image models'; the stem and the head stay fp32 (they run in fp32)."""
    D, M, L, C = cfg["hidden_dim"], cfg["mlp_dim"], cfg["num_layers"], cfg["num_classes"]
    nc, nr = cfg.get("num_class_tokens", 1), cfg.get("num_registers", 0)
    out: Dict[str, np.ndarray] = {}

    def put(name, shape, kind, scale, shift, bf16=True):
        out[name] = tensor("pct/" + name, shape, kind, scale, shift, seed, bf16)

    def bn(prefix, n, signs=None):
        w = np.abs(tensor("pct/" + prefix + "weight", (n,), "uniform", 0.4, 1.0, seed, False))
        out[prefix + "weight"] = (w * np.asarray(signs, dtype=np.float32)) if signs is not None else w
        put(prefix + "bias", (n,), "uniform", 0.2, 0.0, False)
        put(prefix + "running_mean", (n,), "normal", 0.3, 0.0, False)
        put(prefix + "running_var", (n,), "uniform", 0.5, 1.0, False)
        out[prefix + "num_batches_tracked"] = np.asarray(7, dtype=np.int64)

    put("embedder.lin1.weight", (6, 6), "uniform", 1.0 / math.sqrt(6.0), 0.0, False)
    put("embedder.lin1.bias", (6,), "uniform", 1.0 / math.sqrt(6.0), 0.0, False)
    put("embedder.lin2.weight", (D, 6), "uniform", 1.0 / math.sqrt(6.0), 0.0, False)
    put("embedder.lin2.bias", (D,), "uniform", 1.0 / math.sqrt(6.0), 0.0, False)
    bn("embedder.bn1.", 6, signs=(1, -1, 1, 1, -1, 1))
    bn("embedder.bn2.", D)
    put("class_tokens", (1, nc, D), "normal", 0.02, 0.0)
    if nr > 0:
        put("registers", (1, nr, D), "normal", 0.5, 0.0)
    for name, shape, kind, scale, shift in state_dict_spec(dict(cfg, image_size=8, patch_size=8)):
        if name.startswith("encoder.layers."):
            put(name, shape, kind, scale, shift)
    put("head.lin1.weight", (D // 2, D), "uniform", 1.0 / math.sqrt(D), 0.0, False)
    put("head.lin1.bias", (D // 2,), "uniform", 1.0 / math.sqrt(D), 0.0, False)
    put("head.lin2.weight", (C, D // 2), "uniform", 1.0 / math.sqrt(D // 2), 0.0, False)
    put("head.lin2.bias", (C,), "uniform", 1.0 / math.sqrt(D // 2), 0.0, False)
    bn("head.bn1.", D // 2)
    return out


def synth_points(batch: int, n: int, seed: int = 0, dup_frac: float = 0.0) -> np.ndarray:
    """[B, n, 3] fp32 point clouds, uniform in [-1, 1]^3 (NOT rounded to bf16: rounded coordinates would tie distances by the thousand).
    dup_frac > 0: that share of the rows 1.. of every cloud, chosen by the same generator, are copies of row 0 - what the reference's
    data/modelnet40.py random_point_dropout produces."""
    pts = tensor(f"points/{n}", (batch, n, 3), "uniform", 1.0, 0.0, seed, bf16=False)
    if dup_frac > 0.0:
        drop = hash_uniform(f"points/{n}/drop", batch * n, seed).reshape(batch, n) < dup_frac
        drop[:, 0] = False
        pts = np.where(drop[:, :, None], pts[:, :1, :], pts)
    return np.ascontiguousarray(pts, dtype=np.float32)
