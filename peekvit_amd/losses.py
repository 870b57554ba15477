"""Model regularisers behind the reference's interface (reference utils/losses.py; re-exported as peekvit.utils.losses so that the `_target_`
strings of configs/loss/*.yaml resolve): a ModelLoss receives the MODEL after a forward and reads what that forward left on it.

  AViTPonderLoss   mean of encoder.rho_token                                     (A-ViT: the expected depth of a token, plus its remainder)
  AViTDPriorLoss   KL(N(target_depth, 1) over the layers 1..L  ||  the layers' mean halting scores, normalised and clamped to [0.001, 0.999])
  MSELoss          squared (excess over the) budget of the share of tokens each active ResidualModule keeps (its `mask`)
  ChannelMSELoss   the same arithmetic, fed by `channel_budget`
  LossCompose      a weighted sum of such terms, built from {name: {_target_, weight, ...}} with the harness's own `instantiate`

The classes of the reference that no shipped config names (sparsity / entropy / L1 variants) are not provided."""
from __future__ import annotations

import math
from abc import ABC, abstractmethod
from typing import Dict, List, Optional

import torch
from torch import nn


class ModelLoss(nn.Module, ABC):
    """forward(model, **kwargs) -> 0-dim tensor; kwargs a loss does not know are ignored (LossCompose hands every term the same ones)."""

    @abstractmethod
    def forward(self, model, **kwargs):
        ...


def forward_masks(model: nn.Module) -> Dict[str, torch.Tensor]:
    """{module name: mask [B, S, 1]} of every ResidualModule whose `skip` is active, in module order."""
    from .models.residualvit import ResidualModule
    return {name: mod.mask for name, mod in model.named_modules() if isinstance(mod, ResidualModule) and mod.skip not in (None, "none")}


def _excess_sq(v: torch.Tensor, budget: float, strict: bool) -> torch.Tensor:
    d = v - budget
    return (d if strict else torch.relu(d)) ** 2


def budget_mse(model: nn.Module, budget: float, strict: bool = False, skip_layers=(), per_layer: bool = True) -> torch.Tensor:
    """Per active module (those whose index is in skip_layers left out) the share of kept tokens of every image, keep [B].  per_layer: each module
    contributes sum_b excess(keep_b)^2, and the result is the mean over the modules; otherwise keep is averaged over modules AND images first and
    the result is excess(mean)^2.  excess(v) = v - budget (strict) or relu(v - budget); everything is weighted by (2 - budget)."""
    terms = []
    for i, mask in enumerate(forward_masks(model).values()):
        if i in skip_layers:
            continue
        keep = mask.mean(dim=(1, 2))
        terms.append(_excess_sq(keep, budget, strict).sum() if per_layer else keep)
    stacked = torch.stack(terms)
    if not per_layer:
        stacked = _excess_sq(stacked.mean(), budget, strict).sum()
    return (stacked * (2 - budget)).mean()


class MSELoss(ModelLoss):
    def __init__(self, budget: Optional[float] = None, strict: bool = False, skip_layers: Optional[List[int]] = None, per_layer: bool = True, **_):
        super().__init__()
        self.budget, self.strict, self.skip_layers, self.per_layer = budget, strict, list(skip_layers or []), per_layer

    def forward(self, model, budget=None, per_layer: Optional[bool] = None, **kwargs):
        assert budget is not None or self.budget is not None, "budget must be provided either as argument or as class attribute"
        return budget_mse(model, budget if budget is not None else self.budget, self.strict, self.skip_layers,
                          self.per_layer if per_layer is None else per_layer)


class ChannelMSELoss(ModelLoss):
    """MSELoss under another name: the budget of a transmission channel in the middle of the model, not of the whole model."""

    def __init__(self, budget: Optional[float] = None, strict: bool = False, skip_layers: Optional[List[int]] = None, **_):
        super().__init__()
        self.budget, self.strict, self.skip_layers = budget, strict, list(skip_layers or [])

    def forward(self, model, channel_budget=None, **kwargs):
        assert channel_budget or self.budget, "budget must be provided either as argument or as class attribute"
        return budget_mse(model, channel_budget if channel_budget is not None else self.budget, self.strict, self.skip_layers)


class AViTPonderLoss(ModelLoss):
    def __init__(self) -> None:
        super().__init__()

    def forward(self, model, **kwargs):
        return model.encoder.rho_token.mean()


class AViTDPriorLoss(ModelLoss):
    def __init__(self, target_depth: int) -> None:
        super().__init__()
        self.target_depth = target_depth

    def forward(self, model, **kwargs):
        scores = torch.stack(list(model.encoder.halting_score_layer))
        L = scores.shape[0]
        p = (scores / scores.sum()).clamp(0.001, 0.999)
        k = torch.arange(1, L + 1, dtype=scores.dtype, device=scores.device)
        log_target = -0.5 * (k - self.target_depth) ** 2 - 0.5 * math.log(2 * math.pi)          # log N(k; target_depth, 1)
        return nn.functional.kl_div(p.log(), log_target, reduction="batchmean", log_target=True)


class LossCompose:
    """losses_dict: {name: {"_target_": ..., "weight": w (default 1), ...constructor arguments}}."""

    def __init__(self, losses_dict):
        from .harness.config import instantiate
        self.additional_losses = {}
        for name, args in dict(losses_dict).items():
            args = dict(args)
            weight = args.pop("weight", 1.0)
            self.additional_losses[name] = {"weight": weight, "loss_fn": instantiate(args)}

    def compute(self, model, dict_prefix: str = "", return_dict: bool = True, **kwargs):
        """(values {prefix + name: weighted value as a float}, total) or, with return_dict=False, the total alone."""
        values, terms = {}, []
        for name, entry in self.additional_losses.items():
            term = entry["loss_fn"](model, **kwargs) * entry["weight"]
            values[f"{dict_prefix}{name}"] = term.detach().item()
            terms.append(term)
        total = torch.stack(terms).sum()
        return (values, total) if return_dict else total
