"""Generate tests/golden/avit_train.npz by running the REAL reference A-ViT in train mode on CPU with the reference's own loss classes
(utils/losses.py of the reference checkout, oracle.make_golden.REF_ROOT: AViTPonderLoss, AViTDPriorLoss) and the weights of configs/loss/avit_losses.yaml.

Run in the build container only (the reference never travels to the GPU box):

    python scripts/make_golden_avit_train.py

The reference is imported as scripts/make_golden_avit.py imports it.  Its losses module imports omegaconf and hydra, which are not installed: they
get placeholder modules (names only - the fixture calls the two loss classes directly, nothing of either package runs), the way torchvision does.
Weights and images are scripts/make_golden_avit.py's (peekvit_amd.synth, seed 0), labels are arange(batch) % num_classes.  Per case the fixture holds
the three loss values (cross-entropy, ponder, distribution prior - unweighted), the combined loss, every parameter's gradient norm under the combined
loss, the complete pos_embedding gradient, the prior and its pos_embedding gradient at target depth 2 (inside these
4-layer models), and rho_token / counter_token / the layer scores of that forward."""
from __future__ import annotations

import inspect
import os
import sys
import types

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

import numpy as np
import torch

from peekvit_amd import synth
from oracle import make_golden as MG
import make_golden_avit as GA

CASES = ("avit_micro", "avit_cls2_reg2")
TARGET_DEPTH, W_PRIOR, W_PONDER = 11, 0.2, 0.0005          # configs/loss/avit_losses.yaml
SHALLOW_DEPTH = 2          # N(11, 1) has 1e-11 of its mass on the 4 layers of these models: the prior is also recorded at a target inside them


def import_reference_losses():
    cls = GA.import_reference()
    oc = types.ModuleType("omegaconf")
    oc.OmegaConf, oc.DictConfig = type("OmegaConf", (), {}), type("DictConfig", (), {})
    hy, hu = types.ModuleType("hydra"), types.ModuleType("hydra.utils")
    hu.instantiate = None
    hy.utils = hu
    for name, mod in (("omegaconf", oc), ("hydra", hy), ("hydra.utils", hu)):
        sys.modules.setdefault(name, mod)
    from peekvit.utils import losses
    src = os.path.realpath(inspect.getsourcefile(losses.AViTPonderLoss))
    if not src.startswith(MG.REF_ROOT + "/"):
        raise SystemExit(f"resolved the losses module to {src}, not the reference: refusing to write fixtures")
    return cls, losses


def run_case(cls, losses, name):
    kw, batch = GA.CASES[name]
    cfg = {k: kw[k] for k in ("image_size", "patch_size", "num_layers", "num_heads", "hidden_dim", "mlp_dim", "num_classes")}
    cfg.update({k: kw[k] for k in ("num_class_tokens", "num_registers") if k in kw})
    torch.manual_seed(0)
    model = cls(**kw).train()
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(cfg, seed=0).items()}, strict=True)
    x = torch.from_numpy(synth.synth_images(batch, kw["image_size"], seed=0, name="avit"))
    labels = torch.arange(batch) % kw["num_classes"]
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        logits = model(x)
        ce = torch.nn.CrossEntropyLoss()(logits, labels)
        ponder = losses.AViTPonderLoss()(model)
        prior = losses.AViTDPriorLoss(target_depth=TARGET_DEPTH)(model)
        prior2 = losses.AViTDPriorLoss(target_depth=SHALLOW_DEPTH)(model)
        (gpos2,) = torch.autograd.grad(prior2, model.encoder.pos_embedding, retain_graph=True)
        total = ce + W_PRIOR * prior + W_PONDER * ponder
        total.backward()
    finally:
        torch.Tensor.cuda = cuda
    enc = model.encoder
    named = [(n, p) for n, p in model.named_parameters() if p.grad is not None]
    out = {"logits": logits.detach().numpy(), "ce": np.float64(ce.item()), "ponder": np.float64(ponder.item()), "prior": np.float64(prior.item()),
           "total": np.float64(total.item()), "prior_shallow": np.float64(prior2.item()), "grad_pos_embedding_prior_shallow": gpos2.numpy(), "names": np.array([n for n, _ in named]),
           "grad_norms": np.array([float(p.grad.double().norm()) for _, p in named]), "grad_pos_embedding": enc.pos_embedding.grad.numpy(),
           "rho_token": enc.rho_token.detach().numpy(), "counter_token": enc.counter_token.detach().numpy(),
           "halting_score_layer": torch.stack(enc.halting_score_layer).detach().numpy()}
    print(f"{name}: ce {ce.item():.6f} ponder {ponder.item():.6f} prior {prior.item():.6f} total {total.item():.6f}, {len(named)} gradients")
    return out


def main():
    cls, losses = import_reference_losses()
    arrays = {}
    for name in CASES:
        for k, v in run_case(cls, losses, name).items():
            arrays[f"{name}/{k}"] = v
    np.savez_compressed(os.path.join(GA.GOLD, "avit_train.npz"), **arrays)


if __name__ == "__main__":
    main()
