"""Stage 1 (src/training/vae_trainer.py): the VAE and the text encoder trained together, one step at a time.

`VAEStepper` is one batch of VAETrainer.train_epoch (:314-345) and what surrounds it in the trainer: the two param groups
(`vae` at `learning_rate`, `text_encoder` at `text_encoder_lr`, default 0.1 x - :161-175), AdamW or Adam (:178-187), the
per-epoch scheduler (:192-209, advanced by `end_epoch()`), the KL-weight annealing (:225-234) inside `compute_vae_loss`
(:249-286), the two `clip_grad_norm_` calls (max norm 1.0 for the VAE, 0.5 for the text encoder, :341-342) and the checkpoint's
keys (:517-526).  Like `FinalStepper` it returns device scalars and never synchronises with the host inside a step.

Two update paths over the same modules:

  * `update="grouped"` (default): every stepped parameter lives in ONE `ParamArena` / `GradArena` pair, VAE first; the
    backward kernels write the gradients into the arena (`ops.GradSink`), `GradArena.group_norm_sq` reduces both groups' norms
    in one deterministic pass and `GroupedAdamW.step` clips and updates both groups in one launch.
  * `update="torch"`: torch.optim.AdamW / Adam and two `clip_grad_norm_` calls over the separate tensors - the reference's
    own sequence, kept as the twin the tests compare against and as the baseline of tools/bench_vae_step.py.

What is stepped: every VAE parameter, and the text encoder's `requires_grad` parameters except `bert.pooler.*`.  The pooler is
trainable under 'minimal' / 'partial' as in the reference but never receives a gradient (`last_hidden_state` is returned), so
the reference's optimizer skips it (grad is None): it never moves there, and a zero gradient in the arena would decay it.  The
frozen parameters and the pooler stay out of the arenas.

Not built: multi-GPU stage 1, `compute_free_bits_kl` (defined by the reference, never called), logging and sample grids.
"""
import copy
from typing import Any, Dict, Optional

import torch

from ._lib import PsgError
from .ops import WeightCache
from .optim import GradArena, GroupedAdamW, ParamArena

__all__ = ["VAEStepper", "kl_weight_at"]

# keyword -> (section of the reference's config dict, default); `text_encoder_lr` None = 0.1 x learning_rate (:162)
_KEYS = {
    "learning_rate": ("optimization", 1e-4), "text_encoder_lr": ("optimization", None), "optimizer": ("optimization", "adamw"),
    "weight_decay": ("optimization", 0.01), "beta1": ("optimization", 0.9), "beta2": ("optimization", 0.999),
    "scheduler": ("optimization", "constant"), "step_size": ("optimization", 30), "gamma": ("optimization", 0.1),
    "vae_epochs": ("training", 100), "kl_annealing": ("training", True), "kl_anneal_start": ("training", 0),
    "kl_anneal_end": ("training", 50), "kl_weight_start": ("training", 0.0), "kl_weight_end": ("training", 1.0),
}
_OWN = {"update": "grouped", "vae_clip_norm": 1.0, "text_clip_norm": 0.5}       # not in the reference's config
PARTS = ("total_loss", "reconstruction_loss", "perceptual_loss", "kl_loss")


def kl_weight_at(epoch, start, end, weight_start, weight_end):
    """vae_trainer.py:225-234."""
    if epoch < start:
        return weight_start
    if epoch >= end:
        return weight_end
    progress = (epoch - start) / (end - start)
    return weight_start + progress * (weight_end - weight_start)


def _snapshot(obj):
    """A state dict with every tensor cloned (the live ones are views of the arenas, which the next step rewrites)."""
    if torch.is_tensor(obj):
        return obj.detach().clone()
    if isinstance(obj, dict):
        return type(obj)((k, _snapshot(v)) for k, v in obj.items())
    if isinstance(obj, (list, tuple)):
        return type(obj)(_snapshot(v) for v in obj)
    return copy.copy(obj)


class VAEStepper:
    """VAEStepper(vae, text_encoder, criterion, config=None, **keywords): `config` is the reference's config dict (its
    'optimization' and 'training' sections are read), keywords override it: learning_rate, text_encoder_lr, optimizer ('adamw' |
    'adam'; 'grouped' / 'torch' are accepted as 'adamw' with that `update`), weight_decay, beta1, beta2 (read for 'adam' only,
    as in the reference), scheduler ('constant' | 'cosine' | 'step'), step_size, gamma, vae_epochs, kl_annealing,
    kl_anneal_start, kl_anneal_end, kl_weight_start, kl_weight_end, and this class's own update ('grouped' | 'torch'),
    vae_clip_norm (1.0), text_clip_norm (0.5).  `criterion` is a `CombinedLoss`."""

    def __init__(self, vae, text_encoder, criterion, config: Optional[Dict[str, Any]] = None, **kw):
        unknown = set(kw) - set(_KEYS) - set(_OWN)
        if unknown:
            raise TypeError(f"VAEStepper: unknown keyword(s) {sorted(unknown)}")
        cfg = {k: (config or {}).get(section, {}).get(k, default) for k, (section, default) in _KEYS.items()}
        cfg.update(_OWN)
        cfg.update(kw)
        if cfg["optimizer"] in ("grouped", "torch"):
            if "update" in kw and kw["update"] != cfg["optimizer"]:
                raise ValueError(f"optimizer={cfg['optimizer']!r} contradicts update={kw['update']!r}")
            cfg["update"], cfg["optimizer"] = cfg["optimizer"], "adamw"
        if cfg["optimizer"] not in ("adam", "adamw"):
            raise ValueError(f"Unknown optimizer: {cfg['optimizer']}")
        if cfg["update"] not in ("grouped", "torch"):
            raise ValueError(f"Unknown update: {cfg['update']}")
        if cfg["scheduler"] not in ("constant", "cosine", "step"):
            raise ValueError(f"Unknown scheduler: {cfg['scheduler']}")
        if cfg["text_encoder_lr"] is None:
            cfg["text_encoder_lr"] = cfg["learning_rate"] * 0.1
        self.config = cfg
        self.vae, self.text_encoder, self.criterion = vae, text_encoder, criterion
        if not getattr(vae, "trainable", False) or not all(p.requires_grad for p in vae.parameters()):
            raise PsgError("VAEStepper: the VAE is frozen (build it with PokemonVAE(..., trainable=True))")
        if not getattr(text_encoder, "trainable", False):
            raise PsgError("VAEStepper: the text encoder is frozen (build it with TextEncoder(..., trainable=True))")
        self.vae_params = list(vae.parameters())
        self.text_params = [p for n, p in text_encoder.named_parameters() if p.requires_grad and not n.startswith("bert.pooler.")]
        if not self.text_params:
            raise PsgError("VAEStepper: the text encoder has no trainable parameter")
        self.clip_norms = [float(cfg["vae_clip_norm"]), float(cfg["text_clip_norm"])]
        groups = [{"params": self.vae_params, "lr": cfg["learning_rate"], "name": "vae"},
                  {"params": self.text_params, "lr": cfg["text_encoder_lr"], "name": "text_encoder"}]
        # :178-187 - Adam takes the betas and no weight decay, AdamW the weight decay and torch's betas
        adam = cfg["optimizer"] == "adam"
        betas = (cfg["beta1"], cfg["beta2"]) if adam else (0.9, 0.999)
        weight_decay = 0.0 if adam else cfg["weight_decay"]
        self.update = cfg["update"]
        self.params = self.arena = None
        if self.update == "grouped":
            both = self.vae_params + self.text_params
            self.params = ParamArena(both)                 # flat fp32 masters, spatial conv weights OHWI
            self.arena = GradArena(both)                   # every gradient kernel writes its sink
            self.optimizer = GroupedAdamW(groups, self.params, self.arena, betas=betas, weight_decay=weight_decay)
        elif adam:
            self.optimizer = torch.optim.Adam(groups, betas=betas)
        else:
            self.optimizer = torch.optim.AdamW(groups, weight_decay=weight_decay)
        sched = torch.optim.lr_scheduler
        if cfg["scheduler"] == "cosine":                   # :192-209, stepped once per epoch
            self.scheduler = sched.CosineAnnealingLR(self.optimizer, T_max=cfg["vae_epochs"])
        elif cfg["scheduler"] == "step":
            self.scheduler = sched.StepLR(self.optimizer, step_size=cfg["step_size"], gamma=cfg["gamma"])
        else:
            self.scheduler = sched.LambdaLR(self.optimizer, lr_lambda=lambda epoch: 1.0)
        self.epoch, self.global_step, self.best_val_loss = 0, 0, float("inf")

    # -- :225-234 ----------------------------------------------------------------------------------------------------
    def get_kl_weight(self, epoch: int) -> float:
        c = self.config
        return kl_weight_at(epoch, c["kl_anneal_start"], c["kl_anneal_end"], c["kl_weight_start"], c["kl_weight_end"])

    def learning_rates(self):
        """(vae, text_encoder) - what the next step uses."""
        return tuple(float(g["lr"]) for g in self.optimizer.param_groups)

    def end_epoch(self):
        """The trainer's per-epoch `scheduler.step()` (:579); the next step reads the new learning rates."""
        self.scheduler.step()
        self.epoch += 1

    # -- :249-286 ----------------------------------------------------------------------------------------------------
    def _loss(self, images, input_ids, attention_mask, eps):
        """(total, parts [total, reconstruction, perceptual, kl] on the device, kl_weight).  With annealing on, the criterion's
        sum with its kl_weight replaced by the annealed one (what :262-273 recomputes); off, the criterion's own weights."""
        text_emb = self.text_encoder.encode_ids(input_ids, attention_mask)
        out = self.vae(images, text_emb, mode="train", eps=eps)
        klw = self.get_kl_weight(self.epoch)
        crit = self.criterion
        own = crit.kl_weight
        if self.config["kl_annealing"]:
            crit.kl_weight = klw
        try:
            total, parts = crit.forward_tensors(out["reconstructed"], images, out["mu"], out["logvar"])
        finally:
            crit.kl_weight = own
        return total, parts, klw

    def optimizer_phase(self):
        """The end of `train_step`, on the gradients that are there: both groups' norms, then clip + update.  Returns the
        (VAE, text encoder) gradient norms before clipping, device scalars."""
        if self.update == "grouped":
            normsq = self.optimizer.group_norm_sq()
            norms = normsq.sqrt()
            self.optimizer.step(normsq=normsq, max_norms=self.clip_norms)
            self.text_encoder.drop_prepared()              # its packed operands are stamped by version counters only
            return norms[0], norms[1]
        norm_vae = torch.nn.utils.clip_grad_norm_(self.vae_params, self.clip_norms[0])           # :341
        norm_text = torch.nn.utils.clip_grad_norm_(self.text_params, self.clip_norms[1])         # :342
        self.optimizer.step()
        return norm_vae, norm_text

    def train_step(self, images, input_ids, attention_mask, eps=None) -> Dict[str, Any]:
        total, parts, klw = self._loss(images, input_ids, attention_mask, eps)
        if self.update == "grouped":
            self.arena.zero()
            total.backward()
            self.arena.finalize()                          # (joins the weight-gradient side stream; unwritten sinks get zeros)
        else:
            self.optimizer.zero_grad(set_to_none=True)
            total.backward()
        norm_vae, norm_text = self.optimizer_phase()
        self.global_step += 1
        out = dict(zip(PARTS, parts.unbind(0)))
        out.update(kl_weight=klw, grad_norm_vae=norm_vae, grad_norm_text=norm_text)
        return out

    @torch.no_grad()
    def validate_step(self, images, input_ids, attention_mask, eps=None) -> Dict[str, Any]:
        _, parts, klw = self._loss(images, input_ids, attention_mask, eps)
        out = dict(zip(PARTS, parts.unbind(0)))
        out["kl_weight"] = klw
        return out

    # -- :517-556 ----------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, Any]:
        return {"epoch": self.epoch, "vae_state_dict": _snapshot(self.vae.state_dict()),
                "text_encoder_state_dict": _snapshot(self.text_encoder.state_dict()),
                "optimizer_state_dict": _snapshot(self.optimizer.state_dict()),
                "scheduler_state_dict": _snapshot(self.scheduler.state_dict()), "global_step": self.global_step,
                "best_val_loss": self.best_val_loss}

    def load_state_dict(self, state: Dict[str, Any]):
        self.vae.load_state_dict(state["vae_state_dict"])            # (in place: the parameters stay views of the arena)
        self.text_encoder.load_state_dict(state["text_encoder_state_dict"])
        self.optimizer.load_state_dict(state["optimizer_state_dict"])
        self.scheduler.load_state_dict(state["scheduler_state_dict"])
        self.epoch, self.global_step, self.best_val_loss = state["epoch"], state["global_step"], state["best_val_loss"]
        WeightCache.invalidate()
        self.text_encoder.drop_prepared()
