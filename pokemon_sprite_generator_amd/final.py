"""Stage 3 (src/training/final_trainer.py): the BERT text encoder fine-tuned THROUGH the VAE decoder, then both together.

  * `FinalPokemonGenerator` - final_trainer.py:85-256 with the reference's method names.  `encode_and_decode` (:215-236) is
    the training forward: descriptions through the trainable `TextEncoder`, images through the frozen `VAEEncoder` under
    no_grad, then the `VAEDecoder` on its differentiable path, so the image loss reaches `text_emb` and the encoder's
    last layers.  `forward(mode='generate')` (:165-213) is `LatentGenerator`'s strided sampler followed by the decoder.
  * `FinalStepper` - one step of FinalTrainer.train_epoch (:458-485): forward, L1 + 0.1 * MSE (psg_recon_loss_f32, :425-440),
    backward, ONE clip_grad_norm_(1.0) over everything stepped, the optimizer step - and what surrounds it in the trainer: the
    param groups (:383-389, :601-617), AdamW / Adam (:392-401), the per-epoch scheduler (:404-414), `switch_to_joint_training`
    (:590-642) and the checkpoint's keys (:646-655).

Both phases are built.  The text-encoder phase trains the text encoder through the frozen decoder.  The joint phase
(`FinalStepper.switch_to_joint_training`) is opt-in, as stage 1 is: it exists for a generator whose decoder was built with
`VAEDecoder(..., trainable=True)` (`from_checkpoints(..., trainable_decoder=True)`); `unfreeze_vae_decoder` / `unfreeze_unet`
of any other generator raise.  Until the switch such a decoder is frozen and runs as a default one: the same bits, data
gradients only, no weight-gradient launch, prepared weights from `WeightCache` (`VAEDecoder.live_weights`).  The U-Net is
unfrozen by the switch, as in the reference, and nothing else happens to it: `encode_and_decode` never calls it, so no
gradient ever reaches it there and its optimizer group never moves (see `FinalStepper`).

`clip_loss` is an optional callable `(reconstruction, texts) -> scalar`: `clip_loss.CLIPLoss` is the reference's
(final_trainer.py:469-473), with `texts` a list of descriptions or an int64 tensor of CLIP token ids.

Not built: multi-GPU stage 3, a U-Net param group and optimizer-state interchange with the reference's three-group optimizer,
logging, TensorBoard and sample grids, the diffusers variant.
"""
from typing import Any, Callable, Dict, List, Optional

import torch
import torch.nn as nn

from . import ops
from ._lib import PsgError
from .inference import LatentGenerator, LinearNoiseScheduler, load_unet_checkpoint, refuse_v_prediction
from .ops import WeightCache
from .optim import GradArena, GroupedAdamW, ParamArena
from .text_encoder import TextEncoder
from .unet import UNet
from .vae import VAEDecoder, VAEEncoder
from .vae_stepper import _snapshot

__all__ = ["FinalPokemonGenerator", "FinalStepper"]


class FinalPokemonGenerator(nn.Module):
    """final_trainer.py:85-256, constructed from modules (`from_checkpoints` follows the reference's constructor).  `unet` may
    be None for training-only use: `encode_and_decode` never calls it."""

    def __init__(self, vae_encoder: VAEEncoder, vae_decoder: VAEDecoder, unet: Optional[UNet], text_encoder: TextEncoder,
                 noise_scheduler: Optional[LinearNoiseScheduler] = None):
        super().__init__()
        self.vae_encoder, self.vae_decoder, self.unet, self.text_encoder = vae_encoder, vae_decoder, unet, text_encoder
        self.noise_scheduler = noise_scheduler or LinearNoiseScheduler()
        self.latent_dim = vae_decoder.latent_dim
        self.freeze_vae_encoder()
        self.freeze_vae_decoder()
        self.freeze_unet()

    @classmethod
    def from_checkpoints(cls, vae_path: str, diffusion_path: str, text_encoder_config: Dict[str, Any],
                         compute_dtype: torch.dtype = torch.float32, trainable_decoder: bool = False, use_ema: bool = False, **text_encoder_kw):
        """:90-160 - 'vae_state_dict' split into its encoder. / decoder. halves, 'unet_state_dict', and the stage-1
        checkpoint's optional 'text_encoder_state_dict'.  `trainable_decoder`: build the decoder with `trainable=True`, which
        the joint phase needs (it starts frozen either way).  `use_ema`: the U-Net takes the checkpoint's 'ema_unet_state_dict'
        (inference.load_unet_state; an error if it has none).  A checkpoint trained with training.prediction_type =
        "v_prediction" is refused: this class samples with stage 3's eps-only loop."""
        cfg = text_encoder_config
        latent_dim, text_dim = cfg.get("latent_dim", 8), cfg["text_embedding_dim"]
        unet_state, prediction = load_unet_checkpoint(diffusion_path, use_ema=use_ema)        # (first: refused before anything is built)
        refuse_v_prediction(prediction, f"FinalPokemonGenerator.from_checkpoints({diffusion_path})")
        vae_ckpt = torch.load(vae_path, map_location="cpu")
        enc = VAEEncoder(input_channels=3, latent_dim=latent_dim, compute_dtype=compute_dtype)
        dec = VAEDecoder(latent_dim=latent_dim, text_dim=text_dim, output_channels=3, compute_dtype=compute_dtype,
                         trainable=trainable_decoder)
        vsd = vae_ckpt["vae_state_dict"]
        enc.load_state_dict({k[8:]: v for k, v in vsd.items() if k.startswith("encoder.")})
        dec.load_state_dict({k[8:]: v for k, v in vsd.items() if k.startswith("decoder.")})
        unet = UNet(latent_dim=latent_dim, text_dim=text_dim, time_emb_dim=cfg.get("time_emb_dim", 128), num_heads=cfg.get("num_heads", 8),
                    compute_dtype=compute_dtype)
        unet.load_state_dict(unet_state)
        text_encoder_kw.setdefault("trainable", True)
        te = TextEncoder(model_name=cfg["bert_model"], hidden_dim=text_dim, compute_dtype=compute_dtype, **text_encoder_kw)
        if "text_encoder_state_dict" in vae_ckpt:
            te.load_state_dict(vae_ckpt["text_encoder_state_dict"])
        sch = LinearNoiseScheduler(num_timesteps=cfg.get("num_timesteps", 1000), beta_start=cfg.get("beta_start", 0.0001),
                                   beta_end=cfg.get("beta_end", 0.02))
        return cls(enc, dec, unet, te, sch)

    # -- :165-213 ----------------------------------------------------------------------------------------------------
    def forward(self, text_list: List[str], num_inference_steps: int = 50, mode: str = "generate", noise_fn=None) -> torch.Tensor:
        if mode != "generate":
            raise NotImplementedError("Reconstruction mode requires input images")
        if self.unet is None:
            raise PsgError("FinalPokemonGenerator.forward: built without a U-Net (training-only)")
        with torch.no_grad():
            text_emb = self.text_encoder(text_list)
            return LatentGenerator(self.unet, self.noise_scheduler, self.latent_dim, self.vae_decoder)(text_emb, num_inference_steps, noise_fn=noise_fn)

    # -- :215-236 ----------------------------------------------------------------------------------------------------
    def _decode_through(self, images, text_emb):
        with torch.no_grad():
            latent, _, _ = self.vae_encoder(images)
        return self.vae_decoder(latent, text_emb)

    def encode_and_decode(self, images: torch.Tensor, text_list: List[str]) -> torch.Tensor:
        return self._decode_through(images, self.text_encoder(text_list))

    def encode_and_decode_ids(self, images: torch.Tensor, input_ids: torch.Tensor, attention_mask: torch.Tensor, token_type_ids=None) -> torch.Tensor:
        """`encode_and_decode` from token ids (what `TextEncoder.encode_ids` is to its `forward`)."""
        return self._decode_through(images, self.text_encoder.encode_ids(input_ids, attention_mask, token_type_ids))

    # -- :238-256 ----------------------------------------------------------------------------------------------------
    @staticmethod
    def _set_requires_grad(module, flag):
        """Whether any parameter changed."""
        changed = False
        if module is not None:
            for p in module.parameters():
                changed |= p.requires_grad != flag
                p.requires_grad = flag
        return changed

    def _joint_phase_built(self):
        if not getattr(self.vae_decoder, "trainable", False):
            raise PsgError("joint phase not built for this generator: its VAE decoder was built frozen (data gradients only, no "
                           "weight gradients); build it with VAEDecoder(..., trainable=True), or "
                           "from_checkpoints(..., trainable_decoder=True)")

    def freeze_vae_encoder(self):
        self._set_requires_grad(self.vae_encoder, False)

    def freeze_vae_decoder(self):
        """A `trainable=True` decoder goes back to prepared weights from `WeightCache` and data gradients only."""
        if self._set_requires_grad(self.vae_decoder, False):
            WeightCache.invalidate()

    def freeze_unet(self):
        self._set_requires_grad(self.unet, False)

    def unfreeze_vae_decoder(self):
        """The joint phase (:238-241): the decoder's parameters require grad and its forward runs on the live weights."""
        self._joint_phase_built()
        if self._set_requires_grad(self.vae_decoder, True):
            WeightCache.invalidate()

    def unfreeze_unet(self):
        """:248-251.  requires_grad and nothing else (a no-op without a U-Net): the training forward never calls it."""
        self._joint_phase_built()
        self._set_requires_grad(self.unet, True)


# keyword -> (section of the reference's config dict, its key there, default); `vae_decoder_lr` None = 0.1 x lr (:609)
_KEYS = {
    "lr": ("optimization", "text_encoder_lr", 1e-5), "vae_decoder_lr": ("optimization", "vae_decoder_lr", None),
    "optimizer": ("optimization", "optimizer", "adamw"), "weight_decay": ("optimization", "weight_decay", 0.01),
    "beta1": ("optimization", "beta1", 0.9), "beta2": ("optimization", "beta2", 0.999),
    "scheduler": ("optimization", "scheduler", "constant"), "step_size": ("optimization", "step_size", 30),
    "gamma": ("optimization", "gamma", 0.1), "final_epochs": ("training", "final_epochs", 100),
}
PHASES = ("text_encoder", "joint")


def _total_norm(params):
    """The L2 norm of the gradients that are there, a device scalar (what clip_grad_norm_ computes, without the scaling)."""
    grads = [p.grad for p in params if p.grad is not None]
    return torch.linalg.vector_norm(torch.stack(torch._foreach_norm(grads)))


class FinalStepper:
    """One optimisation step of FinalTrainer.train_epoch (:458-485) and the trainer's state around it, in both phases.  The
    results are device scalars: nothing in a step synchronises with the host.  The module's train / eval mode is the caller's
    (`generator.train()` turns BERT's dropout on, as in the reference).

    FinalStepper(generator, lr, weight_decay, optimizer, max_grad_norm, config=None, **keywords): `lr` is the text encoder's
    learning rate (`text_encoder_lr` of the reference's config).  `config` is the reference's config dict (its 'optimization'
    and 'training' sections are read); arguments that are given override it: lr, vae_decoder_lr (None = 0.1 x lr, :609),
    optimizer ('adamw' | 'adam'), weight_decay, beta1, beta2 (read for 'adam' only, as in the reference), scheduler
    ('constant' | 'cosine' | 'step', stepped by `end_epoch()`), final_epochs (the cosine T_max), step_size, gamma, and this
    class's own max_grad_norm (1.0, :482) and update ('torch' | 'grouped').  Without a config, 'adam' takes `weight_decay` as
    torch.optim.Adam's (L2) term, as this class always did; with one it takes none, as the reference's does.

    Phases (`training_phase`).  'text_encoder': one param group, the text encoder at `lr`.  `switch_to_joint_training()`
    (:590-642) unfreezes the decoder and the U-Net and THROWS the optimizer and the scheduler AWAY, as the reference does: the
    new optimizer has the groups `text_encoder` at `lr` and `vae_decoder` at `vae_decoder_lr`, zero moments and step count 0,
    and the scheduler restarts from the base learning rates.  Both groups are clipped by ONE norm (:480-483).

    The reference's third group, `unet`, is left out of the optimizer: `encode_and_decode` never calls the U-Net, so in the
    reference its `.grad` stays None, clip_grad_norm_ skips it and AdamW skips it without applying weight decay - it never
    moves there, so it never moves here, and it does not go into an arena (640 M floats x 4 buffers).  An
    `optimizer_state_dict` is therefore not interchangeable with the reference's three-group one; `model_state_dict` has the
    reference's keys.

    What is stepped: the text encoder's `requires_grad` parameters except `bert.pooler.*` (trainable under 'minimal' /
    'partial' but never reached by a gradient: see vae_stepper.py), and in the joint phase every decoder parameter.

    Two update paths over the same modules:
      * `update="torch"` (default): torch.optim.AdamW / Adam over the groups and one `clip_grad_norm_` over all stepped
        parameters - the reference's own sequence, the twin the tests compare against and the baseline of
        tools/bench_final_step.py.
      * `update="grouped"`: the stepped parameters live in ONE `ParamArena` / `GradArena` pair, text encoder first (the
        reference's group order); the backward kernels write the gradients into the arena, `group_norm_sq` reduces both
        groups' norms in one pass, and `GroupedAdamW.step(..., clip_sets=[0, 0])` clips both by their shared norm and updates
        them under their own learning rates in one launch (psg_adamw_groups_sets_f32).  The switch releases the text-phase
        arenas and builds new ones over both modules."""

    def __init__(self, generator: FinalPokemonGenerator, lr: Optional[float] = None, weight_decay: Optional[float] = None,
                 optimizer: Optional[str] = None, max_grad_norm: float = 1.0, config: Optional[Dict[str, Any]] = None, **kw):
        unknown = set(kw) - set(_KEYS) - {"update"}
        if unknown:
            raise TypeError(f"FinalStepper: unknown keyword(s) {sorted(unknown)}")
        given = dict(kw, lr=lr, weight_decay=weight_decay, optimizer=optimizer)
        cfg = {k: (config or {}).get(section, {}).get(key, default) for k, (section, key, default) in _KEYS.items()}
        cfg.update({k: v for k, v in given.items() if v is not None})
        cfg.setdefault("update", "torch")
        if cfg["optimizer"] not in ("adam", "adamw"):
            raise ValueError(f"Unknown optimizer: {cfg['optimizer']}")
        if cfg["update"] not in ("grouped", "torch"):
            raise ValueError(f"Unknown update: {cfg['update']}")
        if cfg["scheduler"] not in ("constant", "cosine", "step"):
            raise ValueError(f"Unknown scheduler: {cfg['scheduler']}")
        if cfg["vae_decoder_lr"] is None:
            cfg["vae_decoder_lr"] = cfg["lr"] * 0.1
        if cfg["optimizer"] == "adam" and config is not None and weight_decay is None:
            cfg["weight_decay"] = 0.0                                      # :392-396 - the reference's Adam takes none
        if cfg["optimizer"] == "adam" and cfg["update"] == "grouped" and cfg["weight_decay"] != 0:
            raise ValueError("update='grouped' applies AdamW's decoupled weight decay; optimizer='adam' needs weight_decay=0 there")
        self.config, self.update, self.max_grad_norm = cfg, cfg["update"], max_grad_norm
        self.generator = generator
        self.params = [p for p in generator.text_encoder.parameters() if p.requires_grad]
        if not self.params:
            raise PsgError("FinalStepper: the text encoder has no trainable parameter (build it with trainable=True)")
        self.text_params = [p for n, p in generator.text_encoder.named_parameters() if p.requires_grad and not n.startswith("bert.pooler.")]
        self.decoder_params = []
        self.training_phase = "text_encoder"
        self.param_arena = self.arena = None
        self.epoch, self.global_step, self.best_val_loss = 0, 0, float("inf")
        self._setup_optimization()

    # -- :378-414, :600-642 ------------------------------------------------------------------------------------------
    def _setup_optimization(self):
        """A fresh optimizer and scheduler over the current phase's groups (and, grouped, fresh arenas)."""
        cfg = self.config
        groups = [{"params": self.text_params, "lr": cfg["lr"], "name": "text_encoder"}]
        if self.training_phase == "joint":
            groups.append({"params": self.decoder_params, "lr": cfg["vae_decoder_lr"], "name": "vae_decoder"})
        adam = cfg["optimizer"] == "adam"
        betas = (cfg["beta1"], cfg["beta2"]) if adam else (0.9, 0.999)
        if self.update == "grouped":
            for arena in (self.arena, self.param_arena):
                if arena is not None:
                    arena.release()
            stepped = self.text_params + self.decoder_params
            self.param_arena = ParamArena(stepped)         # flat fp32 masters, spatial conv weights OHWI
            self.arena = GradArena(stepped)                # every gradient kernel writes its sink
            self.optimizer = GroupedAdamW(groups, self.param_arena, self.arena, betas=betas, weight_decay=cfg["weight_decay"])
        elif adam:
            self.optimizer = torch.optim.Adam(groups, betas=betas, weight_decay=cfg["weight_decay"])
        else:
            self.optimizer = torch.optim.AdamW(groups, weight_decay=cfg["weight_decay"])
        sched = torch.optim.lr_scheduler
        if cfg["scheduler"] == "cosine":                   # stepped once per epoch (:709)
            self.scheduler = sched.CosineAnnealingLR(self.optimizer, T_max=cfg["final_epochs"])
        elif cfg["scheduler"] == "step":
            self.scheduler = sched.StepLR(self.optimizer, step_size=cfg["step_size"], gamma=cfg["gamma"])
        else:
            self.scheduler = sched.LambdaLR(self.optimizer, lr_lambda=lambda epoch: 1.0)

    def switch_to_joint_training(self):
        """:590-642.  Needs a generator whose decoder was built with trainable=True (`unfreeze_vae_decoder` raises otherwise)."""
        if self.training_phase == "joint":
            return
        self.generator.unfreeze_vae_decoder()
        self.generator.unfreeze_unet()
        self.training_phase = "joint"
        self.decoder_params = list(self.generator.vae_decoder.parameters())
        self._setup_optimization()

    def learning_rates(self):
        """(text_encoder,) or (text_encoder, vae_decoder) - what the next step uses."""
        return tuple(float(g["lr"]) for g in self.optimizer.param_groups)

    def end_epoch(self):
        """The trainer's per-epoch `scheduler.step()` (:709); the next step reads the new learning rates."""
        self.scheduler.step()
        self.epoch += 1

    # -- :425-485 ----------------------------------------------------------------------------------------------------
    def _loss(self, images, input_ids, attention_mask, clip_loss, clip_weight, texts):
        recon = self.generator.encode_and_decode_ids(images, input_ids, attention_mask)
        total, l1, mse = ops.recon_loss(recon, images)
        if clip_loss is not None:
            total = total + clip_weight * clip_loss(recon, texts)
        return total, l1, mse

    def optimizer_phase(self) -> Dict[str, torch.Tensor]:
        """The end of `train_step`, on the gradients that are there: the norms, then ONE clip over everything stepped and the
        update.  Returns `grad_norm` (the shared norm before clipping) and, in the joint phase, `grad_norm_text` and
        `grad_norm_decoder`: device scalars."""
        joint = self.training_phase == "joint"
        if self.update == "grouped":
            G = 2 if joint else 1
            normsq = self.optimizer.group_norm_sq()
            out = {"grad_norm": self.optimizer.set_norms([0] * G, normsq)[0]}
            if joint:
                norms = normsq.sqrt()
                out.update(grad_norm_text=norms[0], grad_norm_decoder=norms[1])
            self.optimizer.step(normsq=normsq, max_norms=[self.max_grad_norm] * G, clip_sets=[0] * G if joint else None)
            self.generator.text_encoder.drop_prepared()    # its packed operands are stamped by version counters only
            return out
        out = {}
        if joint:
            out.update(grad_norm_text=_total_norm(self.text_params), grad_norm_decoder=_total_norm(self.decoder_params))
        out["grad_norm"] = torch.nn.utils.clip_grad_norm_(self.params + self.decoder_params, self.max_grad_norm)     # :482
        self.optimizer.step()
        return out

    def train_step(self, images, input_ids, attention_mask, clip_loss: Optional[Callable] = None, clip_weight: float = 0.1, texts=None):
        total, l1, mse = self._loss(images, input_ids, attention_mask, clip_loss, clip_weight, texts)
        if self.update == "grouped":
            self.arena.zero()
            total.backward()
            self.arena.finalize()                          # (joins the weight-gradient side stream; unwritten sinks get zeros)
        else:
            self.optimizer.zero_grad(set_to_none=True)
            total.backward()
        out = {"loss": total.detach(), "l1_loss": l1, "mse_loss": mse}
        out.update(self.optimizer_phase())
        self.global_step += 1
        return out

    @torch.no_grad()
    def validate_step(self, images, input_ids, attention_mask, clip_loss: Optional[Callable] = None, clip_weight: float = 0.1, texts=None):
        total, l1, mse = self._loss(images, input_ids, attention_mask, clip_loss, clip_weight, texts)
        return {"loss": total, "l1_loss": l1, "mse_loss": mse}

    # -- :644-686 ----------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, Any]:
        return {"epoch": self.epoch, "model_state_dict": _snapshot(self.generator.state_dict()),
                "optimizer_state_dict": _snapshot(self.optimizer.state_dict()),
                "scheduler_state_dict": _snapshot(self.scheduler.state_dict()), "global_step": self.global_step,
                "best_val_loss": self.best_val_loss, "training_phase": self.training_phase}

    def load_state_dict(self, state: Dict[str, Any]):
        """A 'joint' checkpoint switches a stepper that is still in the text-encoder phase first; the phases do not go back."""
        phase = state.get("training_phase", "text_encoder")
        if phase not in PHASES:
            raise ValueError(f"Unknown training phase: {phase}")
        if phase == "joint":
            self.switch_to_joint_training()
        elif self.training_phase == "joint":
            raise PsgError("FinalStepper: a 'text_encoder' checkpoint cannot be loaded after switch_to_joint_training(); build a new stepper")
        self.generator.load_state_dict(state["model_state_dict"])    # (in place: the parameters stay views of the arena)
        self.optimizer.load_state_dict(state["optimizer_state_dict"])
        self.scheduler.load_state_dict(state["scheduler_state_dict"])
        self.epoch, self.global_step, self.best_val_loss = state["epoch"], state["global_step"], state["best_val_loss"]
        WeightCache.invalidate()
        self.generator.text_encoder.drop_prepared()
