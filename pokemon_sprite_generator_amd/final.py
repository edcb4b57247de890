"""Stage 3 (src/training/final_trainer.py): the BERT text encoder fine-tuned THROUGH the frozen VAE decoder.

  * `FinalPokemonGenerator` - final_trainer.py:85-256 with the reference's method names.  `encode_and_decode` (:215-236) is
    the training forward: descriptions through the trainable `TextEncoder`, images through the frozen `VAEEncoder` under
    no_grad, then the frozen `VAEDecoder` on its differentiable path, so the image loss reaches `text_emb` and the encoder's
    last layers.  `forward(mode='generate')` (:165-213) is `LatentGenerator`'s strided sampler followed by the decoder.
  * `FinalStepper` - one step of FinalTrainer.train_epoch (:458-485): forward, L1 + 0.1 * MSE (psg_recon_loss_f32, :425-440),
    backward, clip_grad_norm_(1.0), torch.optim step over the text encoder's requires_grad parameters.

Built: the text-encoder phase.  Not built: the joint phase (`unfreeze_vae_decoder` / `unfreeze_unet` raise - there are no VAE
weight gradients).  `clip_loss` is an optional callable `(reconstruction, texts) -> scalar`: `clip_loss.CLIPLoss` is the
reference's (final_trainer.py:469-473), with `texts` a list of descriptions or an int64 tensor of CLIP token ids.
"""
from typing import Any, Callable, Dict, List, Optional

import torch
import torch.nn as nn

from . import ops
from ._lib import PsgError
from .inference import LatentGenerator, LinearNoiseScheduler
from .text_encoder import TextEncoder
from .unet import UNet
from .vae import VAEDecoder, VAEEncoder

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
                         compute_dtype: torch.dtype = torch.float32, **text_encoder_kw):
        """:90-160 - 'vae_state_dict' split into its encoder. / decoder. halves, 'unet_state_dict', and the stage-1
        checkpoint's optional 'text_encoder_state_dict'."""
        cfg = text_encoder_config
        latent_dim, text_dim = cfg.get("latent_dim", 8), cfg["text_embedding_dim"]
        vae_ckpt = torch.load(vae_path, map_location="cpu")
        enc = VAEEncoder(input_channels=3, latent_dim=latent_dim, compute_dtype=compute_dtype)
        dec = VAEDecoder(latent_dim=latent_dim, text_dim=text_dim, output_channels=3, compute_dtype=compute_dtype)
        vsd = vae_ckpt["vae_state_dict"]
        enc.load_state_dict({k[8:]: v for k, v in vsd.items() if k.startswith("encoder.")})
        dec.load_state_dict({k[8:]: v for k, v in vsd.items() if k.startswith("decoder.")})
        unet = UNet(latent_dim=latent_dim, text_dim=text_dim, time_emb_dim=cfg.get("time_emb_dim", 128), num_heads=cfg.get("num_heads", 8),
                    compute_dtype=compute_dtype)
        unet.load_state_dict(torch.load(diffusion_path, map_location="cpu")["unet_state_dict"])
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
    def _freeze(module):
        if module is not None:
            for p in module.parameters():
                p.requires_grad = False

    def freeze_vae_encoder(self):
        self._freeze(self.vae_encoder)

    def freeze_vae_decoder(self):
        self._freeze(self.vae_decoder)

    def freeze_unet(self):
        self._freeze(self.unet)

    def unfreeze_vae_decoder(self):
        raise PsgError("joint phase not built: the VAE decoder has data gradients only (no weight gradients)")

    def unfreeze_unet(self):
        raise PsgError("joint phase not built: stage 3 trains the text encoder through the frozen decoder only")


class FinalStepper:
    """One optimisation step of FinalTrainer.train_epoch (:458-485) over the text encoder's requires_grad parameters.  The
    results are device scalars: nothing here synchronises with the host.  The module's train / eval mode is the caller's
    (`generator.train()` turns BERT's dropout on, as in the reference)."""

    def __init__(self, generator: FinalPokemonGenerator, lr: float = 1e-5, weight_decay: float = 0.01, optimizer: str = "adamw",
                 max_grad_norm: float = 1.0):
        self.generator = generator
        self.params = [p for p in generator.text_encoder.parameters() if p.requires_grad]
        if not self.params:
            raise PsgError("FinalStepper: the text encoder has no trainable parameter (build it with trainable=True)")
        if optimizer not in ("adam", "adamw"):
            raise ValueError(f"Unknown optimizer: {optimizer}")
        opt = torch.optim.AdamW if optimizer == "adamw" else torch.optim.Adam
        self.optimizer = opt(self.params, lr=lr, weight_decay=weight_decay)
        self.max_grad_norm = max_grad_norm

    def _loss(self, images, input_ids, attention_mask, clip_loss, clip_weight, texts):
        recon = self.generator.encode_and_decode_ids(images, input_ids, attention_mask)
        total, l1, mse = ops.recon_loss(recon, images)
        if clip_loss is not None:
            total = total + clip_weight * clip_loss(recon, texts)
        return total, l1, mse

    def train_step(self, images, input_ids, attention_mask, clip_loss: Optional[Callable] = None, clip_weight: float = 0.1, texts=None):
        total, l1, mse = self._loss(images, input_ids, attention_mask, clip_loss, clip_weight, texts)
        self.optimizer.zero_grad(set_to_none=True)
        total.backward()
        grad_norm = torch.nn.utils.clip_grad_norm_(self.params, self.max_grad_norm)
        self.optimizer.step()
        return {"loss": total.detach(), "l1_loss": l1, "mse_loss": mse, "grad_norm": grad_norm}

    @torch.no_grad()
    def validate_step(self, images, input_ids, attention_mask, clip_loss: Optional[Callable] = None, clip_weight: float = 0.1, texts=None):
        total, l1, mse = self._loss(images, input_ids, attention_mask, clip_loss, clip_weight, texts)
        return {"loss": total, "l1_loss": l1, "mse_loss": mse}
