"""`SpriteGenerator`: the headless `PokemonGradioGenerator` (gradio_app.py:161-465) - a description, or an uploaded image and a
description, to uint8 sprites, every stage on the HIP kernels:

    description -> TextEncoder -> inference.gradio_ddpm_sample (from noise) -> PokemonVAE.decode -> imaging.to_uint8
    image + description -> imaging.pil_to_tensor -> PokemonVAE.encode (the sampled latent) -> imaging.mix_latent
                        -> gradio_ddpm_sample(initial_latent=...) -> decode -> to_uint8

The Gradio UI, the Hugging Face download and the diffusers U-Net variant are not built; INTEGRATION.md shows how the demo
binds this class.  Both methods take one item or a list (a batch), draw their random numbers in the reference's order
(reparameterisation noise, blend noise, sampler noise) and let a caller inject every draw.
"""
from typing import Any, Dict, Optional

import torch

from . import imaging
from ._lib import PsgError
from .guidance import ddim_sample, encode_null_text
from .inference import gradio_ddpm_sample, load_unet_checkpoint
from .objective import prediction_name
from .text_encoder import TextEncoder
from .unet import UNet
from .vae import PokemonVAE

__all__ = ["SpriteGenerator"]


class SpriteGenerator:
    """Built from modules that already live on the GPU: a `PokemonVAE`, a U-Net (any module called as
    `unet(latent, timesteps, text_emb)`), a `TextEncoder` and the linear schedule's constants (gradio_app.py:241-247)."""

    def __init__(self, vae: PokemonVAE, unet: torch.nn.Module, text_encoder: TextEncoder, num_timesteps: int = 1000,
                 beta_start: float = 0.0001, beta_end: float = 0.02, image_size: int = 215, prediction=None):
        self.vae, self.unet, self.text_encoder = vae.eval(), unet.eval(), text_encoder.eval()       # :237-239
        self.prediction_type = prediction_name(prediction)      # what the U-Net returns ("epsilon" / "v_prediction"): both samplers take it
        self.num_timesteps, self.beta_start, self.beta_end = int(num_timesteps), float(beta_start), float(beta_end)
        self.image_size = int(image_size)
        self.latent_dim = vae.latent_dim

    @classmethod
    def from_checkpoints(cls, vae_path: str, diffusion_path: str, config: Dict[str, Any], compute_dtype: torch.dtype = torch.float32,
                         device=None, use_ema: bool = False, **text_encoder_kw):
        """:186-277 with the custom U-Net - `config` is the reference's config dict (its 'model' section is read; a flat dict
        of those keys is taken as that section).  'vae_state_dict', 'unet_state_dict' and the stage-1 checkpoint's optional
        'text_encoder_state_dict', as `FinalPokemonGenerator.from_checkpoints` reads them.  device=None: the current GPU.
        `use_ema`: the U-Net takes the checkpoint's 'ema_unet_state_dict' (inference.load_unet_state; an error if it has none).
        The checkpoint's 'prediction_type' (written by a trainer with training.prediction_type = "v_prediction") decides how the
        samplers read the U-Net's output."""
        cfg = config.get("model", config)
        latent_dim, text_dim = cfg.get("latent_dim", 8), cfg.get("text_embedding_dim", 768)
        unet_state, prediction = load_unet_checkpoint(diffusion_path, use_ema=use_ema)        # (first: refused before anything is built)
        vae_ckpt = torch.load(vae_path, map_location="cpu")
        vae = PokemonVAE(latent_dim=latent_dim, text_dim=text_dim, compute_dtype=compute_dtype)
        vae.load_state_dict(vae_ckpt["vae_state_dict"])
        unet = UNet(latent_dim=latent_dim, text_dim=text_dim, time_emb_dim=cfg.get("time_emb_dim", 128), num_heads=cfg.get("num_heads", 8),
                    compute_dtype=compute_dtype)
        unet.load_state_dict(unet_state)
        te = TextEncoder(model_name=cfg.get("bert_model", "google-bert/bert-base-uncased"), hidden_dim=text_dim,
                         finetune_strategy=cfg.get("bert_finetune_strategy", "minimal"), compute_dtype=compute_dtype, **text_encoder_kw)
        if "text_encoder_state_dict" in vae_ckpt:
            te.load_state_dict(vae_ckpt["text_encoder_state_dict"])
        if device is None:
            if not torch.cuda.is_available():
                raise PsgError("SpriteGenerator.from_checkpoints needs a GPU: the HIP kernels are the only implementation")
            device = torch.device("cuda", torch.cuda.current_device())
        return cls(vae.to(device), unet.to(device), te.to(device), num_timesteps=cfg.get("num_timesteps", 1000),
                   beta_start=cfg.get("beta_start", 0.0001), beta_end=cfg.get("beta_end", 0.02), prediction=prediction)

    # -- helpers ---------------------------------------------------------------------------------------------------------
    def _device(self):
        return next(self.vae.parameters()).device

    def _encode_text(self, descriptions):
        """[B, S, text_dim] from a string, a list of strings, or (input_ids, attention_mask) token tensors."""
        if isinstance(descriptions, str):
            descriptions = [descriptions]
        if isinstance(descriptions, tuple) and len(descriptions) in (2, 3) and all(isinstance(t, torch.Tensor) for t in descriptions):
            return self.text_encoder.encode_ids(*descriptions)
        return self.text_encoder(list(descriptions))

    def _null_text(self, descriptions, S):
        """[S, text_dim]: the empty description encoded to the prompts' token length."""
        like = descriptions[:2] if isinstance(descriptions, tuple) else None
        return encode_null_text(self.text_encoder, S, like)

    def _sample(self, text_emb, num_inference_steps, initial_latent, noise_fn, sampler="gradio", guidance_scale=None, eta=0.0,
                clip=3.0, descriptions=None):
        null = self._null_text(descriptions, text_emb.shape[1]) if guidance_scale is not None else None
        if sampler == "gradio":
            kw = {} if guidance_scale is None else {"guidance_scale": guidance_scale, "null_text": null}
            if self.prediction_type != "epsilon":
                kw["prediction"] = self.prediction_type
            return gradio_ddpm_sample(self.unet, text_emb, num_inference_steps, initial_latent=initial_latent,
                                      num_timesteps=self.num_timesteps, beta_start=self.beta_start, beta_end=self.beta_end,
                                      latent_dim=self.latent_dim, noise_fn=noise_fn, **kw)
        if sampler != "ddim":
            raise PsgError(f"sampler={sampler!r} (\"gradio\" or \"ddim\")")
        betas = torch.linspace(self.beta_start, self.beta_end, self.num_timesteps)        # the demo's linear schedule (:279-288)
        return ddim_sample(self.unet, text_emb, torch.cumprod(1.0 - betas, dim=0), num_inference_steps, eta, guidance_scale, null, clip,
                           initial_latent, noise_fn, latent_dim=self.latent_dim, prediction=self.prediction_type)

    @staticmethod
    def _seed(seed):
        if seed is not None:
            torch.manual_seed(seed)                # (seeds every device's generator too)

    @staticmethod
    def _finish(images, as_pil, single):
        out = imaging.to_uint8(images)
        if not as_pil:
            return out
        pil = [imaging.tensor_to_pil(o) for o in out]
        return pil[0] if single else pil

    # -- :363-392 --------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def generate_from_text(self, descriptions, num_inference_steps: int = 50, seed: Optional[int] = None, noise_fn=None,
                           as_pil: bool = False, sampler: str = "gradio", guidance_scale: Optional[float] = None, eta: float = 0.0,
                           clip: float = 3.0):
        """uint8 [B, S, S, 3] on the device (S = 215).  `noise_fn(i, shape)`: `gradio_ddpm_sample`'s - i = -1 the initial
        latent, i >= 0 the i-th sampler draw.  as_pil=True: PIL images instead (one image for one string, else a list).
        Opt-in: sampler="ddim" (guidance.ddim_sample over the demo's linear schedule, with `eta` and `clip`) and
        `guidance_scale` (either sampler; the null text is the empty description at the prompts' token length)."""
        self._seed(seed)
        text_emb = self._encode_text(descriptions)
        latent = self._sample(text_emb, num_inference_steps, None, noise_fn, sampler, guidance_scale, eta, clip, descriptions)
        return self._finish(self.vae.decode(latent, text_emb), as_pil, isinstance(descriptions, str))

    # -- :394-438 --------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def generate_from_image_and_text(self, images, descriptions, num_inference_steps: int = 50, noise_strength: float = 0.7,
                                     seed: Optional[int] = None, eps=None, noise=None, noise_fn=None, as_pil: bool = False,
                                     sampler: str = "gradio", guidance_scale: Optional[float] = None, eta: float = 0.0,
                                     clip: float = 3.0):
        """`images`: one upload (PIL image, uint8 array or tensor, any size) or a list of them, one per description.  `eps`:
        the encoder's reparameterisation noise, `noise`: the blend's (both default to randn draws, [B, latent_dim, 27, 27]);
        noise_strength <= 0 skips the blend and draws nothing for it.  sampler / guidance_scale / eta / clip: as
        generate_from_text; the blended latent is the chain's initial latent and the full chain runs, as with "gradio"."""
        self._seed(seed)
        dev = self._device()
        single = not isinstance(images, (list, tuple))
        batch = [imaging.pil_to_tensor(im, self.image_size, dev) for im in ([images] if single else images)]
        x = torch.stack(batch) if batch[0].dim() == 3 else torch.cat(batch)
        latent, _, _ = self.vae.encode(x, eps=eps)
        if noise_strength > 0:
            if noise is None:
                noise = torch.randn_like(latent)
            latent = imaging.mix_latent(latent, noise, noise_strength)
        text_emb = self._encode_text(descriptions)
        if text_emb.shape[0] != latent.shape[0]:
            raise PsgError(f"generate_from_image_and_text: {latent.shape[0]} image(s) but {text_emb.shape[0]} description(s)")
        latent = self._sample(text_emb, num_inference_steps, latent, noise_fn, sampler, guidance_scale, eta, clip, descriptions)
        return self._finish(self.vae.decode(latent, text_emb), as_pil, single)
