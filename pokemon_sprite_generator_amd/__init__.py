"""pokemon_sprite_generator_amd — MI355X-native U-Net denoising train step.

Drop-in for the hot path of GabrieleConte/pokemon-sprite-generator
(src/models/unet.py + src/training/improved_diffusion_trainer.py; the frozen VAE and BERT text encoder either side): the same
Python surface, computed by hand-written gfx950 HIP kernels in libpsg_hip.so
(C ABI: include/psg_hip.h).  Importing the package never touches the GPU; using
any op without the built library raises (no CPU fallback).
"""
from ._lib import LIB_PATH, PsgError
from .scheduler import NoiseScheduler
from .unet import CrossAttentionBlock, ResBlock, TimestepEmbedding, UNet, UNetBlock
from .optim import FusedAdamW, GradArena, GroupedAdamW, ParamArena
from .ddp import BucketedAllReduce
from .trainer import DiffusionStepper, DiffusionTrainer, ImprovedDiffusionTrainer
from .inference import LatentGenerator, LinearNoiseScheduler, gradio_ddpm_sample, load_unet_state
from .guidance import DdimRun, cfg_combine, ddim_sample, ddim_tables, ddim_timesteps, text_cond_drop
from .objective import diffusion_loss, min_snr_weights, pred_to_eps, v_target
from .vae import PokemonVAE, VAEDecoder, VAEEncoder
from .text_encoder import TextEncoder
from .losses import CombinedLoss, VGGPerceptualLoss
from .clip_loss import CLIPLoss
from .final import FinalPokemonGenerator, FinalStepper
from .vae_stepper import VAEStepper
from .data import SpriteDataset, SpriteLoader, TokenTable, create_data_loaders, draw_params
from .vae_trainer import VAETrainer
from .final_trainer import FinalTrainer
from .generate import SpriteGenerator

__all__ = ["UNet", "UNetBlock", "ResBlock", "CrossAttentionBlock", "TimestepEmbedding", "NoiseScheduler",
           "ImprovedDiffusionTrainer", "DiffusionTrainer", "DiffusionStepper", "FusedAdamW", "GradArena", "ParamArena",
           "BucketedAllReduce", "LatentGenerator", "LinearNoiseScheduler", "gradio_ddpm_sample", "load_unet_state", "PokemonVAE", "VAEEncoder", "VAEDecoder", "TextEncoder", "VGGPerceptualLoss", "CombinedLoss", "CLIPLoss",
           "FinalPokemonGenerator", "FinalStepper", "GroupedAdamW", "VAEStepper", "SpriteDataset", "SpriteLoader", "create_data_loaders", "draw_params", "SpriteGenerator", "VAETrainer", "FinalTrainer", "TokenTable", "PsgError", "LIB_PATH",
           "DdimRun", "ddim_sample", "ddim_tables", "ddim_timesteps", "cfg_combine", "text_cond_drop",
           "diffusion_loss", "min_snr_weights", "pred_to_eps", "v_target"]
__version__ = "0.1.0"
