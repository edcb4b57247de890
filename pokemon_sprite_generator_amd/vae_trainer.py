"""VAETrainer mirror (reference: src/training/vae_trainer.py:19-626): stage 1's epochs around `VAEStepper`.

The reference's surface - `__init__(config, experiment_name)`, `train()`, `train_epoch`, `validate_epoch`, `generate_samples`,
`save_checkpoint`, `load_checkpoint`, `get_kl_weight` - so `train_3stage.py` runs stage 1 when this class is imported in place
of the reference's, plus the two keywords of `ImprovedDiffusionTrainer`: `components=` and `compute_dtype=`.  The class is thin:
every number comes from `VAEStepper` (vae_stepper.py), the models are this package's `PokemonVAE(trainable=True)`,
`TextEncoder(trainable=True)` and `CombinedLoss`, the batches `data.create_data_loaders` with the text encoder's tokenizer, so
a batch brings its `input_ids` / `attention_mask` from the resident token table and the loop does no host work for the text.

Host reads: the `log_every` lines, and ONE per epoch - the steppers' device scalars are added into a device vector and read at
the epoch's end.  Nothing is ever downloaded: VGG16's weights come from `components={"criterion": CombinedLoss}` or from
`mi355x.vgg_state_dict` (a `torch.save`d state dict of torchvision's `vgg16().features`); without either the constructor raises.

Checkpoint: the stepper's `state_dict()` plus `config`, with `epoch` the epoch just finished - the reference's keys in
`vae_best_model.pth`.  `load_checkpoint` sets `current_epoch = checkpoint["epoch"]`: like the reference, a resumed run trains
that epoch again.  The train loader is pinned to the epoch (`set_epoch`), so it draws the shuffle and the augmentations that
epoch drew the first time; the sample sheet is drawn under `fork_rng`, so monitoring does not move the training random stream.

Not built: multi-GPU stage 1, the matplotlib figure (the sample sheet is a plain grid, imaging.save_sheet).
"""
import os
import time
from typing import Any, Dict, Optional

import torch

from . import _lib
from .imaging import save_sheet
from .trainer import TrainerBase

__all__ = ["VAETrainer", "batch_text_inputs", "compute_dtype_of", "make_loaders", "pin_epoch"]

_DTYPES = {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "fp32": torch.float32, "float32": torch.float32}


def compute_dtype_of(config, compute_dtype):
    """The keyword when given, else `mi355x.dtype` (stages 1 and 3 default to fp32, the reference's precision)."""
    if compute_dtype is not None:
        return compute_dtype
    return _DTYPES[str((config.get("mi355x", {}) or {}).get("dtype", "fp32"))]


def batch_text_inputs(batch, text_encoder, device):
    """(input_ids, attention_mask) of a batch: the loader's (data.TokenTable) when it carries them, else the tokenizer call on
    `full_description` (an injected loader)."""
    if "input_ids" in batch:
        return batch["input_ids"], batch["attention_mask"]
    enc = text_encoder.tokenize(batch["full_description"])
    return enc["input_ids"].to(device), enc["attention_mask"].to(device)


def pin_epoch(loader, epoch):
    if hasattr(loader, "set_epoch"):
        loader.set_epoch(epoch)


def make_loaders(trainer, text_encoder, batch_size):
    """{"train", "val", "test"} of a stage-1 / stage-3 trainer: injected (`components["data_loaders"]`), or this package's with
    the text encoder's tokenizer (`components["tokenizer"]` first), so the three loaders share one token table."""
    comps = trainer._components
    if "data_loaders" in comps:
        return dict(comps["data_loaders"])
    dc = trainer.config["data"]
    kw = {}
    tok = comps.get("tokenizer", getattr(text_encoder, "tokenizer", None))
    if tok is not None:
        tok.padding_side = "right"
        kw["tokenizer"] = tok
    tr, va, te = trainer._component("create_data_loaders")(
        csv_path=dc["csv_path"], image_dir=dc["image_dir"], batch_size=batch_size, val_split=dc["val_split"],
        test_split=dc["test_split"], image_size=dc["image_size"], num_workers=dc.get("num_workers", 0),
        pin_memory=dc.get("pin_memory", False), **kw)
    trainer.logger.info(f"Data loaders created - Train: {len(tr)} batches, Val: {len(va)} batches")
    return {"train": tr, "val": va, "test": te}


class VAETrainer(TrainerBase):
    """Drop-in for the reference class of the same name (stage 1: the VAE and the text encoder trained together).

    components: instances `vae`, `text_encoder`, `criterion`, `data_loaders` ({"train", "val"[, "test"]}), `tokenizer` (for the
    token table when the text encoder has none), or the factory `create_data_loaders`.  `mi355x` keys read here: `dtype`,
    `update` ("grouped" | "torch", VAEStepper's), `vgg_state_dict`."""
    LOG_FILE = "vae_training.log"

    def __init__(self, config: Dict[str, Any], experiment_name: str = "pokemon_vae", components: Optional[Dict[str, Any]] = None,
                 compute_dtype: Optional[torch.dtype] = None):
        self.config, self.experiment_name = config, experiment_name
        self._components = components or {}
        self._mi = config.get("mi355x", {}) or {}
        self.compute_dtype = self.vae_dtype = self.text_dtype = compute_dtype_of(config, compute_dtype)
        self._gpu_data = True                      # (this package's loader, inside the reference tree too)
        if not torch.cuda.is_available():
            raise _lib.PsgError("VAETrainer (MI355X build) needs a GPU; there is no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device())
        print(f"Using device: {self.device}")
        self.setup_directories()
        self.setup_logging()
        self.setup_model()
        self.setup_data_loaders()
        self.setup_optimization()
        self.setup_monitoring()
        self.current_epoch = 0

    # -- setup ------------------------------------------------------------------------------------------------------
    def setup_model(self):
        mc, tc, comps = self.config["model"], self.config["training"], self._components
        if "text_encoder" in comps:
            self.text_encoder = comps["text_encoder"]
        else:
            self.text_encoder = self._component("TextEncoder")(
                model_name=mc["bert_model"], hidden_dim=mc["text_embedding_dim"],
                finetune_strategy=mc.get("bert_finetune_strategy", "minimal"), trainable=True).to(self.device)
        if "vae" in comps:
            self.vae = comps["vae"]
        else:
            from .vae import PokemonVAE
            self.vae = PokemonVAE(latent_dim=mc.get("latent_dim", 8), text_dim=mc["text_embedding_dim"],
                                  compute_dtype=self.compute_dtype, trainable=True).to(self.device)
        if "criterion" in comps:
            self.criterion = comps["criterion"]
        else:
            from .losses import CombinedLoss
            path = self._mi.get("vgg_state_dict")
            if not path or not os.path.exists(str(path)):
                raise _lib.PsgError("VAETrainer: no VGG16 weights for the perceptual loss - set mi355x.vgg_state_dict to a torch.save'd "
                                    f"state dict of torchvision's vgg16().features (got {path!r}), or pass "
                                    "components={'criterion': CombinedLoss(...)}; nothing is downloaded")
            sd = torch.load(path, map_location="cpu")
            sd = {(k[len("features."):] if k.startswith("features.") else k): v for k, v in sd.items() if not k.startswith("classifier.")}
            self.criterion = CombinedLoss(reconstruction_weight=tc.get("reconstruction_weight", 1.0),
                                          perceptual_weight=tc.get("perceptual_weight", 0.1), kl_weight=tc.get("kl_weight", 0.01),
                                          compute_dtype=self.compute_dtype)
            self.criterion.perceptual_loss.vgg_features.load_state_dict(sd)
            self.criterion.to(self.device)
        count = lambda m, grad=False: sum(p.numel() for p in m.parameters() if p.requires_grad or not grad)
        self.logger.info(f"VAE initialized with {count(self.vae)} parameters")
        self.logger.info(f"Total trainable parameters: VAE={count(self.vae, True):,}, TextEncoder={count(self.text_encoder, True):,}")

    def setup_data_loaders(self):
        self.data_loaders = make_loaders(self, self.text_encoder, self.config["data"]["batch_size"])

    def setup_optimization(self):
        from .vae_stepper import VAEStepper
        self.stepper = VAEStepper(self.vae, self.text_encoder, self.criterion, config=self.config,
                                  update=self._mi.get("update", "grouped"))
        self.optimizer, self.scheduler = self.stepper.optimizer, self.stepper.scheduler

    # -- state the reference keeps on the trainer: the stepper's ------------------------------------------------------------
    @property
    def global_step(self) -> int:
        return self.stepper.global_step

    @property
    def best_val_loss(self) -> float:
        return self.stepper.best_val_loss

    @best_val_loss.setter
    def best_val_loss(self, value: float):
        self.stepper.best_val_loss = value

    def get_kl_weight(self, epoch: int) -> float:
        return self.stepper.get_kl_weight(epoch)

    def _inputs(self, batch):
        ids, mask = batch_text_inputs(batch, self.text_encoder, self.device)
        return batch["image"].to(self.device), ids, mask

    # -- epochs (:292-457) --------------------------------------------------------------------------------------------
    def train_epoch(self, epoch: int) -> Dict[str, float]:
        self.current_epoch = self.stepper.epoch = epoch            # (the KL weight reads the stepper's)
        self.vae.train()
        self.text_encoder.train()
        loader = self.data_loaders["train"]
        pin_epoch(loader, epoch)
        num_batches, log_every = len(loader), self.config["training"]["log_every"]
        sums = torch.zeros(3, device=self.device)                  # total, reconstruction, kl
        start = time.time()
        for batch_idx, batch in enumerate(loader):
            r = self.stepper.train_step(*self._inputs(batch))
            sums += torch.stack([r["total_loss"], r["reconstruction_loss"], r["kl_loss"]])
            if batch_idx % log_every == 0:                         # the loop's only host reads
                self.logger.info(f"Epoch {epoch}, Batch {batch_idx}/{num_batches}, Loss: {float(r['total_loss']):.4f}, "
                                 f"Recon: {float(r['reconstruction_loss']):.4f}, KL: {float(r['kl_loss']):.4f}, "
                                 f"KL Weight: {r['kl_weight']:.4f}")
        torch.cuda.synchronize(self.device)                        # the epoch's one synchronise: wall time, then the one read
        epoch_time = time.time() - start
        total, recon, kl = (v / max(num_batches, 1) for v in sums.tolist())
        avg_batch_time = epoch_time / max(num_batches, 1)
        self.logger.info(f"Epoch {epoch} completed in {epoch_time:.1f}s, avg batch time: {avg_batch_time:.2f}s")
        return {"loss": total, "recon_loss": recon, "kl_loss": kl, "epoch_time": epoch_time, "avg_batch_time": avg_batch_time}

    def validate_epoch(self, epoch: int) -> Dict[str, float]:
        self.vae.eval()
        self.text_encoder.eval()
        self.stepper.epoch = epoch
        loader = self.data_loaders["val"]
        sums = torch.zeros(3, device=self.device)
        for batch in loader:
            r = self.stepper.validate_step(*self._inputs(batch))
            sums += torch.stack([r["total_loss"], r["reconstruction_loss"], r["kl_loss"]])
        total, recon, kl = (v / max(len(loader), 1) for v in sums.tolist())
        return {"loss": total, "recon_loss": recon, "kl_loss": kl}

    @torch.no_grad()
    def generate_samples(self, epoch: int, num_samples: int = 8):
        """:459-513 - rows real / reconstructed / sampled from the prior, of the first validation batch."""
        self.vae.eval()
        self.text_encoder.eval()
        batch = next(iter(self.data_loaders["val"]))
        images, ids, mask = self._inputs(batch)
        n = min(num_samples, images.shape[0])
        real = images[:n]
        text_emb = self.text_encoder.encode_ids(ids[:n], mask[:n])
        with torch.random.fork_rng(devices=[self.device]):         # monitoring draws nothing from the training stream
            reconstructed = self.vae(real, text_emb, mode="train")["reconstructed"]
            generated = self.vae.sample(n, text_emb, self.device)
        save_sheet([real, reconstructed, generated], self.sample_dir / f"vae_epoch_{epoch:04d}.png")
        for tag, img in (("Real_Images", real), ("VAE Reconstructed_Images", reconstructed), ("VAE Generated_Images", generated)):
            self.writer.add_images(tag, (img.float() + 1.0) / 2.0, epoch)

    # -- checkpoints (:515-556) ---------------------------------------------------------------------------------------
    def save_checkpoint(self, epoch: int, is_best: bool = False):
        if not is_best:                            # (the reference's periodic checkpoint is commented out: only the best is written)
            return
        ckpt = dict(self.stepper.state_dict(), epoch=epoch, config=self.config)
        torch.save(ckpt, self.checkpoint_dir / "vae_best_model.pth")
        self.logger.info(f"Saved best model at epoch {epoch}")

    def load_checkpoint(self, checkpoint_path: str):
        ckpt = torch.load(checkpoint_path, map_location=self.device)
        self.stepper.load_state_dict(ckpt)
        self.current_epoch = ckpt["epoch"]
        self.logger.info(f"Loaded checkpoint from epoch {self.current_epoch}")

    # -- :558-626 -----------------------------------------------------------------------------------------------------
    def train(self):
        tc = self.config["training"]
        self.logger.info(f"Starting VAE training for {tc['vae_epochs']} epochs")
        for epoch in range(self.current_epoch, tc["vae_epochs"]):
            tm = self.train_epoch(epoch)
            vm = self.validate_epoch(epoch)
            self.stepper.end_epoch()
            klw = self.get_kl_weight(epoch)
            self.logger.info(f"Train - Loss: {tm['loss']:.4f}, Recon: {tm['recon_loss']:.4f}, KL: {tm['kl_loss']:.4f}, KL Weight: {klw:.4f}")
            self.logger.info(f"Val - Loss: {vm['loss']:.4f}, Recon: {vm['recon_loss']:.4f}, KL: {vm['kl_loss']:.4f}")
            for tag, v in (("VAE Train/Loss", tm["loss"]), ("VAE Train/Recon_Loss", tm["recon_loss"]), ("VAE Train/KL_Loss", tm["kl_loss"]),
                           ("VAE Train/KL_Weight", klw), ("VAE Train/Epoch_Time", tm["epoch_time"]),
                           ("VAE Train/Batch_Time", tm["avg_batch_time"]), ("VAE Val/Loss", vm["loss"]),
                           ("VAE Val/Recon_Loss", vm["recon_loss"]), ("VAE Val/KL_Loss", vm["kl_loss"])):
                self.writer.add_scalar(tag, v, epoch)
            if epoch % tc["sample_every"] == 0:
                self.generate_samples(epoch)
            is_best = vm["loss"] < self.best_val_loss
            if is_best:
                self.best_val_loss = vm["loss"]
            if epoch % tc["save_every"] == 0 or is_best:
                self.save_checkpoint(epoch, is_best)
            self.current_epoch = epoch + 1
        self.logger.info("VAE training completed!")
        self.writer.close()
