"""FinalTrainer mirror (reference: src/training/final_trainer.py:259-745): stage 3's epochs around `FinalStepper`.

The reference's surface - `__init__(config, vae_checkpoint_path, diffusion_checkpoint_path, experiment_name)`, `train()`,
`train_epoch`, `validate_epoch`, `generate_samples`, `switch_to_joint_training`, `save_checkpoint`, `load_checkpoint` - plus
`components=` and `compute_dtype=`.  The class is thin: the generator is `FinalPokemonGenerator.from_checkpoints(...,
trainable_decoder=True)`, every step is `FinalStepper`'s, the CLIP term is `CLIPLoss`'s, and the batches come from
`data.create_data_loaders` with the text encoder's tokenizer (input_ids / attention_mask / index from the resident table).

The CLIP text side runs ONCE: the descriptions never change, so `clip.text_features` of every dataset row is computed at
set-up (chunks of the loader's batch size, `clean_text` applied, under no_grad) and a step's loss is
`clip.forward_features(recon, feats[rows])` with `rows = batch["index"]`.  That needs CLIP's tokenizer and a loader with the
token table; otherwise the loss runs CLIP's text tower per batch on `full_description`, as the reference does.

Nothing is downloaded: CLIP comes from `components={"clip_loss": CLIPLoss}` or `mi355x.clip_path` (a local CLIPModel directory
for `CLIPLoss.from_pretrained`); `components={"clip_loss": None}` trains without the term.

Differences from the reference: its `optimizer_state_dict` has a third, never-moving U-Net group (see FinalStepper), so
optimizer state does not interchange in the joint phase; with `scheduler: constant` the reference has no scheduler and crashes
at its first `scheduler.step()`, this class keeps a constant rate.  Not built: multi-GPU stage 3, the matplotlib figure.
"""
import os
from typing import Any, Dict, Optional

import torch

from . import _lib
from .imaging import save_sheet
from .trainer import TrainerBase
from .vae_trainer import batch_text_inputs, compute_dtype_of, make_loaders, pin_epoch

__all__ = ["FinalTrainer"]


class FinalTrainer(TrainerBase):
    """Drop-in for the reference class of the same name (stage 3).

    components: instances `generator` (a FinalPokemonGenerator whose decoder is `trainable=True` when the joint phase is to
    run), `clip_loss` (None: no CLIP term), `data_loaders`, `tokenizer`, or the factory `create_data_loaders`.  `mi355x` keys
    read here: `dtype`, `update` ("torch" | "grouped", FinalStepper's), `clip_path`."""
    LOG_FILE = "final_training.log"

    def __init__(self, config: Dict[str, Any], vae_checkpoint_path: str, diffusion_checkpoint_path: str,
                 experiment_name: str = "pokemon_final", components: Optional[Dict[str, Any]] = None,
                 compute_dtype: Optional[torch.dtype] = None):
        self.config, self.experiment_name = config, experiment_name
        self.vae_checkpoint_path, self.diffusion_checkpoint_path = vae_checkpoint_path, diffusion_checkpoint_path
        self._components = components or {}
        self._mi = config.get("mi355x", {}) or {}
        self.compute_dtype = self.vae_dtype = self.text_dtype = compute_dtype_of(config, compute_dtype)
        self._gpu_data = True
        if not torch.cuda.is_available():
            raise _lib.PsgError("FinalTrainer (MI355X build) needs a GPU; there is no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device())
        print(f"Using device: {self.device}")
        self.setup_directories()
        self.setup_logging()
        self.setup_model()
        self.setup_data_loaders()
        self.setup_optimization()
        self.setup_monitoring()
        self.setup_clip_text()
        self.current_epoch = 0

    # -- setup ------------------------------------------------------------------------------------------------------
    def setup_model(self):
        mc, comps = self.config["model"], self._components
        if "generator" in comps:
            self.generator = comps["generator"]
        else:
            from .final import FinalPokemonGenerator
            self.generator = FinalPokemonGenerator.from_checkpoints(
                self.vae_checkpoint_path, self.diffusion_checkpoint_path, mc, compute_dtype=self.compute_dtype, trainable_decoder=True,
                finetune_strategy=mc.get("bert_finetune_strategy", "minimal")).to(self.device)
        if "clip_loss" in comps:
            self.clip_loss = comps["clip_loss"]
        else:
            from .clip_loss import CLIPLoss
            path = self._mi.get("clip_path")
            if not path or not os.path.exists(str(path)):
                raise _lib.PsgError("FinalTrainer: no CLIP model for the alignment loss - set mi355x.clip_path to a local CLIPModel "
                                    f"directory (got {path!r}), or pass components={{'clip_loss': CLIPLoss(...)}}; nothing is downloaded")
            self.clip_loss = CLIPLoss.from_pretrained(str(path), compute_dtype=self.compute_dtype, device=self.device)
        self.logger.info("Final generator initialized")
        self.logger.info(f"Total parameters: {sum(p.numel() for p in self.generator.parameters())}")
        self.logger.info(f"Trainable parameters: {sum(p.numel() for p in self.generator.parameters() if p.requires_grad)}")

    def setup_data_loaders(self):
        self.data_loaders = make_loaders(self, self.generator.text_encoder, self.config["data"]["batch_size"])

    def setup_optimization(self):
        from .final import FinalStepper
        self.stepper = FinalStepper(self.generator, config=self.config, update=self._mi.get("update", "torch"))

    @torch.no_grad()
    def setup_clip_text(self):
        """`clip_text_features` [N, projection_dim]: the text side of the CLIP loss for every dataset row, or None (per batch)."""
        self.clip_text_features = None
        clip, loader = self.clip_loss, self.data_loaders["train"]
        dataset = getattr(loader, "dataset", None)
        if clip is None or getattr(clip, "tokenizer", None) is None or dataset is None or getattr(loader, "tokens", None) is None:
            return
        texts = [dataset.meta(i)["full_description"] for i in range(len(dataset))]
        step = max(1, int(loader.batch_size))
        feats = [clip.text_features(clip.tokenize(texts[lo:lo + step]).to(self.device)) for lo in range(0, len(texts), step)]
        self.clip_text_features = torch.cat(feats, 0)

    # -- state the reference keeps on the trainer: the stepper's ------------------------------------------------------------
    @property
    def optimizer(self):
        return self.stepper.optimizer

    @property
    def scheduler(self):
        return self.stepper.scheduler

    @property
    def training_phase(self) -> str:
        return self.stepper.training_phase

    @property
    def global_step(self) -> int:
        return self.stepper.global_step

    @property
    def best_val_loss(self) -> float:
        return self.stepper.best_val_loss

    @best_val_loss.setter
    def best_val_loss(self, value: float):
        self.stepper.best_val_loss = value

    def switch_to_joint_training(self):
        self.logger.info("Switching to joint training mode - unfreezing all parameters")
        self.stepper.switch_to_joint_training()

    def _inputs(self, batch):
        ids, mask = batch_text_inputs(batch, self.generator.text_encoder, self.device)
        return batch["image"].to(self.device), ids, mask

    def _clip_term(self, batch, sink):
        """(callable, texts) for FinalStepper.train_step: the CLIP term of the batch, which the callable also adds into `sink`
        (the epoch's `clip_loss` metric is the term itself, not a difference of sums)."""
        clip, feats = self.clip_loss, self.clip_text_features
        if clip is None:
            return None, None
        if feats is not None and "index" in batch:
            term, texts = (lambda recon, rows: clip.forward_features(recon, feats[rows])), batch["index"]
        else:
            term, texts = (lambda recon, descriptions: clip(recon, descriptions)), batch["full_description"]

        def keep(recon, texts):
            value = term(recon, texts)
            sink.add_(value.detach().reshape(1))
            return value
        return keep, texts

    # -- epochs (:446-550) --------------------------------------------------------------------------------------------
    def train_epoch(self, epoch: int) -> Dict[str, float]:
        self.generator.train()
        if self.clip_loss is not None:
            self.clip_loss.eval()
        self.stepper.epoch = epoch
        loader = self.data_loaders["train"]
        pin_epoch(loader, epoch)
        tc = self.config["training"]
        num_batches, log_every, clip_weight = len(loader), tc["log_every"], tc.get("clip_weight", 0.1)
        sums, clip_sum = torch.zeros(3, device=self.device), torch.zeros(1, device=self.device)
        for batch_idx, batch in enumerate(loader):
            before = clip_sum.clone() if batch_idx % log_every == 0 else None
            term, texts = self._clip_term(batch, clip_sum)
            r = self.stepper.train_step(*self._inputs(batch), clip_loss=term, clip_weight=clip_weight, texts=texts)
            sums += torch.stack([r["loss"], r["l1_loss"], r["mse_loss"]])
            if before is not None:                                 # the loop's only host reads
                self.logger.info(f"Epoch {epoch}, Batch {batch_idx}/{num_batches}, Phase: {self.training_phase}, "
                                 f"Total: {float(r['loss']):.4f}, L1: {float(r['l1_loss']):.4f}, MSE: {float(r['mse_loss']):.4f}, "
                                 f"CLIP: {float(clip_sum - before):.4f}")
        loss, l1, mse, clip = (v / max(num_batches, 1) for v in torch.cat([sums, clip_sum]).tolist())   # the one read of the epoch
        return {"loss": loss, "l1_loss": l1, "mse_loss": mse, "clip_loss": clip}

    def validate_epoch(self, epoch: int) -> Dict[str, float]:
        """:516-550 - no CLIP term."""
        self.generator.eval()
        loader = self.data_loaders["val"]
        sums = torch.zeros(3, device=self.device)
        for batch in loader:
            r = self.stepper.validate_step(*self._inputs(batch))
            sums += torch.stack([r["loss"], r["l1_loss"], r["mse_loss"]])
        loss, l1, mse = (v / max(len(loader), 1) for v in sums.tolist())
        return {"loss": loss, "l1_loss": l1, "mse_loss": mse}

    @torch.no_grad()
    def generate_samples(self, epoch: int, num_samples: int = 8):
        """:552-588 - rows real / generated from the descriptions, of the first validation batch."""
        self.generator.eval()
        batch = next(iter(self.data_loaders["val"]))
        real = batch["image"][:num_samples].to(self.device)
        with torch.random.fork_rng(devices=[self.device]):         # monitoring draws nothing from the training stream
            generated = self.generator(batch["full_description"][:num_samples])
        save_sheet([real, generated], self.sample_dir / f"final_epoch_{epoch:04d}.png")
        for tag, img in (("Real_Images", real), ("Generated_Images", generated)):
            self.writer.add_images(tag, (img.float() + 1.0) / 2.0, epoch)

    # -- checkpoints (:644-686) ---------------------------------------------------------------------------------------
    def save_checkpoint(self, epoch: int, is_best: bool = False):
        if not is_best:                            # (the reference's periodic checkpoint is commented out: only the best is written)
            return
        ckpt = dict(self.stepper.state_dict(), epoch=epoch, config=self.config)
        torch.save(ckpt, self.checkpoint_dir / "final_best_model.pth")
        self.logger.info(f"Saved best model at epoch {epoch}")

    def load_checkpoint(self, checkpoint_path: str):
        ckpt = torch.load(checkpoint_path, map_location=self.device)
        self.stepper.load_state_dict(ckpt)         # (a 'joint' checkpoint switches the stepper first)
        self.current_epoch = ckpt["epoch"]
        self.logger.info(f"Loaded checkpoint from epoch {self.current_epoch}")
        self.logger.info(f"Training phase: {self.training_phase}")

    # -- :688-745 -----------------------------------------------------------------------------------------------------
    def train(self):
        tc = self.config["training"]
        self.logger.info(f"Starting final training for {tc['final_epochs']} epochs")
        phase1_epochs = tc.get("phase1_epochs", tc["final_epochs"] // 2)
        for epoch in range(self.current_epoch, tc["final_epochs"]):
            self.logger.info(f"Epoch {epoch + 1}/{tc['final_epochs']}")
            if epoch == phase1_epochs and self.training_phase == "text_encoder":
                self.switch_to_joint_training()
            tm = self.train_epoch(epoch)
            vm = self.validate_epoch(epoch)
            self.stepper.end_epoch()
            self.logger.info(f"Phase: {self.training_phase}")
            self.logger.info(f"Train - Loss: {tm['loss']:.4f}, L1: {tm['l1_loss']:.4f}, MSE: {tm['mse_loss']:.4f}, CLIP: {tm['clip_loss']:.4f}")
            self.logger.info(f"Val - Loss: {vm['loss']:.4f}, L1: {vm['l1_loss']:.4f}, MSE: {vm['mse_loss']:.4f}")
            for tag, v in (("Final Train/Loss", tm["loss"]), ("Final Train/L1_Loss", tm["l1_loss"]), ("Final Train/MSE_Loss", tm["mse_loss"]),
                           ("Final Train/CLIP_Loss", tm["clip_loss"]), ("Final Val/Loss", vm["loss"]), ("Final Val/L1_Loss", vm["l1_loss"]),
                           ("Final Val/MSE_Loss", vm["mse_loss"])):
                self.writer.add_scalar(tag, v, epoch)
            if epoch % tc["sample_every"] == 0:
                self.generate_samples(epoch)
            is_best = vm["loss"] < self.best_val_loss
            if is_best:
                self.best_val_loss = vm["loss"]
            if epoch % tc["save_every"] == 0 or is_best:
                self.save_checkpoint(epoch, is_best)
            self.current_epoch = epoch + 1
        self.logger.info("Final training completed!")
        self.writer.close()
