"""What the stage-1 / stage-3 trainer suites share: the data (tests/golden/sprites), the tokenizers, the configuration, the
models of tests/test_vae_stepper_gpu.py and tests/test_final_joint_gpu.py (hashgen "stress" VAE, a 2-layer BERT without
dropout, tests/vgg_ref.py's VGG16, tests/clip_ref.py's "hook" CLIP) and the recording wrapper around a trainer's epochs.

Data: `descriptions_semicolon.csv` is the fixture list that yields 8 sprites (001-009 without 004), which
`val_split 0.25, test_split 0.125` splits 5 / 2 / 1; `pokemon_tab.csv` drops the sprite without a description and yields 7.
Batch 2 with drop_last: 2 train batches per epoch, one validation batch of 2."""
import os

import torch

from oracle import hashgen
from tests import clip_ref, sprite_ref, text_cases as TC, text_grad_cases as TG, vgg_ref

DEV = "cuda"
SEED = 77
CSV = os.path.join(sprite_ref.SPRITE_DIR, "descriptions_semicolon.csv")
BATCH, TRAIN_BATCHES, SIDE = 2, 2, 215
CLIP_NAME = "hook"                       # 215-pixel images on a narrow one-layer tower, 16 text positions


def bert_config():
    return dict(TC.bert_config(2), hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)


def bert_tokenizer():
    from transformers import BertTokenizer
    return BertTokenizer(vocab_file=TC.VOCAB)


class ClipTokenizer:
    """Stands in for CLIPTokenizer: BOS 1, one id in [3, 61] per word (the first 3 + len(text) % 9 words), EOS 63 - the highest
    id of the "hook" vocabulary, which is what the text tower pools at - then EOS as padding to the longest text."""

    def __call__(self, texts, return_tensors="pt", padding=True, truncation=True, max_length=16):
        rows = []
        for t in texts:
            words = t.split(" ")[:3 + len(t) % 9][:max_length - 2]
            rows.append([1] + [3 + sum(map(ord, w)) % 59 for w in words] + [63])
        S = max(len(r) for r in rows)
        return {"input_ids": torch.tensor([r + [63] * (S - len(r)) for r in rows], dtype=torch.int64)}


def config(tmp, **training):
    """The keys of config/train_config.yaml the two trainers read."""
    tr = {"vae_epochs": 2, "final_epochs": 2, "phase1_epochs": 1, "log_every": 1, "save_every": 1, "sample_every": 1,
          "kl_annealing": True, "kl_anneal_start": 0, "kl_anneal_end": 2, "kl_weight_start": 0.0, "kl_weight_end": 1e-4,
          "reconstruction_weight": 1.0, "perceptual_weight": 0.1, "kl_weight": 0.01, "clip_weight": 0.1}
    tr.update(training)
    return {
        "experiment_dir": str(tmp),
        "model": {"bert_model": "stub", "text_embedding_dim": 256, "latent_dim": 8, "bert_finetune_strategy": "minimal"},
        "data": {"csv_path": CSV, "image_dir": sprite_ref.SPRITE_DIR, "batch_size": BATCH, "image_size": SIDE, "num_workers": 0,
                 "pin_memory": False, "val_split": 0.25, "test_split": 0.125},
        "training": tr,
        "optimization": {"optimizer": "adamw", "learning_rate": 1e-4, "text_encoder_lr": 1e-4, "weight_decay": 0.01,
                         "scheduler": "step", "step_size": 1, "gamma": 0.5},       # halved per epoch: never 0 within a test
    }


def world(psg):
    """The state dicts, made once and left unchanged."""
    vae = psg.PokemonVAE(8, 256, trainable=True)
    vae_sd = hashgen.fill_unet_state({k: tuple(v.shape) for k, v in vae.state_dict().items()}, SEED, "stress")
    te = psg.TextEncoder(bert_config=bert_config(), hidden_dim=256, trainable=True, finetune_strategy="minimal")
    return {"vae": vae_sd, "te": TG.state_dict(te), "crit": {"perceptual_loss." + k: v for k, v in vgg_ref.vgg_state_dict().items()},
            "clip": {"model." + k: v for k, v in clip_ref.state_dict(CLIP_NAME).items()}}


def text_encoder(psg, w, tokenizer=None):
    te = psg.TextEncoder(bert_config=bert_config(), hidden_dim=256, trainable=True, finetune_strategy="minimal",
                         tokenizer=tokenizer or bert_tokenizer())
    te.load_state_dict(w["te"])
    return te.to(DEV)


def vae_parts(psg, w):
    """(vae, text_encoder, criterion) of stage 1, fp32, on the device."""
    vae = psg.PokemonVAE(8, 256, trainable=True)
    vae.load_state_dict(w["vae"])
    return vae.to(DEV), text_encoder(psg, w), psg.CombinedLoss(state_dict=w["crit"]).to(DEV)


def small_unet(psg):
    """Stands in for the U-Net: stage 3's training never calls it, the generator and the stepper only touch its parameters."""
    torch.manual_seed(5)
    return psg.UNetBlock(64, 64, 128, 256, has_attention=True, num_heads=4)


def generator(psg, w):
    """Stage 3's generator with a trainable decoder; `forward` (the sampler, which needs the real U-Net) is replaced by the
    decoder on drawn latents, enough for the sample sheet."""
    enc, dec = psg.VAEEncoder(3, 8), psg.VAEDecoder(8, 256, 3, trainable=True)
    enc.load_state_dict({k[8:]: v for k, v in w["vae"].items() if k.startswith("encoder.")})
    dec.load_state_dict({k[8:]: v for k, v in w["vae"].items() if k.startswith("decoder.")})
    gen = psg.FinalPokemonGenerator(enc, dec, small_unet(psg), text_encoder(psg, w)).to(DEV)

    def generate(texts, **kw):
        with torch.no_grad():
            return gen.vae_decoder(torch.randn(len(texts), 8, 27, 27, device=DEV), gen.text_encoder(texts))
    gen.forward = generate
    return gen


def clip(psg, w, tokenizer=True):
    return psg.CLIPLoss(clip_ref.CONFIGS[CLIP_NAME], state_dict=w["clip"], tokenizer=ClipTokenizer() if tokenizer else None, device=DEV)


def loaders(psg):
    tr, va, te = psg.create_data_loaders(CSV, sprite_ref.SPRITE_DIR, batch_size=BATCH, val_split=0.25, test_split=0.125,
                                         image_size=SIDE, device=DEV, tokenizer=bert_tokenizer())
    return {"train": tr, "val": va, "test": te}


def record(trainer, after_epoch=None):
    """Wrap train_epoch / validate_epoch of a trainer instance: returns the list the (kind, epoch, metrics) triples go to.
    `after_epoch(trainer, epoch)` runs right after each train_epoch and its result is appended as ("state", epoch, result)."""
    log = []
    train_epoch, validate_epoch = trainer.train_epoch, trainer.validate_epoch

    def te(epoch):
        m = train_epoch(epoch)
        log.append(("train", epoch, m))
        if after_epoch is not None:
            log.append(("state", epoch, after_epoch(trainer, epoch)))
        return m

    def ve(epoch):
        m = validate_epoch(epoch)
        log.append(("val", epoch, m))
        return m
    trainer.train_epoch, trainer.validate_epoch = te, ve
    return log


def snapshot(module):
    return {n: p.detach().clone() for n, p in module.named_parameters()}


def mean_of(rows, keys, n):
    """The trainers' epoch mean: the steps' device scalars added into one fp32 device vector, read once, divided on the host."""
    sums = torch.zeros(len(keys), device=DEV)
    for r in rows:
        sums += torch.stack([r[k] for k in keys])
    return [v / n for v in sums.tolist()]
