"""What the text inputs of a batch cost, and what stage 3 gains from computing CLIP's text side once.

  inputs   per-batch time of `input_ids` / `attention_mask` / key lengths at batch 4, 32 and 256 over 898 descriptions:
           OLD  the tokenizer call on the batch's strings (padding=True, truncation=True, max_length=256) + the upload of both
                tensors + `mask.sum(1)` on the device: a host timer around the window, which ends in a device synchronise;
           NEW  `TokenTable.batch(idx, rows)` - one launch of psg_token_batch: device events around the call (gpu_ms) and a host
                timer around the same window without a synchronise inside (host_ms: what the training loop's thread spends).
           The tokenizer is bert-base-uncased's when the local cache has it, else the test vocabulary's BertTokenizer (the same
           Python class, a 267-word vocabulary: most words become [UNK], the per-word work is the same); the line says which.
           The descriptions are generated: 898 sentences of 18-45 vocabulary words after "Pokemon named X.".
  stage3   `FinalTrainer.train_epoch` per batch at batch 4 in the text-encoder phase with the CLIP term: text features cached
           at set-up against CLIP's text tower run per batch.  ViT-B/32's real widths and depths with generated weights (the
           weights do not change the time), a 12-layer BERT-base text encoder, 40 training sprites (the 8 fixture sprites
           repeated) = 10 batches per epoch; device events around the epoch, divided by the batch count.

3 warm-up and 10 timed iterations each, median and range.  One JSON line per measurement.

    python tools/bench_text_inputs.py [inputs] [stage3]
"""
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pokemon_sprite_generator_amd as psg  # noqa: E402
from oracle import hashgen  # noqa: E402
from tests import sprite_ref, text_cases as TC  # noqa: E402

WARMUP, TIMED = 3, 10
N_TEXTS = 898
DEV = "cuda"


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def tokenizer():
    from transformers import BertTokenizer
    try:
        return BertTokenizer.from_pretrained("bert-base-uncased", local_files_only=True), "bert-base-uncased (local cache)"
    except Exception:                          # noqa: BLE001 - not in the cache
        return BertTokenizer(vocab_file=TC.VOCAB), "test vocabulary (tests/golden/text_vocab.txt)"


def sentences(n):
    words = [w for w in TC.vocab_words() if w.isalpha()]
    out = []
    for k in range(n):
        m = 18 + int(hashgen.randint((1,), 5, k, 0, 28))
        idx = hashgen.randint((m,), 6, k, 0, len(words)).tolist()
        out.append(f"Pokemon named {words[idx[0]].capitalize()}. " + " ".join(words[i] for i in idx[1:]) + ".")
    return out


class Texts:
    def __init__(self, texts):
        self.texts, self.device = texts, torch.device(DEV, torch.cuda.current_device())

    def __len__(self):
        return len(self.texts)

    def meta(self, i):
        return {"full_description": self.texts[i]}


def bench_inputs():
    tok, which = tokenizer()
    tok.padding_side = "right"
    ds = Texts(sentences(N_TEXTS))
    t0 = time.perf_counter()
    table = psg.TokenTable(ds, tok)
    build_s = time.perf_counter() - t0
    print(json.dumps({"what": "token_table_build", "tokenizer": which, "rows": len(ds), "L": table.table.shape[1],
                      "mean_len": round(sum(table.lens_host) / len(ds), 1), "seconds_once": round(build_s, 3)}))
    for B in (4, 32, 256):
        order = torch.randperm(len(ds), generator=torch.Generator().manual_seed(B)).tolist()
        order_dev = torch.tensor(order, dtype=torch.int64, device=DEV)
        old, new_gpu, new_host = [], [], []
        for it in range(WARMUP + TIMED):
            lo = (it * B) % (len(ds) - B)
            rows, idx = order[lo:lo + B], order_dev[lo:lo + B]
            texts = [ds.texts[r] for r in rows]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            enc = tok(texts, return_tensors="pt", padding=True, truncation=True, max_length=256)
            ids, mask = enc["input_ids"].to(DEV), enc["attention_mask"].to(DEV)
            kv = mask.sum(1, dtype=torch.int32)
            torch.cuda.synchronize()
            t_old = (time.perf_counter() - t0) * 1e3
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            ids2, mask2 = table.batch(idx, rows)
            e1.record()
            t_host = (time.perf_counter() - t0) * 1e3
            torch.cuda.synchronize()
            assert torch.equal(ids, ids2) and torch.equal(mask, mask2) and int(kv.sum()) == int(mask2.sum())
            if it >= WARMUP:
                old.append(t_old), new_gpu.append(e0.elapsed_time(e1)), new_host.append(t_host)
        print(json.dumps({"what": "text_inputs", "tokenizer": which, "batch": B, "old_ms": summary(old), "new_gpu_ms": summary(new_gpu),
                          "new_host_ms": summary(new_host)}))


CLIP_B32 = {"projection_dim": 512,
            "vision_config": {"hidden_size": 768, "intermediate_size": 3072, "num_hidden_layers": 12, "num_attention_heads": 12,
                              "image_size": 224, "patch_size": 32, "layer_norm_eps": 1e-5, "hidden_act": "quick_gelu"},
            "text_config": {"vocab_size": 49408, "hidden_size": 512, "intermediate_size": 2048, "num_hidden_layers": 12,
                            "num_attention_heads": 8, "max_position_embeddings": 77, "eos_token_id": 2, "layer_norm_eps": 1e-5,
                            "hidden_act": "quick_gelu"}}


class ClipTokens:
    """CLIPTokenizer's shape of output without its vocabulary: BOS, one id per word, EOS = the highest id, EOS-padded."""

    def __call__(self, texts, return_tensors="pt", padding=True, truncation=True, max_length=77):
        rows = [[49406] + [1000 + sum(map(ord, w)) % 40000 for w in t.split(" ")][:max_length - 2] + [49407] for t in texts]
        S = max(len(r) for r in rows)
        return {"input_ids": torch.tensor([r + [49407] * (S - len(r)) for r in rows], dtype=torch.int64)}


def bench_stage3(dtype=torch.bfloat16):
    tmp = tempfile.mkdtemp(prefix="psg_stage3_")
    try:
        texts = sentences(48)
        with open(os.path.join(tmp, "descriptions.csv"), "w") as fh:
            for k in range(48):
                shutil.copy(os.path.join(sprite_ref.SPRITE_DIR, f"{sprite_ref.FIXTURE_NUMBERS[k % 8]:03d}.png"), os.path.join(tmp, f"{k + 1:03d}.png"))
                fh.write(f"Name{k};{texts[k].split('. ', 1)[1]}\n")
        cfg = {"experiment_dir": os.path.join(tmp, "exp"),
               "model": {"bert_model": "-", "text_embedding_dim": 256, "latent_dim": 8},
               "data": {"csv_path": os.path.join(tmp, "descriptions.csv"), "image_dir": tmp, "batch_size": 4, "image_size": 215,
                        "num_workers": 0, "pin_memory": False, "val_split": 0.1, "test_split": 0.1},
               "training": {"final_epochs": 100, "log_every": 1000, "save_every": 1000, "sample_every": 1000, "clip_weight": 0.1},
               "optimization": {"optimizer": "adamw", "text_encoder_lr": 1e-5, "weight_decay": 0.01, "scheduler": "constant"},
               "mi355x": {"update": "grouped"}}
        from transformers import BertTokenizer
        vae = psg.PokemonVAE(8, 256)
        vae_sd = hashgen.fill_unet_state({k: tuple(v.shape) for k, v in vae.state_dict().items()}, 77, "stress")
        enc, dec = psg.VAEEncoder(3, 8, compute_dtype=dtype), psg.VAEDecoder(8, 256, 3, compute_dtype=dtype, trainable=True)
        enc.load_state_dict({k[8:]: v for k, v in vae_sd.items() if k.startswith("encoder.")})
        dec.load_state_dict({k[8:]: v for k, v in vae_sd.items() if k.startswith("decoder.")})
        te = psg.TextEncoder(bert_config=TC.bert_config(12), hidden_dim=256, finetune_strategy="minimal", compute_dtype=dtype, trainable=True,
                             tokenizer=BertTokenizer(vocab_file=TC.VOCAB))
        te.load_state_dict(TC.state_dict(te))
        gen = psg.FinalPokemonGenerator(enc, dec, None, te).to(DEV)
        torch.manual_seed(0)
        clip = psg.CLIPLoss(CLIP_B32, tokenizer=ClipTokens(), compute_dtype=dtype, device=DEV)
        tr = psg.FinalTrainer(cfg, "-", "-", "bench", components={"generator": gen, "clip_loss": clip}, compute_dtype=dtype)
        feats, nb = tr.clip_text_features, len(tr.data_loaders["train"])
        assert feats is not None and nb == 10
        times = {"cached": [], "per_batch": []}
        for it in range(WARMUP + TIMED):
            for mode in ("cached", "per_batch"):              # alternating: both see the same clocks
                tr.clip_text_features = feats if mode == "cached" else None
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                m = tr.train_epoch(it)
                e1.record()
                torch.cuda.synchronize()
                assert m["clip_loss"] != 0.0
                if it >= WARMUP:
                    times[mode].append(e0.elapsed_time(e1) / nb)
        print(json.dumps({"what": "stage3_train_epoch_ms_per_batch", "batch": 4, "dtype": str(dtype).split(".")[-1], "phase": tr.training_phase,
                          "update": "grouped", "batches_per_epoch": nb, "cached_text_side": summary(times["cached"]),
                          "per_batch_text_tower": summary(times["per_batch"])}))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["inputs", "stage3"]
    if "inputs" in which:
        bench_inputs()
    if "stage3" in which:
        bench_stage3()
