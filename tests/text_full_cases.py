"""The case of the 'full' fine-tuning fixture (tests/golden/text_encoder_full_grad.npz, made by tools/make_golden_text_full.py
from the reference module's own forward + backward): unlike the text cases it is driven by token IDS, so that the word table
is read and its gradient written at many rows, token type 1 occurs, and one id repeats often enough to need accumulation.
Weights and cotangent are tests/text_grad_cases.py's; everything is rebuilt here from oracle.hashgen."""
import torch

from oracle import hashgen
from tests import text_cases as TC
from tests import text_grad_cases as GC

CASE = "F"
LAYERS, HIDDEN_DIM = 2, 256
B, S = 4, 40
LENGTHS = (40, 23, 2, 33)                 # live tokens per sample ([CLS] and [SEP]s included); right padding after them
FIRST_SEGMENT = (17, 10, 2, 33)           # tokens of segment A ([CLS] .. first [SEP]); what follows is segment B, token type 1
PAD, UNK, CLS, SEP = 0, 1, 2, 3           # tests/golden/text_vocab.txt
HOT_ID = 57                               # forced at HOT_SHARE of the body positions
HOT_SHARE = 0.30
SEED_IDS = 2323
COL_STRIDE = 8
GRAD_SAMPLE = GC.GRAD_SAMPLE
SCORE_STD_WINDOW = GC.SCORE_STD_WINDOW
EMBED_TABLES = ("bert.embeddings.word_embeddings.weight", "bert.embeddings.position_embeddings.weight",
                "bert.embeddings.token_type_embeddings.weight")
# what the generator asserts of the ids (and the CPU test re-asserts from the stored ones)
MIN_DISTINCT, MIN_HOT, MIN_HOT_SAMPLES, MIN_UNUSED, MIN_TYPE1_SHARE, MIN_PAD_SHARE = 40, 20, 3, 100, 0.25, 0.25


def bert_config():
    return TC.bert_config(LAYERS)


def inputs():
    """(input_ids, attention_mask, token_type_ids), int64 [B, S]."""
    vocab = bert_config()["vocab_size"]
    body = hashgen.randint((B, S), SEED_IDS, 1, 4, vocab)
    hot = hashgen.uniform((B, S), SEED_IDS, 2) < (2.0 * HOT_SHARE - 1.0)
    body = torch.where(hot, torch.full_like(body, HOT_ID), body)
    ids = torch.full((B, S), PAD, dtype=torch.int64)
    mask = torch.zeros((B, S), dtype=torch.int64)
    tt = torch.zeros((B, S), dtype=torch.int64)
    for b, (n, a) in enumerate(zip(LENGTHS, FIRST_SEGMENT)):
        ids[b, :n] = body[b, :n]
        ids[b, 0] = CLS
        ids[b, a - 1] = SEP
        ids[b, n - 1] = SEP
        mask[b, :n] = 1
        tt[b, a:n] = 1
    ids[0, 5] = UNK
    ids[3, 7] = vocab - 1
    return ids, mask, tt


def id_facts(ids, mask, tt, vocab):
    """The properties of the ids the fixture is there for, as a dict of counts."""
    live = mask.bool()
    counts = torch.bincount(ids[live], minlength=vocab)
    top = int(counts[4:].argmax()) + 4
    return {
        "distinct": int((torch.bincount(ids.reshape(-1), minlength=vocab) > 0).sum()),
        "hot_id": top, "hot_count": int(counts[top]), "hot_samples": int(((ids == top) & live).any(1).sum()),
        "unused": int((torch.bincount(ids.reshape(-1), minlength=vocab) == 0).sum()),
        "type1": int(tt[live].sum()), "live": int(live.sum()), "padded": int((~live).sum()), "positions": ids.numel(),
        "has_unk": bool((ids[live] == UNK).any()), "has_last": bool((ids[live] == vocab - 1).any()),
    }


def check_id_facts(f):
    assert f["distinct"] >= MIN_DISTINCT, f
    assert f["hot_count"] >= MIN_HOT and f["hot_samples"] >= MIN_HOT_SAMPLES, f
    assert f["unused"] >= MIN_UNUSED, f
    assert f["type1"] >= MIN_TYPE1_SHARE * f["live"], f
    assert f["padded"] >= MIN_PAD_SHARE * f["positions"], f
    assert f["has_unk"] and f["has_last"], f


def state_dict(module):
    return GC.state_dict(module)


def cotangent(shape):
    return GC.cotangent(CASE, shape)
