"""CPU suite of the resident token table (data.TokenTable, psg_token_batch) and of the stage-1 / stage-3 trainers' surface:
the host restatement of a batch against the tokenizer's own padded batch, truncation, the loader's batch keys with and
without a table, the new ABI entry's argument validation, and the trainers' refusal to run without a GPU.  Nothing here
launches a kernel.

The fixture descriptions map almost entirely to [UNK] under the test vocabulary (rows 2,1,...,1,3), so the subsets are also
checked on texts built from the vocabulary's own words, whose ids tell the rows apart."""
import os

import pytest
import torch

from oracle import hashgen
from tests import sprite_ref as R, text_cases as TC

SEMI = os.path.join(R.SPRITE_DIR, "descriptions_semicolon.csv")
TAB = os.path.join(R.SPRITE_DIR, "pokemon_tab.csv")
KEYS = {"image", "description", "full_description", "national_number", "name"}
# row subsets of a 9-row table: with and without the longest row (row 4 below), a single row, repeats, every row
SUBSETS = ([4, 0, 7], [0, 1, 2], [3], [5, 5, 1], list(range(9)), [8, 4], [8, 0])


@pytest.fixture(scope="module")
def data():
    from pokemon_sprite_generator_amd import data as D
    return D


@pytest.fixture(scope="module")
def tokenizer():
    from transformers import BertTokenizer
    return BertTokenizer(vocab_file=TC.VOCAB)


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def _words(n, tid):
    words = [w for w in TC.vocab_words() if not w.startswith("[") and not w.startswith("##")]
    return " ".join(words[i] for i in hashgen.randint((n,), 31, tid, 0, len(words)).tolist())


class _Texts:
    """Stands in for a SpriteDataset: TokenTable reads len(), meta(i)["full_description"] and device."""
    device = torch.device("cpu")

    def __init__(self, texts):
        self.texts = list(texts)

    def __len__(self):
        return len(self.texts)

    def meta(self, i):
        return {"full_description": self.texts[i]}


VOCAB_TEXTS = [_words(n, k) for k, n in enumerate((5, 17, 3, 9, 40, 1, 22, 8, 12))]     # row 4 is the longest


def _restated(table, rows):
    """TokenTable.batch on the host: the padded length from lens_host, the rows from the table."""
    S = max(table.lens_host[r] for r in rows)
    ids = torch.full((len(rows), S), table.pad_id, dtype=torch.int64)
    mask = torch.zeros(len(rows), S, dtype=torch.int64)
    for b, r in enumerate(rows):
        n = min(table.lens_host[r], S)
        ids[b, :n] = table.table[r, :n].to(torch.int64)
        mask[b, :n] = 1
    return ids, mask


@pytest.mark.parametrize("source", ["vocabulary", "semicolon", "tab"])
def test_batches_equal_the_tokenizers(data, tokenizer, source):
    if source == "vocabulary":
        ds = _Texts(VOCAB_TEXTS)
    else:
        ds = data.SpriteDataset(SEMI if source == "semicolon" else TAB, R.SPRITE_DIR, device="cpu")
    table = data.TokenTable(ds, tokenizer)
    N = len(ds)
    assert table.table.dtype == torch.int32 and tuple(table.table.shape) == (N, max(table.lens_host))
    assert table.lens.dtype == torch.int32 and table.lens.tolist() == table.lens_host and table.pad_id == tokenizer.pad_token_id == 0
    if source == "vocabulary":
        assert len({tuple(r) for r in table.table.tolist()}) == N            # the ids tell the rows apart
        assert max(range(N), key=lambda i: table.lens_host[i]) == 4
    for rows in SUBSETS:
        rows = [r % N for r in rows]
        texts = [ds.meta(r)["full_description"] for r in rows]
        want = tokenizer(texts, return_tensors="pt", padding=True, truncation=True, max_length=256)
        ids, mask = _restated(table, rows)
        assert torch.equal(ids, want["input_ids"]) and torch.equal(mask, want["attention_mask"]), (source, rows)
        own = data.padded_batch([table.table[r, :table.lens_host[r]].tolist() for r in rows], table.pad_id)
        assert torch.equal(own[0], ids) and torch.equal(own[1], mask)
    with_longest, without = _restated(table, [4 % N, 0])[0], _restated(table, [5 % N, 2])[0]
    if source == "vocabulary":
        assert with_longest.shape[1] == table.table.shape[1] and without.shape[1] < table.table.shape[1]


def test_a_long_text_truncates_to_256(data, tokenizer):
    long = " ".join(["the"] * 400)
    table = data.TokenTable(_Texts([long, "a pokemon"]), tokenizer)
    want = tokenizer([long], return_tensors="pt", padding=True, truncation=True, max_length=256)
    assert tuple(want["input_ids"].shape) == (1, 256) and table.lens_host == [256, 4] and tuple(table.table.shape) == (2, 256)
    ids, mask = _restated(table, [0])
    assert torch.equal(ids, want["input_ids"]) and torch.equal(mask, want["attention_mask"])
    both = tokenizer([long, "a pokemon"], return_tensors="pt", padding=True, truncation=True, max_length=256)
    ids, mask = _restated(table, [0, 1])
    assert torch.equal(ids, both["input_ids"]) and torch.equal(mask, both["attention_mask"])


def test_loader_batch_keys_with_and_without_a_table(data, tokenizer, monkeypatch):
    """The kernels are replaced by stand-ins (CPU): what is checked is the batch dict the loader assembles."""
    monkeypatch.setattr(data, "augment", lambda src, idx, params, mean=None: torch.zeros(idx.shape[0], 3, src.shape[1], src.shape[1]))

    def fake_token_batch(table, lens, idx, S, pad_id):
        ids, mask = data.padded_batch([table[r, :lens[r]].tolist() for r in idx.tolist()], pad_id, S)
        return ids, mask, mask.sum(1, dtype=torch.int32)
    monkeypatch.setattr(data, "token_batch", fake_token_batch)
    plain = data.create_data_loaders(SEMI, R.SPRITE_DIR, batch_size=2, val_split=0.25, test_split=0.125, device="cpu")
    assert [len(l.indices) for l in plain] == [5, 2, 1] and all(l.tokens is None for l in plain)
    for loader in plain:
        for batch in loader:
            assert set(batch) == KEYS
    with_table = data.create_data_loaders(SEMI, R.SPRITE_DIR, batch_size=2, val_split=0.25, test_split=0.125, device="cpu",
                                          tokenizer=tokenizer)
    assert with_table[0].tokens is not None and with_table[0].tokens is with_table[1].tokens is with_table[2].tokens
    seen = 0
    for loader, ref in zip(with_table, plain):
        loader.set_epoch(0), ref.set_epoch(0)
        for batch, old in zip(loader, ref):
            assert set(batch) == KEYS | {"input_ids", "attention_mask", "index"}
            assert batch["full_description"] == old["full_description"]
            want = tokenizer(batch["full_description"], return_tensors="pt", padding=True, truncation=True, max_length=256)
            assert torch.equal(batch["input_ids"], want["input_ids"]) and torch.equal(batch["attention_mask"], want["attention_mask"])
            assert batch["index"].dtype == torch.int64
            assert [loader.dataset.meta(i)["name"] for i in batch["index"].tolist()] == batch["name"]
            seen += 1
    assert seen == 2 + 1 + 1


def test_token_batch_rejects_bad_arguments_without_gpu(lib):
    ok = 0x1000
    good = [ok, ok, 9, 31, ok, 3, 31, 0, ok, ok, ok, None]
    for k in (0, 1, 4, 8, 9, 10):                                            # every pointer
        args = list(good)
        args[k] = None
        assert lib.psg_token_batch(*args) == -6, k                           # PSG_ERR_ARG
        assert b"null" in lib.psg_last_error()
    for N, L, B, S in ((9, 31, 3, 32), (9, 31, 0, 31), (0, 31, 3, 31), (9, 0, 3, 1), (9, 31, 3, 0), (-1, 31, 3, 31), (9, 31, -3, 31),
                       (9, 31, 3, -1), (9, 31, 65536, 31)):
        assert lib.psg_token_batch(ok, ok, N, L, ok, B, S, 0, ok, ok, ok, None) == -1, (N, L, B, S)      # PSG_ERR_SHAPE
    assert b"psg_token_batch" in lib.psg_last_error()


def test_trainers_exist_and_need_a_gpu():
    import pokemon_sprite_generator_amd as psg
    from pokemon_sprite_generator_amd.trainer import TrainerBase
    assert issubclass(psg.VAETrainer, TrainerBase) and issubclass(psg.FinalTrainer, TrainerBase)
    assert issubclass(psg.ImprovedDiffusionTrainer, TrainerBase) and psg.TokenTable is psg.data.TokenTable
    assert (psg.VAETrainer.LOG_FILE, psg.ImprovedDiffusionTrainer.LOG_FILE, psg.FinalTrainer.LOG_FILE) == (
        "vae_training.log", "diffusion_training.log", "final_training.log")
    if not torch.cuda.is_available():                  # (with one, the -m gpu suites build and run them)
        with pytest.raises(psg.PsgError, match="needs a GPU"):
            psg.VAETrainer({"experiment_dir": "unused"}, "x")
        with pytest.raises(psg.PsgError, match="needs a GPU"):
            psg.FinalTrainer({"experiment_dir": "unused"}, "vae.pth", "diffusion.pth", "x")
