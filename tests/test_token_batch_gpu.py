"""-m gpu: psg_token_batch (csrc/sprites.hip) against a torch restatement, bit for bit, and `TokenTable.batch` on the sprite
fixtures against the tokenizer's own padded batch.

The table is `hashgen.randint` with a row-specific value in column 0, so every row is distinct; the lengths cover 1, L and
values between.  The three outputs are views inside sentinel-filled buffers with a guard region either side: the guards must
come back untouched."""
import os

import pytest
import torch

from oracle import hashgen
from tests import sprite_ref as R, text_cases as TC

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
PAD = 7                                   # not 0: a pad written as 0 by mistake shows
SENTINEL = {torch.int64: -0x5A5A5A5A5A5A5A5B, torch.int32: -0x5A5A5A5B}
# (N, L, B, S) -> the indices; every case also holds rows 0 and N - 1
CASES = {
    "one": ((1, 1, 1, 1), [0]),
    "s_equals_l": ((9, 31, 3, 31), [8, 0, 4]),
    "row_longer_than_s": ((9, 31, 4, 26), [0, 8, 3, 5]),                 # lens[3] = 31 > S: the min is exercised
    "off_wave_repeats": ((5, 256, 33, 65), [0, 4] + [(3 * k) % 5 for k in range(31)]),
    "full_width": ((5, 256, 2, 256), [4, 0]),
    "outside": ((9, 31, 6, 31), [0, -1, 8, 9, 2, -(2 ** 40)]),             # -1, N and a far one among valid rows
    "two_blocks_per_row": ((3, 700, 3, 700), [2, 0, 1]),                  # S past one 256-lane block, not a multiple of it
}


@pytest.fixture(scope="module")
def data():
    from pokemon_sprite_generator_amd import _lib, data as D
    _lib.init(0)
    return D


def _table(N, L, name):
    t = hashgen.randint((N, L), 11, hashgen.name_id(f"tok.{name}"), 8, 30000).to(torch.int32)
    t[:, 0] = torch.arange(N, dtype=torch.int32) + 40000                   # distinct rows
    lens = hashgen.randint((N,), 11, hashgen.name_id(f"tok.{name}.len"), 1, L + 1).to(torch.int32)
    lens[0], lens[N - 1] = 1, L
    if N > 3:
        lens[3] = L
    for r in range(N):
        t[r, int(lens[r]):] = PAD                                          # right-padded, as TokenTable builds it
    return t, lens


def _guarded(shape, dtype):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), SENTINEL[dtype], dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _want(table, lens, idx, S):
    B = len(idx)
    ids = torch.full((B, S), PAD, dtype=torch.int64)
    mask = torch.zeros(B, S, dtype=torch.int64)
    kv = torch.zeros(B, dtype=torch.int32)
    for b, r in enumerate(idx):
        if 0 <= r < table.shape[0]:
            n = min(int(lens[r]), S)
            ids[b, :n] = table[r, :n].to(torch.int64)
            mask[b, :n] = 1
            kv[b] = n
    return ids, mask, kv


@pytest.mark.parametrize("case", list(CASES))
def test_kernel_equals_the_restatement_and_keeps_the_guards(data, case):
    from pokemon_sprite_generator_amd import _lib
    (N, L, B, S), idx = CASES[case]
    assert len(idx) == B and 0 in idx and N - 1 in idx
    table, lens = _table(N, L, case)
    want = _want(table, lens, idx, S)
    if case == "row_longer_than_s":
        assert int(lens[3]) > S and int(want[2][2]) == S
    bufs = [_guarded((B, S), torch.int64), _guarded((B, S), torch.int64), _guarded((B,), torch.int32)]
    t_dev, l_dev, i_dev = table.to(DEV), lens.to(DEV), torch.tensor(idx, dtype=torch.int64, device=DEV)
    lib = _lib.init(0)
    _lib.check(lib.psg_token_batch(_lib.ptr(t_dev), _lib.ptr(l_dev), N, L, _lib.ptr(i_dev), B, S, PAD, _lib.ptr(bufs[0][1]),
                                   _lib.ptr(bufs[1][1]), _lib.ptr(bufs[2][1]), _lib.stream_ptr()), "psg_token_batch")
    torch.cuda.synchronize()
    for (buf, view), ref, name in zip(bufs, want, ("ids", "mask", "kv_len")):
        assert torch.equal(view.cpu(), ref), (case, name)
        s = SENTINEL[buf.dtype]
        assert bool((buf[:GUARD] == s).all()) and bool((buf[GUARD + view.numel():] == s).all()), (case, name, "guard")
    if case == "outside":
        for b in (1, 3, 5):
            assert bool((want[0][b] == PAD).all()) and int(want[1][b].sum()) == 0 and int(want[2][b]) == 0
    # the module's wrapper: the same three tensors
    got = data.token_batch(t_dev, l_dev, i_dev, S, PAD)
    assert all(torch.equal(g.cpu(), w) for g, w in zip(got, want))
    assert got[0].dtype == got[1].dtype == torch.int64 and got[2].dtype == torch.int32


@pytest.mark.parametrize("csv", ["descriptions_semicolon.csv", "pokemon_tab.csv"])
def test_token_table_batches_equal_the_tokenizers(data, csv):
    from transformers import BertTokenizer
    tok = BertTokenizer(vocab_file=TC.VOCAB)
    ds = data.SpriteDataset(os.path.join(R.SPRITE_DIR, csv), R.SPRITE_DIR, device=DEV)
    table = data.TokenTable(ds, tok)
    assert table.table.is_cuda and table.lens.is_cuda and table.table.dtype == torch.int32
    N = len(ds)
    longest = max(range(N), key=lambda i: table.lens_host[i])
    others = [i for i in range(N) if table.lens_host[i] < table.lens_host[longest]]
    for rows in ([longest, others[0]], others[:3], [others[1]], list(range(N)), [others[0], others[0], longest]):
        want = tok([ds.meta(r)["full_description"] for r in rows], return_tensors="pt", padding=True, truncation=True, max_length=256)
        ids, mask = table.batch(torch.tensor(rows, dtype=torch.int64, device=DEV), rows)
        assert ids.is_cuda and torch.equal(ids.cpu(), want["input_ids"]) and torch.equal(mask.cpu(), want["attention_mask"]), rows
    # the loader hands the same tensors out, next to the strings they stand for
    tr, va, te = data.create_data_loaders(os.path.join(R.SPRITE_DIR, csv), R.SPRITE_DIR, batch_size=2, val_split=0.25, test_split=0.125,
                                          device=DEV, tokenizer=tok)
    for batch in list(tr) + list(va):
        want = tok(batch["full_description"], return_tensors="pt", padding=True, truncation=True, max_length=256)
        assert torch.equal(batch["input_ids"].cpu(), want["input_ids"]) and torch.equal(batch["attention_mask"].cpu(), want["attention_mask"])
        assert [ds.meta(i)["name"] for i in batch["index"].tolist()] == batch["name"]
