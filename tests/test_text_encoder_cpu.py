"""CPU suite of the frozen BERT text encoder: the new entry points are exported and bound, their argument validation
returns error codes before anything is launched, the TextEncoder's state-dict layout equals the reference module's
(recorded in tests/golden/text_encoder.npz) and its tokenization reproduces the fixture's ids and masks."""
import ctypes as C
import os

import pytest
import torch

from tests import text_cases as TC

NEW_SYMBOLS = ("psg_layernorm", "psg_bert_embed_ln", "psg_attn_fwd_varlen")
A16 = 0x10000                     # a 16-byte aligned stand-in address: validation never dereferences it


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_new_symbols_exported_and_bound(lib):
    from pokemon_sprite_generator_amd import _lib
    import pokemon_sprite_generator_amd as psg
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psg_hip.h")).read()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES and f"{n}(" in hdr
    assert "TextEncoder" in psg.__all__ and psg.TextEncoder.__module__ == "pokemon_sprite_generator_amd.text_encoder"


def _ln(lib, x=A16, ldx=768, r=None, ldr=0, y=A16, ldy=768, g=A16, b=A16, rows=4, N=768, eps=1e-12, xd=0, yd=0):
    return lib.psg_layernorm(x, ldx, r, ldr, y, ldy, g, b, rows, N, eps, xd, yd, None)


def test_layernorm_argument_validation(lib):
    assert _ln(lib, x=None) == -6                                   # PSG_ERR_ARG
    assert _ln(lib, xd=7) == -2 and _ln(lib, yd=3) == -2            # PSG_ERR_DTYPE
    for N in (0, 12, 4104, 8192):                                   # not a multiple of 8 / above 4096
        assert _ln(lib, N=N, ldx=8192, ldy=8192) == -1, N
        assert b"row width" in lib.psg_last_error()
    assert _ln(lib, rows=0) == -1
    assert _ln(lib, ldx=512) == -1                                  # row stride below N
    assert _ln(lib, r=A16, ldr=512) == -1
    assert _ln(lib, x=A16 + 8) == -3                                # misaligned row start (PSG_ERR_ALIGN)
    assert _ln(lib, ldx=772, ldy=772, N=768) == -3                  # stride not a multiple of 8 elements
    assert _ln(lib, r=A16 + 4, ldr=768) == -3
    assert _ln(lib, eps=-1.0) == -6


def _emb(lib, ids=A16, tt=None, y=A16, ldy=768, B=2, S=16, N=768, vocab=100, max_pos=512, tv=2, eps=1e-12, dt=0, w=A16):
    return lib.psg_bert_embed_ln(ids, tt, w, A16, A16, A16, A16, y, ldy, B, S, N, vocab, max_pos, tv, eps, dt, None)


def test_embed_ln_argument_validation(lib):
    assert _emb(lib, ids=None) == -6
    assert _emb(lib, dt=5) == -2
    assert _emb(lib, S=513) == -1                                   # more positions than embeddings
    assert b"position" in lib.psg_last_error()
    assert _emb(lib, N=100, ldy=100) == -1
    assert _emb(lib, vocab=0) == -1
    assert _emb(lib, ldy=700) == -1
    assert _emb(lib, w=A16 + 4) == -3
    assert _emb(lib, ldy=772) == -3


def _av(lib, kv=A16, B=2, heads=12, L=32, S=32, d=64, drop=0.0, dt=1, ld=2304, lse=None):
    return lib.psg_attn_fwd_varlen(A16, ld, A16, ld, A16, ld, A16, 768, lse, B, heads, L, S, d, 0.125, drop, 0, dt, kv, None)


def test_attn_varlen_argument_validation(lib):
    assert _av(lib, kv=None) == -6                                  # kv_len is required
    assert _av(lib, drop=0.1) == -6                                 # forward-only entry: no dropout
    assert b"drop_p" in lib.psg_last_error()
    assert _av(lib, dt=4) == -2
    assert _av(lib, d=66) == -1
    assert _av(lib, S=5000, L=5000) == -1
    assert _av(lib, ld=700) == -1                                   # row stride < heads * d


@pytest.mark.parametrize("case", sorted(TC.CASES))
def test_state_dict_layout_matches_reference(golden, case):
    from pokemon_sprite_generator_amd.text_encoder import TextEncoder
    c = TC.CASES[case]
    with torch.device("meta"):
        enc = TextEncoder(bert_config=TC.bert_config(c["layers"]), hidden_dim=c["hidden_dim"])
    want = [str(s) for s in golden("text_encoder.npz")[f"{case}_state_dict"]]
    assert TC.key_shapes(enc) == want
    assert any(k.startswith("bert.pooler.") for k in enc.state_dict())
    assert any(k.startswith("projection.") for k in enc.state_dict()) == (c["hidden_dim"] != 768)
    assert not any(p.requires_grad for p in enc.parameters())       # frozen, inference only
    assert enc.launches_per_call() == 1 + 7 * c["layers"] + (c["hidden_dim"] != 768) + 1


def test_finetune_strategy_validated():
    from pokemon_sprite_generator_amd.text_encoder import TextEncoder
    with torch.device("meta"):
        for s in ("none", "minimal", "partial", "full"):
            TextEncoder(bert_config=TC.bert_config(1), finetune_strategy=s)
        with pytest.raises(ValueError):
            TextEncoder(bert_config=TC.bert_config(1), finetune_strategy="most")


@pytest.mark.parametrize("case", sorted(TC.CASES))
def test_tokenization_reproduces_fixture(golden, case):
    transformers = pytest.importorskip("transformers")
    from pokemon_sprite_generator_amd.text_encoder import TextEncoder
    c = TC.CASES[case]
    tok = transformers.BertTokenizer(vocab_file=TC.VOCAB, do_lower_case=True)
    tok.padding_side = "left"                                       # forward enforces right padding whatever it was given
    with torch.device("meta"):
        enc = TextEncoder(bert_config=TC.bert_config(c["layers"]), hidden_dim=c["hidden_dim"], tokenizer=tok)
    g = golden("text_encoder.npz")
    inputs = enc.tokenize(c["texts"])
    assert inputs["input_ids"].tolist() == g[f"{case}_input_ids"].tolist()
    assert inputs["attention_mask"].tolist() == g[f"{case}_attention_mask"].tolist()
    assert inputs["token_type_ids"].tolist() == g[f"{case}_token_type_ids"].tolist()
    assert inputs["input_ids"].shape[1] <= 256


def test_encode_needs_gpu_parameters():
    from pokemon_sprite_generator_amd import PsgError
    from pokemon_sprite_generator_amd.text_encoder import TextEncoder
    enc = TextEncoder(bert_config=dict(TC.bert_config(1), hidden_size=64, num_attention_heads=4, intermediate_size=128), hidden_dim=64)
    with pytest.raises(PsgError):
        enc.encode_ids(torch.zeros(1, 4, dtype=torch.int64), torch.ones(1, 4, dtype=torch.int64))
    with pytest.raises(PsgError):
        enc(["no tokenizer was given"])
