"""CPU suite of the embedding-table gradients (finetune_strategy 'full' with train_embeddings=True): requires_grad on the meta
device against the names the reference's own method set (tests/golden/text_encoder_full_grad.npz); the fixture's ids have the
properties it exists for and its report agrees with it; psg_bert_embed_ln_bwd / psg_embed_scatter reject bad arguments
before any launch; the fp64 reference of the GPU tests (tests/embed_ref.py) agrees with transformers' BertEmbeddings, and its
comparator rejects the defects a scatter-add can have."""
import os
import re

import pytest
import torch

from tests import embed_ref as ER
from tests import text_full_cases as FC
from tests.util import TOL, maxrel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("psg_bert_embed_ln_bwd", "psg_bert_embed_ln_bwd_workspace_bytes", "psg_embed_scatter", "psg_embed_scatter_workspace_bytes",
               "psg_embed_scatter_chunk_rows")
A16 = 0x10000                     # a 16-byte aligned stand-in address: validation never dereferences it
C = FC.CASE


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def _meta(**kw):
    from pokemon_sprite_generator_amd.text_encoder import TextEncoder
    with torch.device("meta"):
        return TextEncoder(bert_config=FC.bert_config(), hidden_dim=FC.HIDDEN_DIM, **kw)


def _names(enc):
    return sorted(n for n, p in enc.named_parameters() if p.requires_grad)


# ---------------------------------------------------------------------------------------------------------------- the class
def test_full_with_train_embeddings_sets_the_reference_requires_grad(golden):
    from pokemon_sprite_generator_amd import PsgError
    g = golden("text_encoder_full_grad.npz")
    want = [str(s) for s in g[f"{C}_requires_grad"]]
    enc = _meta(finetune_strategy="full", trainable=True, train_embeddings=True)
    assert _names(enc) == want == sorted(n for n, _ in enc.named_parameters())       # 'full': everything, the pooler included
    assert enc.first_trainable_layer() == 0 and not enc.training
    enc.requires_grad_(False)
    enc._apply_finetune_strategy()
    assert _names(enc) == want
    assert enc.launches_per_call() == 1 + 7 * FC.LAYERS + 1 + 1
    # without the keyword the refusal stands, and names the keyword
    with pytest.raises(PsgError, match="embedding gradients"):
        _meta(finetune_strategy="full", trainable=True)
    with pytest.raises(PsgError, match="train_embeddings"):
        _meta(finetune_strategy="full", trainable=True, train_embeddings=False)
    # trainable=False: the keyword has no effect
    frozen = _meta(finetune_strategy="full", train_embeddings=True)
    assert _names(frozen) == [] and not frozen.train().training
    # another strategy: the keyword has no effect either
    for strategy in ("none", "minimal", "partial"):
        a, b = _meta(finetune_strategy=strategy, trainable=True, train_embeddings=True), _meta(finetune_strategy=strategy, trainable=True)
        assert _names(a) == _names(b) and not any(n.startswith("bert.embeddings.") for n in _names(a)), strategy


def test_pad_token_id_is_an_optional_config_key():
    from pokemon_sprite_generator_amd.text_encoder import TextEncoder, config_dict
    assert "pad_token_id" not in config_dict(FC.bert_config())
    assert config_dict(dict(FC.bert_config(), pad_token_id=5))["pad_token_id"] == 5
    with torch.device("meta"):
        a = TextEncoder(bert_config=FC.bert_config())
        b = TextEncoder(bert_config=dict(FC.bert_config(), pad_token_id=5))
    assert a.pad_token_id == 0 and a.bert.embeddings.word_embeddings.padding_idx == 0          # BertConfig's default
    assert b.pad_token_id == 5 and b.bert.embeddings.word_embeddings.padding_idx == 5

    class Cfg:
        pass
    cfg = Cfg()
    for k, v in dict(FC.bert_config(), pad_token_id=3, hidden_act="gelu").items():
        setattr(cfg, k, v)
    assert config_dict(cfg)["pad_token_id"] == 3


def test_from_reference_passes_the_keyword_on():
    import inspect
    from pokemon_sprite_generator_amd.text_encoder import TextEncoder
    sig = inspect.signature(TextEncoder.from_reference)
    assert sig.parameters["train_embeddings"].default is False
    assert inspect.signature(TextEncoder.__init__).parameters["train_embeddings"].default is False


# ---------------------------------------------------------------------------------------------------------------- the fixture
def test_fixture_ids_and_report(golden):
    g = golden("text_encoder_full_grad.npz")
    ids, mask, tt = (torch.from_numpy(g[f"{C}_{k}"]) for k in ("input_ids", "attention_mask", "token_type_ids"))
    want = FC.inputs()
    assert all(torch.equal(a, b) for a, b in zip((ids, mask, tt), want))
    vocab = FC.bert_config()["vocab_size"]
    facts = FC.id_facts(ids, mask, tt, vocab)
    FC.check_id_facts(facts)
    assert mask.sum(1).tolist() == list(FC.LENGTHS) and tuple(ids.shape) == (FC.B, FC.S)
    assert not ids[~mask.bool()].any() and not tt[~mask.bool()].any()            # right padding: id 0, type 0
    assert (ids[:, 0] == FC.CLS).all()
    rep = open(os.path.join(ROOT, "tests", "golden", "REPORT_text_full_grad.txt")).read()
    assert f"distinct {facts['distinct']}, hot id {facts['hot_id']} x {facts['hot_count']} over {facts['hot_samples']} samples" in rep
    assert f"unused vocabulary rows {facts['unused']}" in rep and f"token type 1 on {facts['type1']} of {facts['live']}" in rep
    assert f"padded {facts['padded']} of {facts['positions']}" in rep
    lo, hi = FC.SCORE_STD_WINDOW
    stds = [float(v) for v in re.search(r"score std per layer ([0-9. ]+)", rep).group(1).split()]
    assert len(stds) == FC.LAYERS and all(lo <= s <= hi for s in stds)
    names, none = [str(s) for s in g[f"{C}_grad_names"]], [str(s) for s in g[f"{C}_grad_none"]]
    assert sorted(names + none) == [str(s) for s in g[f"{C}_requires_grad"]]
    assert none == ["bert.pooler.dense.bias", "bert.pooler.dense.weight"]
    assert f"gradients {len(names)}, grad None {len(none)}" in rep
    # the per-row norms: shapes, the padding row, the rows no id names, the positions past S
    w, p, t = (g[f"{C}_row_norms::{n}"] for n in FC.EMBED_TABLES)
    assert w.shape == (vocab,) and p.shape == (512,) and t.shape == (2,) and w.dtype == p.dtype == t.dtype == "float64"
    used = torch.bincount(ids[mask.bool()], minlength=vocab).numpy() > 0
    assert w[FC.PAD] == 0.0 and (w[~used] == 0).all() and (w[used] > 0).all()
    assert (p[:FC.S] > 0).all() and (p[FC.S:] == 0).all() and (t > 0).all()
    assert "word row 0 exactly zero: True" in rep
    for n, r in zip(FC.EMBED_TABLES, (w, p, t)):
        assert abs(float((r ** 2).sum() ** 0.5) - g[f"{C}_grad_d::{n}"][0]) < 1e-9 * g[f"{C}_grad_d::{n}"][0], n


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_new_symbols_exported_and_bound(lib):
    from pokemon_sprite_generator_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "psg_hip.h")).read()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES and f"{n}(" in hdr, n
    assert 1 <= lib.psg_embed_scatter_chunk_rows() <= 512


def _elb(lib, ids=A16, tt=None, word=A16, pos=A16, typ=A16, g=A16, dy=A16, lddy=768, dz=A16, dg=A16, db=A16, acc=0, B=4, S=32, N=768,
         vocab=30522, max_pos=512, tv=2, eps=1e-12, dyd=0, ws=A16, ws_bytes=1 << 30):
    return lib.psg_bert_embed_ln_bwd(ids, tt, word, pos, typ, g, dy, lddy, dz, dg, db, acc, B, S, N, vocab, max_pos, tv, eps, dyd, ws, ws_bytes, None)


def test_bert_embed_ln_bwd_argument_validation(lib):
    for k in ("ids", "word", "pos", "typ", "g", "dy", "dz"):
        assert _elb(lib, **{k: None}) == -6, k                        # PSG_ERR_ARG
        assert b"null" in lib.psg_last_error()
    assert _elb(lib, ws=None) == -6                                   # parameter sums asked for, no workspace
    assert _elb(lib, dyd=7) == -2                                     # PSG_ERR_DTYPE
    for N in (0, 12, 4104, 8192):
        assert _elb(lib, N=N, lddy=8192) == -1, N                     # PSG_ERR_SHAPE
        assert b"row width" in lib.psg_last_error()
    assert _elb(lib, B=0) == -1 and _elb(lib, S=0) == -1 and _elb(lib, vocab=0) == -1 and _elb(lib, tv=0) == -1
    assert _elb(lib, S=513) == -1
    assert b"position" in lib.psg_last_error()
    assert _elb(lib, lddy=512) == -1
    assert _elb(lib, eps=-1.0) == -6
    assert _elb(lib, dy=A16 + 4) == -3 and _elb(lib, dz=A16 + 8) == -3 and _elb(lib, word=A16 + 4) == -3 and _elb(lib, g=A16 + 4) == -3
    assert _elb(lib, lddy=772) == -3 and _elb(lib, ws=A16 + 4) == -3  # PSG_ERR_ALIGN
    need = lib.psg_bert_embed_ln_bwd_workspace_bytes(128, 768)
    assert need > 0 and need % 16 == 0 and need == lib.psg_layernorm_bwd_workspace_bytes(128, 768)
    assert _elb(lib, ws_bytes=need - 1) == -4                         # PSG_ERR_WORKSPACE
    assert b"workspace" in lib.psg_last_error()
    assert lib.psg_bert_embed_ln_bwd_workspace_bytes(0, 768) == 0 and lib.psg_bert_embed_ln_bwd_workspace_bytes(128, 0) == 0


def _esc(lib, dz=A16, lddz=768, key=A16, perm=A16, out=A16, rows=128, N=768, V=30522, skip=0, acc=0, ws=A16, ws_bytes=1 << 30):
    return lib.psg_embed_scatter(dz, lddz, key, perm, out, rows, N, V, skip, acc, ws, ws_bytes, None)


def test_embed_scatter_argument_validation(lib):
    for k in ("dz", "key", "perm", "out", "ws"):
        assert _esc(lib, **{k: None}) == -6, k
        assert b"null" in lib.psg_last_error()
    for N in (0, 12, 4104):
        assert _esc(lib, N=N, lddz=8192) == -1, N
        assert b"row width" in lib.psg_last_error()
    assert _esc(lib, rows=0) == -1 and _esc(lib, V=0) == -1 and _esc(lib, rows=1 << 31) == -1
    assert _esc(lib, lddz=512) == -1
    assert _esc(lib, dz=A16 + 4) == -3 and _esc(lib, out=A16 + 8) == -3 and _esc(lib, ws=A16 + 4) == -3 and _esc(lib, lddz=770) == -3
    need = lib.psg_embed_scatter_workspace_bytes(128, 768)
    assert need > 0 and need % 16 == 0
    assert _esc(lib, ws_bytes=need - 1) == -4
    assert b"workspace" in lib.psg_last_error()
    assert lib.psg_embed_scatter_workspace_bytes(0, 768) == 0 and lib.psg_embed_scatter_workspace_bytes(128, 0) == 0


def test_bert_embed_refuses_cpu_tensors():
    from pokemon_sprite_generator_amd import PsgError, ops
    with pytest.raises(PsgError):
        ops.bert_embed(torch.zeros(1, 2, dtype=torch.int64), None, torch.zeros(5, 8), torch.zeros(4, 8), torch.zeros(2, 8), torch.ones(8),
                       torch.zeros(8), 1e-12)


# ---------------------------------------------------------------------------------------------------------------- the reference
def _case(B=5, S=21, V=50, P=64, N=200, run=0, seed=7):
    gen = torch.Generator().manual_seed(seed)
    ids = torch.randint(4, V - 1, (B, S), generator=gen)
    ids[torch.rand(B, S, generator=gen) < 0.3] = 9                      # a repeated id
    if run:
        ids.view(-1)[:run] = 9
    ids[0, 0], ids[1, 3], ids[2, 5] = 1, V - 1, 1
    ids[:, S - 4:] = 0                                                  # right padding
    tt = (torch.rand(B, S, generator=gen) < 0.5).long()
    tt[:, S - 4:] = 0
    r = lambda *s: torch.rand(*s, generator=gen) * 2 - 1
    return ids, tt, r(V, N) * 0.05, r(P, N) * 0.05, r(2, N) * 0.05, 1 + 0.1 * r(N), 0.1 * r(N), r(B * S, N)


def test_reference_agrees_with_transformers_bert_embeddings():
    from transformers import BertConfig
    from transformers.models.bert.modeling_bert import BertEmbeddings
    ids, tt, word, pos, typ, gamma, beta, dy = _case()
    V, N = word.shape
    eps = 1e-12
    emb = BertEmbeddings(BertConfig(vocab_size=V, hidden_size=N, max_position_embeddings=pos.shape[0], type_vocab_size=2, layer_norm_eps=eps,
                                    pad_token_id=0)).double().eval()
    emb.load_state_dict({"word_embeddings.weight": word.double(), "position_embeddings.weight": pos.double(),
                         "token_type_embeddings.weight": typ.double(), "LayerNorm.weight": gamma.double(), "LayerNorm.bias": beta.double()},
                        strict=False)
    y = emb(input_ids=ids, token_type_ids=tt).reshape(-1, N)
    y.backward(dy.double())
    ref = ER.embed_reference(ids, tt, word, pos, typ, gamma, beta, eps, 0, dy)
    assert maxrel(ref["y"], y) < 1e-12
    for k, p in (("word", emb.word_embeddings.weight), ("pos", emb.position_embeddings.weight), ("type", emb.token_type_embeddings.weight),
                 ("gamma", emb.LayerNorm.weight), ("beta", emb.LayerNorm.bias)):
        assert maxrel(ref[k], p.grad) < 1e-12, k
    assert not ref["word"][0].any() and ids.eq(0).any()                 # padding_idx: no gradient although the cotangent is not zero
    z = ER.zero_rows(ids, tt, V, pos.shape[0], 2, 0)
    for k in ER.TABLES:                                                 # the structural zeros are zeros of the reference
        assert not ref[k][z[k]].any() and bool((ref[k][~z[k]].abs().sum(1) > 0).all()), k
    # an id outside the table: the row leaves the graph
    bad = ids.clone()
    bad[3, 2] = V
    rb = ER.embed_reference(bad, tt, word, pos, typ, gamma, beta, eps, 0, dy)
    assert not rb["dz"][3 * ids.shape[1] + 2].any() and all(bool(torch.isfinite(rb[k]).all()) for k in ER.GRADS)


def test_comparator_rejects_injected_defects(lib):
    """Each defect a scatter-add backward can have turns a passing result (the fp64 reference rounded to fp32) into one the
    comparator refuses at the fp32 bar of the GPU test."""
    chunk = lib.psg_embed_scatter_chunk_rows()
    ids, tt, word, pos, typ, gamma, beta, dy = _case(B=6, S=40, run=2 * chunk + 5)
    V, N = word.shape
    P, S = pos.shape[0], ids.shape[1]
    tol = 2 * TOL[torch.float32]
    ref = ER.embed_reference(ids, tt, word, pos, typ, gamma, beta, 1e-12, 0, dy)
    zeros = ER.zero_rows(ids, tt, V, P, 2, 0)
    good = {k: ref[k].float() for k in ER.GRADS}
    ER.check_embed(good, ref, tol, zeros)
    flat, dz = ids.view(-1), ref["dz"]

    def scatter(rows_of, table_rows, src):
        out = torch.zeros(table_rows, N, dtype=torch.float64)
        out.index_add_(0, rows_of, src)
        return out

    def bad(**kw):
        with pytest.raises(AssertionError):
            ER.check_embed(dict(good, **kw), ref, tol, zeros)

    live = flat != 0
    # the pad row not zeroed
    bad(word=scatter(flat, V, dz).float())
    # duplicates not accumulated: the last occurrence wins
    last = torch.zeros(V, N, dtype=torch.float64)
    last[flat[live]] = dz[live]
    bad(word=last.float())
    # position and token-type gradients swapped
    bad(pos=good["type"], type=good["pos"])
    # position rows at or beyond S non-zero (indexed by the flat row, not by t % S)
    wrong = scatter(torch.arange(flat.numel()) % P, P, dz).float()
    assert wrong[S:].any()
    bad(pos=wrong)
    # a long run's tail chunk dropped
    hot = (flat == 9).nonzero().view(-1)
    assert hot.numel() >= 2 * chunk + 5
    keep = torch.ones_like(live)
    keep[hot[2 * chunk:]] = False
    bad(word=scatter(flat[live & keep], V, dz[live & keep]).float())
    # dgamma and dbeta swapped
    bad(gamma=good["beta"], beta=good["gamma"])
    # dz rounded to bf16 before the scatter: refused at the fp32 bar, table by table
    dzb = dz.float().bfloat16().double()
    bad(word=scatter(flat[live], V, dzb[live]).float())
    bad(pos=scatter(torch.arange(flat.numel()) % S, P, dzb).float())
    bad(type=scatter(tt.view(-1), 2, dzb).float())
