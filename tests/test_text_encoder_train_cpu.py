"""CPU suite of text-encoder fine-tuning: the LayerNorm backward and the key-length attention training pair are exported,
bound and declared; their argument validation returns the library's codes before anything is launched; on the meta device
`TextEncoder(trainable=True)` sets requires_grad exactly as the reference's strategy does (names recorded in
tests/golden/text_encoder_grad.npz); the generator's report agrees with the fixture."""
import os
import re

import pytest
import torch

from tests import text_cases as TC
from tests import text_grad_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("psg_layernorm_bwd", "psg_layernorm_bwd_workspace_bytes", "psg_attn_fwd_varlen_train", "psg_attn_bwd_varlen")
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
    hdr = open(os.path.join(ROOT, "include", "psg_hip.h")).read()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES and f"{n}(" in hdr, n


def _lnb(lib, x=A16, ldx=768, r=None, ldr=0, dy=A16, lddy=768, g=A16, dz=A16, lddz=768, dg=A16, db=A16, acc=0, rows=100, N=768,
         eps=1e-12, xd=0, dyd=0, ws=A16, ws_bytes=1 << 30):
    return lib.psg_layernorm_bwd(x, ldx, r, ldr, dy, lddy, g, dz, lddz, dg, db, acc, rows, N, eps, xd, dyd, ws, ws_bytes, None)


def test_layernorm_bwd_argument_validation(lib):
    for k in ("x", "dy", "g", "dz"):
        assert _lnb(lib, **{k: None}) == -6, k                       # PSG_ERR_ARG
    assert _lnb(lib, ws=None) == -6                                  # parameter sums asked for, no workspace
    assert _lnb(lib, xd=7) == -2 and _lnb(lib, dyd=3) == -2          # PSG_ERR_DTYPE
    for N in (0, 12, 4104, 8192):                                    # the forward's row-width domain
        assert _lnb(lib, N=N, ldx=8192, lddy=8192, lddz=8192) == -1, N
        assert b"row width" in lib.psg_last_error()
    assert _lnb(lib, rows=0) == -1
    assert _lnb(lib, ldx=512) == -1 and _lnb(lib, lddy=512) == -1 and _lnb(lib, lddz=512) == -1
    assert _lnb(lib, r=A16, ldr=512) == -1
    assert _lnb(lib, x=A16 + 8) == -3 and _lnb(lib, dy=A16 + 4) == -3 and _lnb(lib, dz=A16 + 8) == -3      # PSG_ERR_ALIGN
    assert _lnb(lib, ldx=772, lddy=772, lddz=772) == -3
    assert _lnb(lib, r=A16 + 4, ldr=768) == -3
    assert _lnb(lib, ws=A16 + 4) == -3
    assert _lnb(lib, eps=-1.0) == -6
    need = lib.psg_layernorm_bwd_workspace_bytes(100, 768)
    assert need > 0 and need % 16 == 0
    assert _lnb(lib, ws_bytes=need - 1) == -4                        # PSG_ERR_WORKSPACE
    assert b"workspace" in lib.psg_last_error()
    # the need grows with the rows and depends on nothing but (rows, N)
    assert lib.psg_layernorm_bwd_workspace_bytes(65536, 768) > need == lib.psg_layernorm_bwd_workspace_bytes(100, 768)


def _avt(lib, kv=A16, B=2, heads=12, L=32, S=32, d=64, drop=0.1, dt=1, ld=2304, lse=A16, q=A16):
    return lib.psg_attn_fwd_varlen_train(q, ld, A16, ld, A16, ld, A16, 768, lse, B, heads, L, S, d, 0.125, drop, 0, dt, kv, None)


def _abv(lib, kv=A16, B=2, heads=12, L=32, S=32, d=64, drop=0.1, dt=1, ld=2304, ldg=2304, lse=A16, delta=A16, dq=A16):
    return lib.psg_attn_bwd_varlen(A16, ld, A16, ld, A16, ld, A16, 768, A16, 768, lse, delta, dq, ldg, A16, ldg, A16, ldg, B, heads, L, S, d,
                                   0.125, drop, 0, dt, kv, None)


def test_attn_varlen_train_argument_validation(lib):
    assert _avt(lib, kv=None) == -6 and _abv(lib, kv=None) == -6     # kv_len is required
    assert _avt(lib, lse=None) == -6                                 # the training forward saves lse
    assert _avt(lib, q=None) == -6 and _abv(lib, delta=None) == -6 and _abv(lib, dq=None) == -6
    for drop in (-0.1, 1.0, 1.5):                                    # drop_p outside [0, 1)
        assert _avt(lib, drop=drop) == -6 and _abv(lib, drop=drop) == -6, drop
        assert b"drop_p" in lib.psg_last_error()
    assert _avt(lib, dt=4) == -2 and _abv(lib, dt=4) == -2
    assert _avt(lib, d=66) == -1 and _abv(lib, d=66) == -1
    assert _avt(lib, S=5000, L=5000) == -1 and _abv(lib, S=5000, L=5000) == -1      # LDS need
    assert _avt(lib, ld=700) == -1 and _abv(lib, ld=700) == -1       # row stride < heads * d
    assert _abv(lib, ldg=700) == -1
    assert _avt(lib, ld=2306) == -3                                  # row strides multiples of 4
    # the forward-only entry keeps its contract
    assert lib.psg_attn_fwd_varlen(A16, 2304, A16, 2304, A16, 2304, A16, 768, None, 2, 12, 32, 32, 64, 0.125, 0.1, 0, 1, A16, None) == -6


def _meta(case, **kw):
    from pokemon_sprite_generator_amd.text_encoder import TextEncoder
    c = GC.CASES[case]
    with torch.device("meta"):
        return TextEncoder(bert_config=TC.bert_config(c["layers"]), hidden_dim=c["hidden_dim"], finetune_strategy=c["strategy"], **kw)


@pytest.mark.parametrize("case", sorted(GC.CASES))
def test_trainable_sets_the_reference_requires_grad(golden, case):
    g = golden("text_encoder_grad.npz")
    want = [str(s) for s in g[f"{case}_requires_grad"]]
    enc = _meta(case, trainable=True)
    assert GC.trainable_names(enc) == want
    assert not enc.training                                          # built in eval mode, like the frozen class
    enc.train()
    assert enc.training and enc.bert.training
    # a sweep that freezes everything, then the reference's public method restores the set
    enc.requires_grad_(False)
    assert GC.trainable_names(enc) == []
    enc._apply_finetune_strategy()
    assert GC.trainable_names(enc) == want
    # the default constructor is the frozen class: nothing trainable, .train() ignored, the launch count as before
    frozen = _meta(case)
    assert GC.trainable_names(frozen) == [] and not frozen.train().training
    frozen._apply_finetune_strategy()
    assert GC.trainable_names(frozen) == []
    c = GC.CASES[case]
    assert frozen.launches_per_call() == 1 + 7 * c["layers"] + (c["hidden_dim"] != 768) + 1
    first = {"none": c["layers"], "minimal": c["layers"] - 2, "partial": c["layers"] - 4}[c["strategy"]]
    assert enc.first_trainable_layer() == first and frozen.first_trainable_layer() == c["layers"]


def test_full_strategy_is_refused_when_trainable():
    from pokemon_sprite_generator_amd import PsgError
    from pokemon_sprite_generator_amd.text_encoder import TextEncoder
    with torch.device("meta"):
        with pytest.raises(PsgError, match="embedding gradients"):
            TextEncoder(bert_config=TC.bert_config(1), finetune_strategy="full", trainable=True)
        TextEncoder(bert_config=TC.bert_config(1), finetune_strategy="full")            # frozen: accepted as before
        enc = TextEncoder(bert_config=dict(TC.bert_config(1), hidden_dropout_prob=0.2, attention_probs_dropout_prob=0.0), trainable=True)
    assert enc.hidden_dropout_prob == 0.2 and enc.attention_probs_dropout_prob == 0.0
    with torch.device("meta"):
        assert TextEncoder(bert_config=TC.bert_config(1)).hidden_dropout_prob == 0.1    # BertConfig's default


def test_report_is_consistent_with_fixture(golden):
    g = golden("text_encoder_grad.npz")
    rep = open(os.path.join(ROOT, "tests", "golden", "REPORT_text_grad.txt")).read()
    lo, hi = GC.SCORE_STD_WINDOW
    assert f"x {GC.QK_FACTOR:g}" in rep
    for case, c in GC.CASES.items():
        line = next(l for l in rep.splitlines() if l.startswith(f"case {case}:"))
        assert f"strategy {c['strategy']}, layers {c['layers']}, hidden_dim {c['hidden_dim']}" in line
        shape = tuple(int(v) for v in g[f"{case}_out_shape"])
        assert f"out {shape}" in line and shape[2] == c["hidden_dim"] and shape[1] <= 256
        stds = [float(v) for v in line.split("score std per layer")[1].split()]
        assert len(stds) == c["layers"] and all(lo <= s <= hi for s in stds), (case, stds)
        lens = [int(v) for v in re.search(r"token counts \[([^\]]*)\]", line).group(1).split(",")]
        assert lens == g[f"{case}_attention_mask"].sum(1).tolist()
        names, none = [str(s) for s in g[f"{case}_grad_names"]], [str(s) for s in g[f"{case}_grad_none"]]
        assert sorted(names + none) == [str(s) for s in g[f"{case}_requires_grad"]]
        assert f"gradients {len(names)}, grad None {len(none)}" in line
        # the pooler is trainable and never reached: last_hidden_state is what the encoder returns
        assert none == ([] if c["strategy"] == "none" else ["bert.pooler.dense.bias", "bert.pooler.dense.weight"])
        for n in names:
            d, s = g[f"{case}_grad_d::{n}"], g[f"{case}_grad_s::{n}"]
            assert s.size <= GC.GRAD_SAMPLE and d[0] > 0, n
        assert g[f"{case}_out_cols"].shape == (shape[0], shape[1], -(-shape[2] // GC.COL_STRIDE[case]))
