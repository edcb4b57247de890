"""-m gpu: the embedding-table gradients of the BERT text encoder (finetune_strategy 'full' with train_embeddings=True).

psg_bert_embed_ln_bwd and psg_embed_scatter through the C ABI and through `ops.bert_embed` against the fp64 reference of
tests/embed_ref.py on the same rounded inputs (exact zeros, guard rows, accumulate, NULL outputs, equal bits on a second
run, dropout, an id outside the table); the whole `TextEncoder(..., 'full', trainable=True, train_embeddings=True)` forward
+ backward against the reference module's (tests/golden/text_encoder_full_grad.npz), fp32 and bf16; the same bits as the
other strategies; train mode; an AdamW loop; one FinalStepper.train_step."""
import numpy as np
import pytest
import torch

from tests import embed_ref as ER
from tests import text_full_cases as FC
from tests.test_text_encoder_gpu import _u
from tests.test_text_encoder_train_gpu import FP32_TOL, _check_key_bias_is_zero, _key_bias_sibling
from tests.util import TOL, check_digest, maxrel, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-12
C = FC.CASE
GUARD = 123.0


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    return _lib.init(0)


# ---------------------------------------------------------------------------------------------------------------- kernels
# name -> B, S, vocab, max_pos, token types given, a run of 2 * chunk_rows + 5 positions of the hot id
SHAPES = {
    "b3s7": (3, 7, 50, 128, False, False),
    "b5s67": (5, 67, 50, 128, True, False),
    "long": (16, 96, 50, 128, True, True),
    "vocab": (4, 32, 30522, 512, True, False),
}
KERNEL_CASES = [(s, N) for s in ("b3s7", "b5s67") for N in (200, 768, 4096)] + [("long", 768), ("vocab", 768)]
HOT = 9


def _operands(lib, shape, N, dt, bad_row=None):
    B, S, V, P, typed, long_run = SHAPES[shape]
    gen = torch.Generator().manual_seed(31 + B * S + N)
    ids = torch.randint(4, V - 1, (B, S), generator=gen)
    ids[torch.rand(B, S, generator=gen) < 0.25] = HOT                   # a repeated id; most of the vocabulary stays unused
    if long_run:
        ids.view(-1)[S:S + 2 * lib.psg_embed_scatter_chunk_rows() + 5] = HOT
    ids[0, 0], ids[1, 1], ids[2, 2] = 1, V - 1, 1
    pad = max(1, S // 5)
    ids[1:, S - pad:] = 0                                               # right padding with id 0 (sample 0 is full)
    tt = None
    if typed:
        tt = (torch.rand(B, S, generator=gen) < 0.5).long()
        tt[1:, S - pad:] = 0
        tt = tt.to(DEV)
    if bad_row is not None:
        ids.view(-1)[bad_row] = V
    s = 100 * N + B
    return dict(ids=ids.to(DEV), tt=tt, word=_u((V, N), s + 1) * 0.05, pos=_u((P, N), s + 2) * 0.05, typ=_u((2, N), s + 3) * 0.05,
                gamma=_u((N,), s + 4) * 0.2 + 1.0, beta=_u((N,), s + 5) * 0.1, dy=_u((B * S, N), s + 6, dt))


def _guarded(rows, N, fill=float("nan")):
    """[rows, N] view filled with `fill` between two guard rows."""
    buf = torch.full((rows + 2, N), GUARD, device=DEV)
    buf[1:-1] = fill
    return buf, buf[1:-1]


def _guards_ok(buf):
    return bool((buf[0] == GUARD).all()) and bool((buf[-1] == GUARD).all())


def _sorted_keys(o):
    B, S = o["ids"].shape
    rows = B * S
    j = torch.arange(rows, device=DEV)
    word = torch.sort(o["ids"].view(-1), stable=True)
    typ = torch.sort(o["tt"].view(-1), stable=True) if o["tt"] is not None else (torch.zeros_like(j), j)
    return {"word": (word[0], word[1], 0), "pos": (j // B, (j % B) * S + j // B, -1), "type": (typ[0], typ[1], -1)}


def _raw(lib, o, bufs, acc, dg=True, db=True):
    """psg_bert_embed_ln_bwd + the three scatters into the views of `bufs`."""
    from pokemon_sprite_generator_amd._lib import check, dtype_code, ptr, stream_ptr
    B, S = o["ids"].shape
    V, N = o["word"].shape
    rows = B * S
    need = max(lib.psg_bert_embed_ln_bwd_workspace_bytes(rows, N), lib.psg_embed_scatter_workspace_bytes(rows, N))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    check(lib.psg_bert_embed_ln_bwd(ptr(o["ids"]), ptr(o["tt"]), ptr(o["word"]), ptr(o["pos"]), ptr(o["typ"]), ptr(o["gamma"]), ptr(o["dy"]), N,
                                    ptr(bufs["dz"]), ptr(bufs["gamma"] if dg else None), ptr(bufs["beta"] if db else None), int(acc), B, S, N, V,
                                    o["pos"].shape[0], 2, EPS, dtype_code(o["dy"].dtype), ptr(ws), need, stream_ptr()), "psg_bert_embed_ln_bwd")
    for name, (key, perm, skip) in _sorted_keys(o).items():
        if name in bufs:
            out = bufs[name]
            check(lib.psg_embed_scatter(ptr(bufs["dz"]), N, ptr(key), ptr(perm), ptr(out), rows, N, out.shape[0], skip, int(acc), ptr(ws), need,
                                        stream_ptr()), "psg_embed_scatter")


def _buffers(o, fill=float("nan")):
    B, S = o["ids"].shape
    V, N = o["word"].shape
    sizes = {"dz": B * S, "word": V, "pos": o["pos"].shape[0], "type": 2, "gamma": 1, "beta": 1}
    whole, views = {}, {}
    for k, r in sizes.items():
        whole[k], views[k] = _guarded(r, N, fill)
    return whole, views


def _reference(o, **kw):
    return ER.embed_reference(o["ids"], o["tt"], o["word"], o["pos"], o["typ"], o["gamma"], o["beta"], EPS, 0, o["dy"], **kw)


def _flat(views):
    return {k: (v.reshape(-1) if k in ("gamma", "beta") else v) for k, v in views.items()}


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape,N", KERNEL_CASES)
def test_embed_backward_kernels(lib, shape, N, dt):
    from pokemon_sprite_generator_amd import ops
    o = _operands(lib, shape, N, dt)
    B, S = o["ids"].shape
    V, P = o["word"].shape[0], o["pos"].shape[0]
    tol = 2 * TOL[dt]
    ref = _reference(o)
    zeros = ER.zero_rows(o["ids"], o["tt"], V, P, 2, 0)
    assert zeros["word"][0] and zeros["word"].sum() > 1 and zeros["pos"][S:].all() and not zeros["pos"][:S].any() and not zeros["word"][[1, V - 1, HOT]].any()
    if shape == "long":
        chunk = lib.psg_embed_scatter_chunk_rows()
        assert int((o["ids"] == HOT).sum()) >= 2 * chunk + 5 and min(int((o["tt"] == t).sum()) for t in (0, 1)) > 2 * chunk
    # accumulate = 0 into NaN-filled buffers: every element written, structural zeros exact, guard rows untouched
    whole, first = _buffers(o)
    _raw(lib, o, first, 0)
    errs = ER.check_embed(_flat(first), ref, tol, zeros)
    print(f"embed bwd {shape} N={N} {dt}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(_guards_ok(w) for w in whole.values())
    # a second run: equal bits
    whole2, second = _buffers(o)
    _raw(lib, o, second, 0)
    assert all(torch.equal(first[k], second[k]) for k in first)
    # accumulate = 1: old + (completed sum), rows without a key untouched
    base = {k: _u(tuple(v.shape), 50 + i) for i, (k, v) in enumerate(first.items())}
    whole3, third = _buffers(o)
    for k in third:
        third[k].copy_(base[k])
    _raw(lib, o, third, 1)
    for k in ("word", "pos", "type", "gamma", "beta"):
        assert torch.equal(third[k], base[k] + first[k]), k
    for k in ER.TABLES:
        assert torch.equal(third[k][zeros[k].to(DEV)], base[k][zeros[k].to(DEV)]), k
    assert torch.equal(third["dz"], first["dz"]) and all(_guards_ok(w) for w in whole3.values())
    # NULL outputs are skipped
    whole4, fourth = _buffers(o)
    _raw(lib, o, {k: fourth[k] for k in ("dz", "word", "gamma", "beta")}, 0, dg=False)
    assert torch.equal(fourth["dz"], first["dz"]) and torch.equal(fourth["beta"], first["beta"]) and torch.equal(fourth["word"], first["word"])
    assert bool(torch.isnan(fourth["gamma"]).all()) and bool(torch.isnan(fourth["pos"]).all())
    _raw(lib, o, {"dz": fourth["dz"]}, 0, dg=False, db=False)
    assert torch.equal(fourth["dz"], first["dz"]) and bool(torch.isnan(fourth["gamma"]).all())
    # the autograd node: the forward is psg_bert_embed_ln's bits, the gradients are the C ABI's bits
    from pokemon_sprite_generator_amd._lib import check, dtype_code, ptr, stream_ptr
    y0 = torch.empty((B * S, N), dtype=dt, device=DEV)
    check(lib.psg_bert_embed_ln(ptr(o["ids"]), ptr(o["tt"]), ptr(o["word"]), ptr(o["pos"]), ptr(o["typ"]), ptr(o["gamma"]), ptr(o["beta"]), ptr(y0), N,
                                B, S, N, V, P, 2, EPS, dtype_code(dt), stream_ptr()), "psg_bert_embed_ln")
    params = {k: o[k].clone().requires_grad_(True) for k in ("word", "pos", "typ", "gamma", "beta")}
    y = ops.bert_embed(o["ids"], o["tt"], params["word"], params["pos"], params["typ"], params["gamma"], params["beta"], EPS, 0, dt)
    assert y.dtype == dt and torch.equal(y.detach(), y0)
    y.backward(o["dy"])
    for k, n in (("word", "word"), ("pos", "pos"), ("typ", "type"), ("gamma", "gamma"), ("beta", "beta")):
        assert params[k].grad.dtype == torch.float32 and torch.equal(params[k].grad, first[n].reshape(params[k].shape)), k
    # parameters that want no gradient are skipped
    only = {k: o[k].clone().requires_grad_(k in ("pos", "beta")) for k in ("word", "pos", "typ", "gamma", "beta")}
    ops.bert_embed(o["ids"], o["tt"], only["word"], only["pos"], only["typ"], only["gamma"], only["beta"], EPS, 0, dt).backward(o["dy"])
    assert only["word"].grad is None and only["typ"].grad is None and only["gamma"].grad is None
    assert torch.equal(only["pos"].grad, first["pos"]) and torch.equal(only["beta"].grad, first["beta"].reshape(-1))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_id_outside_the_table_contributes_nothing(lib, dt):
    shape, N = "b5s67", 768
    B, S, V, P, _, _ = SHAPES[shape]
    bad_row = 2 * S + 11
    o = _operands(lib, shape, N, dt, bad_row=bad_row)
    assert int(o["ids"].view(-1)[bad_row]) == V and bool(torch.isfinite(o["dy"][bad_row].float()).all()) and bool(o["dy"][bad_row].any())
    whole, got = _buffers(o)
    _raw(lib, o, got, 0)
    errs = ER.check_embed(_flat(got), _reference(o), 2 * TOL[dt], ER.zero_rows(o["ids"], o["tt"], V, P, 2, 0))      # finite, and the reference's
    assert not got["dz"][bad_row].any() and all(_guards_ok(w) for w in whole.values())
    print(f"id == V, {dt}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_embed_node_with_dropout(lib, dt):
    from pokemon_sprite_generator_amd import ops
    from pokemon_sprite_generator_amd._lib import check, dtype_code, ptr, stream_ptr
    shape, N, p, seed = "b5s67", 768, 0.3, 24680
    o = _operands(lib, shape, N, dt)
    B, S = o["ids"].shape
    V, P = o["word"].shape[0], o["pos"].shape[0]
    params = {k: o[k].clone().requires_grad_(True) for k in ("word", "pos", "typ", "gamma", "beta")}
    args = (o["ids"], o["tt"], params["word"], params["pos"], params["typ"], params["gamma"], params["beta"], EPS, 0, dt)
    plain = ops.bert_embed(*args).detach()
    y = ops.bert_embed(*args, drop_p=p, seed=seed)
    want = plain.clone()
    check(lib.psg_dropout_apply(ptr(want), N, ptr(want), N, B * S, N, p, seed, 1.0 / (1.0 - p), dtype_code(dt), stream_ptr()), "psg_dropout_apply")
    assert torch.equal(y.detach(), want)                               # psg_bert_embed_ln, then the in-place dropout of _encode_train
    keep = (y.detach() != 0) | (plain == 0)
    rate = float(keep.float().mean())
    assert abs(rate - (1 - p)) < 0.02, rate
    y.backward(o["dy"])
    ref = _reference(o, keep=keep, p=p)
    got = {"word": params["word"].grad, "pos": params["pos"].grad, "type": params["typ"].grad, "gamma": params["gamma"].grad, "beta": params["beta"].grad}
    errs = ER.check_embed(got, ref, 2 * TOL[dt], ER.zero_rows(o["ids"], o["tt"], V, P, 2, 0), names=("word", "pos", "type", "gamma", "beta"))
    print(f"embed node p={p} {dt}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    again = {k: o[k].clone().requires_grad_(True) for k in params}
    ops.bert_embed(o["ids"], o["tt"], again["word"], again["pos"], again["typ"], again["gamma"], again["beta"], EPS, 0, dt, drop_p=p,
                   seed=seed).backward(o["dy"])
    assert all(torch.equal(again[k].grad, params[k].grad) for k in params)


# ---------------------------------------------------------------------------------------------------------------- model
def _build(dt=torch.float32, strategy="full", trainable=True, train_embeddings=True):
    from pokemon_sprite_generator_amd.text_encoder import TextEncoder
    enc = TextEncoder(bert_config=FC.bert_config(), hidden_dim=FC.HIDDEN_DIM, finetune_strategy=strategy, compute_dtype=dt, trainable=trainable,
                      train_embeddings=train_embeddings)
    enc.load_state_dict(FC.state_dict(enc), strict=True)
    return enc.to(DEV)


def _inputs(golden):
    g = golden("text_encoder_full_grad.npz")
    return tuple(torch.from_numpy(g[f"{C}_{k}"]) for k in ("input_ids", "attention_mask", "token_type_ids")) + (g,)


def _loss(y):
    return (y * FC.cotangent(y.shape).to(y.device)).sum()


def test_model_gradients_match_reference_fp32(lib, golden):
    """Forward + backward of L = sum(y * G) in eval mode against the reference module's under 'full': output columns, every
    stored gradient sample and norm within max-rel 1e-3; per-row norms of the three tables within 1e-3 of the largest row norm,
    zero rows exactly zero; the trainable parameters without a gradient are the fixture's (the pooler)."""
    enc = _build()
    ids, mask, tt, g = _inputs(golden)
    y = enc.encode_ids(ids, mask, tt)
    assert y.requires_grad and y.dtype == torch.float32 and tuple(y.shape) == tuple(g[f"{C}_out_shape"])
    _loss(y).backward()
    e_out = maxrel(y[:, :, ::FC.COL_STRIDE].cpu(), torch.from_numpy(g[f"{C}_out_cols"]))
    print(f"case {C} fp32: output max-rel {e_out:.2e}")
    assert e_out <= FP32_TOL, e_out
    named = dict(enc.named_parameters())
    assert sorted(n for n, p in named.items() if p.requires_grad) == [str(s) for s in g[f"{C}_requires_grad"]]
    assert sorted(n for n, p in named.items() if p.requires_grad and p.grad is None) == [str(s) for s in g[f"{C}_grad_none"]]
    for n in (str(s) for s in g[f"{C}_grad_names"]):
        assert named[n].grad is not None and named[n].grad.dtype == torch.float32, n
        if _key_bias_sibling(n):
            _check_key_bias_is_zero(g, C, n, named[n].grad, FP32_TOL)
            continue
        check_digest(named[n].grad, g[f"{C}_grad_d::{n}"], g[f"{C}_grad_s::{n}"], FP32_TOL, what=f"{C}:{n}")
    for n in FC.EMBED_TABLES:
        want = g[f"{C}_row_norms::{n}"]
        got = named[n].grad.double().norm(dim=1).cpu().numpy()
        err = float(np.abs(got - want).max() / want.max())
        print(f"case {C} fp32 {n}: row norms within {err:.2e} of the largest")
        assert err < FP32_TOL, (n, err)
        assert not named[n].grad[torch.from_numpy(want == 0).to(DEV)].any(), n


def test_model_gradients_match_reference_bf16(lib, golden):
    """The bf16 leg against the same fp32 fixture at the bars of test_text_encoder_train_gpu's bf16 leg: the vector of
    per-parameter gradient norms rel-L2 < 1e-2, every norm within 2 %, every stored sample rel-L2 < 4e-2, output columns
    rel-L2 < 3e-2, key-bias gradients within 2 % of their query-bias sibling's norm; table rows that are zero in the fixture
    exactly zero."""
    enc = _build(torch.bfloat16)
    ids, mask, tt, g = _inputs(golden)
    y = enc.encode_ids(ids, mask, tt)
    _loss(y).backward()
    e_out = rel_l2(y[:, :, ::FC.COL_STRIDE].cpu(), torch.from_numpy(g[f"{C}_out_cols"]))
    named = dict(enc.named_parameters())
    names = [str(s) for s in g[f"{C}_grad_names"]]
    for n in [n for n in names if _key_bias_sibling(n)]:
        _check_key_bias_is_zero(g, C, n, named[n].grad, 0.02)
    names = [n for n in names if not _key_bias_sibling(n)]
    ref = np.array([g[f"{C}_grad_d::{n}"][0] for n in names])
    norms = np.array([float(named[n].grad.double().norm()) for n in names])
    vec_rel = float(np.linalg.norm(norms - ref) / np.linalg.norm(ref))
    each = np.abs(norms - ref) / (ref + 1e-12)
    worst, worst_n = 0.0, ""
    for n in names:
        d, s_ref = g[f"{C}_grad_d::{n}"], g[f"{C}_grad_s::{n}"]
        sample = named[n].grad.detach().reshape(-1).double().cpu()[::int(d[2])].float().numpy()
        assert sample.shape == s_ref.shape, n
        e = float(np.linalg.norm(sample - s_ref) / (np.linalg.norm(s_ref) + 1e-30))
        if e > worst:
            worst, worst_n = e, n
    print(f"case {C} bf16 vs reference fixture: output rel-L2 {e_out:.2e}; per-param norm vector rel-L2 {vec_rel:.2e}, worst single "
          f"{each.max():.2e} ({names[int(each.argmax())]}); worst sample rel-L2 {worst:.2e} ({worst_n})")
    assert e_out < 3e-2, e_out
    assert vec_rel < 1e-2 and each.max() < 0.02, f"per-parameter grad norms: vector {vec_rel:.2e}, worst {each.max():.2e} at {names[int(each.argmax())]}"
    assert worst < 4e-2, (worst, worst_n)
    assert sorted(n for n, p in named.items() if p.requires_grad and p.grad is None) == [str(s) for s in g[f"{C}_grad_none"]]
    for n in FC.EMBED_TABLES:
        assert named[n].grad.dtype == torch.float32
        assert not named[n].grad[torch.from_numpy(g[f"{C}_row_norms::{n}"] == 0).to(DEV)].any(), n


def _run(enc, ids, mask, tt, seed):
    from pokemon_sprite_generator_amd.unet import _SeedStream
    torch.manual_seed(seed)
    _SeedStream.counter = 0
    return enc.encode_ids(ids, mask, tt)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_full_has_the_bits_of_the_other_strategies(lib, golden, dt):
    """Equal weights, equal seeds: the embedding node changes no launch - eval and train mode outputs equal 'partial''s."""
    ids, mask, tt, _ = _inputs(golden)
    full, part = _build(dt), _build(dt, strategy="partial", train_embeddings=False)
    assert part.first_trainable_layer() == 0 and not part.bert.embeddings.word_embeddings.weight.requires_grad
    a, b = _run(full, ids, mask, tt, 3), _run(part, ids, mask, tt, 3)
    assert a.requires_grad and b.requires_grad and torch.equal(a, b)
    frozen = _build(dt, trainable=False)
    with torch.no_grad():
        assert torch.equal(frozen.encode_ids(ids, mask, tt), full.encode_ids(ids, mask, tt))
    eval_y = a.detach()
    full.train(), part.train()
    a, b = _run(full, ids, mask, tt, 3), _run(part, ids, mask, tt, 3)
    assert torch.equal(a, b) and not torch.equal(a.detach(), eval_y)
    with torch.no_grad():                                               # no graph: the node is not used, the bits stay
        assert torch.equal(_run(full, ids, mask, tt, 3), a)


def test_train_mode_gradients_are_reproducible(lib, golden):
    ids, mask, tt, _ = _inputs(golden)
    enc = _build(torch.bfloat16).train()

    def grads(seed):
        enc.zero_grad(set_to_none=True)
        _loss(_run(enc, ids, mask, tt, seed)).backward()
        return {n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None}
    g1, g2, g3 = grads(5), grads(5), grads(6)
    assert set(FC.EMBED_TABLES) <= set(g1) and g1.keys() == g2.keys() == g3.keys()
    assert all(torch.isfinite(v).all() for v in g1.values())
    assert all(torch.equal(g1[k], g2[k]) for k in g1)
    assert all(not torch.equal(g1[k], g3[k]) for k in FC.EMBED_TABLES)


def test_adamw_steps_move_exactly_the_rows_that_were_read(lib, golden):
    ids, mask, tt, _ = _inputs(golden)
    enc = _build(torch.bfloat16)
    before = {n: p.detach().clone() for n, p in enc.named_parameters()}
    train = [p for p in enc.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(train, lr=1e-3, weight_decay=0.0)
    outs = []
    for _ in range(3):
        opt.zero_grad()
        y = enc.encode_ids(ids, mask, tt)
        outs.append(y.detach().clone())
        _loss(y).backward()
        opt.step()
    w_name, p_name, t_name = FC.EMBED_TABLES
    named = dict(enc.named_parameters())
    used = torch.bincount(ids[mask.bool()], minlength=before[w_name].shape[0]) > 0
    assert used[FC.PAD] == False and used.sum() > 40                    # noqa: E712  (padding positions are not live)
    moved = (named[w_name].detach() != before[w_name]).any(1).cpu()
    assert torch.equal(moved, used)                                     # the tokens present move; the pad row and unused rows keep their bits
    moved_p = (named[p_name].detach() != before[p_name]).any(1).cpu()
    assert moved_p[:FC.S].all() and not moved_p[FC.S:].any()
    assert (named[t_name].detach() != before[t_name]).any(1).all()
    for n, p in named.items():
        if n.startswith("bert.pooler."):
            assert torch.equal(p.detach(), before[n]), n
        elif n not in FC.EMBED_TABLES:
            assert not torch.equal(p.detach(), before[n]), n
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])      # nothing stale is cached
    with torch.no_grad():
        after = enc.encode_ids(ids, mask, tt)
    assert not torch.equal(after, outs[2])
    fresh = _build(torch.bfloat16, trainable=False)
    fresh.load_state_dict(enc.state_dict(), strict=True)
    assert torch.equal(fresh.encode_ids(ids, mask, tt), after)


def test_final_stepper_trains_the_word_table(lib, golden):
    import pokemon_sprite_generator_amd as psg
    from oracle import hashgen
    from tests import final_cases as FIN
    ids, mask, tt, _ = _inputs(golden)
    ids, mask = ids[:2], mask[:2]
    te = _build(torch.float32)
    enc, dec = psg.VAEEncoder(3, 8), psg.VAEDecoder(8, 256, 3)
    enc.load_state_dict(hashgen.fill_unet_state({k: tuple(v.shape) for k, v in enc.state_dict().items()}, 11, "stress"))
    dec.load_state_dict(FIN.decoder_state({k: v.shape for k, v in dec.state_dict().items()}))
    gen = psg.FinalPokemonGenerator(enc, dec, None, te).to(DEV)
    st = psg.FinalStepper(gen, lr=1e-3, weight_decay=0.0)
    word = te.bert.embeddings.word_embeddings.weight
    assert any(p is word for p in st.params)
    before = word.detach().clone()
    res = st.train_step(FIN.inputs("b2")[2].to(DEV), ids, mask)
    assert all(bool(torch.isfinite(v)) for v in res.values()), res
    assert bool(torch.isfinite(word).all()) and not torch.equal(word.detach(), before) and torch.equal(word.detach()[FC.PAD], before[FC.PAD])
