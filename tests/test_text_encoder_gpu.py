"""-m gpu: the frozen BERT text encoder on the kernels.

psg_layernorm / psg_bert_embed_ln against torch's layer_norm and embedding sums; psg_attn_fwd_varlen against SDPA with
transformers' finfo.min key mask on every kernel family (and bitwise equal to psg_attn_fwd at full key lengths); the
whole TextEncoder against the reference module's outputs (tests/golden/text_encoder.npz, cases A and B, every position);
padding invariance of a text's rows; the trainer building this class with `mi355x.text_dtype`.
tests/test_ln_kernels_gpu.py holds psg_layernorm and psg_bert_embed_ln to element-wise fp64 bounds on every instantiation."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import text_cases as TC
from tests.util import maxrel, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    return _lib.init(0)


def _u(shape, seed, dtype=torch.float32, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return ((torch.rand(shape, device=DEV, generator=g) * 2 - 1) * scale).to(dtype)


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("N", [256, 768, 1024, 4096, 200])
@pytest.mark.parametrize("res", [False, True])
def test_layernorm(lib, N, res):
    from pokemon_sprite_generator_amd.text_encoder import layer_norm
    rows = 333
    g, b = _u((N,), 3) * 0.2 + 1.0, _u((N,), 4) * 0.1
    for xd, yd in ((torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32)):
        x = _u((rows, N), 1, xd, 3.0) + 0.5
        r = _u((rows, N), 2, xd, 2.0) if res else None
        y = layer_norm(x, g, b, 1e-5, residual=r, out_dtype=yd)
        assert y.dtype == yd
        src = x.float() + r.float() if res else x.float()
        ref = F.layer_norm(src.double(), (N,), g.double(), b.double(), 1e-5)
        if xd == torch.float32 or yd == torch.float32:
            assert maxrel(y, ref) < 1e-5, (N, res, xd, yd, maxrel(y, ref))
        else:
            assert rel_l2(y, ref) < 1e-2, (N, res, rel_l2(y, ref))
    # the residual is an operand of the kernel, not an extra pass: same bits as the pre-added input (fp32)
    if res:
        x, r = _u((rows, N), 1, scale=3.0), _u((rows, N), 2, scale=2.0)
        assert torch.equal(layer_norm(x, g, b, 1e-12, residual=r), layer_norm(x + r, g, b, 1e-12))


# ---------------------------------------------------------------------------------------------------------------- embeddings
@pytest.mark.parametrize("N", [256, 768, 1024])
def test_embed_ln(lib, N):
    from pokemon_sprite_generator_amd import _lib
    from pokemon_sprite_generator_amd._lib import check, ptr, stream_ptr
    B, S, V, P, T = 3, 37, 500, 64, 2
    we, pe, te = _u((V, N), 5, scale=0.05), _u((P, N), 6, scale=0.05), _u((T, N), 7, scale=0.05)
    g, b = _u((N,), 8) * 0.2 + 1.0, _u((N,), 9) * 0.1
    ids = torch.randint(0, V, (B, S), device=DEV)
    tt = torch.randint(0, T, (B, S), device=DEV)
    ids[1, 5], ids[2, 0], ids[2, 36], tt[0, 3] = V, -1, 1 << 40, 2                    # out of range: NaN rows
    bad = torch.zeros(B, S, dtype=torch.bool, device=DEV)
    bad[1, 5] = bad[2, 0] = bad[2, 36] = bad[0, 3] = True
    for dt in (torch.float32, torch.bfloat16):
        for with_tt in (True, False):
            y = torch.empty((B, S, N), dtype=dt, device=DEV)
            check(lib.psg_bert_embed_ln(ptr(ids), ptr(tt) if with_tt else None, ptr(we), ptr(pe), ptr(te), ptr(g), ptr(b), ptr(y), N, B, S, N,
                                        V, P, T, 1e-12, _lib.dtype_code(dt), stream_ptr()), "psg_bert_embed_ln")
            t = tt if with_tt else torch.zeros_like(tt)
            bad_now = bad if with_tt else bad & ~((torch.arange(B, device=DEV)[:, None] == 0) & (torch.arange(S, device=DEV)[None] == 3))
            ok = ~bad_now
            src = (we[ids.clamp(0, V - 1)] + te[t.clamp(0, T - 1)]) + pe[:S][None]
            ref = F.layer_norm(src.double(), (N,), g.double(), b.double(), 1e-12)
            assert torch.isnan(y[bad_now]).all() and torch.isfinite(y[ok]).all()
            if dt == torch.float32:
                assert maxrel(y[ok], ref[ok]) < 1e-5
            else:
                assert rel_l2(y[ok], ref[ok]) < 1e-2


# ---------------------------------------------------------------------------------------------------------------- attention
FAMILIES = {torch.bfloat16: [(1, 0), (0, 1)], torch.float32: [(2, 2), (0, 1)]}   # (psg_attn_set_paths mask, psg_attn_path_counts slot)


def _counts(lib):
    c = [C.c_int64() for _ in range(3)]
    lib.psg_attn_path_counts(*[C.byref(x) for x in c])
    return [x.value for x in c]


def _sdpa_ref(qkv, kv_len, heads):
    B, S, E3 = qkv.shape
    E = E3 // 3
    d = E // heads
    q, k, v = (t.double().view(B, S, heads, d).transpose(1, 2) for t in qkv.split(E, -1))
    mask = (torch.arange(S, device=qkv.device)[None] < kv_len[:, None].long()).double()
    amask = (1.0 - mask)[:, None, None, :] * torch.finfo(torch.float32).min
    return F.scaled_dot_product_attention(q, k, v, attn_mask=amask).transpose(1, 2).reshape(B, S, E)


@pytest.mark.parametrize("S", [7, 32, 100, 256])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_attn_varlen_matches_masked_sdpa(lib, S, dt):
    from pokemon_sprite_generator_amd.text_encoder import attention_varlen
    heads, d = 4, 64
    B = 4
    qkv = _u((B, S, 3 * heads * d), 11 + S, dt, 2.0)
    kv_len = torch.tensor([1, S // 2 + 1, S, max(1, S - 3)], dtype=torch.int32, device=DEV)
    ref = _sdpa_ref(qkv, kv_len, heads)
    try:
        for mask, slot in FAMILIES[dt]:
            lib.psg_attn_set_paths(mask)
            c0 = _counts(lib)
            o = attention_varlen(qkv, kv_len, heads)
            torch.cuda.synchronize()
            c1 = _counts(lib)
            assert c1[slot] - c0[slot] == 1, (S, dt, mask, c0, c1)
            err = maxrel(o, ref) if dt == torch.float32 else rel_l2(o, ref)
            assert err < (1e-5 if dt == torch.float32 else 1e-2), (S, dt, mask, err)
            # a masked key contributes nothing: garbage (even NaN) past kv_len does not reach the output
            junk = qkv.clone()
            for b_, n in enumerate(kv_len.tolist()):
                junk[b_, n:, heads * d:] = float("nan")
            assert torch.equal(attention_varlen(junk, kv_len, heads), o)
    finally:
        lib.psg_attn_set_paths(3)


@pytest.mark.parametrize("S", [7, 100, 256])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_attn_varlen_full_length_is_bitwise_attn_fwd(lib, S, dt):
    from pokemon_sprite_generator_amd import ops
    from pokemon_sprite_generator_amd.text_encoder import attention_varlen
    heads = 12
    qkv = _u((3, S, 3 * heads * 64), 21 + S, dt, 2.0)
    kv_len = torch.full((3,), S, dtype=torch.int32, device=DEV)
    try:
        for mask, _ in FAMILIES[dt]:
            lib.psg_attn_set_paths(mask)
            with torch.no_grad():
                a = ops.attention_self(qkv, heads)
            assert torch.equal(attention_varlen(qkv, kv_len, heads), a), (S, dt, mask)
    finally:
        lib.psg_attn_set_paths(3)


# ---------------------------------------------------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def models():
    from pokemon_sprite_generator_amd.text_encoder import TextEncoder
    out = {}
    for case, c in TC.CASES.items():
        enc = TextEncoder(bert_config=TC.bert_config(c["layers"]), hidden_dim=c["hidden_dim"])
        enc.load_state_dict(TC.state_dict(enc), strict=True)
        out[case] = enc.to(DEV)
    return out


def _inputs(golden, case):
    g = golden("text_encoder.npz")
    return (torch.from_numpy(g[f"{case}_input_ids"]), torch.from_numpy(g[f"{case}_attention_mask"]),
            torch.from_numpy(g[f"{case}_token_type_ids"]), g)


@pytest.mark.parametrize("case", sorted(TC.CASES))
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_model_matches_reference_fixture(lib, golden, models, case, dt):
    enc = models[case]
    enc.compute_dtype = dt
    ids, mask, tt, g = _inputs(golden, case)
    y = enc.encode_ids(ids, mask, tt)
    assert y.dtype == torch.float32 and tuple(y.shape) == tuple(g[f"{case}_out_shape"])
    got = y[:, :, ::TC.COL_STRIDE[case]].cpu()
    ref = torch.from_numpy(g[f"{case}_out_cols"])
    assert torch.isfinite(got).all()
    if dt == torch.float32:
        assert maxrel(got, ref) <= 1e-3, maxrel(got, ref)
        assert abs(float(y.double().norm()) - g[f"{case}_out_stats"][0]) / g[f"{case}_out_stats"][0] < 1e-4
    else:
        assert rel_l2(got, ref) < 3e-2, rel_l2(got, ref)


def test_padding_invariance(lib, golden, models):
    """A text's real-token rows do not depend on how far its batch is padded."""
    enc = models["A"]
    enc.compute_dtype = torch.float32
    ids, mask, tt, _ = _inputs(golden, "A")
    full = enc.encode_ids(ids, mask, tt)
    for b in range(ids.shape[0]):
        n = int(mask[b].sum())
        alone = enc.encode_ids(ids[b:b + 1, :n], mask[b:b + 1, :n], tt[b:b + 1, :n])
        assert maxrel(alone[0], full[b, :n]) < 1e-5, (b, maxrel(alone[0], full[b, :n]))


def test_trainer_builds_text_encoder(lib, golden, tmp_path, monkeypatch):
    import pokemon_sprite_generator_amd as psg
    from pokemon_sprite_generator_amd import text_encoder as te
    from tests.test_trainer_gpu import _VAEStub, _config, _loaders
    cfg_b = dict(TC.bert_config(1))
    loaded = []

    def fake_pretrained(name):                          # stands in for the local HF cache: config + weights, no tokenizer
        loaded.append(name)
        with torch.device("meta"):
            shapes = te.TextEncoder(bert_config=cfg_b, hidden_dim=768).bert.state_dict()
        return None, cfg_b, {k: TC.weight("bert." + k, v.shape) for k, v in shapes.items()}

    monkeypatch.setattr(te, "_from_pretrained", fake_pretrained)
    config = _config(tmp_path, epochs=1)
    config["mi355x"] = {"text_dtype": "bf16"}
    comps = {"vae_encoder": _VAEStub(), "data_loaders": _loaders()}
    tr = psg.ImprovedDiffusionTrainer(config, "unused.pth", "text", components=comps, compute_dtype=torch.bfloat16)
    assert isinstance(tr.text_encoder, te.TextEncoder) and loaded == ["stub"]
    assert tr.text_encoder.compute_dtype == torch.bfloat16 and tr.text_dtype == torch.bfloat16
    assert tr.text_encoder.hidden_dim == 256 and not tr.text_encoder.training
    ids, mask, tt, _ = _inputs(golden, "A")
    y = tr.text_encoder.encode_ids(ids, mask, tt)
    assert tuple(y.shape) == (3, ids.shape[1], 256) and torch.isfinite(y).all()
    # an injected factory still wins
    config["mi355x"] = {}
    made = []

    class _Injected(torch.nn.Module):
        def __init__(self, **k):
            super().__init__()
            made.append(k)

    comps = {"vae_encoder": _VAEStub(), "data_loaders": _loaders(), "TextEncoder": _Injected}
    tr2 = psg.ImprovedDiffusionTrainer(config, "unused.pth", "text2", components=comps, compute_dtype=torch.bfloat16)
    assert made == [{"model_name": "stub", "hidden_dim": 256}] and isinstance(tr2.text_encoder, _Injected)
    assert tr2.text_dtype == torch.float32
