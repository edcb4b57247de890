"""-m gpu: the VAE has one forward body per module (pokemon_sprite_generator_amd/vae.py), so

  * a frozen module and a trainable one give the same bits under no_grad, and the forward value of a with-grad call is the
    no_grad value;
  * every prepared weight follows `ops.WeightCache`'s one stamp: a block called through its own `forward` sees an update
    that bumps the version counter and one written through `.data` + `WeightCache.invalidate()` (raw-pointer optimizers);
  * a collected module leaves no entry in the `WeightCache`.

The decoder's image is computed in 8 output columns by a with-grad call and in 4 by a no_grad call, two different launches.
The version of vae.py with two forwards per module gave the same bits for both in fp32 and in bf16 (measured when the two
were merged), so the bitwise assertion applies here too, not the bar of test_vae_decoder_golden."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


@pytest.fixture(scope="module")
def psg():
    import pokemon_sprite_generator_amd as m
    from pokemon_sprite_generator_amd import _lib
    _lib.init(0)
    return m


def _rand(*shape, seed):
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(DEV)


def _twin(make, dtype, trainable, src=None):
    """A module from `make()` on the device, computing in `dtype`; with `src`'s weights when given."""
    torch.manual_seed(1234)
    m = make()
    if src is not None:
        m.load_state_dict(src.state_dict())
    m.compute_dtype = dtype
    for p in m.parameters():
        p.requires_grad_(trainable)
    return m.to(DEV)


def _as_tuple(y):
    return tuple(y) if isinstance(y, (tuple, list)) else (y,)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(_as_tuple(a), _as_tuple(b), strict=True))


# ------------------------------------------------------------------------------------------------- one path, same bits
@DTYPES
@pytest.mark.parametrize("cin,cout", [(32, 64), (32, 32)], ids=["shortcut", "identity"])
def test_resnet_block_one_path(psg, dtype, cin, cout):
    frozen = _twin(lambda: psg.vae.ResNetBlock(cin, cout), dtype, False)
    trainable = _twin(lambda: psg.vae.ResNetBlock(cin, cout), dtype, True, frozen)
    x = _rand(1, cin, 5, 7, seed=1)
    with torch.no_grad():
        y = frozen(x)
        assert torch.equal(trainable(x), y)
    yg = frozen(x.clone().requires_grad_())
    assert yg.requires_grad and torch.equal(yg.detach(), y)


@DTYPES
def test_cross_attention_block_one_path(psg, dtype):
    frozen = _twin(lambda: psg.vae.CrossAttentionBlock(32, 256), dtype, False)
    trainable = _twin(lambda: psg.vae.CrossAttentionBlock(32, 256), dtype, True, frozen)
    x, text = _rand(1, 32, 4, 6, seed=2), _rand(1, 3, 256, seed=3)
    with torch.no_grad():
        y = frozen(x, text)
        assert torch.equal(trainable(x, text), y)
    yg = frozen(x.clone().requires_grad_(), text.clone().requires_grad_())
    assert yg.requires_grad and torch.equal(yg.detach(), y)


@DTYPES
def test_encoder_one_path(psg, dtype):
    frozen = _twin(lambda: psg.VAEEncoder(3, 8), dtype, False)
    trainable = _twin(lambda: psg.VAEEncoder(3, 8, trainable=True), dtype, True, frozen)
    x, eps = _rand(1, 3, 215, 215, seed=4), _rand(1, 8, 27, 27, seed=5)
    with torch.no_grad():
        y = frozen(x, eps=eps)
        assert _same(trainable(x, eps=eps), y)
    yg = trainable(x, eps=eps)
    assert all(t.requires_grad for t in yg) and _same([t.detach() for t in yg], y)


@DTYPES
def test_decoder_one_path(psg, dtype):
    frozen = _twin(lambda: psg.VAEDecoder(8, 256, 3), dtype, False)
    trainable = _twin(lambda: psg.VAEDecoder(8, 256, 3, trainable=True), dtype, True, frozen)
    lat, text = _rand(1, 8, 27, 27, seed=6), _rand(1, 3, 256, seed=7)
    with torch.no_grad():
        y = frozen(lat, text)
        assert torch.equal(trainable(lat, text), y)
    for yg in (trainable(lat, text), frozen(lat, text.clone().requires_grad_())):      # the image in 8 output columns, not 4
        assert yg.requires_grad and torch.equal(yg.detach(), y)


# ------------------------------------------------------------------------------------------------------------ staleness
def _update(module, bump, ops):
    """New weights: in place under no_grad (the version counters move), or through `.data` + WeightCache.invalidate()."""
    with torch.no_grad():
        for p in module.parameters():
            (p if bump else p.data).mul_(0.75).add_(0.01)
    if not bump:
        ops.WeightCache.invalidate()


@DTYPES
@pytest.mark.parametrize("bump", [False, True], ids=["invalidate", "version"])
def test_blocks_see_a_weight_update_through_their_own_forward(psg, dtype, bump):
    ops = psg.ops
    dec = _twin(lambda: psg.PokemonVAE(8, 256, trainable=True), dtype, True).decoder
    res, att = dec.block5_resnet1, dec.block5_attn
    res.compute_dtype = att.compute_dtype = dtype
    x, xa, text = _rand(1, 64, 5, 7, seed=8), _rand(1, 32, 4, 6, seed=9), _rand(1, 3, 256, seed=10)
    with torch.no_grad():
        before = res(x), att(xa, text)
        _update(dec, bump, ops)
        after = res(x), att(xa, text)                              # the blocks' own forward: the decoder is never called
        fresh = (_twin(lambda: psg.vae.ResNetBlock(64, 32), dtype, False, res)(x),
                 _twin(lambda: psg.vae.CrossAttentionBlock(32, 256), dtype, False, att)(xa, text))
    for b, a, f, name in zip(before, after, fresh, ("ResNetBlock", "CrossAttentionBlock")):
        assert torch.equal(a, f), f"{name} computed with stale weights"
        assert not torch.equal(a, b), name


@DTYPES
@pytest.mark.parametrize("bump", [False, True], ids=["invalidate", "version"])
def test_encoder_and_decoder_see_a_weight_update(psg, dtype, bump):
    ops = psg.ops
    vae = _twin(lambda: psg.PokemonVAE(8, 256, trainable=True), dtype, True)
    vae.encoder.compute_dtype = vae.decoder.compute_dtype = dtype
    img, eps = _rand(1, 3, 215, 215, seed=11), _rand(1, 8, 27, 27, seed=12)
    lat, text = _rand(1, 8, 27, 27, seed=13), _rand(1, 3, 256, seed=14)
    with torch.no_grad():
        before = vae.encoder(img, eps=eps), vae.decoder(lat, text)
        _update(vae, bump, ops)
        after = vae.encoder(img, eps=eps), vae.decoder(lat, text)
        fresh = (_twin(lambda: psg.VAEEncoder(3, 8), dtype, False, vae.encoder)(img, eps=eps),
                 _twin(lambda: psg.VAEDecoder(8, 256, 3), dtype, False, vae.decoder)(lat, text))
    for b, a, f, name in zip(before, after, fresh, ("VAEEncoder", "VAEDecoder")):
        assert _same(a, f), f"{name} computed with stale weights"
        assert not _same(a, b), name


# ------------------------------------------------------------------------------------------------------------- lifetime
@DTYPES
def test_collected_decoders_leave_the_weight_cache(psg, dtype):
    ops = psg.ops
    lat, text = _rand(1, 8, 27, 27, seed=15), _rand(1, 3, 256, seed=16)
    gc.collect()
    n0 = len(ops.WeightCache._entries)
    for _ in range(3):
        dec = _twin(lambda: psg.VAEDecoder(8, 256, 3), dtype, False)
        with torch.no_grad():
            dec(lat, text)
        del dec
        gc.collect()
    assert len(ops.WeightCache._entries) == n0
