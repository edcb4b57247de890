"""-m gpu: `SpriteGenerator`, the headless PokemonGradioGenerator (gradio_app.py:161-465), against the chain composed by hand
from its parts - the same kernels on the same inputs, so equality means the same bits.  A PokemonVAE, a two-layer BERT driven
through token ids and a stand-in U-Net (a fixed linear function of the latent: the samplers have their own tests against the
reference); B = 2, three inference steps, every random draw injected."""
import numpy as np
import pytest
import torch

from oracle import hashgen
from tests import text_cases as TC
from tests import text_grad_cases as GC

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 3


class StandInUNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.tensor(0.25))
        self.shift = torch.nn.Parameter(torch.tensor(-0.05))

    def forward(self, latent, timesteps, text_emb):
        return latent * self.scale + self.shift


def _draw(tag, shape):
    return hashgen.uniform(tuple(shape), 77, hashgen.name_id(f"generate.{tag}")) * 1.7


def noise_fn(i, shape):
    return _draw(f"z{i}", shape).to(DEV)


@pytest.fixture(scope="module")
def psg():
    import pokemon_sprite_generator_amd as m
    from pokemon_sprite_generator_amd import _lib
    _lib.init(0)
    return m


@pytest.fixture(scope="module")
def gen(psg):
    vae = psg.PokemonVAE(latent_dim=8, text_dim=256)
    vae.load_state_dict(hashgen.fill_unet_state({k: tuple(v.shape) for k, v in vae.state_dict().items()}, 11, "stress"))
    te = psg.TextEncoder(bert_config=TC.bert_config(2), hidden_dim=256, finetune_strategy="none")
    te.load_state_dict(GC.state_dict(te), strict=True)
    return psg.SpriteGenerator(vae.to(DEV), StandInUNet().to(DEV), te.to(DEV))


@pytest.fixture(scope="module")
def tokens(golden):
    g = golden("text_encoder_grad.npz")
    return torch.from_numpy(g["M_input_ids"])[:2], torch.from_numpy(g["M_attention_mask"])[:2]


@pytest.fixture(scope="module")
def uploads():
    rng = np.random.default_rng(5)
    return [rng.integers(0, 256, (180, 300, 3), dtype=np.uint8) for _ in range(2)]         # 300 x 180 RGB


def _by_hand(psg, gen, uploads, tokens, strength):
    from pokemon_sprite_generator_amd import imaging
    x = torch.stack([imaging.pil_to_tensor(u, 215, DEV) for u in uploads])
    latent, _, _ = gen.vae.encode(x, eps=_draw("eps", (2, 8, 27, 27)).to(DEV))
    if strength > 0:
        latent = imaging.mix_latent(latent, _draw("noise", (2, 8, 27, 27)).to(DEV), strength)
    text = gen.text_encoder.encode_ids(*tokens)
    latent = psg.gradio_ddpm_sample(gen.unet, text, STEPS, initial_latent=latent, noise_fn=noise_fn)
    return imaging.to_uint8(gen.vae.decode(latent, text))


def _generate(gen, uploads, tokens, strength, **kw):
    return gen.generate_from_image_and_text(uploads, tokens, num_inference_steps=STEPS, noise_strength=strength,
                                            eps=_draw("eps", (2, 8, 27, 27)), noise=_draw("noise", (2, 8, 27, 27)), noise_fn=noise_fn, **kw)


def test_image_and_text_equals_the_chain_by_hand(psg, gen, uploads, tokens):
    got = _generate(gen, uploads, tokens, 0.7)
    assert got.dtype == torch.uint8 and got.shape == (2, 215, 215, 3) and got.is_cuda
    assert torch.equal(got, _by_hand(psg, gen, uploads, tokens, 0.7))
    assert not torch.equal(got[0], got[1])
    assert len(torch.unique(got)) > 16                                   # (an image, not a constant)


def test_noise_strength_zero_skips_the_mix(psg, gen, uploads, tokens):
    got = _generate(gen, uploads, tokens, 0.0)
    assert torch.equal(got, _by_hand(psg, gen, uploads, tokens, 0.0))
    assert not torch.equal(got, _by_hand(psg, gen, uploads, tokens, 0.7))
    state = torch.cuda.get_rng_state()                                   # ... and draws nothing for it
    gen.generate_from_image_and_text(uploads, tokens, num_inference_steps=STEPS, noise_strength=0.0, eps=_draw("eps", (2, 8, 27, 27)),
                                     noise_fn=noise_fn)
    assert torch.equal(state, torch.cuda.get_rng_state())


def test_non_rgb_uploads_are_converted_first(gen, tokens):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(6)
    rgba = Image.fromarray(rng.integers(0, 256, (90, 120, 4), dtype=np.uint8), "RGBA")
    grey = Image.fromarray(rng.integers(0, 256, (250, 230), dtype=np.uint8), "L")
    got = _generate(gen, [rgba, grey], tokens, 0.7)
    assert torch.equal(got, _generate(gen, [rgba.convert("RGB"), grey.convert("RGB")], tokens, 0.7))


def test_text_only_equals_sampler_decode_to_uint8(psg, gen, tokens):
    from pokemon_sprite_generator_amd import imaging
    got = gen.generate_from_text(tokens, num_inference_steps=STEPS, noise_fn=noise_fn)
    text = gen.text_encoder.encode_ids(*tokens)
    latent = psg.gradio_ddpm_sample(gen.unet, text, STEPS, noise_fn=noise_fn)
    assert got.dtype == torch.uint8 and got.shape == (2, 215, 215, 3)
    assert torch.equal(got, imaging.to_uint8(gen.vae.decode(latent, text)))


def test_seed_reproduces_the_bytes(gen, uploads, tokens):
    a = gen.generate_from_image_and_text(uploads, tokens, num_inference_steps=STEPS, seed=123)
    b = gen.generate_from_image_and_text(uploads, tokens, num_inference_steps=STEPS, seed=123)
    c = gen.generate_from_image_and_text(uploads, tokens, num_inference_steps=STEPS, seed=124)
    assert torch.equal(a, b) and not torch.equal(a, c)
    t1 = gen.generate_from_text(tokens, num_inference_steps=STEPS, seed=9)
    assert torch.equal(t1, gen.generate_from_text(tokens, num_inference_steps=STEPS, seed=9))


def test_as_pil_and_single_items(psg, gen, uploads, tokens):
    pytest.importorskip("PIL")
    ref = _generate(gen, uploads, tokens, 0.7)
    pil = _generate(gen, uploads, tokens, 0.7, as_pil=True)
    assert len(pil) == 2 and all(p.mode == "RGB" and p.size == (215, 215) for p in pil)
    assert np.array_equal(np.asarray(pil[1]), ref[1].cpu().numpy())
    one = (tokens[0][:1], tokens[1][:1])
    single = gen.generate_from_image_and_text(uploads[0], one, num_inference_steps=STEPS, eps=_draw("eps", (2, 8, 27, 27))[:1],
                                              noise=_draw("noise", (2, 8, 27, 27))[:1], noise_fn=lambda i, shape: noise_fn(i, (2,) + tuple(shape[1:]))[:1],
                                              as_pil=True)
    assert single.mode == "RGB" and single.size == (215, 215)
    with pytest.raises(psg.PsgError):
        gen.generate_from_image_and_text(uploads, one, num_inference_steps=STEPS)         # two images, one description
