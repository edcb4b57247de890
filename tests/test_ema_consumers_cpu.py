"""CPU suite for `use_ema=` of the stage-2 checkpoint consumers: `inference.load_unet_state`, `SpriteGenerator.from_checkpoints`
and `FinalPokemonGenerator.from_checkpoints` read 'ema_unet_state_dict' when asked, 'unet_state_dict' by default, and refuse a
checkpoint without the EMA section - with the stand-in modules of tests/test_generate_cpu.py; nothing here launches a kernel."""
import pytest
import torch

from tests.test_generate_cpu import _StandIn


def _checkpoints(tmp_path, with_ema):
    torch.save({"vae_state_dict": {"encoder.a": torch.ones(2), "decoder.b": torch.ones(3)}}, tmp_path / "vae.pth")
    ck = {"unet_state_dict": {"final_conv.2.bias": torch.zeros(8)}, "global_step": 7}
    if with_ema:
        ck["ema_unet_state_dict"], ck["ema_decay"] = {"final_conv.2.bias": torch.full((8,), 0.5)}, 0.999
    torch.save(ck, tmp_path / "unet.pth")
    return str(tmp_path / "vae.pth"), str(tmp_path / "unet.pth")


def test_load_unet_state(tmp_path):
    import pokemon_sprite_generator_amd as psg
    _, with_ema = _checkpoints(tmp_path, True)
    assert float(psg.load_unet_state(with_ema)["final_conv.2.bias"][0]) == 0.0                     # the default is the raw weights
    assert float(psg.load_unet_state(with_ema, use_ema=True)["final_conv.2.bias"][0]) == 0.5
    assert float(psg.load_unet_state(torch.load(with_ema), use_ema=True)["final_conv.2.bias"][0]) == 0.5      # a loaded dict
    _, without = _checkpoints(tmp_path, False)
    assert float(psg.load_unet_state(without)["final_conv.2.bias"][0]) == 0.0
    with pytest.raises(psg.PsgError, match="ema_unet_state_dict"):
        psg.load_unet_state(without, use_ema=True)


@pytest.mark.parametrize("which", ["sprite", "final"])
def test_from_checkpoints_use_ema(monkeypatch, tmp_path, which):
    import pokemon_sprite_generator_amd as psg
    from pokemon_sprite_generator_amd import final, generate
    if which == "sprite":
        for name in ("PokemonVAE", "UNet", "TextEncoder"):
            monkeypatch.setattr(generate, name, type(name, (_StandIn,), {}))
        build = lambda v, u, **kw: generate.SpriteGenerator.from_checkpoints(v, u, {"text_embedding_dim": 128}, device="cpu", **kw)
    else:
        for name in ("VAEEncoder", "VAEDecoder", "UNet", "TextEncoder"):
            monkeypatch.setattr(final, name, type(name, (_StandIn,), {}))
        monkeypatch.setattr(final.FinalPokemonGenerator, "__init__", lambda self, enc, dec, unet, te, sch: object.__setattr__(self, "unet", unet))
        build = lambda v, u, **kw: final.FinalPokemonGenerator.from_checkpoints(v, u, {"text_embedding_dim": 128, "bert_model": "some/bert"}, **kw)
    vae_path, unet_path = _checkpoints(tmp_path, True)
    assert float(build(vae_path, unet_path).unet.loaded["final_conv.2.bias"][0]) == 0.0
    assert float(build(vae_path, unet_path, use_ema=False).unet.loaded["final_conv.2.bias"][0]) == 0.0
    assert float(build(vae_path, unet_path, use_ema=True).unet.loaded["final_conv.2.bias"][0]) == 0.5
    vae_path, unet_path = _checkpoints(tmp_path, False)
    assert float(build(vae_path, unet_path).unet.loaded["final_conv.2.bias"][0]) == 0.0
    with pytest.raises(psg.PsgError, match="ema_unet_state_dict"):
        build(vae_path, unet_path, use_ema=True)
