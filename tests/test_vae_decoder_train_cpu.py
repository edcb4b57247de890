"""The trainable VAE decoder's host side (no GPU): the constructor keyword and the parameter flags of VAEDecoder / PokemonVAE,
`ops.pad_rows` (the 3-channel image conv's parameters in 8 rows) under autograd and through ops.GradSink, and the record
tests/golden/vae_decoder_grad_bf16.json (tools/make_golden_vae_decoder.py) that the GPU test's bf16 bar is read from."""
import pytest
import torch

from tests import vae_decoder_ref as R


def test_trainable_flag_sets_the_parameter_flags():
    import pokemon_sprite_generator_amd as psg
    frozen, train = psg.VAEDecoder(), psg.VAEDecoder(8, 256, 3, trainable=True)
    assert len(list(frozen.parameters())) == 144 and not any(p.requires_grad for p in frozen.parameters())
    assert len(list(train.parameters())) == len(train.state_dict()) == 144 and all(p.requires_grad for p in train.parameters())
    assert frozen.trainable is False and train.trainable is True
    assert list(frozen.state_dict()) == list(train.state_dict())
    with pytest.raises(psg.PsgError):                                       # no CPU fallback on either path
        train(torch.zeros(1, 8, 27, 27), torch.zeros(1, 4, 256))
    with pytest.raises(psg.PsgError):
        frozen(torch.zeros(1, 8, 27, 27), torch.zeros(1, 4, 256))
    vae = psg.PokemonVAE()                                                  # the default VAE is what it was
    assert vae.trainable is False and vae.encoder.trainable is False and vae.decoder.trainable is False
    assert not any(p.requires_grad for p in vae.parameters())
    tv = psg.PokemonVAE(8, 256, trainable=True)
    assert tv.encoder.trainable and tv.decoder.trainable and all(p.requires_grad for p in tv.parameters())
    assert list(tv.state_dict()) == list(vae.state_dict()) and len(tv.state_dict()) == 214


def test_pad_rows_gradient_is_the_unpadded_rows_and_reaches_a_sink():
    from pokemon_sprite_generator_amd import ops
    w = torch.arange(3 * 4 * 3 * 3, dtype=torch.float32).reshape(3, 4, 3, 3).requires_grad_(True)
    b = torch.tensor([1.0, 2.0, 3.0], requires_grad=True)
    w8, b8 = ops.pad_rows(w, 5), ops.pad_rows(b, 5)
    assert tuple(w8.shape) == (8, 4, 3, 3) and tuple(b8.shape) == (8,) and w8.is_contiguous()
    assert torch.equal(w8[:3], w.detach()) and not w8[3:].any() and torch.equal(b8, torch.tensor([1.0, 2, 3, 0, 0, 0, 0, 0]))
    gw, gb = torch.randn(8, 4, 3, 3), torch.randn(8)
    torch.autograd.backward([w8, b8], [gw, gb])
    assert torch.equal(w.grad, gw[:3]) and torch.equal(b.grad, gb[:3])
    # registered: first use in a step writes the view, later uses accumulate, autograd gets nothing
    w.grad = None
    owner, ready = object(), []
    view = torch.full((3, 4, 3, 3), float("nan"))
    try:
        ops.GradSink.register(w, view, 0, on_ready=ready.append, owner=owner)
        ops.GradSink.begin_step(owner)
        ops.pad_rows(w, 5).backward(gw)
        assert w.grad is None and torch.equal(view, gw[:3]) and ready == [0] and ops.GradSink.unwritten(owner) == []
        ops.pad_rows(w, 5).backward(gw)
        assert w.grad is None and torch.equal(view, 2 * gw[:3])
    finally:
        ops.GradSink.unregister(owner)


def test_the_bf16_record_names_every_parameter_of_every_case():
    import pokemon_sprite_generator_amd as psg
    gold = R.load_bf16_golden()
    assert gold["tag"] == R.TAG
    assert set(gold["cases"]) == set(R.CASES)
    names = set(psg.VAEDecoder().state_dict())
    assert set(R.ZERO_GRAD) | set(R.ZERO_GRAD.values()) <= names
    for case, rec in gold["cases"].items():
        assert set(rec["rel_l2"]) == names, case
        assert all(0.0 <= v < 1.0 for v in rec["rel_l2"].values()), case        # a bf16 run, not noise
        assert all(0.0 < rec[k] < 1.0 for k in ("image", "latent", "text")), case


def test_case_inputs_have_the_declared_shapes():
    for case, (B, S, (lh, lw)) in R.CASES.items():
        lat, text, img = R.inputs(case)
        assert tuple(lat.shape) == (B, 8, lh, lw) and tuple(text.shape) == (B, S, 256) and tuple(img.shape) == (B, 3, 215, 215)
    assert all(c % R.CASES["s20"][1] for c in (512, 256, 128, 64, 32))         # s20: S divides no channel count
