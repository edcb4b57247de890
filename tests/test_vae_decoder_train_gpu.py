"""-m gpu: VAEDecoder(trainable=True) / PokemonVAE(trainable=True) - stage 1's decoder on the HIP kernels - against fp64
autograd of oracle.vae_oracle.vae_decode (run on the device) under loss = final_cases.recon_loss(decoder(latent, text), img),
on the cases of tests/vae_decoder_ref.py (s20: B1, S20, 27x27 latent; b2: B2, S32, 5x6 latent).

fp32: the image, the gradient of every one of the 144 parameters, d latent and d text at the project's fp32 bar (max-rel < 1e-3,
FP32_TOL of tests/test_vae_gpu.py).  bf16: per-parameter rel-L2 < max(4e-2, 1.5 x what torch bf16 autograd of the oracle measures
for that parameter on the CPU, tests/golden/vae_decoder_grad_bf16.json by tools/make_golden_vae_decoder.py) - never taken from
our own error; the image at the frozen decoder's bf16 bar (rel-L2 < 3e-2, tests/test_vae_gpu.py).  The gradients of
block5_resnet{1,2}.conv1.bias are exactly zero in exact arithmetic (GroupNorm(32, 32) removes a per-channel constant): they are
checked absolutely, <= 1e-3 x the max-abs of their conv2.bias sibling's gradient.

Measured on MI355X (b2 / s20).  fp32: image max-rel 3.8e-6 / 6.8e-6, d latent 2.0e-6 / 2.3e-6, d text 1.2e-6 / 6.7e-7, worst
per-parameter max-rel 2.7e-6 (block5_attn.norm.weight) / 1.6e-6 (latent_proj.weight), the zero-gradient biases 6e-8 - 1.3e-7 of
their siblings.  bf16, with the slim weight-gradient route active (8 launches in b2, 15 in s20): image rel-L2 1.3e-2 / 1.4e-2;
d latent 2.5e-2 / 4.3e-2 (torch bf16 2.4e-2 / 4.5e-2), d text 1.7e-2 / 9.6e-3; worst per-parameter rel-L2 2.6e-2
(block2_attn.norm.weight) / 3.2e-2 (latent_proj.weight: torch bf16 3.3e-2), worst own / torch ratio 2.7 (final_conv.2.bias in b2:
8.2e-3 against torch's 3.1e-3, bar 4e-2) / 1.0; the zero-gradient biases 4e-5 - 7e-5 of their siblings (torch bf16 4e-4 - 6e-4).
SGD: the five losses follow the fp64 oracle's to 7e-8 relative; the decoder's weights move the image by 4e-4 per step, below the
fp32 bar, so staleness is asserted bitwise against a fresh module."""
import pytest
import torch

from oracle import hashgen, vae_oracle as V
from tests import vae_decoder_ref as R
from tests.util import h, maxrel, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP32_TOL = 1e-3
BF16_FLOOR = 4e-2
BF16_IMAGE = 3e-2                                     # the frozen decoder's bf16 bar (tests/test_vae_gpu.py)
SGD_LR = 1e-3                                         # picked on the CPU: the oracle's loss decreases over the three steps
SGD_SEED = 77


@pytest.fixture(scope="module")
def psg():
    import pokemon_sprite_generator_amd as m
    from pokemon_sprite_generator_amd import _lib
    _lib.init(0)
    yield m
    m.ops.GradSink.unregister_all()
    m.ops.WeightCache.clear()


@pytest.fixture(scope="module")
def cases(psg):
    """Per case: the weights, the inputs on the device and the fp64 reference, computed once and left unchanged."""
    sd = R.decoder_state(psg.VAEDecoder())
    out = {}
    for case in R.CASES:
        lat, text, img = R.inputs(case)
        ref, dlat, dtext, image = R.oracle_run(sd, lat, text, img, torch.float64, device=DEV)
        out[case] = (sd, lat.to(DEV), text.to(DEV), img.to(DEV), ref, dlat, dtext, image)
    return out


def _decoder(psg, sd, dtype=torch.float32, trainable=True):
    dec = psg.VAEDecoder(8, 256, 3, compute_dtype=dtype, trainable=trainable)
    dec.load_state_dict(sd)
    return dec.to(DEV)


def _step(psg, dec, lat, text, img, inputs_grad=True):
    """One forward + backward; returns (image, d latent, d text)."""
    lat, text = lat.clone().requires_grad_(inputs_grad), text.clone().requires_grad_(inputs_grad)
    image = dec(lat, text)
    psg.ops.recon_loss(image, img)[0].backward()
    return image.detach(), lat.grad, text.grad


def _grads(dec):
    return {n: p.grad for n, p in dec.named_parameters()}


def test_trainable_keyword_constructs(psg):
    """On the parent commit the keyword does not exist."""
    dec = psg.VAEDecoder(8, 256, 3, trainable=True)
    assert dec.trainable is True and len(list(dec.parameters())) == len(dec.state_dict()) == 144
    assert all(p.requires_grad for p in dec.parameters())
    vae = psg.PokemonVAE(8, 256, trainable=True)
    assert vae.trainable and vae.encoder.trainable and vae.decoder.trainable and all(p.requires_grad for p in vae.parameters())


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_fp32_image_and_all_gradients(psg, cases, case):
    sd, lat, text, img, ref, dlat, dtext, image = cases[case]
    assert R.zero_grad_names(ref) == set(R.ZERO_GRAD)
    dec = _decoder(psg, sd)
    slim0 = psg.ops.SlimStats.launches
    got, glat, gtext = _step(psg, dec, lat, text, img)
    assert psg.ops.SlimStats.launches == slim0                     # fp32 keeps going to psg_conv_wgrad
    assert got.dtype == torch.float32 and tuple(got.shape) == (lat.shape[0], 3, 215, 215)
    for name, a, b in (("image", got, image), ("d latent", glat, dlat), ("d text", gtext, dtext)):
        e = maxrel(a, b)
        print(f"{case} fp32 {name}: max-rel {e:.2e}")
        assert e < FP32_TOL, (name, e)
    grads = _grads(dec)
    assert len(grads) == len(dec.state_dict()) == len(ref) and all(g is not None for g in grads.values())
    worst = (0.0, "")
    for n, g in grads.items():
        assert g.shape == ref[n].shape, n
        if n in R.ZERO_GRAD:
            z, sibling = float(g.abs().max()), float(ref[R.ZERO_GRAD[n]].abs().max())
            print(f"{case} fp32 {n}: max |g| {z:.2e} = {z / sibling:.2e} of its sibling's {sibling:.2e}")
            assert z <= 1e-3 * sibling, (n, z, sibling)
            continue
        e = maxrel(g, ref[n])
        print(f"{case} fp32 {n}: max-rel {e:.2e}")
        worst = max(worst, (e, n))
        assert e < FP32_TOL, (n, e)
    print(f"{case} fp32 worst per-parameter max-rel {worst[0]:.2e} ({worst[1]})")


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_bf16_gradients_against_the_recorded_torch_bf16(psg, cases, case):
    sd, lat, text, img, ref, dlat, dtext, image = cases[case]
    gold = R.load_bf16_golden()
    assert gold["tag"] == R.TAG
    rec = gold["cases"][case]
    assert set(rec["rel_l2"]) == set(ref)
    dec = _decoder(psg, sd, torch.bfloat16)
    slim0 = psg.ops.SlimStats.launches
    got, glat, gtext = _step(psg, dec, lat, text, img)
    # the slim weight-gradient route is active where it was adopted: block 5's seven convolutions and the image convolution
    # (215 x 215) in both cases, block 4's seven (108 x 108) in s20; b2's lower blocks (20 x 24 and below) are too small
    assert psg.ops.SlimStats.launches - slim0 == {"s20": 15, "b2": 8}[case]
    e = rel_l2(got, image)
    print(f"{case} bf16 image: rel-L2 {e:.2e} (torch bf16 {rec['image']:.2e})")
    assert e < BF16_IMAGE, e
    for name, a, b in (("latent", glat, dlat), ("text", gtext, dtext)):
        e, bar = rel_l2(a, b), max(BF16_FLOOR, 1.5 * rec[name])
        print(f"{case} bf16 d {name}: rel-L2 {e:.2e} (torch bf16 {rec[name]:.2e}, bar {bar:.2e})")
        assert e < bar, (name, e, bar)
    worst, worst_ratio = (0.0, ""), (0.0, "")
    for n, g in _grads(dec).items():
        bar = max(BF16_FLOOR, 1.5 * rec["rel_l2"][n])
        e = R.param_error(n, g, ref)
        print(f"{case} bf16 {n}: {'max|g| / sibling' if n in R.ZERO_GRAD else 'rel-L2'} {e:.2e} (torch bf16 {rec['rel_l2'][n]:.2e}, bar {bar:.2e})")
        if n not in R.ZERO_GRAD:
            worst, worst_ratio = max(worst, (e, n)), max(worst_ratio, (e / max(rec["rel_l2"][n], 1e-30), n))
        assert e < bar, (n, e, bar)
    print(f"{case} bf16 worst rel-L2 {worst[0]:.2e} ({worst[1]}); worst own / torch ratio {worst_ratio[0]:.2f} ({worst_ratio[1]})")


def test_the_frozen_contract_still_holds(psg, cases):
    sd, lat, text, img = cases["s20"][:4]
    # a default decoder refuses a parameter made trainable by hand, as before
    frozen = _decoder(psg, sd, trainable=False)
    assert frozen.trainable is False and not any(p.requires_grad for p in frozen.parameters())
    frozen.block3_attn.k.weight.requires_grad = True
    with pytest.raises(psg.PsgError, match="requires_grad"):
        frozen(lat, text.clone().requires_grad_(True))
    frozen.block3_attn.k.weight.requires_grad = False
    # no_grad on a trainable decoder is the frozen decoder's inference path, bit for bit
    dec = _decoder(psg, sd)
    with torch.no_grad():
        a, b = dec(lat, text), frozen(lat, text)
    assert a.grad_fn is None and torch.equal(a, b)
    # asking for weight gradients does not change the data path
    f_img, f_dlat, f_dtext = _step(psg, frozen, lat, text, img)
    assert all(p.grad is None for p in frozen.parameters())
    t_img, t_dlat, t_dtext = _step(psg, dec, lat, text, img)
    assert all(p.grad is not None for p in dec.parameters())
    assert torch.equal(t_img, f_img) and torch.equal(t_dlat, f_dlat) and torch.equal(t_dtext, f_dtext)
    # the blocks called on their own keep their guard
    with pytest.raises(psg.PsgError, match="requires_grad"):
        dec.block5_resnet1(torch.zeros(1, 64, 4, 4, device=DEV, requires_grad=True))


def _vae_loss_oracle(p, img, text, eps):
    enc = {k[len("encoder."):]: v for k, v in p.items() if k.startswith("encoder.")}
    dec = {k[len("decoder."):]: v for k, v in p.items() if k.startswith("decoder.")}
    latent, mu, logvar = V.vae_encode(enc, img, eps)
    recon = V.vae_decode(dec, latent, text)
    return (recon - img).abs().mean() + -0.5 * torch.mean(1 + logvar - mu.pow(2) - logvar.exp()), latent


def test_weights_that_move_are_seen(psg):
    """Three SGD steps and one raw-pointer update of PokemonVAE(trainable=True) against the fp64 oracle taking the same steps
    (on the device), then a no_grad decode at the updated weights: no stale prepared operand on either path."""
    ops = psg.ops
    vae = psg.PokemonVAE(8, 256, trainable=True)
    sd = hashgen.fill_unet_state({k: tuple(v.shape) for k, v in vae.state_dict().items()}, SGD_SEED, "stress")
    vae.load_state_dict(sd)
    vae = vae.to(DEV)
    img, text, eps = (t.to(DEV) for t in (h((1, 3, 215, 215), "vaedec.sgd.img", 1.0), h((1, 20, 256), "vaedec.sgd.text", 3.0 ** 0.5),
                                          h((1, 8, 27, 27), "vaedec.sgd.eps", 1.0)))
    p64 = {k: v.to(DEV, torch.float64).requires_grad_(True) for k, v in sd.items()}

    def oracle_step():
        loss, latent = _vae_loss_oracle(p64, img.double(), text.double(), eps.double())
        grads = torch.autograd.grad(loss, list(p64.values()))
        with torch.no_grad():
            for v, g in zip(p64.values(), grads):
                v.sub_(SGD_LR * g)
        return float(loss), latent.detach()

    def own_loss():
        out = vae(img, text, mode="train", eps=eps)
        assert out["reconstructed"].grad_fn is not None and set(out) == {"reconstructed", "latent", "mu", "logvar"}
        return ops.recon_loss(out["reconstructed"], img, 1.0, 0.0)[0] + ops.kl_loss(out["mu"], out["logvar"])

    lat_fix = h((1, 8, 27, 27), "vaedec.sgd.lat", 3.0 ** 0.5).to(DEV)

    def fresh():
        m = psg.PokemonVAE(8, 256, trainable=True)
        m.load_state_dict({k: v.detach().clone() for k, v in vae.state_dict().items()})
        return m.to(DEV)

    with torch.no_grad():                                      # the inference operands are prepared BEFORE any update
        before = vae.decode(lat_fix, text)
    opt = torch.optim.SGD(vae.parameters(), lr=SGD_LR)
    own, want = [], []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        loss = own_loss()
        loss.backward()
        assert all(p.grad is not None for p in vae.parameters())
        opt.step()
        own.append(float(loss))
        want.append(oracle_step()[0])
    print(f"SGD losses own {own} oracle {want}")
    for i in (0, 1):
        assert abs(own[i] - want[i]) < 1e-3 * abs(want[i]), (i, own, want)
    assert want[2] < want[0] and own[2] < own[0], (own, want)
    with torch.no_grad():                                      # prepared again, at the SGD-updated weights
        mid = vae.decode(lat_fix, text)
        assert not torch.equal(mid, before) and torch.equal(mid, fresh().decode(lat_fix, text))
    # a fourth update written through raw pointers: the data moves, the version counters do not
    opt.zero_grad(set_to_none=True)
    loss = own_loss()
    loss.backward()
    with torch.no_grad():
        for p in vae.parameters():
            p.data.add_(p.grad, alpha=-SGD_LR)
    ops.WeightCache.invalidate()
    own.append(float(loss))
    want.append(oracle_step()[0])
    loss5 = own_loss()
    own.append(float(loss5))
    want.append(float(_vae_loss_oracle(p64, img.double(), text.double(), eps.double())[0]))
    print(f"raw-pointer update: losses own {own[3:]} oracle {want[3:]}")
    for i in (3, 4):
        assert abs(own[i] - want[i]) < 1e-3 * abs(want[i]), (i, own, want)
    # The decoder's weights move the image by less than the fp32 bar in one step (4e-4, measured on the CPU oracle), so "no
    # stale operand" is asserted bitwise against a fresh module holding the updated weights, on both paths; the oracle
    # comparison says the updated weights are the right ones.
    new = fresh()
    o = new(img, text, eps=eps)
    assert torch.equal(loss5.detach(), (ops.recon_loss(o["reconstructed"], img, 1.0, 0.0)[0] + ops.kl_loss(o["mu"], o["logvar"])).detach())
    with torch.no_grad():
        after = vae.decode(lat_fix, text)
        assert not torch.equal(after, mid) and torch.equal(after, new.decode(lat_fix, text))
        mu = vae.encode(img)[1]
        assert torch.equal(mu, new.encode(img)[1])
        ref = V.vae_decode({k[len("decoder."):]: v for k, v in p64.items() if k.startswith("decoder.")}, lat_fix.double(), text.double())
        mu_ref = V.vae_encode({k[len("encoder."):]: v for k, v in p64.items() if k.startswith("encoder.")}, img.double(), eps.double())[1]
    e, e_mu = maxrel(after, ref), maxrel(mu, mu_ref)
    print(f"no_grad at the updated weights: decode max-rel {e:.2e} (before the updates {maxrel(before, ref):.2e}), encode mu {e_mu:.2e}")
    assert e < FP32_TOL and e_mu < FP32_TOL, (e, e_mu)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_two_runs_are_bitwise_equal(psg, cases, dtype):
    sd, lat, text, img = cases["b2"][:4]
    runs = []
    for _ in range(2):
        dec = _decoder(psg, sd, dtype)
        image, dlat, dtext = _step(psg, dec, lat, text, img)
        runs.append((image, dlat, dtext, _grads(dec)))
    for a, b in zip(runs[0][:3], runs[1][:3]):
        assert torch.equal(a, b)
    assert len(runs[0][3]) == 144
    for n, g in runs[0][3].items():
        assert torch.equal(g, runs[1][3][n]), n


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_grad_sink_delivery(psg, cases, dtype):
    """Every decoder parameter registered with ops.GradSink: one backward fills every view with what `.grad` gets otherwise,
    final_conv.2.weight / .bias at their own [3,32,3,3] / [3] shapes (delivered through `ops.pad_rows`' small copy)."""
    sd, lat, text, img = cases["s20"][:4]
    ops = psg.ops
    dec = _decoder(psg, sd, dtype)
    _step(psg, dec, lat, text, img, inputs_grad=False)
    want = {n: g.clone() for n, g in _grads(dec).items()}
    assert tuple(want["final_conv.2.weight"].shape) == (3, 32, 3, 3) and tuple(want["final_conv.2.bias"].shape) == (3,)
    dec.zero_grad(set_to_none=True)
    owner = object()
    views, ready = {}, []
    try:
        for i, (n, p) in enumerate(dec.named_parameters()):
            views[n] = torch.full_like(p, float("nan"), dtype=torch.float32)
            ops.GradSink.register(p, views[n], i, on_ready=ready.append, owner=owner)
        ops.GradSink.begin_step(owner)
        assert len(ops.GradSink.unwritten(owner)) == 144
        _step(psg, dec, lat, text, img, inputs_grad=False)
        assert ops.GradSink.unwritten(owner) == [] and sorted(ready) == list(range(144))
        for n, p in dec.named_parameters():
            assert p.grad is None, n
            assert torch.equal(views[n], want[n]), n
        _step(psg, dec, lat, text, img, inputs_grad=False)          # a second backward in the same step accumulates
        for n, p in dec.named_parameters():
            assert p.grad is None, n
            assert torch.equal(views[n], 2 * want[n]), n
    finally:
        ops.GradSink.unregister(owner)
