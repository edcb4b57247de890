"""-m gpu: VAEEncoder(trainable=True) - stage 1's encoder on the HIP kernels - against fp64 autograd of
oracle.vae_oracle.vae_encode with the same eps, under loss = mean(latent * G) + ops.kl_loss(mu, logvar).

fp32: outputs and the gradient of every one of the 70 parameters at the project's fp32 bar (max-rel < 1e-3, FP32_TOL of
tests/test_vae_gpu.py).  bf16: per-parameter rel-L2 < max(4e-2, 1.5 x what torch bf16 autograd of the oracle measures for that
parameter) - the rule of tests/test_text_encoder_train_gpu.py (BF16_SAMPLE_BAR); the torch figures are recorded by
tests/test_conv4s2_cpu.py in tests/golden/vae_encoder_grad_bf16.json, never taken from our own error.  The gradient of
encoder.2.conv1.bias is exactly zero in exact arithmetic (GroupNorm(32, 32) removes a per-channel constant; fp64 leaves 4e-17,
torch fp32 1.6e-8): it is checked absolutely, on the scale of its sibling encoder.2.conv2.bias.

Measured on MI355X (B2, 23x27, stress weights).  fp32: outputs max-rel <= 2.0e-6, worst per-parameter max-rel 5.7e-6
(encoder.5.norm1.weight), the zero-gradient bias 2.1e-7 of its sibling.  bf16: outputs rel-L2 1.2e-2 / 1.4e-2 / 1.4e-2; worst
per-parameter rel-L2 5.8e-2 (encoder.2.conv2.bias: torch bf16 6.3e-2, bar 9.5e-2; the early layers are the far end of the
chain in both), worst own / torch ratio 2.5 (logvar_proj.bias: 1.4e-2 against torch's 5.7e-3, bar 4e-2); the zero-gradient
bias 2.6e-3 of its sibling (torch bf16 3.9e-3).  Real size (B1, 215x215, fp32): worst 3.7e-6 (encoder.0.weight)."""
import pytest
import torch

from tests import conv4s2_ref as R
from tests.util import maxrel, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP32_TOL = 1e-3
BF16_FLOOR = 4e-2


@pytest.fixture(scope="module")
def psg():
    import pokemon_sprite_generator_amd as m
    from pokemon_sprite_generator_amd import _lib
    _lib.init(0)
    yield m
    m.ops.GradSink.unregister_all()
    m.ops.WeightCache.clear()


@pytest.fixture(scope="module")
def small(psg):
    """Weights, inputs and the fp64 reference of the B2 23x27 case, computed once."""
    sd = R.encoder_state({k: tuple(v.shape) for k, v in psg.VAEEncoder().state_dict().items()})
    img, eps, G = R.encoder_inputs()
    ref, ref_out = R.oracle_run(sd, img, eps, G, torch.float64, device=DEV)
    return sd, img.to(DEV), eps.to(DEV), G.to(DEV), ref, ref_out


def _encoder(psg, sd, dtype=torch.float32, trainable=True):
    enc = psg.VAEEncoder(3, 8, compute_dtype=dtype, trainable=trainable)
    enc.load_state_dict(sd)
    return enc.to(DEV)


def _step(psg, enc, img, eps, G):
    """One forward + backward; returns (latent, mu, logvar)."""
    latent, mu, logvar = enc(img, eps=eps)
    ((latent * G).mean() + psg.ops.kl_loss(mu, logvar)).backward()
    return latent, mu, logvar


def _grads(enc):
    return {n: p.grad for n, p in enc.named_parameters()}


def test_fp32_outputs_and_all_70_gradients(psg, small):
    sd, img, eps, G, ref, ref_out = small
    enc = _encoder(psg, sd)
    out = _step(psg, enc, img, eps, G)
    assert all(t.dtype == torch.float32 and t.shape == (2, 8, 3, 4) and t.grad_fn is not None for t in out)
    for got, want, name in zip(out, ref_out, ("latent", "mu", "logvar")):
        e = maxrel(got, want)
        print(f"fp32 {name}: max-rel {e:.2e}")
        assert e < FP32_TOL, (name, e)
    grads = _grads(enc)
    assert len(grads) == 70 and all(g is not None for g in grads.values())
    sibling = float(ref[R.ZERO_GRAD_SIBLING].abs().max())
    worst = (0.0, "")
    for n, g in grads.items():
        if n == R.ZERO_GRAD:
            z = float(g.abs().max())
            print(f"fp32 {n}: max |g| {z:.2e} = {z / sibling:.2e} of its sibling's {sibling:.2e}")
            assert z <= 1e-3 * sibling, (n, z, sibling)
            continue
        e = maxrel(g, ref[n])
        print(f"fp32 {n}: max-rel {e:.2e}")
        worst = max(worst, (e, n))
        assert e < FP32_TOL, (n, e)
    print(f"fp32 worst per-parameter max-rel {worst[0]:.2e} ({worst[1]})")


def test_bf16_gradients_against_the_recorded_torch_bf16(psg, small):
    sd, img, eps, G, ref, ref_out = small
    rec = R.load_bf16_golden()["rel_l2"]
    assert set(rec) == set(ref)
    enc = _encoder(psg, sd, torch.bfloat16)
    out = _step(psg, enc, img, eps, G)
    for got, want, name in zip(out, ref_out, ("latent", "mu", "logvar")):
        e = rel_l2(got, want)
        print(f"bf16 {name}: rel-L2 {e:.2e}")
        assert e < 3e-2, (name, e)                                   # the frozen encoder's bf16 bar (tests/test_vae_gpu.py)
    sibling = float(ref[R.ZERO_GRAD_SIBLING].abs().max())
    worst, worst_ratio = (0.0, ""), (0.0, "")
    for n, g in _grads(enc).items():
        bar = max(BF16_FLOOR, 1.5 * rec[n])
        e = float(g.abs().max()) / sibling if n == R.ZERO_GRAD else rel_l2(g, ref[n])
        print(f"bf16 {n}: {'max|g| / sibling' if n == R.ZERO_GRAD else 'rel-L2'} {e:.2e} (torch bf16 {rec[n]:.2e}, bar {bar:.2e})")
        if n != R.ZERO_GRAD:
            worst, worst_ratio = max(worst, (e, n)), max(worst_ratio, (e / max(rec[n], 1e-30), n))
        assert e < bar, (n, e, bar)
    print(f"bf16 worst rel-L2 {worst[0]:.2e} ({worst[1]}); worst own / torch ratio {worst_ratio[0]:.2f} ({worst_ratio[1]})")


def test_fp32_real_size(psg):
    """B1, 215x215: mu / logvar and the gradients of the three 4x4 convolutions and of the two projections."""
    names = [f"encoder.{i}.{s}" for i in (0, 3, 6) for s in ("weight", "bias")] + [f"{p}_proj.{s}" for p in ("mu", "logvar") for s in ("weight", "bias")]
    sd = R.encoder_state({k: tuple(v.shape) for k, v in psg.VAEEncoder().state_dict().items()}, seed=R.ENC_SEED + 1)
    img, eps, G = R.encoder_inputs((1, 3, 215, 215), (27, 27))
    ref, ref_out = R.oracle_run(sd, img, eps, G, torch.float64, only=set(names), device=DEV)
    enc = _encoder(psg, sd)
    out = _step(psg, enc, img.to(DEV), eps.to(DEV), G.to(DEV))
    assert out[0].shape == (1, 8, 27, 27)
    for got, want, name in zip(out[1:], ref_out[1:], ("mu", "logvar")):
        assert maxrel(got, want) < FP32_TOL, name
    grads = _grads(enc)
    for n in names:
        e = maxrel(grads[n], ref[n])
        print(f"real size fp32 {n}: max-rel {e:.2e}")
        assert e < FP32_TOL, (n, e)


def test_default_encoder_stays_frozen_and_no_grad_is_the_frozen_path(psg, small):
    sd, img, eps, G, _, _ = small
    frozen = _encoder(psg, sd, trainable=False)
    assert not any(p.requires_grad for p in frozen.parameters())
    with torch.enable_grad():
        f_out = frozen(img, eps=eps)
    assert all(t.grad_fn is None and not t.requires_grad for t in f_out)
    enc = _encoder(psg, sd)
    with torch.no_grad():
        t_out = enc(img, eps=eps)
    assert all(t.grad_fn is None for t in t_out)
    for a, b in zip(t_out, f_out):
        assert torch.equal(a, b)
    with pytest.raises(psg.PsgError, match="requires_grad"):
        enc(img.clone().requires_grad_(True), eps=eps)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_two_runs_and_a_raw_pointer_update_are_bitwise(psg, small, dtype):
    sd, img, eps, G, _, _ = small
    enc = _encoder(psg, sd, dtype)
    o1 = _step(psg, enc, img, eps, G)
    g1 = {n: g.clone() for n, g in _grads(enc).items()}
    enc.zero_grad(set_to_none=True)
    o2 = _step(psg, enc, img, eps, G)
    for a, b in zip(o1, o2):
        assert torch.equal(a, b)
    for n, g in _grads(enc).items():
        assert torch.equal(g, g1[n]), n
    # an optimizer that writes through raw pointers: the data moves, the version counters do not
    enc.zero_grad(set_to_none=True)
    with torch.no_grad():
        for i, p in enumerate(enc.parameters()):
            p.data.add_(0.01 * (1 + i % 3) * torch.sign(p.data))
    psg.ops.WeightCache.invalidate()
    o3 = _step(psg, enc, img, eps, G)
    assert not torch.equal(o3[1], o1[1])
    fresh = _encoder(psg, {k: v.detach().clone() for k, v in enc.state_dict().items()}, dtype)
    o4 = _step(psg, fresh, img, eps, G)
    for a, b in zip(o3, o4):
        assert torch.equal(a, b)
    gf = _grads(fresh)
    for n, g in _grads(enc).items():
        assert torch.equal(g, gf[n]), n
    with torch.no_grad():                                           # the inference launches see the update too
        for a, b in zip(enc(img, eps=eps), fresh(img, eps=eps)):
            assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_grad_sink_delivery(psg, small, dtype):
    sd, img, eps, G, _, _ = small
    ops = psg.ops
    enc = _encoder(psg, sd, dtype)
    _step(psg, enc, img, eps, G)
    want = {n: g.clone() for n, g in _grads(enc).items()}
    enc.zero_grad(set_to_none=True)
    owner = object()
    views, ready = {}, []
    try:
        for i, (n, p) in enumerate(enc.named_parameters()):
            views[n] = torch.full_like(p, float("nan"), dtype=torch.float32)
            ops.GradSink.register(p, views[n], i, on_ready=ready.append, owner=owner)
        ops.GradSink.begin_step(owner)
        assert len(ops.GradSink.unwritten(owner)) == 70
        _step(psg, enc, img, eps, G)
        assert ops.GradSink.unwritten(owner) == [] and sorted(ready) == list(range(70))
        for n, p in enc.named_parameters():
            assert p.grad is None, n
            assert torch.equal(views[n], want[n]), n
        _step(psg, enc, img, eps, G)                                # a second backward in the same step accumulates
        for n, p in enc.named_parameters():
            assert p.grad is None, n
            assert torch.equal(views[n], 2 * want[n]), n
    finally:
        ops.GradSink.unregister(owner)
