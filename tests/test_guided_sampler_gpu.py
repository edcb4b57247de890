"""-m gpu: the DDIM chain and the guided forms of the existing chains (guidance.py, DiffusionStepper.sample,
gradio_ddpm_sample) against the restatements of tests/guided_ref.py and tests/step_ref.py, on the bits: the U-Net - a stub, or
the full-width one - supplies eps, and everything the samplers do with it is restated in numpy float32."""
import numpy as np
import pytest
import torch

from oracle import hashgen
from tests import guided_ref as G
from tests import step_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def psg():
    import pokemon_sprite_generator_amd as m
    from pokemon_sprite_generator_amd import _lib
    _lib.init(0)
    return m


def _h(shape, tag, scale=1.0):
    return hashgen.uniform(tuple(shape), 91, hashgen.name_id(f"guided.{tag}")) * scale


class StubUNet(torch.nn.Module):
    """eps as a fixed elementwise function of (x, t, text); keeps the batch size and timestep of every call."""

    def __init__(self):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.tensor(0.35))
        self.calls = []

    def forward(self, x, t, text):
        self.calls.append((x.shape[0], int(t[0].item()) if not torch.cuda.is_current_stream_capturing() else -1))
        return x * self.scale + text[:, :1, :1].reshape(-1, 1, 1, 1) * 0.5 - (t.float() * 1e-3).reshape(-1, 1, 1, 1) * 0.2


class Noise:
    """noise_fn(i, shape) with a record of what was asked for."""

    def __init__(self, tag):
        self.tag, self.asked = tag, []

    def __call__(self, i, shape):
        self.asked.append(i)
        return (_h(shape, f"{self.tag}.{i}", 1.7)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _restated_ddim(unet, text, null, abar, k, eta, w, clip, noise):
    """The chain of guided_ref with eps from the same module on the same batch composition ([x; x] with [text; null] when
    guided), so eps has the bits the sampler saw."""
    n = text.shape[0]
    ts = G.ddim_timesteps(len(abar), k)
    tab = G.ddim_tables(abar, ts, eta)
    text2 = torch.cat([text, null.unsqueeze(0).expand(n, -1, -1)]) if w is not None else text

    def predict(x, t, j):
        xt = torch.from_numpy(x).to(DEV)
        xin = torch.cat([xt, xt]) if w is not None else xt
        with torch.no_grad():
            out = unet(xin, torch.full((xin.shape[0],), t, device=DEV, dtype=torch.long), text2).float()
        return (_np(out[:n]), _np(out[n:])) if w is not None else _np(out)
    x_T = _np(noise(-1, (n, 8, 27, 27)))
    return G.chain(x_T, predict, tab, ts, w=w, clip=clip, eta=eta, noise=lambda i: _np(noise(i, (n, 8, 27, 27))))


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("eta", [0.0, 0.7])
@pytest.mark.parametrize("w", [None, 2.5], ids=["unguided", "guided"])
def test_ddim_sample_on_a_stub_equals_the_restated_chain(psg, w, eta, use_graph):
    n, k = 3, 5
    unet = StubUNet().to(DEV)
    text, null = _h((n, 4, 16), "stub.text").to(DEV), _h((4, 16), "stub.null").to(DEV)
    abar = _np(psg.NoiseScheduler().alphas_cumprod).astype(np.float32)
    noise, trace = Noise("stub"), []
    out = psg.ddim_sample(unet, text, torch.from_numpy(abar), num_steps=k, eta=eta, guidance_scale=w, null_text=null if w is not None else None,
                          noise_fn=noise, trace=trace, use_graph=use_graph)
    torch.cuda.synchronize()
    assert noise.asked == ([-1] if eta == 0 else [-1, 0, 1, 2, 3]), "z is drawn only when eta > 0, and not on the last step"
    if not use_graph:
        ts = [int(t) for t in G.ddim_timesteps(1000, k)]
        assert unet.calls == [(2 * n if w is not None else n, t) for t in ts], "one forward per step, at batch 2n when guided"
    want = _restated_ddim(StubUNet().to(DEV), text, null, abar, k, eta, w, 3.0, Noise("stub"))
    assert len(trace) == k
    for j in range(k):
        assert R.same_bits(_np(trace[j]), want[j]), f"step {j}"
    assert R.same_bits(_np(out), want[-1]) and out.shape == (n, 8, 27, 27)


def test_ddim_sample_argument_errors(psg):
    unet = StubUNet().to(DEV)
    text = _h((2, 4, 16), "stub.text2").to(DEV)
    abar = psg.NoiseScheduler().alphas_cumprod
    with pytest.raises(ValueError, match="null_text"):
        psg.ddim_sample(unet, text, abar, num_steps=3, guidance_scale=2.0)
    with pytest.raises(ValueError):
        psg.ddim_sample(unet, text, abar, num_steps=0)
    with pytest.raises(ValueError, match="clip"):
        psg.ddim_sample(unet, text, abar, num_steps=3, clip=-1.0)
    # clip = 0 and an initial latent: the restated chain without the clamp; nothing is drawn
    noise = Noise("never")
    x_T = _h((2, 8, 27, 27), "stub.init", 2.0).to(DEV)
    keep = x_T.clone()
    out = psg.ddim_sample(unet, text, abar, num_steps=3, clip=0.0, initial_latent=x_T, noise_fn=noise)
    assert noise.asked == [] and torch.equal(x_T, keep)
    ts = G.ddim_timesteps(1000, 3)
    tab = G.ddim_tables(_np(abar).astype(np.float32), ts, 0.0)
    ref = StubUNet().to(DEV)

    def predict(x, t, j):
        with torch.no_grad():
            return _np(ref(torch.from_numpy(x).to(DEV), torch.full((2,), t, device=DEV, dtype=torch.long), text))
    assert R.same_bits(_np(out), G.chain(_np(x_T), predict, tab, ts)[-1])


def test_guided_gradio_chain_is_combine_plus_its_own_update(psg):
    from pokemon_sprite_generator_amd.inference import _f32, _sqrt32
    n, steps, w = 3, 4, 3.0
    unet = StubUNet().to(DEV)
    text, null = _h((n, 4, 16), "gr.text").to(DEV), _h((4, 16), "gr.null").to(DEV)
    noise, trace = Noise("gr"), []
    out = psg.gradio_ddpm_sample(unet, text, steps, noise_fn=noise, trace=trace, guidance_scale=w, null_text=null)
    assert unet.calls and all(b == 2 * n for b, _ in unet.calls) and len(unet.calls) == steps
    # the restated chain: gradio_app.py:343-358's scalars, cfg_combine, sampler_update mode 3
    betas = torch.linspace(0.0001, 0.02, 1000)
    alphas = 1.0 - betas
    acp = torch.cumprod(alphas, dim=0)
    tsteps = torch.linspace(999, 0, steps, dtype=torch.long)
    ref, rn = StubUNet().to(DEV), Noise("gr")
    x = _np(rn(-1, (n, 8, 27, 27)))
    text2 = torch.cat([text, null.unsqueeze(0).expand(n, -1, -1)])
    draws = 0
    one = np.float32(1.0)
    for i, t in enumerate(tsteps):
        xt = torch.from_numpy(x).to(DEV)
        with torch.no_grad():
            o = ref(torch.cat([xt, xt]), torch.full((2 * n,), int(t), device=DEV, dtype=torch.long), text2)
        eps = G.cfg_combine(_np(o[:n]), _np(o[n:]), w)
        a_t, ac_t = _f32(alphas[t]), _f32(acp[t])
        k0, k1 = float((one - a_t) / _sqrt32(one - ac_t)), float(_sqrt32(a_t))
        z, c2, c3 = None, 0.0, 0.0
        if i < steps - 1 and tsteps[i + 1] > 0:
            z = _np(rn(draws, (n, 8, 27, 27)))
            draws += 1
            a_n = _f32(alphas[tsteps[i + 1]])
            c2, c3 = float(_sqrt32(a_n)), float(_sqrt32(one - a_n))
        x = R.sampler_update(x, eps, z, 3, k0, k1, c2, c3)
        assert R.same_bits(_np(trace[i]), x), f"step {i}"
    assert R.same_bits(_np(out), x) and noise.asked == rn.asked
    # ... and without the new arguments the chain is the one it was: one forward at batch n per step
    unet.calls.clear()
    psg.gradio_ddpm_sample(unet, text, steps, noise_fn=Noise("gr"))
    assert [b for b, _ in unet.calls] == [n] * steps


# ------------------------------------------------------------------------------------------------ the full-width U-Net
@pytest.fixture(scope="module")
def wide(psg):
    """One fp32 full-width U-Net with its stepper, text and null text for n = 2."""
    dev = torch.device(DEV, 0)
    torch.manual_seed(0)
    unet = psg.UNet(compute_dtype=torch.float32).to(dev)
    st = psg.DiffusionStepper(unet, psg.NoiseScheduler(), distributed=False)
    text, null = _h((2, 32, 256), "wide.text").to(dev), _h((32, 256), "wide.null").to(dev)
    yield st, text, null
    st.close()


class EpsHook:
    def __init__(self, module):
        self.outs = []
        self.h = module.register_forward_hook(lambda m, a, o: self.outs.append(o.detach().float().cpu().numpy().copy()))

    def close(self):
        self.h.remove()


def test_full_width_guided_ddim_eager_graph_and_restatement(psg, wide):
    st, text, null = wide
    n, k, w = 2, 4, 2.0
    abar = st.noise_scheduler.alphas_cumprod
    ts = G.ddim_timesteps(1000, k)
    tab = G.ddim_tables(_np(abar).astype(np.float32), ts, 0.0)
    # eager, one step at a time: the hooked eps, the restated step, and the two halves of the input buffer
    hook = EpsHook(st.unet)
    run = psg.DdimRun(st.unet, text, abar, num_steps=k, guidance_scale=w, null_text=null, noise_fn=Noise("wide"), use_graph=False)
    eager = []
    x = _np(run.x).copy()
    try:
        assert run.remaining() == k and run.xin.shape[0] == 2 * n
        for j in range(k):
            run.step()
            torch.cuda.synchronize()
            eps = hook.outs[j]
            assert eps.shape[0] == 2 * n and len(hook.outs) == j + 1
            x = G.guided_update(x, eps[:n], eps[n:], None, tab, j, w, 3.0)
            assert R.same_bits(_np(run.x), x), f"step {j}: not the restated update of the eps the U-Net returned"
            assert torch.equal(run.xin[:n], run.xin[n:]), f"step {j}: the unconditional half of the input differs"
            eager.append(run.x.clone())
        assert run.remaining() == 0
        with pytest.raises(StopIteration):
            run.step()
    finally:
        hook.close()
        run.close()
    # the same chain through ddim_sample with a captured step body
    trace = []
    out = psg.ddim_sample(st.unet, text, abar, num_steps=k, guidance_scale=w, null_text=null, noise_fn=Noise("wide"), trace=trace,
                          use_graph=True)
    torch.cuda.synchronize()
    assert len(trace) == k and all(torch.equal(a, b) for a, b in zip(trace, eager)), "graph replays must equal the eager loop on the bits"
    assert torch.equal(out, eager[-1])
    # ... and through the stepper
    got = st.sample(text, n, noise_fn=Noise("wide"), sampler="ddim", num_steps=k, guidance_scale=w, null_text=null)
    assert torch.equal(got, eager[-1])


def test_full_width_guided_ddpm_is_combine_plus_the_existing_update(psg, wide):
    st, text, null = wide
    n, w, steps = 2, 1.5, 3
    c1, c2, sg = (_np(t) for t in st.noise_scheduler.step_tables(st.device))
    hook, trace, noise = EpsHook(st.unet), [], Noise("ddpm")
    try:
        st.sample(text, n, fast_sampling=True, noise_fn=noise, trace=trace, max_steps=steps, guidance_scale=w, null_text=null, use_graph=False)
        torch.cuda.synchronize()
    finally:
        hook.close()
    order = list(reversed(range(0, 1000, 50)))[:steps]
    rn = Noise("ddpm")
    x = _np(rn(-1, (n, 8, 27, 27)))
    assert len(hook.outs) == steps and len(trace) == steps
    for i, t in enumerate(order):
        eps = G.cfg_combine(hook.outs[i][:n], hook.outs[i][n:], w)
        x = R.ddpm_update(x, eps, _np(rn(i, (n, 8, 27, 27))), c1, c2, sg, t)
        assert R.same_bits(_np(trace[i]), x), f"step {i}"


def test_default_sample_is_the_sampler_run(psg, wide):
    """DiffusionStepper.sample() with default arguments against SamplerRun driven directly: the same bits, and the same class."""
    from pokemon_sprite_generator_amd.trainer import SamplerRun
    st, text, _ = wide
    got, trace = None, []
    got = st.sample(text, 2, noise_fn=Noise("plain"), trace=trace, max_steps=3)
    assert type(st.sampler(text, 2, noise_fn=Noise("plain"), max_steps=3)) is SamplerRun
    run = SamplerRun(st, text, 2, True, Noise("plain"), 8, 27, None, 3)
    for j in range(3):
        run.step()
        assert torch.equal(run.x, trace[j])
    assert torch.equal(run.x, got)
    with pytest.raises(ValueError):
        st.sample(text, 2, sampler="euler")
    with pytest.raises(ValueError, match="null_text"):
        st.sample(text, 2, guidance_scale=2.0)
