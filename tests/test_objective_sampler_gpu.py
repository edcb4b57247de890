"""-m gpu: the samplers on a v-predicting U-Net (prediction="v_prediction": guidance.ddim_sample / DdimRun,
DiffusionStepper.sample, inference.gradio_ddpm_sample) against the restatements of tests/objective_ref.py, on the bits: the
U-Net - a stub, or the full-width one - supplies v, and everything the samplers do with it is restated in numpy float32.  The
stub, the noise source and the output hook are tests/test_guided_sampler_gpu.py's."""
import math

import numpy as np
import pytest
import torch

from tests import guided_ref as G
from tests import objective_ref as O
from tests import step_ref as R
from tests.test_guided_sampler_gpu import EpsHook, Noise, StubUNet, _h, _np

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


@pytest.fixture(scope="module")
def psg():
    import pokemon_sprite_generator_amd as m
    from pokemon_sprite_generator_amd import _lib
    _lib.init(0)
    return m


class OracleV(torch.nn.Module):
    """v_t = sqrt(abar_t) e - sqrt(1 - abar_t) x0 of a fixed (x0, e), whatever x is: fp64 on the host, one rounding to fp32."""

    def __init__(self, abar, x0, e):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))
        self.abar, self.x0, self.e = abar, x0, e

    def forward(self, x, t, text):
        a = float(self.abar[int(t[0].item())])
        v = (math.sqrt(a) * self.e - math.sqrt(1 - a) * self.x0).astype(np.float32)
        return torch.from_numpy(v).to(x.device).reshape(x.shape)


@pytest.mark.parametrize("k", [1, 5, 20])
def test_ddim_on_the_oracle_v_recovers_x0(psg, k):
    """The eta = 0, clip = 0 chain ends at x0 within the first-order bound of the CPU suite (objective_ref.v_recovery_bound)."""
    n = 1
    abar = _np(psg.NoiseScheduler().alphas_cumprod).astype(np.float32)
    rng = np.random.default_rng(0)
    x0, e = rng.uniform(-2.5, 2.5, n * 5832), rng.standard_normal(n * 5832)
    ts = G.ddim_timesteps(1000, k)
    a = float(abar[ts[0]])
    x_T = torch.from_numpy((math.sqrt(a) * x0 + math.sqrt(1 - a) * e).astype(np.float32)).reshape(n, 8, 27, 27).to(DEV)
    unet = OracleV(abar, x0, e).to(DEV)
    out = psg.ddim_sample(unet, torch.zeros(n, 4, 16, device=DEV), torch.from_numpy(abar), num_steps=k, clip=0.0, initial_latent=x_T,
                          prediction="v_prediction")
    bound = O.v_recovery_bound(abar, ts, x0, e, U)
    err = np.abs(_np(out).astype(np.float64).reshape(-1) - x0)
    print(f"V RECOVERY gpu k={k}: max abs error {err.max():.3g}, worst err / bound {(err / bound).max():.3g}")
    assert bool((err <= bound).all())
    # ... and it is the restated chain on the bits
    want = O.chain(_np(x_T).reshape(-1), O.oracle_v(abar, x0, e, np.float32), G.ddim_tables(abar, ts, 0.0), ts, O.PRED_V)[-1]
    assert R.same_bits(_np(out).reshape(-1), want)


def _restated_ddim(unet, text, null, abar, k, eta, w, clip, noise, prediction):
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
    return O.chain(x_T, predict, tab, ts, prediction, w=w, clip=clip, eta=eta, noise=lambda i: _np(noise(i, (n, 8, 27, 27))))


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("eta", [0.0, 0.7])
@pytest.mark.parametrize("w", [None, 2.5], ids=["unguided", "guided"])
def test_v_ddim_on_a_stub_equals_the_restated_chain(psg, w, eta, use_graph):
    """The stub's output read as v: the chain is the restated v chain, and differs from the eps chain on the same stub."""
    n, k = 3, 5
    unet = StubUNet().to(DEV)
    text, null = _h((n, 4, 16), "stub.text").to(DEV), _h((4, 16), "stub.null").to(DEV)
    abar = _np(psg.NoiseScheduler().alphas_cumprod).astype(np.float32)
    noise, trace = Noise("stub"), []
    out = psg.ddim_sample(unet, text, torch.from_numpy(abar), num_steps=k, eta=eta, guidance_scale=w, null_text=null if w is not None else None,
                          noise_fn=noise, trace=trace, use_graph=use_graph, prediction="v_prediction")
    torch.cuda.synchronize()
    assert noise.asked == ([-1] if eta == 0 else [-1, 0, 1, 2, 3])
    want = _restated_ddim(StubUNet().to(DEV), text, null, abar, k, eta, w, 3.0, Noise("stub"), O.PRED_V)
    assert len(trace) == k
    for j in range(k):
        assert R.same_bits(_np(trace[j]), want[j]), f"step {j}"
    assert R.same_bits(_np(out), want[-1])
    eps_chain = _restated_ddim(StubUNet().to(DEV), text, null, abar, k, eta, w, 3.0, Noise("stub"), O.PRED_EPS)
    assert not R.same_bits(want[0], eps_chain[0])
    if not use_graph and eta == 0:                                  # prediction="epsilon" spelled out is the chain of today
        got = psg.ddim_sample(StubUNet().to(DEV), text, torch.from_numpy(abar), num_steps=k, guidance_scale=w,
                              null_text=null if w is not None else None, noise_fn=Noise("stub"), prediction="epsilon")
        assert R.same_bits(_np(got), eps_chain[-1])
    with pytest.raises(ValueError):
        psg.ddim_sample(unet, text, torch.from_numpy(abar), num_steps=k, prediction="x0")


@pytest.mark.parametrize("w", [None, 3.0], ids=["unguided", "guided"])
def test_v_gradio_chain_is_pred_to_eps_plus_its_own_update(psg, w):
    from pokemon_sprite_generator_amd.inference import _f32, _sqrt32
    n, steps = 3, 4
    unet = StubUNet().to(DEV)
    text, null = _h((n, 4, 16), "gr.text").to(DEV), _h((4, 16), "gr.null").to(DEV)
    noise, trace = Noise("gr"), []
    kw = {} if w is None else dict(guidance_scale=w, null_text=null)
    out = psg.gradio_ddpm_sample(unet, text, steps, noise_fn=noise, trace=trace, prediction="v_prediction", **kw)
    nb = n if w is None else 2 * n
    assert len(unet.calls) == steps and all(b == nb for b, _ in unet.calls)
    betas = torch.linspace(0.0001, 0.02, 1000)
    alphas = 1.0 - betas
    acp = torch.cumprod(alphas, dim=0)
    tabA, tabB = (np.sqrt(acp.double().numpy()).astype(np.float32), np.sqrt(1.0 - acp.double().numpy()).astype(np.float32))
    tsteps = torch.linspace(999, 0, steps, dtype=torch.long)
    ref, rn = StubUNet().to(DEV), Noise("gr")
    x = _np(rn(-1, (n, 8, 27, 27)))
    text2 = torch.cat([text, null.unsqueeze(0).expand(n, -1, -1)]) if w is not None else text
    draws = 0
    one = np.float32(1.0)
    for i, t in enumerate(tsteps):
        xt = torch.from_numpy(x).to(DEV)
        with torch.no_grad():
            o = ref(torch.cat([xt, xt]) if w is not None else xt, torch.full((nb,), int(t), device=DEV, dtype=torch.long), text2)
        eps = O.pred_to_eps(x, _np(o[:n]), _np(o[n:]) if w is not None else None, 0.0 if w is None else w, tabA, tabB, int(t), O.PRED_V)
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


# ------------------------------------------------------------------------------------------------ the full-width U-Net
@pytest.fixture(scope="module")
def wide(psg):
    """One fp32 full-width U-Net with a v-prediction stepper, text and null text for n = 2."""
    dev = torch.device(DEV, 0)
    torch.manual_seed(0)
    unet = psg.UNet(compute_dtype=torch.float32).to(dev)
    st = psg.DiffusionStepper(unet, psg.NoiseScheduler(), distributed=False, prediction_type="v_prediction")
    text, null = _h((2, 32, 256), "wide.text").to(dev), _h((32, 256), "wide.null").to(dev)
    yield st, text, null
    st.close()


def test_full_width_guided_v_ddim_eager_graph_and_restatement(psg, wide):
    st, text, null = wide
    n, k, w = 2, 4, 2.0
    abar = st.noise_scheduler.alphas_cumprod
    ts = G.ddim_timesteps(1000, k)
    tab = G.ddim_tables(_np(abar).astype(np.float32), ts, 0.0)
    hook = EpsHook(st.unet)
    run = st.sampler(text, n, noise_fn=Noise("wide"), sampler="ddim", num_steps=k, guidance_scale=w, null_text=null, use_graph=False)
    assert type(run) is psg.DdimRun and run.prediction == O.PRED_V, "the stepper's own prediction type is the default"
    eager = []
    x = _np(run.x).copy()
    try:
        for j in range(k):
            run.step()
            torch.cuda.synchronize()
            v = hook.outs[j]
            assert v.shape[0] == 2 * n and len(hook.outs) == j + 1
            x = O.guided_update_pred(x, v[:n], v[n:], None, tab, j, w, 3.0, O.PRED_V)
            assert R.same_bits(_np(run.x), x), f"step {j}: not the restated v update of what the U-Net returned"
            assert torch.equal(run.xin[:n], run.xin[n:]), f"step {j}: the unconditional half of the input differs"
            eager.append(run.x.clone())
    finally:
        hook.close()
        run.close()
    trace = []
    out = psg.ddim_sample(st.unet, text, abar, num_steps=k, guidance_scale=w, null_text=null, noise_fn=Noise("wide"), trace=trace,
                          use_graph=True, prediction="v_prediction")
    torch.cuda.synchronize()
    assert len(trace) == k and all(torch.equal(a, b) for a, b in zip(trace, eager)), "graph replays must equal the eager loop on the bits"
    assert torch.equal(out, eager[-1])
    got = st.sample(text, n, noise_fn=Noise("wide"), sampler="ddim", num_steps=k, guidance_scale=w, null_text=null)
    assert torch.equal(got, eager[-1])


@pytest.mark.parametrize("w", [None, 1.5], ids=["unguided", "guided"])
def test_full_width_v_ddpm_is_pred_to_eps_plus_the_existing_update(psg, wide, w):
    st, text, null = wide
    n, steps = 2, 3
    c1, c2, sg = (_np(t) for t in st.noise_scheduler.step_tables(st.device))
    tabA, tabB = _np(st.noise_scheduler.sqrt_alphas_cumprod), _np(st.noise_scheduler.sqrt_one_minus_alphas_cumprod)
    hook, trace, noise = EpsHook(st.unet), [], Noise("ddpm")
    kw = {} if w is None else dict(guidance_scale=w, null_text=null)
    try:
        st.sample(text, n, fast_sampling=True, noise_fn=noise, trace=trace, max_steps=steps, use_graph=False, **kw)
        torch.cuda.synchronize()
    finally:
        hook.close()
    order = list(reversed(range(0, 1000, 50)))[:steps]
    rn = Noise("ddpm")
    x = _np(rn(-1, (n, 8, 27, 27)))
    assert len(hook.outs) == steps and len(trace) == steps
    for i, t in enumerate(order):
        o = hook.outs[i]
        assert o.shape[0] == (n if w is None else 2 * n)
        eps = O.pred_to_eps(x, o[:n], o[n:] if w is not None else None, 0.0 if w is None else w, tabA, tabB, t, O.PRED_V)
        x = R.ddpm_update(x, eps, _np(rn(i, (n, 8, 27, 27))), c1, c2, sg, t)
        assert R.same_bits(_np(trace[i]), x), f"step {i}"
    # prediction="epsilon" on the same stepper: the chain of a stepper built without the argument (today's launches)
    t2 = []
    st.sample(text, n, noise_fn=Noise("ddpm"), trace=t2, max_steps=1, use_graph=False, prediction="epsilon", **kw)
    o = hook.outs[0]
    eps = G.cfg_combine(o[:n], o[n:], w) if w is not None else o
    rn = Noise("ddpm")
    x = R.ddpm_update(_np(rn(-1, (n, 8, 27, 27))), eps, _np(rn(0, (n, 8, 27, 27))), c1, c2, sg, order[0])
    assert R.same_bits(_np(t2[0]), x)


# ------------------------------------------------------------------------------------------------ checkpoint consumers
def test_latent_generator_refuses_a_v_checkpoint(psg):
    from pokemon_sprite_generator_amd import inference
    ckpt = {"unet_state_dict": {}, "prediction_type": "v_prediction"}
    state, pred = inference.load_unet_checkpoint(ckpt)
    assert pred == "v_prediction" and inference.checkpoint_prediction_type({"unet_state_dict": {}}) == "epsilon"
    unet = StubUNet().to(DEV)
    with pytest.raises(psg.PsgError, match="v_prediction"):
        psg.LatentGenerator(unet, prediction=pred)
    gen = psg.LatentGenerator(unet, prediction=inference.checkpoint_prediction_type({"unet_state_dict": {}}))      # eps: as before
    assert gen.unet is unet
    with pytest.raises(psg.PsgError, match="stage 3"):
        inference.refuse_v_prediction("v_prediction", "FinalPokemonGenerator.from_checkpoints")


def test_sprite_generator_reads_the_checkpoint_key(psg, tmp_path, monkeypatch):
    """from_checkpoints hands the checkpoint's prediction type to the generator, whose samplers then take prediction=."""
    from pokemon_sprite_generator_amd import generate
    seen = {}

    class _Stop(Exception):
        pass

    def fake_load(path, use_ema=False, **kw):
        return {}, "v_prediction"

    def fake_torch_load(path, **kw):
        raise _Stop()
    monkeypatch.setattr(generate, "load_unet_checkpoint", fake_load)
    monkeypatch.setattr(torch, "load", fake_torch_load)
    with pytest.raises(_Stop):                                     # (the key is read first; the test stops before anything is built)
        psg.SpriteGenerator.from_checkpoints("vae.pth", "unet.pth", {})
    monkeypatch.undo()
    # the constructor argument from_checkpoints passes, and what the two samplers receive
    class _VAE(torch.nn.Module):
        latent_dim = 8
    gen = psg.SpriteGenerator(_VAE(), StubUNet().to(DEV), torch.nn.Identity(), prediction="v_prediction")
    assert gen.prediction_type == "v_prediction" and psg.SpriteGenerator(_VAE(), StubUNet().to(DEV), torch.nn.Identity()).prediction_type == "epsilon"
    monkeypatch.setattr(generate, "gradio_ddpm_sample", lambda *a, **k: seen.update(gradio=k))
    monkeypatch.setattr(generate, "ddim_sample", lambda *a, **k: seen.update(ddim=k))
    text = _h((2, 4, 16), "gen.text").to(DEV)
    gen._sample(text, 3, None, None)
    gen._sample(text, 3, None, None, sampler="ddim")
    assert seen["gradio"]["prediction"] == "v_prediction" and seen["ddim"]["prediction"] == "v_prediction"
    # ... and end to end on the stub: the generator's gradio chain is gradio_ddpm_sample(prediction="v_prediction")
    monkeypatch.undo()
    a = gen._sample(text, 3, None, Noise("gen"))
    b = psg.gradio_ddpm_sample(StubUNet().to(DEV), text, 3, noise_fn=Noise("gen"), prediction="v_prediction")
    c = psg.gradio_ddpm_sample(StubUNet().to(DEV), text, 3, noise_fn=Noise("gen"))
    assert torch.equal(a, b) and not torch.equal(a, c)
