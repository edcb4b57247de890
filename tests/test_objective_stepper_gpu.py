"""-m gpu: v-prediction and Min-SNR weighting in DiffusionStepper (prediction_type=, min_snr_gamma=; one psg_diffusion_loss_f32
launch in psg_smooth_l1_f32's place) and the trainer keys around them, on the full-width bf16 U-Net at batch 8 (built as
tests/test_ema_stepper_gpu.py builds it; its helpers and the stubs of tests/test_trainer_gpu.py are imported).  Steps are
compared on the bits; the loss value against the fp64 reference of tests/objective_ref.py within its derived bound."""
import numpy as np
import pytest
import torch

from tests import objective_ref as O
from tests import step_ref as R
from tests.test_ema_stepper_gpu import TODAY_KEYS, _batches, _same, _stepper, _unet
from tests.test_text_drop_gpu import _state, _trainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, GAMMA = 8, 5.0
V = dict(prediction_type="v_prediction", min_snr_gamma=GAMMA)


@pytest.fixture(scope="module")
def psg():
    import pokemon_sprite_generator_amd as m
    from pokemon_sprite_generator_amd import _lib
    _lib.init(0)
    return m


@pytest.fixture(scope="module")
def no_dropout():
    """Dropout seeds are drawn per call: off, so that twin steppers see the same masks (none)."""
    import pokemon_sprite_generator_amd.unet as U
    old, U.ATTN_DROPOUT = U.ATTN_DROPOUT, 0.0
    yield
    U.ATTN_DROPOUT = old


def _t_batch(seed):
    """One batch whose timesteps lie on both sides of the gamma = 5 truncation (t <= 260) and at both ends."""
    lat, txt, t, nz = _batches(1, B=B, seed=seed)[0]
    t = torch.tensor([0, 260, 261, 999, 999, 500, 17, 261], device=DEV)
    return 2.0 * lat, txt, t, nz                                    # (N(0, 2^2) latents: the clamp to +-3 acts)


def test_options_off_is_the_stepper_of_today(psg, no_dropout):
    """prediction_type="epsilon", min_snr_gamma=None: the psg_smooth_l1_f32 call of a stepper built without the arguments - loss,
    gradient norm, masters, moments, shadow and the seed stream, bit for bit over two steps."""
    import pokemon_sprite_generator_amd.unet as U
    batches = _batches(2, B=B, seed=11)
    rec = {}
    for name, kw in (("plain", {}), ("off", dict(prediction_type="epsilon", min_snr_gamma=None))):
        st = _stepper(psg, **kw)
        assert not st.objective_enabled and st.loss_weights is None and st.prediction_type == "epsilon"
        outs, counts = [], []
        for lat, txt, t, nz in batches:
            c0 = U._SeedStream.counter
            o = st.train_step(lat, txt, t, noise=nz)
            counts.append(U._SeedStream.counter - c0)
            outs.append((o["loss"].clone(), o["grad_norm"].clone(), int(o["nan_flag"].item())))
        ev = st.eval_loss(*batches[0][:3], noise=batches[0][3])[0].clone()
        rec[name] = (outs, counts, _state(st), ev, st.steps_done())
        st.close()
    a, b = rec["plain"], rec["off"]
    assert a[4] == b[4] == 2 and a[1] == b[1], "the seed stream moved"
    for (la, ga, fa), (lb, gb, fb) in zip(a[0], b[0]):
        assert fa == fb == 0 and _same(la, lb) and _same(ga, gb)
    for k, v in a[2].items():
        assert _same(b[2][k], v), f"{k} differs from a stepper built without the arguments"
    assert _same(a[3], b[3])
    with pytest.raises(ValueError):
        psg.DiffusionStepper(None, psg.NoiseScheduler(), prediction_type="x0")


@pytest.fixture(scope="module")
def v_twins(psg, no_dropout):
    """`st`: a v-prediction + Min-SNR stepper; `tw`: a twin from the same seeds built WITHOUT the arguments, whose step the tests
    assemble from the public pieces."""
    st, tw = _stepper(psg, **V), _stepper(psg)
    assert _same(st.params.flat, tw.params.flat) and st.objective_enabled and not tw.objective_enabled
    yield st, tw
    st.close()
    tw.close()


def _tables(st):
    s = st.noise_scheduler
    return tuple(getattr(s, n).cpu().numpy().astype(np.float32) for n in ("alphas_cumprod", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"))


def test_eval_loss_is_the_weighted_v_loss_of_the_forward(psg, v_twins):
    st, _ = v_twins
    lat, txt, t, nz = _t_batch(21)
    abar, tabA, tabB = _tables(st)
    wtab = O.min_snr_weights(abar, GAMMA, O.PRED_V)
    assert R.same_bits(st.loss_weights.cpu(), wtab) and st.loss_weights.is_cuda
    loss, flag = st.eval_loss(lat, txt, t, noise=nz)
    assert int(flag.item()) == 0
    # the forward the test runs itself (eval mode: no dropout; the kernels are deterministic)
    with torch.no_grad():
        st.unet.eval()
        noisy = st.noise_scheduler.add_noise(lat, nz, t, clamp=True)
        pred = st.unet(noisy, t, txt).float()
    flat = lambda v: v.detach().float().cpu().numpy().reshape(B, -1)             # noqa: E731
    ref = O.diffusion_loss(flat(pred), flat(lat), flat(nz), t.cpu().numpy(), tabA, tabB, wtab, O.PRED_V, 0.1, 1.0, 1, vec=True)
    r = torch.as_tensor(ref["loss"], dtype=torch.float64).reshape(1)
    ratio = R.check(loss.reshape(1), r, r.abs(), torch.float32, "eval_loss v + min-snr", ref["depth_loss"], extra=ref["extra_loss"])
    print(f"RATIO eval_loss v + min-snr {ratio:.3g} (loss {float(loss):.6g})")
    # not the uniform eps loss, and not the unweighted v loss
    plain = O.diffusion_loss(flat(pred), flat(lat), flat(nz), t.cpu().numpy(), tabA, tabB, None, O.PRED_V, 0.1, 1.0, 1, vec=True)
    assert float(plain["loss"]) > 1.5 * float(loss)                 # (every weight is < 1, most of this batch's far below)
    # the public wrapper gives the same bits, and v_target the kernel's target
    from pokemon_sprite_generator_amd import objective
    l2, g2 = objective.diffusion_loss(pred, lat, nz, t, st.noise_scheduler, "v_prediction", st.loss_weights, 0.1, True, want_grad=False)
    assert g2 is None and _same(l2, loss)
    tg = objective.v_target(lat, nz, t, st.noise_scheduler, clamp=True)
    assert R.same_bits(tg.cpu().numpy().reshape(B, -1), O.v_target(flat(lat), flat(nz), t.cpu().numpy(), tabA, tabB, 1))


def test_train_step_is_the_step_assembled_from_the_public_pieces(psg, v_twins):
    from pokemon_sprite_generator_amd import objective
    st, tw = v_twins
    assert _same(st.params.flat, tw.params.flat)
    lat, txt, t, nz = _t_batch(22)
    out = st.train_step(lat, txt, t, noise=nz)
    # the twin: add_noise, forward, objective.diffusion_loss, backward, the optimizer step
    tw.unet.train()
    tw.flag.zero_()
    noisy = tw.noise_scheduler.add_noise(lat, nz, t, clamp=True, flag=tw.flag)
    tw.arena.zero()
    pred = tw.unet(noisy, t, txt)
    wtab = psg.min_snr_weights(tw.noise_scheduler.alphas_cumprod, GAMMA, "v_prediction").to(DEV)
    loss, dpred = objective.diffusion_loss(pred, lat, nz, t, tw.noise_scheduler, "v_prediction", wtab, 0.1, True, True, tw.flag)
    pred.backward(dpred)
    tw.arena.finalize()
    normsq = tw.arena.grad_norm_sq()
    tw.optimizer.step(normsq=normsq, max_norm=tw.max_grad_norm, skip_flag=tw.flag)
    torch.cuda.synchronize()
    assert int(out["nan_flag"].item()) == 0 and int(tw.flag.item()) == 0
    assert _same(out["loss"], loss) and _same(out["grad_norm"], normsq.sqrt())
    assert float(out["loss"]) > 0 and float(out["grad_norm"]) > 0
    a, b = _state(st), _state(tw)
    for k in a:
        assert _same(a[k], b[k]), f"{k} differs from the step assembled from the public pieces"
    assert st.steps_done() == tw.steps_done()


def test_graphed_v_step_equals_the_eager_twin(psg):
    """capture_train_step with the objective on: 2 warm-up steps and 2 replays against a twin's 4 eager steps under the same
    SeedSource mode, masters bit for bit - the weight table and t live on the device, the graph holds nothing new."""
    from pokemon_sprite_generator_amd import ops
    lat, txt, t, _ = _t_batch(3)
    try:
        word = ops.SeedSource.enable(torch.device(DEV, 0))
        word.zero_()
        a = _stepper(psg, **V)
        torch.manual_seed(5)
        losses = []
        for _ in range(4):
            losses.append(a.train_step(lat, txt, t)["loss"].clone())
        torch.cuda.synchronize()
        pa, wa = a.params.flat.clone(), int(word.item())
        a.close()
        del a
        word.zero_()
        b = _stepper(psg, **V)
        torch.manual_seed(5)
        gs = b.capture_train_step(lat, txt, t, warmup=2)
        got = []
        for _ in range(2):
            got.append(gs.run(lat, txt, t)["loss"].clone())
        torch.cuda.synchronize()
        assert b.steps_done() == 4 and int(word.item()) == wa
        assert _same(b.params.flat, pa), "graph replays must take the eager steps bit for bit"
        assert _same(got[0], losses[2]) and _same(got[1], losses[3])
        b.close()
    finally:
        ops.SeedSource.disable()


@pytest.fixture(scope="module")
def gpu_init(psg):
    from pokemon_sprite_generator_amd import trainer as trainer_mod
    mp = pytest.MonkeyPatch()
    mp.setattr(trainer_mod, "UNet", lambda *a, **k: _unet(psg, *a, **k))
    yield
    mp.undo()


def test_trainer_keys_checkpoint_keys_and_the_mismatch_error(psg, gpu_init, no_dropout, tmp_path, monkeypatch):
    torch.manual_seed(0)
    tr = _trainer(psg, tmp_path, "v", prediction_type="v_prediction", min_snr_gamma=GAMMA)
    assert tr.prediction_type == "v_prediction" and tr.min_snr_gamma == GAMMA
    assert tr.stepper.prediction_type == "v_prediction" and tr.stepper.min_snr_gamma == GAMMA and tr.stepper.objective_enabled
    lat, txt, t, nz = _t_batch(31)
    out = tr.train_step(lat, txt, t, noise=nz)
    assert int(out["nan_flag"].item()) == 0 and tr.optimizer.steps_done() == 1
    saved = {}
    monkeypatch.setattr(torch, "save", lambda obj, path: saved.update(obj))
    tr.save_checkpoint(0, is_best=True)
    assert set(saved) == TODAY_KEYS | {"prediction_type", "min_snr_gamma"}
    assert saved["prediction_type"] == "v_prediction" and saved["min_snr_gamma"] == GAMMA
    v_ckpt = dict(saved)
    # a trainer without the keys: today's checkpoint, and it refuses the v checkpoint before it loads anything
    tr.stepper.close()
    torch.manual_seed(0)
    te = _trainer(psg, tmp_path, "e", min_snr_gamma=0)
    assert te.prediction_type == "epsilon" and te.min_snr_gamma is None and not te.stepper.objective_enabled
    saved.clear()
    te.save_checkpoint(0, is_best=True)
    assert set(saved) == TODAY_KEYS
    before = te.stepper.params.flat.clone()
    monkeypatch.setattr(torch, "load", lambda path, **k: v_ckpt)
    with pytest.raises(psg.PsgError, match="prediction_type"):
        te.load_checkpoint("v.pth")
    assert _same(te.stepper.params.flat, before)
    te.stepper.close()
