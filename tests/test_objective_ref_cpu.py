"""-m "not gpu": the host side of objective.py (min_snr_weights) and the references of tests/objective_ref.py - the weight tables
against their definition, the v algebra and the oracle-v DDIM chain against bounds derived from the roundings of the tables and
of the operations, every planted mistake of objective_ref.MISTAKES shown to break the bound it bears on, and the refusals of the
three C entries (rejected on the host before any launch, so they run without a GPU)."""
import math
import os

import numpy as np
import pytest
import torch

from tests import objective_ref as O
from tests import step_ref as R
from tests.gemm_ref import A_FLOOR, F32_ROUND

U = 2.0 ** -24
U64 = 2.0 ** -53
T = 1000
GAMMA = 5.0


@pytest.fixture(scope="module")
def psg():
    import pokemon_sprite_generator_amd as m
    return m


@pytest.fixture(scope="module")
def schedules(psg):
    """name -> (abar, sqrt(abar), sqrt(1 - abar)) fp32 [1000] numpy: stage 2's cosine-clipped schedule with NoiseScheduler's own
    tables, and the linear one of stage 3 / the demo."""
    out = {}
    for name, s in (("cosine", psg.NoiseScheduler()), ("linear", psg.LinearNoiseScheduler())):
        out[name] = tuple(getattr(s, n).cpu().numpy().astype(np.float32) for n in ("alphas_cumprod", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"))
    return out


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------------- weight tables
@pytest.mark.parametrize("gamma", [GAMMA, 1.0, 20.0])
@pytest.mark.parametrize("name", ["cosine", "linear"])
def test_weights_are_their_definition_to_one_rounding(psg, schedules, name, gamma):
    """w_eps snr == min(snr, gamma) and w_v (snr + 1) == min(snr, gamma): the table is ONE fp32 rounding (2^-24 relative) of
    the fp64 value; the fp64 evaluation itself (snr, the product) adds a few 2^-53: 8 of them are allowed."""
    abar = schedules[name][0]
    snr = O.snr64(abar)
    want = np.minimum(snr, gamma)
    for pred, code, denom in (("epsilon", O.PRED_EPS, snr), ("v_prediction", O.PRED_V, snr + 1.0)):
        w = psg.min_snr_weights(torch.from_numpy(abar), gamma, pred)
        assert w.dtype == torch.float32 and tuple(w.shape) == (T,) and not w.is_cuda
        assert bool(torch.isfinite(w).all()) and float(w.min()) >= 0.0 and float(w.max()) <= 1.0
        assert R.same_bits(w, O.min_snr_weights(abar, gamma, code)), f"{name} {pred}: not the restated table"
        rel = np.abs(w.numpy().astype(np.float64) * denom - want) / want
        print(f"WEIGHTS {name} gamma={gamma} {pred}: worst relative error {rel.max():.3g} (one rounding: {U:.3g})")
        assert float(rel.max()) <= U + 8 * U64
    # the planted mistake: the eps formula in the v table misses by a factor (snr + 1) / snr
    bad = O.min_snr_weights(abar, gamma, O.PRED_V, mistake="eps_weight_for_v").astype(np.float64)
    assert float((np.abs(bad * (snr + 1.0) - want) / want).max()) > 1e3 * U


def test_gamma_5_truncates_exactly_t_up_to_260_of_stage2(psg, schedules):
    abar = schedules["cosine"][0]
    snr = O.snr64(abar)
    assert abs(snr[0] - 9997.34) < 0.01 and abs(snr[-1] - 0.0032) < 1e-4
    w = psg.min_snr_weights(torch.from_numpy(abar), GAMMA, "epsilon").numpy()
    cut = np.nonzero(w < 1.0)[0]
    assert cut.tolist() == list(range(261)) and bool((w[261:] == 1.0).all())
    wv = psg.min_snr_weights(torch.from_numpy(abar), GAMMA, "v_prediction").numpy()
    assert R.same_bits(wv[261:], abar[261:])                       # untruncated: snr / (snr + 1) = abar, exactly
    assert bool((wv[:261] < abar[:261]).all())


def test_weight_limits_and_refusals(psg):
    """abar = 1: both 0.  abar = 0: eps 1, v 0.  Values outside [0, 1] are clipped first.  No NaN anywhere."""
    ends = torch.tensor([1.0, 0.0, 0.5, 1.5, -0.25], dtype=torch.float32)
    assert psg.min_snr_weights(ends, GAMMA, "epsilon").tolist() == [0.0, 1.0, 1.0, 0.0, 1.0]
    assert psg.min_snr_weights(ends, GAMMA, "v_prediction").tolist() == [0.0, 0.0, 0.5, 0.0, 0.0]
    assert psg.min_snr_weights(ends, 0.5, "epsilon").tolist() == [0.0, 1.0, 0.5, 0.0, 1.0]
    for g in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            psg.min_snr_weights(ends, g, "epsilon")
    with pytest.raises(ValueError):
        psg.min_snr_weights(ends, GAMMA, "x0")
    with pytest.raises(ValueError):
        psg.min_snr_weights(torch.tensor([float("nan")]), GAMMA)


# -------------------------------------------------------------------------------------------------------------- algebra
def _x0_e(seed=0, n=8 * 27 * 27):
    rng = np.random.default_rng(seed)
    return rng.uniform(-2.5, 2.5, n).astype(np.float32), rng.standard_normal(n).astype(np.float32)


@pytest.mark.parametrize("name", ["cosine", "linear"])
def test_v_algebra_recovers_x0_and_eps(schedules, name):
    """x_t = A x0 + B eps (noise_add) and v = A eps - B x0 (v_target), then x0' = A x_t - B v = (A^2 + B^2) x0 and
    eps' = B x_t + A v = (A^2 + B^2) eps (pred_to_eps).  D = max |A^2 + B^2 - 1| of the fp32 tables; every one of the four
    values built is two products and a sum, each moving it by at most 2 2^-24 (|x0| + |eps|) (A, B <= 1), and the second pair
    carries the first pair's error on with weights A + B <= sqrt(2): 2 + 2 sqrt(2) 2 < 8.
    bound = D |value| + 8 2^-24 (|x0| + |eps|).  The sign and the swap mistakes break it."""
    abar, tabA, tabB = schedules[name]
    D = float(np.abs(tabA.astype(np.float64) ** 2 + tabB.astype(np.float64) ** 2 - 1.0).max())
    print(f"TABLES {name}: max |A^2 + B^2 - 1| = {D:.3g}")
    assert D < 4 * U * 2                                        # two squares of values rounded to fp32
    x0, e = _x0_e()
    n = x0.size
    worst = 0.0
    for t in (0, 1, 260, 261, 500, 998, 999):
        tt = np.array([t])
        xt, _ = R.noise_add(x0[None], e[None], tt, tabA, tabB, 0)
        v = O.v_target(x0[None], e[None], tt, tabA, tabB, 0)
        x0r = O.guided_update_pred(xt[0], v[0], None, None, np.array([[tabA[t]], [tabB[t]], [1.0], [0.0], [0.0]], dtype=np.float32), 0, 0.0, 0.0, O.PRED_V)
        er = O.pred_to_eps(xt[0], v[0], None, 0.0, tabA, tabB, t, O.PRED_V)
        slack = 8 * U * (np.abs(x0.astype(np.float64)) + np.abs(e.astype(np.float64)))
        for got, ref in ((x0r, x0), (er, e)):
            bound = D * np.abs(ref.astype(np.float64)) + slack
            err = np.abs(got.astype(np.float64) - ref)
            worst = max(worst, float((err / bound).max()))
            assert bool((err <= bound).all()), f"{name} t={t}"
        for mistake in ("v_sign", "ab_swapped"):
            vb = O.v_target(x0[None], e[None], tt, tabA, tabB, 0, mistake=mistake)
            eb = O.pred_to_eps(xt[0], vb[0], None, 0.0, tabA, tabB, t, O.PRED_V)
            assert float((np.abs(eb.astype(np.float64) - e) / (D * np.abs(e) + slack)).max()) > 10.0, f"{mistake} in the target, t={t}"
            eb = O.pred_to_eps(xt[0], v[0], None, 0.0, tabA, tabB, t, O.PRED_V, mistake=mistake)
            assert float((np.abs(eb.astype(np.float64) - e) / (D * np.abs(e) + slack)).max()) > 10.0, f"{mistake} in pred_to_eps, t={t}"
    print(f"ALGEBRA {name}: worst err / bound {worst:.3g} over {n} elements and 7 timesteps")


def test_eps_mode_is_the_eps_kernel_and_the_combine(schedules):
    """PRED_EPS: guided_update_pred is guided_ref.guided_update, pred_to_eps is the combine (or the prediction itself)."""
    from tests import guided_ref as G
    abar = schedules["cosine"][0]
    tab = G.ddim_tables(abar, G.ddim_timesteps(T, 7), 0.7)
    x0, e = _x0_e(3, 1001)
    u, z = _x0_e(4, 1001)
    for j in (0, 3, 6):
        want = G.guided_update(x0, e, u, z, tab, j, 2.5, 3.0)
        assert R.same_bits(O.guided_update_pred(x0, e, u, z, tab, j, 2.5, 3.0, O.PRED_EPS), want)
    assert R.same_bits(O.pred_to_eps(None, e, u, 2.5, None, None, 5, O.PRED_EPS), G.cfg_combine(e, u, 2.5))
    assert R.same_bits(O.pred_to_eps(None, e, None, 2.5, None, None, 5, O.PRED_EPS), e)


# ------------------------------------------------------------------------------------------------------ oracle-v chain
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("k", (1, 5, 20))
@pytest.mark.parametrize("name", ["cosine", "linear"])
def test_oracle_v_chain_recovers_x0(psg, schedules, name, k, dtype):
    """The eta = 0, clip = 0 chain on the oracle's v ends at x0 within objective_ref.v_recovery_bound; the sign and the swap
    mistakes in the step break it."""
    abar = schedules[name][0]
    ts = psg.ddim_timesteps(T, k)
    x0, e = (v.astype(np.float64) for v in _x0_e())
    u_op = U if dtype == np.float32 else U64
    bound = O.v_recovery_bound(abar, ts, x0, e, u_op)
    a = float(abar[ts[0]])
    xT = (math.sqrt(a) * x0 + math.sqrt(1 - a) * e).astype(dtype)
    tab = psg.ddim_tables(torch.from_numpy(abar), ts, 0.0).numpy()
    predict = O.oracle_v(abar, x0, e, dtype)
    end = O.chain(xT, predict, tab, ts, O.PRED_V, dtype=dtype)[-1]
    err = np.abs(end.astype(np.float64) - x0)
    print(f"V RECOVERY {name} k={k} {np.dtype(dtype).name}: max abs error {err.max():.3g}, worst err / bound {(err / bound).max():.3g}")
    assert end.dtype == dtype and bool((err <= bound).all())
    for mistake in ("v_sign", "ab_swapped"):
        bad = O.chain(xT, predict, tab, ts, O.PRED_V, dtype=dtype, mistake=mistake)[-1]
        assert float((np.abs(bad.astype(np.float64) - x0) / bound).max()) > 10.0, mistake


def test_first_v_step_does_not_amplify(psg, schedules):
    """What v-prediction is for: at t = 999 an error d of the network's output moves the eps chain's x0 by S1 / S0 d (17.7 d on
    stage 2's schedule) and the v chain's by S1 d (< d)."""
    abar = schedules["cosine"][0]
    s0, s1 = math.sqrt(float(abar[999])), math.sqrt(1 - float(abar[999]))
    assert 17.0 < s1 / s0 < 18.5 and s1 < 1.0


# ---------------------------------------------------------------------------------------- the loss reference and its bound
def _loss_case(B, chw, seed=0):
    rng = np.random.default_rng(seed)
    x0 = (2.0 * rng.standard_normal((B, chw))).astype(np.float32)
    noise = rng.standard_normal((B, chw)).astype(np.float32)
    t = np.array(([0, 260, 261, 999, 999, 500, 0] * (B // 7 + 1))[:B], dtype=np.int64)
    return x0, noise, t


def _bound(ref, depth, extra):
    return F32_ROUND * abs(ref) + depth * U * abs(ref) + extra + A_FLOOR


@pytest.mark.parametrize("vec", [False, True], ids=["scalar", "float4"])
@pytest.mark.parametrize("prediction", [O.PRED_EPS, O.PRED_V], ids=["eps", "v"])
def test_loss_reference_bound_holds_the_fp32_restatement_and_notices_mistakes(psg, schedules, prediction, vec):
    """The fp32 restatement of the loss sits inside the fp64 reference's bound; each planted mistake that bears on the loss or
    the gradient leaves it.  (91, 5832) = 530 712 elements: past 2 RED_CAP, so the scalar path takes three trips and the dropped
    second trip is a real loss of elements; on the float4 path the grid covers 4 RED_CAP elements per trip, so the case is run
    at the scalar path only."""
    abar, tabA, tabB = schedules["cosine"]
    wtab = psg.min_snr_weights(torch.from_numpy(abar), GAMMA, prediction).numpy()
    B, chw = 91, 5832
    x0, noise, t = _loss_case(B, chw)
    rng = np.random.default_rng(7)
    tg = O.target(prediction, x0, noise, t, tabA, tabB, 1)
    pred = (tg + 0.1 * rng.standard_normal((B, chw))).astype(np.float32)
    args = (pred, x0, noise, t, tabA, tabB, wtab, prediction, 0.1, 1.0, 1, vec)
    ref = O.diffusion_loss(*args)
    got = O.diffusion_loss(*args, dtype=torch.float32)
    lb = _bound(float(ref["loss"]), ref["depth_loss"], ref["extra_loss"])
    lerr = abs(float(got["loss"]) - float(ref["loss"]))
    gb = ref["grad"].abs() * F32_ROUND + ref["S_grad"] * ref["depth_grad"] * U + ref["extra_grad"] + A_FLOOR
    gerr = (got["grad"].double() - ref["grad"]).abs()
    print(f"LOSS REF pred={prediction} vec={vec}: loss {float(ref['loss']):.6g}, err / bound {lerr / lb:.3g} (depth {ref['depth_loss']}); "
          f"grad worst err / bound {float((gerr / gb).max()):.3g}")
    assert lerr <= lb and bool((gerr <= gb).all())
    mistakes = ["w_by_element", "mean_over_B"] + (["drop_trip"] if not vec else []) + (["unclamped_x0", "v_sign", "ab_swapped"] if prediction == O.PRED_V else [])
    for m in mistakes:
        bad = O.diffusion_loss(*args, mistake=m)
        off = abs(float(bad["loss"]) - float(ref["loss"])) / lb
        goff = float(((bad["grad"] - ref["grad"]).abs() / gb).max())
        print(f"  mistake {m}: loss off by {off:.3g} bounds, grad by {goff:.3g}")
        if m != "w_by_element":            # (weights permuted over i.i.d. residuals: the SUM hardly moves, every element's gradient does)
            assert off > 10.0, m
        if m != "drop_trip":               # (the gradient of a dropped element is still written by the reference's formula)
            assert goff > 10.0, m


def test_loss_case_exercises_both_branches_and_the_clamp(schedules):
    abar, tabA, tabB = schedules["cosine"]
    x0, noise, t = _loss_case(91, 5832)
    rng = np.random.default_rng(7)
    d = 0.1 * rng.standard_normal(x0.shape)
    quad = float((np.abs(d) < 0.1).mean())
    clamped = float((np.abs(x0) > 3).mean())
    assert 0.2 <= quad <= 0.8 and 0.05 <= clamped <= 0.25


def test_unclamped_target_differs_only_where_the_clamp_acts(schedules):
    abar, tabA, tabB = schedules["cosine"]
    x0, noise, t = _loss_case(5, 1001)
    a = O.v_target(x0, noise, t, tabA, tabB, 1)
    b = O.v_target(x0, noise, t, tabA, tabB, 1, mistake="unclamped_x0")
    assert R.same_bits(b, O.v_target(x0, noise, t, tabA, tabB, 0))
    assert bool((a != b).any()) and bool((a == b)[np.abs(x0) <= 3].all())


# --------------------------------------------------------------------------------------------- refusals through the C ABI
def test_refusals_without_gpu(lib):
    """Rejected on the host before any launch: code and message.  The fake pointers are never read."""
    from pokemon_sprite_generator_amd import _lib
    P = 4096

    def err():
        return lib.psg_last_error().decode()

    def loss(pred=P, x0=P, noise=P, t=P, tabA=P, tabB=P, wtab=P, prediction=1, grad=P, target_out=P, loss_out=P, flag=P, beta=0.1, B=2, chw=8,
             num_t=10, ws=P):
        return lib.psg_diffusion_loss_f32(pred, x0, noise, t, tabA, tabB, wtab, prediction, grad, target_out, loss_out, flag, beta, 1.0, B, chw,
                                          num_t, 1, ws, None)
    for name in ("pred", "noise", "t", "loss_out", "ws"):
        assert loss(**{name: None}) == _lib.ERR_ARG and err() == "diffusion_loss: null pointer", name
    for name in ("x0", "tabA", "tabB"):
        assert loss(**{name: None}) == _lib.ERR_ARG and "v-prediction needs" in err(), name
    for p in (-1, 2, 7):
        assert loss(prediction=p) == _lib.ERR_ARG and err() == f"diffusion_loss: prediction {p}"
    for kw in (dict(B=-1), dict(chw=0), dict(chw=-3), dict(num_t=0), dict(beta=0.0), dict(beta=-0.1), dict(beta=float("nan"))):
        assert loss(**kw) == _lib.ERR_SHAPE and err().startswith("diffusion_loss: bad shape"), kw
    assert loss(B=0) == _lib.OK                                                    # an empty batch: nothing launched
    assert loss(B=0, prediction=0, x0=None, tabA=None, tabB=None, wtab=None, grad=None, target_out=None, flag=None) == _lib.OK

    def upd(x=P, pc=P, tab=P, step=P, k=3, clip=3.0, n=8, prediction=1):
        return lib.psg_guided_update_pred_f32(x, P, pc, P, P, tab, k, step, 1.0, clip, n, prediction, None)
    for name in ("x", "pc", "tab", "step"):
        assert upd(**{name: None}) == _lib.ERR_ARG and err() == "guided_update_pred: null pointer", name
    assert upd(clip=-0.5) == _lib.ERR_ARG and err().startswith("guided_update_pred: clip=-0.5")
    assert upd(clip=float("nan")) == _lib.ERR_ARG
    for k in (0, -2):
        assert upd(k=k) == _lib.ERR_ARG and err().endswith(f"k={k}")
    for p in (-1, 2):
        assert upd(prediction=p) == _lib.ERR_ARG and err() == f"guided_update_pred: prediction {p}"
    for n in (0, -5):
        assert upd(n=n) == _lib.OK and upd(n=n, prediction=0) == _lib.OK

    def p2e(x=P, pc=P, pu=P, tabA=P, tabB=P, num_t=10, t_dev=P, prediction=1, out=2 * P, n=8):
        return lib.psg_pred_to_eps_f32(x, pc, pu, 1.5, tabA, tabB, num_t, t_dev, prediction, out, n, None)
    for name in ("pc", "out", "t_dev"):
        assert p2e(**{name: None}) == _lib.ERR_ARG and err() == "pred_to_eps: null pointer", name
    for name in ("x", "tabA", "tabB"):
        assert p2e(**{name: None}) == _lib.ERR_ARG and "v-prediction needs" in err(), name
    for p in (-1, 2):
        assert p2e(prediction=p) == _lib.ERR_ARG and err() == f"pred_to_eps: prediction {p}"
    assert p2e(num_t=0) == _lib.ERR_SHAPE
    for n in (0, -5):
        assert p2e(n=n) == _lib.OK
    assert p2e(prediction=0, pu=None, out=P, x=None, tabA=None, tabB=None) == _lib.OK       # eps, unguided, in place: nothing to do
