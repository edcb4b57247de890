"""-m "not gpu": the schedule side of guidance.py (ddim_timesteps, ddim_tables) against the restatements of
tests/guided_ref.py, and the restatements themselves against what a DDIM step must do - every bound is derived here from the
roundings of the tables and of the operations, and every planted mistake of guided_ref.MISTAKES is shown to break one."""
import math

import numpy as np
import pytest
import torch

from tests import guided_ref as G
from tests import step_ref as R

U = 2.0 ** -24                 # unit roundoff of fp32: one rounding moves a value by at most U times its magnitude
U64 = 2.0 ** -53
T = 1000
KS = (1, 2, 7, 20, 50, 1000)
ETAS = (0.0, 0.5, 1.0)


@pytest.fixture(scope="module")
def psg():
    import pokemon_sprite_generator_amd as m
    return m


@pytest.fixture(scope="module")
def schedules(psg):
    """name -> fp32 alphas_cumprod [1000] as numpy: stage 2's cosine-clipped schedule and the linear one of stage 3 / the demo."""
    return {"cosine": psg.NoiseScheduler().alphas_cumprod.cpu().numpy().astype(np.float32),
            "linear": psg.LinearNoiseScheduler().alphas_cumprod.cpu().numpy().astype(np.float32)}


# --------------------------------------------------------------------------------------------- 1. tables and timesteps
@pytest.mark.parametrize("k", KS)
def test_timesteps_equal_the_restatement(psg, k):
    ts = psg.ddim_timesteps(T, k)
    want = G.ddim_timesteps(T, k)
    assert ts.dtype == np.int64 and ts.shape == (k,) and np.array_equal(ts, want)
    assert int(ts[0]) == T - 1 and bool((np.diff(ts) < 0).all())
    if k > 1:
        assert int(ts[-1]) == 0


def test_timesteps_refuse_a_bad_k(psg):
    for k in (0, -1, T + 1):
        with pytest.raises(ValueError):
            psg.ddim_timesteps(T, k)
    assert list(psg.ddim_timesteps(5, 5)) == [4, 3, 2, 1, 0]


@pytest.mark.parametrize("eta", ETAS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["cosine", "linear"])
def test_tables_equal_the_restatement_on_the_bits(psg, schedules, name, k, eta):
    abar = schedules[name]
    ts = psg.ddim_timesteps(T, k)
    got = psg.ddim_tables(torch.from_numpy(abar), ts, eta)
    assert got.dtype == torch.float32 and tuple(got.shape) == (5, k) and not got.is_cuda
    want = G.ddim_tables(abar, ts, eta)
    assert R.same_bits(got, want)
    assert bool(torch.isfinite(got).all()) and float(got[2, -1]) == 1.0 and float(got[3, -1]) == 0.0 and float(got[4, -1]) == 0.0
    if eta == 0:
        assert not bool(got[4].any())
    elif k > 1:
        assert float(got[4, :-1].min()) > 0.0


# ------------------------------------------------------------------------------------------------ 2. oracle-eps recovery
def _ideal(abar, ts):
    """The table in exact (fp64) values of the fp32 abar: rows s0, s1, p0, p1 at eta = 0."""
    a_t = abar[ts].astype(np.float64)
    a_p = np.concatenate([a_t[1:], [1.0]])
    return np.sqrt(a_t), np.sqrt(1 - a_t), np.sqrt(a_p), np.sqrt(1 - a_p)


def _recovery_bound(abar, ts, x0, e, u_op, de=None):
    """First-order bound on |x_final - x0| of the eta = 0, clip = 0 chain started at x_T = s0 x0 + s1 e with a predictor that
    returns e.  With exact tables and arithmetic every step maps s0 x0 + s1 e to p0 x0 + p1 e exactly and the chain ends at x0.
    One step  x' = fl(fl(P0 fl(fl(x - fl(S1 e)) / S0)) + fl(P1 e))  with tables rounded to fp32 (relative U each) and every
    operation rounded (relative u_op) adds at most, with a = |x0|, b = |e| element by element,
        L = p0/s0 ((U + u_op) s1 b + u_op s0 a)        the product S1 e, then the difference, which is s0 x0
          + 2 (U + u_op) p0 a                          the division by S0 and the product with P0
          + (U + u_op) p1 b + u_op (p0 a + p1 b)       the product P1 e and the sum
          + (p0 s1/s0 + p1) de                         an error de of the predictor's e (guided: the combine's roundings)
    and an error of x is carried on multiplied by dx'/dx = p0/s0 >= 1 at every later step.  The rounding of x_T itself,
    u_op |x_T|, passes all steps.  Second-order terms are < 1e-4 of this (the first-order total is < 1e-4 of |x|): x 1.001."""
    s0, s1, p0, p1 = _ideal(abar, ts)
    a, b = np.abs(x0).astype(np.float64), np.abs(e).astype(np.float64)
    de = 0.0 if de is None else de
    k = len(ts)
    gain_after = np.ones(k)
    for j in range(k - 2, -1, -1):
        gain_after[j] = gain_after[j + 1] * p0[j + 1] / s0[j + 1]
    total = u_op * (s0[0] * a + s1[0] * b) * gain_after[0] * p0[0] / s0[0]
    for j in range(k):
        L = (p0[j] / s0[j] * ((U + u_op) * s1[j] * b + u_op * s0[j] * a) + 2 * (U + u_op) * p0[j] * a + (U + u_op) * p1[j] * b
             + u_op * (p0[j] * a + p1[j] * b) + (p0[j] * s1[j] / s0[j] + p1[j]) * de)
        total = total + L * gain_after[j]
    return 1.001 * total


def _x0_e(seed=0, n=8 * 27 * 27):
    rng = np.random.default_rng(seed)
    return rng.uniform(-2.5, 2.5, n), rng.standard_normal(n)


def _x_T(abar, ts, x0, e, dtype):
    a = float(abar[ts[0]])
    return (math.sqrt(a) * x0 + math.sqrt(1 - a) * e).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("k", (1, 5, 20))
@pytest.mark.parametrize("name", ["cosine", "linear"])
def test_oracle_eps_chain_recovers_x0(psg, schedules, name, k, dtype):
    """... and the two table mistakes break the bound.  ("no_recompute" cannot act at clip = 0 and "w_on_c" needs guidance:
    they are planted in the two tests below.)"""
    abar = schedules[name]
    ts = psg.ddim_timesteps(T, k)
    x0, e = _x0_e()
    u_op = U if dtype == np.float32 else U64
    bound = _recovery_bound(abar, ts, x0, e, u_op)
    xT = _x_T(abar, ts, x0, e, dtype)
    pred = lambda x, t, j: e.astype(dtype)                                   # noqa: E731
    tab = psg.ddim_tables(torch.from_numpy(abar), ts, 0.0).numpy()
    end = G.chain(xT, pred, tab, ts, dtype=dtype)[-1]
    err = np.abs(end.astype(np.float64) - x0)
    print(f"RECOVERY {name} k={k} {np.dtype(dtype).name}: max abs error {err.max():.3g}, worst err / bound {(err / bound).max():.3g}")
    assert end.dtype == dtype and bool((err <= bound).all())
    for mistake in ("ap_at_t", "z_last"):
        bad = G.chain(xT, pred, G.ddim_tables(abar, ts, 0.0, mistake=mistake), ts, dtype=dtype, mistake=mistake)[-1]
        assert float((np.abs(bad.astype(np.float64) - x0) / bound).max()) > 10.0, mistake


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["cosine", "linear"])
def test_guided_oracle_chain_recovers_x0(psg, schedules, name, dtype):
    """The same recovery through the combine: eps_u = rd(e - w d), eps_c = rd(eps_u + d), so that eps_u + w (eps_c - eps_u) = e
    up to de <= u (|eps_u| + |w| |eps_c| + 2 |w d| + |e|): the roundings r_u, r_c of the two operands enter as r_u + w r_c, the
    difference and the product with w each add u |w d| (the product also carries the difference's u |d| times w), the sum
    u |e|.  w = 2 is exact in fp32.  "w_on_c" breaks it."""
    abar, k, w = schedules[name], 5, 2.0
    ts = psg.ddim_timesteps(T, k)
    x0, e = _x0_e(1)
    d = np.random.default_rng(7).standard_normal(e.shape) * 0.5
    eu = (e - w * d).astype(dtype)
    ec = (eu.astype(np.float64) + d).astype(dtype)
    u_op = U if dtype == np.float32 else U64
    de = u_op * (np.abs(eu) + w * np.abs(ec) + 2 * w * np.abs(d) + np.abs(e)).astype(np.float64)
    bound = _recovery_bound(abar, ts, x0, e, u_op, de=de)
    xT = _x_T(abar, ts, x0, e, dtype)
    tab = psg.ddim_tables(torch.from_numpy(abar), ts, 0.0).numpy()
    pred = lambda x, t, j: (ec, eu)                                          # noqa: E731
    end = G.chain(xT, pred, tab, ts, w=w, dtype=dtype)[-1]
    err = np.abs(end.astype(np.float64) - x0)
    print(f"GUIDED RECOVERY {name} {np.dtype(dtype).name}: max abs error {err.max():.3g}, worst err / bound {(err / bound).max():.3g}")
    assert bool((err <= bound).all())
    bad = G.chain(xT, pred, tab, ts, w=w, dtype=dtype, mistake="w_on_c")[-1]
    assert float((np.abs(bad.astype(np.float64) - x0) / bound).max()) > 10.0
    # the combine on its own, and w = 1 gives eps_c back up to the two roundings of (eps_c - eps_u) + eps_u
    assert np.array_equal(G.cfg_combine(ec, eu, 0.0, dtype), eu)
    one = G.cfg_combine(ec, eu, 1.0, dtype).astype(np.float64)
    assert bool((np.abs(one - ec) <= u_op * (np.abs(ec - eu.astype(np.float64)) + np.abs(ec))).all())


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_clamped_step_keeps_x_consistent(schedules, dtype):
    """Where the clamp acts, e is recomputed so that x = S0 c + S1 e still holds.  A step whose target is its own timestep
    (P0 = S0, P1 = S1: a table built by hand) must then return x itself, clamped or not:
        x' = fl(fl(S0 c) + fl(S1 fl(fl(x - fl(S0 c)) / S1)))   differs from x by at most
        u (2 |S0 c| + 3 |x - S0 c| + |x|)   (the product S0 c counted on both sides; the difference, the quotient and the second
        product on |x - S0 c|; the sum on |x|), and where nothing clamps by u (2 |S1 e| + 3 |x - S1 e| + |x|) likewise.
    "no_recompute" breaks it on the clamped elements."""
    a = float(schedules["cosine"][400])
    tab = np.array([[math.sqrt(a)], [math.sqrt(1 - a)], [math.sqrt(a)], [math.sqrt(1 - a)], [0.0]], dtype=np.float32)
    S0, S1 = float(tab[0, 0]), float(tab[1, 0])
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(4000) * 2).astype(dtype)
    e = rng.standard_normal(4000).astype(dtype)
    clip = 1.0
    got, acted = G.guided_update(x, e, None, None, tab, 0, 0.0, clip, dtype, want_mask=True)
    share = float(acted.mean())
    print(f"CLAMPED share {share:.3f}")
    assert 0.0 < share < 1.0
    u_op = U if dtype == np.float32 else U64
    x64, e64 = x.astype(np.float64), e.astype(np.float64)
    c = np.clip((x64 - S1 * e64) / S0, -clip, clip)
    inner = np.where(acted, np.abs(S0 * c), np.abs(S1 * e64))
    bound = 1.001 * u_op * (2 * inner + 3 * (np.abs(x64) + inner) + np.abs(x64))
    assert bool((np.abs(got.astype(np.float64) - x64) <= bound).all())
    bad = G.guided_update(x, e, None, None, tab, 0, 0.0, clip, dtype, mistake="no_recompute")
    off = np.abs(bad.astype(np.float64) - x64) / bound
    assert float(off[acted].min()) > 10.0 and bool((off[~acted] <= 1.0).all())


# ------------------------------------------------------------------------------- 3. eta = 1 on consecutive timesteps
def _tables64(abar, t, eta=1.0):
    """The step t -> t - 1 in fp64, never rounded to fp32: (s0, s1, p0, p1, sigma)."""
    a_t, a_p = float(abar[t]), float(abar[t - 1])
    sg = eta * math.sqrt((1 - a_p) / (1 - a_t)) * math.sqrt(max(1 - a_t / a_p, 0.0))
    return math.sqrt(a_t), math.sqrt(1 - a_t), math.sqrt(a_p), math.sqrt(max(1 - a_p - sg * sg, 0.0)), sg


@pytest.mark.parametrize("t", (999, 500, 37, 1))
@pytest.mark.parametrize("name", ["cosine", "linear"])
def test_eta_one_is_the_posterior_variance_step(schedules, name, t):
    """In exact arithmetic the eta = 1 step t -> t - 1 is DDPM's posterior step with alpha_t = abar_t / abar_{t-1}:
    sqrt(1/alpha) (x - beta e / sqrt(1 - abar_t)) + sqrt(beta (1 - abar_{t-1}) / (1 - abar_t)) z.  In fp64 both sides are a
    dozen operations on terms no larger than p0/s0 |x|, (p1 + p0 s1/s0) |e| (the two parts of e's coefficient cancel to
    beta / (sqrt(alpha) s1)) and sigma |z|: 32 fp64 roundings of their sum cover both.  One term is larger: both sides form
    1 - abar_t / abar_{t-1} from a rounded quotient, an absolute 2^-53 alpha on a difference of size beta, r = 2^-53 alpha / beta
    relative (1e-12 at t = 1).  It reaches the formula's coefficient of e (r ce), sigma on either side (r / 2 each), and P1 =
    sqrt(1 - abar_{t-1} - sigma^2) through sigma^2 (r sigma^2 / (2 p1))."""
    abar = schedules[name]
    s0, s1, p0, p1, sg = _tables64(abar, t)
    tab = np.array([[s0], [s1], [p0], [p1], [sg]], dtype=np.float64)
    rng = np.random.default_rng(t)
    x, e, z = rng.standard_normal(500) * 2, rng.standard_normal(500), rng.standard_normal(500)
    got = G.guided_update(x, e, None, z, tab, 0, 0.0, 0.0, np.float64)
    a_t, a_p = float(abar[t]), float(abar[t - 1])
    alpha = a_t / a_p
    beta = 1 - alpha
    want = math.sqrt(1 / alpha) * (x - beta * e / math.sqrt(1 - a_t)) + math.sqrt(beta * (1 - a_p) / (1 - a_t)) * z
    r = U64 * alpha / beta
    ce = beta / (math.sqrt(alpha) * s1)
    bound = (32 * U64 * (p0 / s0 * np.abs(x) + (p1 + p0 * s1 / s0) * np.abs(e) + sg * np.abs(z))
             + r * ((ce + sg * sg / (2 * p1)) * np.abs(e) + sg * np.abs(z)))
    err = np.abs(got - want)
    print(f"POSTERIOR {name} t={t}: max abs difference {err.max():.3g}, worst / bound {(err / bound).max():.3g}")
    assert bool((err <= bound).all())
    # (the package's fp32 table of the same step is the fp64 one rounded once)
    from pokemon_sprite_generator_amd import ddim_tables
    assert R.same_bits(ddim_tables(torch.from_numpy(abar), [t, t - 1], 1.0)[:, 0], torch.tensor([s0, s1, p0, p1, sg], dtype=torch.float64).float())


@pytest.mark.parametrize("t", (999, 500, 37, 1))
def test_eta_one_against_the_stage3_sampler_update(psg, t):
    """The fp32 step against step_ref.sampler_update mode 1 on LinearNoiseScheduler's own fp32 tables (c0 = sqrt_recip_alphas,
    c1 = betas, c2 = sqrt_one_minus_alphas_cumprod, c3 = sqrt(posterior_variance)).  The two agree up to
      * the scheduler's tables: alphas = fl(1 - betas) (absolute 2^-25) and abar_t = fl(abar_{t-1} alphas_t) (relative U), so the
        beta' = 1 - abar_t / abar_{t-1} that DDIM sees differs from betas_t by at most db = 1.5 U, a RELATIVE db / beta (7e-4 at
        t = 1); c0 = fl(sqrt(fl(1 / alpha))): 1.5 U, and alpha' against alpha another U / 2 under the root; c2 = fl(sqrt(fl(1 - abar))):
        1.5 U; posterior_variance = three fp32 operations on fl(1 - abar) values: 5 U, 2.5 U under the root, + U for the root;
      * DDIM's own five table entries, U each: 2 on x's coefficient P0/S0, 2 on P1 and 3 on P0 S1/S0 (the two parts of e's), 1 on
        sigma;
      * the operations: 6 roundings on DDIM's side, 5 on the scheduler's, each at most U times the sum of the absolute terms.
    x 1.001 for the second order."""
    sch = psg.LinearNoiseScheduler()
    abar = sch.alphas_cumprod.numpy().astype(np.float32)
    tab = psg.ddim_tables(sch.alphas_cumprod, [t, t - 1], 1.0).numpy()
    rng = np.random.default_rng(100 + t)
    x, e, z = ((rng.standard_normal(2000) * s).astype(np.float32) for s in (2.0, 1.0, 1.0))
    got = G.guided_update(x, e, None, z, tab, 0, 0.0, 0.0, np.float32)
    c3 = np.float32(math.sqrt(float(sch.posterior_variance[t])))
    want = R.sampler_update(x, e, z, 1, float(sch.sqrt_recip_alphas[t]), float(sch.betas[t]), float(sch.sqrt_one_minus_alphas_cumprod[t]), float(c3))
    s0, s1, p0, p1, sg = _tables64(abar, t)
    beta, alpha = float(sch.betas[t]), float(sch.alphas[t])
    db = 1.5 * U
    ax, ae, az = (np.abs(v).astype(np.float64) for v in (x, e, z))
    cx, ce1, ce2 = p0 / s0, p1, p0 * s1 / s0
    ce = beta / (math.sqrt(alpha) * s1)
    bound = 1.001 * (ax * cx * (2.0 + 2) * U + ae * (ce * (db / beta + 3.5 * U) + (2 * ce1 + 3 * ce2) * U) + az * sg * (db / (2 * beta) + 4.5 * U)
                     + 6 * U * (cx * ax + (ce1 + ce2) * ae + sg * az) + 5 * U * (cx * ax + ce * ae + sg * az))
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"STAGE3 t={t}: max abs difference {err.max():.3g}, worst / bound {(err / bound).max():.3g}")
    assert bool((err <= bound).all())
    # a step that takes a_p at t_j does not move towards t - 1 at all: far outside
    bad = G.guided_update(x, e, None, z, G.ddim_tables(abar, [t, t - 1], 1.0, mistake="ap_at_t"), 0, 0.0, 0.0, np.float32)
    assert float((np.abs(bad.astype(np.float64) - want) / bound).max()) > 10.0


# ------------------------------------------------------------------------------------------ 4. a clamp that never clamps
@pytest.mark.parametrize("guided", [False, True])
def test_a_clamp_that_never_acts_changes_no_bit(psg, schedules, guided):
    ts = psg.ddim_timesteps(T, 7)
    tab = psg.ddim_tables(torch.from_numpy(schedules["cosine"]), ts, 0.7).numpy()
    rng = np.random.default_rng(11)
    x, ec, eu, z = (rng.standard_normal(3001).astype(np.float32) * s for s in (3.0, 1.0, 1.0, 1.0))
    for j in (0, 3, 6):
        a = G.guided_update(x, ec, eu if guided else None, z, tab, j, 7.5, 0.0)
        b, acted = G.guided_update(x, ec, eu if guided else None, z, tab, j, 7.5, 1e30, want_mask=True)
        assert not bool(acted.any()) and R.same_bits(a, b)
        c, acted = G.guided_update(x, ec, eu if guided else None, z, tab, j, 7.5, 0.25, want_mask=True)
        assert bool(acted.any()) and not R.same_bits(a, c)


def test_z_on_the_last_step_is_a_mistake_the_chain_shows(psg, schedules):
    """eta > 0: the correct chain draws k - 1 times; "z_last" draws k times and ends somewhere else."""
    abar = schedules["linear"]
    ts = psg.ddim_timesteps(T, 4)
    rng = np.random.default_rng(5)
    xT, e = rng.standard_normal(100).astype(np.float32), rng.standard_normal(100).astype(np.float32)
    zs = rng.standard_normal((4, 100)).astype(np.float32)
    asked = []

    def noise(i):
        asked.append(i)
        return zs[i]
    good = G.chain(xT, lambda x, t, j: e, G.ddim_tables(abar, ts, 1.0), ts, eta=1.0, noise=noise)[-1]
    assert asked == [0, 1, 2]
    asked.clear()
    bad = G.chain(xT, lambda x, t, j: e, G.ddim_tables(abar, ts, 1.0, mistake="z_last"), ts, eta=1.0, noise=noise, mistake="z_last")[-1]
    assert asked == [0, 1, 2, 3] and not R.same_bits(good, bad)
    asked.clear()
    G.chain(xT, lambda x, t, j: e, G.ddim_tables(abar, ts, 0.0), ts, eta=0.0, noise=noise)
    assert asked == []


# ------------------------------------------------------------------------------------------------------ 5. text drop
@pytest.mark.parametrize("seed", (1234, 99))
@pytest.mark.parametrize("p", (0.0, 0.1, 0.5))
@pytest.mark.parametrize("B", (1, 5, 8, 64, 3))
def test_text_drop_mask_is_the_dropout_hash_at_the_sample_index(B, p, seed):
    from tests import drop_ref
    rng = np.random.default_rng(B)
    text, null = rng.standard_normal((B, 6)).astype(np.float32), rng.standard_normal(6).astype(np.float32)
    out, dropped = G.text_cond_drop(text, null, seed, p)
    keep = drop_ref.keep_flat(seed, np.arange(B), p)
    assert np.array_equal(dropped.astype(bool), ~keep) and dropped.dtype == np.int32
    assert R.same_bits(out[keep], text[keep]) and all(R.same_bits(r, null) for r in out[~keep])
    if p == 0:
        assert not dropped.any()


def test_text_drop_counts_of_seed_1234():
    assert int(G.text_drop_mask(1234, 8, 0.5).sum()) == 3
    assert int(G.text_drop_mask(1234, 64, 0.1).sum()) == 7
