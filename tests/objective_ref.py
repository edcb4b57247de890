"""References for the objective kernels of csrc/objective.hip (psg_diffusion_loss_f32, psg_guided_update_pred_f32,
psg_pred_to_eps_f32) and for objective.min_snr_weights (test infrastructure, not a conftest).

Two kinds, as in tests/step_ref.py and tests/guided_ref.py:
  * bit-exact entries (the kernels use __fmul_rn / __fadd_rn / __fsub_rn): numpy, one operation at a time in the kernel's
    documented order, dtype = float32 for THE BITS or float64 for the same formula on exactly widened operands - `v_target`,
    `guided_update_pred`, `pred_to_eps`, `chain`;
  * the weighted loss and its gradient: torch fp64 of the fp32 values the kernel read, with the rounding depth derived in
    `diffusion_loss`'s docstring, held to row_ref.check's bound  r_out |ref| + depth 2^-24 S + extra + A_FLOOR.

`mistake` plants an error (tests/test_objective_ref_cpu.py shows that each breaks the bound it bears on):
    "v_sign"          v with the wrong sign: B x0 - A noise (target); x0 = S0 x + S1 v, e = S1 x - S0 v (step, pred_to_eps)
    "ab_swapped"      tabA and tabB (S0 and S1) change places
    "w_by_element"    the weight read at t[i mod B] of flat element i instead of at t[sample of i]
    "eps_weight_for_v"  min_snr_weights: min(snr, gamma) / snr used for v-prediction
    "unclamped_x0"    the v target built from x0 although add_noise clamped it
    "mean_over_B"     the loss divided by B instead of B chw
    "drop_trip"       the second trip of the grid-stride loop never added"""
import math

import numpy as np
import torch

from tests import guided_ref as G
from tests import step_ref as R
from tests.row_ref import U

F32, F64 = np.float32, np.float64
PRED_EPS, PRED_V = 0, 1            # enum psg_prediction
MISTAKES = ("v_sign", "ab_swapped", "w_by_element", "eps_weight_for_v", "unclamped_x0", "mean_over_B", "drop_trip")


# ------------------------------------------------------------------------------------------------------- weight tables
def snr64(abar32):
    """abar / (1 - abar) in fp64 from the fp32 table values (inf at abar = 1)."""
    a = np.asarray(abar32, dtype=F32).astype(F64)
    with np.errstate(divide="ignore"):
        return a / (1.0 - a)


def min_snr_weights(abar32, gamma, prediction, mistake=None):
    """[T] float32, one Python-float evaluation per entry, one rounding: min(snr, gamma) / snr (eps) or / (snr + 1) (v), with
    the documented limits: abar = 1 -> 0 for both; abar = 0 -> 1 (eps), 0 (v)."""
    out = np.zeros(len(abar32), dtype=F32)
    eps_form = prediction == PRED_EPS or mistake == "eps_weight_for_v"
    for i, a in enumerate(np.asarray(abar32, dtype=F32)):
        a = min(max(float(a), 0.0), 1.0)
        if a >= 1.0:
            w = 0.0
        elif a <= 0.0:
            w = 1.0 if eps_form else 0.0
        else:
            snr = a / (1.0 - a)
            w = min(snr, float(gamma)) / (snr if eps_form else snr + 1.0)
        out[i] = w
    return out


# -------------------------------------------------------------------------------------------------- bit-exact entries
def _tab_at(tabA, tabB, t, dtype, mistake):
    num_t = len(tabA)
    tc = np.clip(np.asarray(t), 0, num_t - 1)
    a, c = np.asarray(tabA, dtype=F32)[tc].astype(dtype), np.asarray(tabB, dtype=F32)[tc].astype(dtype)
    return (c, a) if mistake == "ab_swapped" else (a, c)


def v_target(x0, noise, t, tabA, tabB, do_clamp, dtype=F32, mistake=None):
    """fl(fl(A noise) - fl(B clamp3?(x0))), A = tabA[clamped t[b]]; x0, noise [B, chw]."""
    a, c = _tab_at(tabA, tabB, t, dtype, mistake)
    x = R.clamp3(np.asarray(x0, dtype=F32)) if do_clamp and mistake != "unclamped_x0" else np.asarray(x0, dtype=F32)
    x, nz = x.astype(dtype), np.asarray(noise, dtype=F32).astype(dtype)
    with np.errstate(all="ignore"):
        pa, pb = (a[:, None] * nz).astype(dtype), (c[:, None] * x).astype(dtype)
        r = (pb - pa).astype(dtype) if mistake == "v_sign" else (pa - pb).astype(dtype)
    assert r.dtype == dtype
    return r


def target(prediction, x0, noise, t, tabA, tabB, do_clamp, dtype=F32, mistake=None):
    if prediction == PRED_EPS:
        return np.asarray(noise, dtype=F32).astype(dtype)
    return v_target(x0, noise, t, tabA, tabB, do_clamp, dtype, mistake)


def guided_update_pred(x, pred_c, pred_u, z, tab, j, w, clip, prediction, dtype=F32, mistake=None):
    """psg_guided_update_pred_f32 for step j of tab [5, k].  PRED_EPS: guided_ref.guided_update itself.  PRED_V: the combine,
    x0 = fl(fl(S0 x) - fl(S1 p)), e = fl(fl(S1 x) + fl(S0 p)), then guided_update's clamp / eps recompute / update lines."""
    if prediction == PRED_EPS:
        return G.guided_update(x, pred_c, pred_u, z, tab, j, w, clip, dtype)
    k = tab.shape[1]
    j = min(max(int(j), 0), k - 1)
    S0, S1, P0, P1, SG = (dtype(tab[r, j]) for r in range(5))
    x, p = np.asarray(x).astype(dtype), np.asarray(pred_c).astype(dtype)
    clip = dtype(F32(clip))
    q0, q1 = (S1, S0) if mistake == "ab_swapped" else (S0, S1)
    with np.errstate(all="ignore"):
        if pred_u is not None:
            p = G.cfg_combine(p, pred_u, w, dtype)
        if mistake == "v_sign":
            x0 = ((q0 * x).astype(dtype) + (q1 * p).astype(dtype)).astype(dtype)
            e = ((q1 * x).astype(dtype) - (q0 * p).astype(dtype)).astype(dtype)
        else:
            x0 = ((q0 * x).astype(dtype) - (q1 * p).astype(dtype)).astype(dtype)
            e = ((q1 * x).astype(dtype) + (q0 * p).astype(dtype)).astype(dtype)
        if clip > 0:
            c = np.clip(x0, -clip, clip).astype(dtype)                   # NaN stays NaN
            acted = c != x0
            e = np.where(acted, ((x - (S0 * c).astype(dtype)).astype(dtype) / S1).astype(dtype), e).astype(dtype)
            x0 = c
        r = ((P0 * x0).astype(dtype) + (P1 * e).astype(dtype)).astype(dtype)
        if z is not None:
            r = (r + (SG * np.asarray(z).astype(dtype)).astype(dtype)).astype(dtype)
    assert r.dtype == dtype
    return r


def pred_to_eps(x, pred_c, pred_u, w, tabA, tabB, t, prediction, dtype=F32, mistake=None):
    """psg_pred_to_eps_f32: p = the combine (or pred_c); PRED_EPS: p; PRED_V: fl(fl(tabB[t] x) + fl(tabA[t] p)), t clamped."""
    p = np.asarray(pred_c).astype(dtype)
    with np.errstate(all="ignore"):
        if pred_u is not None:
            p = G.cfg_combine(p, pred_u, w, dtype)
        if prediction == PRED_EPS:
            return p
        a, c = _tab_at(tabA, tabB, np.array([t]), dtype, mistake)
        a, c = a[0], c[0]
        xb, pa = (c * np.asarray(x).astype(dtype)).astype(dtype), (a * p).astype(dtype)
        r = (xb - pa).astype(dtype) if mistake == "v_sign" else (xb + pa).astype(dtype)
    assert r.dtype == dtype
    return r


def chain(x_T, predict, tab, ts, prediction, w=None, clip=0.0, eta=0.0, noise=None, dtype=F32, mistake=None):
    """guided_ref.chain with guided_update_pred: predict(x, t_j, j) -> pred_c, or (pred_c, pred_u) when w is not None."""
    x = np.asarray(x_T).astype(dtype)
    k, draws, out = len(ts), 0, []
    for j in range(k):
        p = predict(x, int(ts[j]), j)
        pc, pu = (p if w is not None else (p, None))
        z = None
        if eta > 0 and j < k - 1:
            z = noise(draws)
            draws += 1
        x = guided_update_pred(x, pc, pu, z, tab, j, 0.0 if w is None else w, clip, prediction, dtype, mistake)
        out.append(x)
    return out


# ------------------------------------------------------------------------------------------------------ the weighted loss
def loss_is_vec(chw, aligned=True):
    """Whether psg_diffusion_loss_f32 takes its float4 path."""
    return chw % 4 == 0 and aligned


def diffusion_loss(pred, x0, noise, t, tabA, tabB, wtab, prediction, beta, grad_scale, do_clamp, vec, dtype=torch.float64,
                   mistake=None):
    """loss = (1 / n) sum_i w_b smoothl1_beta(pred_i - target_i), n = B chw, and grad = w_b smoothl1'(d_i) / n grad_scale, on
    pred, x0, noise [B, chw] float32 numpy, t [B] -> dict(loss, depth_loss, extra_loss, grad, S_grad, depth_grad, extra_grad).
    dtype fp64: the reference (the target included, from exactly widened operands); fp32: the kernel's arithmetic restated in
    torch, which must sit inside the bound.

    Roundings of the kernel (library built with -ffp-contract=off: one rounding per fp32 operation), beyond step_ref.smooth_l1:
      target (PRED_V): two products and a subtraction: |target_32 - target| <= 3 2^-24 S_t, S_t = |A noise| + |B x0| (each
        product moves by 2^-24 of itself, the difference by 2^-24 of a value <= S_t).  PRED_EPS: the noise itself, no rounding.
      loss: a term is smooth_l1's (4 roundings, its docstring) times w: 5.  smoothl1_beta is 1-Lipschitz in d, so the target's
        error moves a term by at most w 3 2^-24 S_t: extra_loss = (1 / n) sum w 3 2^-24 S_t, outside the depth.  A lane adds
        its terms serially - `vec` (float4 path): 4 per trip of the grid-stride loop over n / 4 items, else 1 per trip over n -
        and the fixed tree of step_ref.red_tree follows (the same 1024 x 256 grid, a finish kernel of the same shape):
        depth_loss = 5 + additions of a lane + red_tree, on S = loss (all terms are non-negative).
      grad: fl(p - target), / beta (the linear branch has fewer), the rounding of 1 / n, fl(w / n), the product with
        grad_scale and the product with the branch value: depth 6 on S = |grad|.  smoothl1' is (1 / beta)-Lipschitz in d
        everywhere (also across the branch point, where both branches give |g| = 1), so the target's error adds
        extra_grad = 3 2^-24 S_t / beta w / n |grad_scale|."""
    B, chw = pred.shape
    n = B * chw
    t = np.asarray(t)
    num_t = len(tabA) if tabA is not None else (len(wtab) if wtab is not None else 1 << 30)
    tc = np.clip(t, 0, num_t - 1)
    np_dt = F64 if dtype == torch.float64 else F32
    tg_np = target(prediction, x0, noise, t, tabA, tabB, do_clamp, np_dt, mistake)
    if prediction == PRED_V:
        a, c = _tab_at(tabA, tabB, t, F64, None)
        xc = R.clamp3(np.asarray(x0, dtype=F32)) if do_clamp else np.asarray(x0, dtype=F32)
        with np.errstate(all="ignore"):
            S_t = np.abs(a[:, None] * noise.astype(F64)) + np.abs(c[:, None] * xc.astype(F64))
    else:
        S_t = np.zeros((B, chw))
    w_b = np.ones(B) if wtab is None else np.asarray(wtab, dtype=F32)[tc].astype(F64)
    w_el = np.broadcast_to(w_b[:, None], (B, chw))
    if mistake == "w_by_element" and wtab is not None:
        w_el = w_b[np.arange(n) % B].reshape(B, chw)
    p = torch.from_numpy(np.ascontiguousarray(pred)).to(dtype).reshape(-1)
    tg = torch.from_numpy(np.ascontiguousarray(tg_np)).to(dtype).reshape(-1)
    w = torch.from_numpy(np.ascontiguousarray(w_el)).to(dtype).reshape(-1)
    St = torch.from_numpy(np.ascontiguousarray(S_t)).reshape(-1)
    beta, gs = R.f32(beta), R.f32(grad_scale)
    d = p - tg
    ad = d.abs()
    terms = w * torch.where(ad < beta, 0.5 * d * d / beta, ad - 0.5 * beta)
    W = 4 if vec else 1
    items = n // W
    if mistake == "drop_trip":
        terms = R._drop_trip(terms, n, R.RED_CAP * W)
    denom = B if mistake == "mean_over_B" else n
    inv_n = 1.0 / denom if dtype == torch.float64 else float(F32(1.0) / F32(denom))
    loss = terms.sum() * inv_n
    g = torch.where(ad < beta, d / beta, torch.where(d > 0, 1.0, -1.0).to(dtype)) * (w * inv_n * gs)
    depth_loss = 5 + R.red_trips(items) * W + R.red_tree(R.red_blocks(items))
    extra_loss = float((w.double() * 3 * U * St).sum() / n)
    extra_grad = 3 * U * St / beta * w.double() * abs(gs) / n
    return dict(loss=loss, depth_loss=depth_loss, extra_loss=extra_loss, grad=g, S_grad=g.abs(), depth_grad=6, extra_grad=extra_grad,
                S_t=S_t)


def loss_flags(pred, tgt, t, num_t):
    """The bits psg_diffusion_loss_f32 ORs in: PRED_BAD for a non-finite pred, T_RANGE for a t outside the table, LOSS_BAD for
    a non-finite loss (a non-finite pred or target makes it so)."""
    f = 0
    if not np.isfinite(pred).all():
        f |= R.FLAG_PRED_BAD | R.FLAG_LOSS_BAD
    if not np.isfinite(tgt).all():
        f |= R.FLAG_LOSS_BAD
    if ((np.asarray(t) < 0) | (np.asarray(t) >= num_t)).any():
        f |= R.FLAG_T_RANGE
    return f


# --------------------------------------------------------------------------------------------------- the oracle-v chain
def v_recovery_bound(abar, ts, x0, e, u_op):
    """First-order bound on |x_final - x0| of the eta = 0, clip = 0 v chain started at x_T = s0 x0 + s1 e with a predictor that
    returns v_j = s0 e - s1 x0 rounded to the working precision (dv = u_op |v|).  With exact tables (s0^2 + s1^2 = 1) and
    arithmetic a step gives x0^ = x0, e^ = e and maps s0 x0 + s1 e to p0 x0 + p1 e; the chain ends at x0.  With a = |x0|, b = |e|,
    m_x = s0 a + s1 b >= |x| and m_v = s0 b + s1 a >= |v|, one step with tables rounded to fp32 (relative U each) and every
    operation rounded (relative u_op) adds at most
        dx0 = (U + u_op) (s0 m_x + s1 m_v) + u_op a + s1 dv         the two products, the difference (which is x0), the oracle
        de  = (U + u_op) (s1 m_x + s0 m_v) + u_op b + s0 dv         likewise for e^
        L   = p0 dx0 + p1 de + (U + 2 u_op) (p0 a + p1 b)           the products with P0, P1 and the sum
    and an error of x is carried on multiplied by dx'/dx = p0 s0 + p1 s1 <= 1 at every later step (guided_ref's eps chain
    carries it on with p0 / s0 >= 1: there is no division here).  The rounding of x_T itself, u_op |x_T|, passes all steps.
    Second-order terms are < 1e-4 of this: x 1.001."""
    a_t = np.asarray(abar)[ts].astype(F64)
    a_p = np.concatenate([a_t[1:], [1.0]])
    s0, s1, p0, p1 = np.sqrt(a_t), np.sqrt(1 - a_t), np.sqrt(a_p), np.sqrt(1 - a_p)
    a, b = np.abs(x0).astype(F64), np.abs(e).astype(F64)
    k = len(ts)
    gain = p0 * s0 + p1 * s1
    gain_after = np.ones(k)
    for j in range(k - 2, -1, -1):
        gain_after[j] = gain_after[j + 1] * gain[j + 1]
    total = u_op * (s0[0] * a + s1[0] * b) * gain_after[0] * gain[0]
    for j in range(k):
        m_x, m_v = s0[j] * a + s1[j] * b, s0[j] * b + s1[j] * a
        dv = u_op * m_v
        dx0 = (U + u_op) * (s0[j] * m_x + s1[j] * m_v) + u_op * a + s1[j] * dv
        de = (U + u_op) * (s1[j] * m_x + s0[j] * m_v) + u_op * b + s0[j] * dv
        L = p0[j] * dx0 + p1[j] * de + (U + 2 * u_op) * (p0[j] * a + p1[j] * b)
        total = total + L * gain_after[j]
    return 1.001 * total


def oracle_v(abar, x0, e, dtype):
    """predict(x, t, j) of the oracle: v_t = sqrt(abar_t) e - sqrt(1 - abar_t) x0 in fp64, rounded once to dtype."""
    def predict(x, t, j):
        a = float(abar[t])
        return (math.sqrt(a) * e - math.sqrt(1 - a) * x0).astype(dtype)
    return predict
