"""Numpy restatements of the guidance / DDIM kernels (psg_text_cond_drop_f32, psg_cfg_combine_f32, psg_guided_update_f32) and
of guidance.ddim_timesteps / ddim_tables (test infrastructure, not a conftest).

Every elementwise entry takes dtype = numpy float32 - the kernel's own arithmetic, one rounding per operation in the
documented order: THE BITS - or float64 (the fp32 operands widened exactly), and `mistake`, a planted error:
    "ap_at_t"    ddim_tables: a_p taken at t_j instead of t_{j+1}
    "w_on_c"     the combine with w applied to eps_c alone: eps_u + (w eps_c - eps_u)
    "no_recompute"  guided_update: e not recomputed where the clamp acted
    "z_last"     the chain does not end clean: after the last step a_p = abar[0] instead of 1 (ddim_tables), so sigma of the
                 last step is not 0, and the chain adds z on the last step (chain)
tests/test_guided_ref_cpu.py checks the restatements; the GPU tests hold the kernels and the samplers to their bits."""
import math
from fractions import Fraction

import numpy as np

from tests import drop_ref

F32, F64 = np.float32, np.float64
MISTAKES = ("ap_at_t", "w_on_c", "no_recompute", "z_last")


def ddim_timesteps(T, k):
    """Round-half-up of (T - 1) (k - 1 - j) / (k - 1) in exact rationals; [T - 1] for k = 1."""
    if not 1 <= k <= T:
        raise ValueError("k")
    if k == 1:
        return np.array([T - 1], dtype=np.int64)
    return np.array([math.floor(Fraction((T - 1) * (k - 1 - j), k - 1) + Fraction(1, 2)) for j in range(k)], dtype=np.int64)


def ddim_tables(abar32, ts, eta, mistake=None):
    """[5, k] float32: one Python-float (fp64) evaluation per entry from the fp32 table values, one rounding."""
    abar = [float(v) for v in np.asarray(abar32, dtype=F32)]
    k = len(ts)
    tab = np.zeros((5, k), dtype=F32)
    for j in range(k):
        a_t = abar[int(ts[j])]
        if mistake == "ap_at_t":
            a_p = a_t
        elif j + 1 < k:
            a_p = abar[int(ts[j + 1])]
        else:
            a_p = abar[0] if mistake == "z_last" else 1.0
        sigma = float(eta) * math.sqrt((1.0 - a_p) / (1.0 - a_t)) * math.sqrt(max(1.0 - a_t / a_p, 0.0))
        tab[:, j] = [math.sqrt(a_t), math.sqrt(1.0 - a_t), math.sqrt(a_p), math.sqrt(max(1.0 - a_p - sigma * sigma, 0.0)), sigma]
    return tab


def cfg_combine(eps_c, eps_u, w, dtype=F32, mistake=None):
    """fl(eps_u + fl(w fl(eps_c - eps_u)))."""
    c, u, w = np.asarray(eps_c).astype(dtype), np.asarray(eps_u).astype(dtype), dtype(F32(w))
    with np.errstate(all="ignore"):
        if mistake == "w_on_c":
            r = (u + ((w * c).astype(dtype) - u).astype(dtype)).astype(dtype)
        else:
            r = (u + (w * (c - u).astype(dtype)).astype(dtype)).astype(dtype)
    assert r.dtype == dtype
    return r


def guided_update(x, eps_c, eps_u, z, tab, j, w, clip, dtype=F32, mistake=None, want_mask=False):
    """psg_guided_update_f32 for step j of tab [5, k] (j clamped to 0..k-1).  eps_u / z: None = absent.  want_mask: also the
    mask of the elements on which the clamp acted."""
    k = tab.shape[1]
    j = min(max(int(j), 0), k - 1)
    S0, S1, P0, P1, SG = (dtype(tab[r, j]) for r in range(5))           # (an fp32 table widens exactly; an fp64 one is the caller's)
    x, e = np.asarray(x).astype(dtype), np.asarray(eps_c).astype(dtype)
    clip = dtype(F32(clip))
    with np.errstate(all="ignore"):
        if eps_u is not None:
            e = cfg_combine(e, eps_u, w, dtype, mistake)
        x0 = ((x - (S1 * e).astype(dtype)).astype(dtype) / S0).astype(dtype)
        acted = np.zeros(x.shape, dtype=bool)
        if clip > 0:
            c = np.clip(x0, -clip, clip).astype(dtype)                   # NaN stays NaN
            acted = c != x0                                             # (true at a NaN, as in the kernel)
            if mistake != "no_recompute":
                e = np.where(acted, ((x - (S0 * c).astype(dtype)).astype(dtype) / S1).astype(dtype), e).astype(dtype)
            x0 = c
        r = ((P0 * x0).astype(dtype) + (P1 * e).astype(dtype)).astype(dtype)
        if z is not None:
            r = (r + (SG * np.asarray(z).astype(dtype)).astype(dtype)).astype(dtype)
    assert r.dtype == dtype
    return (r, acted) if want_mask else r


def chain(x_T, predict, tab, ts, w=None, clip=0.0, eta=0.0, noise=None, dtype=F32, mistake=None):
    """The DDIM chain: predict(x, t_j, j) -> eps_c, or (eps_c, eps_u) when w is not None; noise(i) -> the i-th z, drawn when
    eta > 0 and not on the last step.  Returns the list of latents after every step."""
    x = np.asarray(x_T).astype(dtype)
    k, draws, out = len(ts), 0, []
    for j in range(k):
        p = predict(x, int(ts[j]), j)
        ec, eu = (p if w is not None else (p, None))
        z = None
        if eta > 0 and (j < k - 1 or mistake == "z_last"):
            z = noise(draws)
            draws += 1
        x = guided_update(x, ec, eu, z, tab, j, 0.0 if w is None else w, clip, dtype, mistake)
        out.append(x)
    return out


def text_drop_mask(seed, B, p):
    """True where sample b is DROPPED: not drop_keep at element index b."""
    return ~drop_ref.keep_flat(int(seed) & 0xFFFFFFFFFFFFFFFF, np.arange(B), float(F32(p)))


def text_cond_drop(text, null_text, seed, p):
    """psg_text_cond_drop_f32: (out [B, row], dropped int32 [B])."""
    text = np.asarray(text, dtype=F32)
    m = text_drop_mask(seed, text.shape[0], p)
    out = np.where(m[:, None], np.asarray(null_text, dtype=F32).reshape(1, -1), text.reshape(text.shape[0], -1)).astype(F32)
    return out.reshape(text.shape), m.astype(np.int32)
