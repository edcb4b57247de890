"""References and derived bounds for the EMA that psg_adamw_dev_ema_f32 keeps in the optimizer's pass (test infrastructure,
not a conftest).  tests/test_ema_ref_cpu.py checks them against each other and against planted mistakes;
tests/test_ema_kernels_gpu.py and tests/test_ema_stepper_gpu.py hold the kernels to them.

The kernel (include/psg_hip.h), with p' the parameter value the AdamW update just computed and k = *step_dev + 1:

    d    = ema_decay                                        ema_warmup == 0
    d    = min(ema_decay, fl(fl(1 + k) / fl(10 + k)))       otherwise
    omd  = fl(1 - d)
    ema' = fl(fl(d ema) + fl(omd p'))

every operation rounded to nearest on its own (no FMA).  `ema_f32` restates that in numpy float32, rounding for rounding: the
kernel must give its bits.  `ema_f64` is the exact expression in fp64 with a bound in the style of tests/step_ref.py
(row_ref.check: r_out |ref| + depth 2^-24 S + extra + A_FLOOR):

  * 1 + k and 10 + k are integers below 2^24: exact.  The quotient rounds once, d^ = d (1 + dq), |dq| <= 2^-24, and `min` picks
    one of its operands: exact.  Without the warm-up, or where ema_decay is the smaller, d^ is the fp32 argument itself: dq = 0.
  * omd^ = fl(1 - d^) = (1 - d^)(1 + ds).  Against the exact 1 - d it is off by |d| |dq| absolutely and |ds| relatively.  The
    first is NOT small against 1 - d when d is close to 1 (0.9999: four decimal digits are gone), so it does not go into
    `depth`: it is its own term  extra = 2^-24 |d| |p'|, present only where the rounded quotient is the decay in use.
  * the two products round once each.  The term d ema passes dq and its product: 2 roundings.  The term (1 - d) p' passes ds
    and its product: 2 roundings (and the extra term above).  depth = 2 on S = |d ema| + |(1 - d) p'|.
  * the sum is the output rounding, r_out |ref| (row_ref.check's F32_ROUND), which also covers the second-order terms.

mistake= plants "k_off_by_one" (the warm-up from *step_dev instead of *step_dev + 1) and "swap" (d and 1 - d exchanged)."""
import numpy as np
import torch

from tests.row_ref import U, check  # noqa: F401
from tests.gemm_ref import A_FLOOR, F32_ROUND

F32 = np.float32
F64 = torch.float64
MISTAKES = ("k_off_by_one", "swap")


def f32(x):
    return float(F32(x))


def warmup_f32(k):
    """fl(fl(1 + k) / fl(10 + k)) as a numpy float32."""
    kf = F32(k)
    return F32(F32(F32(1) + kf) / F32(F32(10) + kf))


def decay_f32(ema_decay, warmup, k):
    """(d, fl(1 - d)) as numpy float32 scalars: the kernel's own values for the 1-based step k."""
    d = F32(ema_decay)
    if warmup:
        d = min(d, warmup_f32(k))
    return F32(d), F32(F32(1) - F32(d))


def decay_exact(ema_decay, warmup, k):
    """(d as a Python float in exact arithmetic on the fp32 argument, whether the warm-up's quotient is the one in use)."""
    d = f32(ema_decay)
    if warmup:
        w = (1.0 + k) / (10.0 + k)
        if w < d:
            return w, True
    return d, False


def ema_f32(ema, p_new, ema_decay, warmup, k):
    """The kernel's arithmetic on numpy float32 arrays, one rounding per operation.  Two fp32 torch tensors (any device: the
    640 M-element arenas stay on theirs) take torch's elementwise product and sum instead - one rounding each as well, the
    scalars being fp32 values already; tests/test_ema_ref_cpu.py holds the two forms to the same bits."""
    d, omd = decay_f32(ema_decay, warmup, k)
    if torch.is_tensor(ema):
        assert ema.dtype == p_new.dtype == torch.float32
        return ema * float(d) + p_new * float(omd)
    ema, p_new = np.asarray(ema, dtype=F32), np.asarray(p_new, dtype=F32)
    r = (d * ema).astype(F32) + (omd * p_new).astype(F32)
    assert r.dtype == F32
    return r


def ema_f64(ema, p_new, ema_decay, warmup, k, mistake=None):
    """-> (ref, S, depth, extra): fp64 tensors of ema's shape (depth a number); see the module docstring."""
    e, p = (torch.as_tensor(np.asarray(t)).detach().to(F64) if not torch.is_tensor(t) else t.detach().to(F64) for t in (ema, p_new))
    d, quotient = decay_exact(ema_decay, warmup, k - 1 if mistake == "k_off_by_one" else k)
    a, b = (1.0 - d, d) if mistake == "swap" else (d, 1.0 - d)
    t1, t2 = a * e, b * p
    extra = U * abs(d) * p.abs() if quotient else torch.zeros_like(p)
    return t1 + t2, t1.abs() + t2.abs(), 2, extra


def check_ema(got, ema, p_new, ema_decay, warmup, k, what):
    """got (fp32) against ema_f64's bound; returns the worst err / bound."""
    ref, S, depth, extra = ema_f64(ema, p_new, ema_decay, warmup, k)
    g = torch.as_tensor(np.asarray(got)) if not torch.is_tensor(got) else got
    return check(g, ref, S, torch.float32, what, depth, extra=extra)


def drift(ema0, p, ema_decay, warmup, steps, k0=1):
    """`steps` updates towards a constant p, the first at 1-based step k0 -> (ref, bound), fp64 tensors.
    ref is the exact recursion e_k = d_k e_{k-1} + (1 - d_k) p = p + (prod d_k)(e_0 - p).  The bound sums the per-step bound
    b_k of ema_f64 (at the exact e_{k-1}) geometrically: the kernel starts step k from e_{k-1} + E_{k-1}, and the error it
    inherits is multiplied by d^_k and rounded with the product and the sum, so
        E_k <= d_k (1 + 3 x 2^-24) E_{k-1} + b_k (1 + 3 x 2^-24),   E_0 = 0."""
    e = torch.as_tensor(np.asarray(ema0)).to(F64) if not torch.is_tensor(ema0) else ema0.detach().to(F64)
    p = torch.as_tensor(np.asarray(p)).to(F64) if not torch.is_tensor(p) else p.detach().to(F64)
    e0, E, prod = e.clone(), torch.zeros_like(e), 1.0
    for k in range(k0, k0 + steps):
        d, _ = decay_exact(ema_decay, warmup, k)
        ref, S, depth, extra = ema_f64(e, p, ema_decay, warmup, k)
        b = ref.abs() * F32_ROUND + S * depth * U + extra + A_FLOOR
        E = (d * E + b) * (1 + 3 * U)
        e, prod = ref, prod * d
    closed = p + prod * (e0 - p)
    assert torch.allclose(e, closed, rtol=1e-12, atol=1e-300), "the recursion and its closed form disagree"
    return e, E


def fold(ema0, masters, ema_decay, warmup, k0=1):
    """ema_f32 folded over a list of fp32 master snapshots (the p' of steps k0, k0 + 1, ...)."""
    e = ema0 if torch.is_tensor(ema0) else np.asarray(ema0, dtype=F32)
    for i, p in enumerate(masters):
        e = ema_f32(e, p, ema_decay, warmup, k0 + i)
    return e
