"""float64 reference of GroupNorm (+SiLU) forward / backward on channels-last [B, HW, C] and a per-element error bound for
every output of the launches: y, mean, rstd, dx, dgamma, dbeta (test infrastructure, not a conftest; the style of
tests/gemm_ref.py, whose constants it shares).

The reference takes the operands as the kernel read them (bf16-representable x / dy / dres for a bf16 launch, fp32 gamma /
beta / eps) in any row stride, and computes per (sample, group) in fp64

    mu, var (biased), rstd = 1 / sqrt(var + eps)          xhat = (x - mu) rstd
    y  = [silu](xhat gamma + beta)                        dz = dy [silu'](xhat gamma + beta)
    dx = rstd (dz gamma - s1 - xhat s2) + dres            s1 = mean_g(dz gamma), s2 = mean_g(dz gamma xhat)
    dgamma = sum_{b,hw} dz xhat (+ prefill)               dbeta = sum_{b,hw} dz (+ prefill)

Every bound has one shape:  |got - ref| <= r_out |ref| + C_GN 2^-24 M (+ extra),  r_out the output's own rounding
(gemm_ref.BF16_ROUND / F32_ROUND) and M the sum of the absolute values of the terms that are added to form the output:

    y       M = ACT_SLOPE (|x| + |mu|) rstd |gamma| + |beta|; the |mu| term admits the folded form x sc + sh the kernels use
            (sh = beta - mu sc is as large as the product it cancels); extra = ACT_APPROX (|y| + |z|) for the bf16 fast SiLU
    mean    M = mean_g |x|
    rstd    relative: |got / ref - 1| <= F32_ROUND + C_GN 2^-24 (1 + E[x^2] / (var + eps)) - the cancellation of the split
            route's E[x^2] - mu^2
    dx      M = rstd (|dz gamma| + |s1| + xa |s2|) + |dres| with xa = (|x| + |mu|) rstd for |xhat|; s1 and s2 carry the
            reduction terms e1 = c_acc(n) mean_g |dz gamma|, e2 = c_acc(n) mean_g (|dz gamma| xa), n = HW Cg:
            extra = rstd (e1 + xa e2)   (gemm_ref.c_acc(n) = 2^-24 sqrt(max(1024, n)))
    dgamma  M = sqrt(max(1024, B HW)) sum |dz| xa,  dbeta: M = sqrt(max(1024, B HW)) sum |dz|;  extra = F32_ROUND |prefill|

C_GN is not chosen but measured (tests/test_gn_ref_cpu.py::test_c_gn_is_four_times_torchs_own_error): over every case of
tests/gn_cases.py the smallest c at which torch's own fp32 F.group_norm (+ F.silu, autograd backward; for bf16 the same
on pre-rounded inputs, y and dx rounded to bf16) passes each bound against this reference is C_TORCH; C_GN = 4 C_TORCH,
one value for all outputs.  The margin covers the kernels' different but fixed summation order and their one extra folding
step, nothing else.  tests/golden/REPORT_groupnorm_routes.txt lists the measured values per output.
"""
import math
import types

import torch

from tests.gemm_ref import A_FLOOR, ACT_APPROX, ACT_SLOPE, BF16_ROUND, F32_ROUND, act, act_grad, c_acc

TWO24 = 2.0 ** -24
# largest smallest-passing c of torch's fp32 restatement over the case table (y of an fp32 case; see the report)
C_TORCH = 1.69
C_GN = 4.0 * C_TORCH

OUTPUTS = ("y", "mean", "rstd", "dx", "dgamma", "dbeta")


def _sq(n):
    return c_acc(n) / TWO24


def f32(v):
    """A Python float as the launch receives it (c_float)."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def reference(x, gamma, beta, G, eps, silu, dy=None, dres=None, prefill=None, bf16=False):
    """fp64 reference and magnitudes.  x, dy, dres: [B, HW, C] (any strides); gamma, beta: [C]; prefill: (dgamma0, dbeta0) of
    an accumulating launch or None.  Returns a namespace with, per output name o of OUTPUTS, o (fp64), o_mag (M above; for
    rstd already times |rstd|) and o_extra (absolute term or None).  Backward outputs only with dy."""
    B, HW, C = x.shape
    Cg = C // G
    kind = "silu" if silu else "none"
    eps = f32(eps)
    X = x.detach().double().reshape(B, HW, G, Cg)
    g = gamma.detach().double().reshape(1, 1, G, Cg)
    b = beta.detach().double().reshape(1, 1, G, Cg)
    mu = X.mean((1, 3), keepdim=True)
    var = ((X - mu) ** 2).mean((1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (X - mu) * rstd
    xa = (X.abs() + mu.abs()) * rstd
    z = xh * g + b
    y = act(z, kind)
    r = types.SimpleNamespace(B=B, HW=HW, C=C, G=G)
    r.y = y.reshape(B, HW, C)
    r.y_mag = (ACT_SLOPE[kind] * xa * g.abs() + b.abs()).reshape(B, HW, C)
    r.y_extra = (ACT_APPROX[kind] * (y.abs() + z.abs())).reshape(B, HW, C) if (bf16 and silu) else None
    r.mean = mu.reshape(B, G)
    r.mean_mag = X.abs().mean((1, 3))
    r.mean_extra = None
    r.rstd = rstd.reshape(B, G)
    r.rstd_mag = r.rstd * (1.0 + (X ** 2).mean((1, 3)) / (var.reshape(B, G) + eps))
    r.rstd_extra = None
    if dy is None:
        return r
    dz = dy.detach().double().reshape(B, HW, G, Cg)
    if silu:
        dz = dz * act_grad(z, kind)
    t = dz * g
    ta = t.abs()
    n = HW * Cg
    s1 = t.mean((1, 3), keepdim=True)
    s2 = (t * xh).mean((1, 3), keepdim=True)
    e1 = c_acc(n) * ta.mean((1, 3), keepdim=True)
    e2 = c_acc(n) * (ta * xa).mean((1, 3), keepdim=True)
    dx = rstd * (t - s1 - xh * s2)
    mag = rstd * (ta + s1.abs() + xa * s2.abs())
    red = rstd * (e1 + xa * e2)
    dx, mag, red = dx.reshape(B, HW, C), mag.reshape(B, HW, C), red.reshape(B, HW, C)
    if dres is not None:
        dr = dres.detach().double()
        dx, mag = dx + dr, mag + dr.abs()
    r.dx, r.dx_mag, r.dx_extra = dx, mag, red
    r.dgamma = (dz * xh).sum((0, 1)).reshape(C)
    r.dgamma_mag = _sq(B * HW) * (dz.abs() * xa).sum((0, 1)).reshape(C)
    r.dbeta = dz.sum((0, 1)).reshape(C)
    r.dbeta_mag = _sq(B * HW) * dz.abs().sum((0, 1)).reshape(C)
    r.dgamma_extra = r.dbeta_extra = None
    if prefill is not None:
        pg, pb = prefill[0].detach().double(), prefill[1].detach().double()
        r.dgamma, r.dbeta = r.dgamma + pg, r.dbeta + pb
        r.dgamma_extra, r.dbeta_extra = F32_ROUND * pg.abs(), F32_ROUND * pb.abs()
    return r


def _parts(got, ref, out_dtype, extra):
    g = got.detach().to(device=ref.device, dtype=torch.float64)
    assert g.shape == ref.shape, f"shape {tuple(g.shape)} vs reference {tuple(ref.shape)}"
    fixed = ref.abs() * (BF16_ROUND if out_dtype == torch.bfloat16 else F32_ROUND) + A_FLOOR
    if extra is not None:
        fixed = fixed + extra
    return g, (g - ref).abs(), fixed


def check(got, ref, mag, out_dtype, what, extra=None, c=C_GN):
    """Assert |got - ref| <= r_out |ref| + c 2^-24 mag + extra + A_FLOOR for every element; return the worst err / bound.
    A NaN in got fails.  The message names the worst element."""
    g, err, fixed = _parts(got, ref, out_dtype, extra)
    bound = fixed + c * TWO24 * mag
    ratio = err / bound
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    worst = float(ratio.max())
    if not worst <= 1.0:
        i = int(ratio.argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
        nbad = int((ratio > 1.0).sum())
        raise AssertionError(f"{what}: {nbad} of {ratio.numel()} elements out of bound; worst at {idx}: got {float(g.reshape(-1)[i]):.9g}, "
                             f"ref {float(ref.reshape(-1)[i]):.9g}, |err| {float(err.reshape(-1)[i]):.3g} > bound "
                             f"{float(bound.reshape(-1)[i]):.3g} (err/bound {worst:.3g})")
    return worst


def smallest_c(got, ref, mag, out_dtype, extra=None):
    """The smallest c at which check() passes: max over the elements of (err - r_out |ref| - extra - A_FLOOR) / (2^-24 mag)."""
    _, err, fixed = _parts(got, ref, out_dtype, extra)
    over = (err - fixed).clamp_min(0.0)
    c = torch.where(over > 0, over / (TWO24 * mag), torch.zeros_like(over))
    c = torch.where(torch.isnan(c), torch.full_like(c, math.inf), c)
    return float(c.max())


def out_dtype(name, dtype):
    """The type an output is stored in: y and dx in the launch's, the statistics and parameter gradients in fp32."""
    return dtype if name in ("y", "dx") else torch.float32


def check_all(got, r, dtype, what, names=None, c=C_GN):
    """check() for every output in `got` (a dict name -> tensor); returns name -> worst err / bound."""
    res = {}
    for name in (names or [n for n in OUTPUTS if n in got]):
        res[name] = check(got[name], getattr(r, name), getattr(r, name + "_mag"), out_dtype(name, dtype), f"{what} {name}",
                          extra=getattr(r, name + "_extra"), c=c)
    return res
