"""float64 references, per-element bounds and comparators for the row kernels of csrc/text_encoder.hip: psg_layernorm,
psg_layernorm_bwd, psg_bert_embed_ln, psg_bert_embed_ln_bwd and psg_embed_scatter (test infrastructure, not a conftest; the
style of tests/gn_ref.py and tests/row_ref.py, whose constants and comparators it shares).  tests/test_ln_ref_cpu.py checks
the references against torch, measures the constant and shows that every bound notices a subtly wrong result;
tests/test_ln_kernels_gpu.py holds the kernels to them on the cases of tests/ln_cases.py.

LayerNorm.  A row of width N is GroupNorm with B = rows, HW = 1, C = N, G = 1, so the reference is gn_ref.reference on the
operands as the kernel reads them: bf16 widened exactly, the residual added in fp32 first (one rounding, as the kernel's
v += t), eps as a C float.

  y, dz     |got - ref| <= r_out |ref| + C_LN 2^-24 M (+ extra) with gn_ref's M and extra (y: (|z| + |mu|) rstd |gamma| + |beta|;
            dz: rstd (|g| + |s1| + xa |s2|), extra the reduction terms of s1 and s2).  Nothing in it allows for the
            cancellation of a one-pass E[z^2] - mu^2: the kernel is two-pass and is held to that.  C_LN is not chosen but
            measured: C_TORCH is the smallest c at which torch's own fp32 F.layer_norm on the CPU (autograd backward; bf16
            operands pre-rounded, bf16 outputs rounded) passes every y and dz bound over the whole case table, and
            C_LN = 4 C_TORCH.  The margin covers the kernel's different but fixed summation order (8 CPL serial additions per
            lane, then a 6-level butterfly) and nothing else.  tests/golden/REPORT_text_rows.txt lists the measured values.
  dgamma,   row_ref.check with a depth counted from layernorm_bwd_kernel / ln_param_sum_kernel.  A term dy x_hat (dbeta: dy) is
  dbeta     added to a wave's register sum over LNB_RPW = 16 serial rows, meets the other waves in 3 LDS additions, is one of
            ceil(nwg / 4) workgroup partials a lane of ln_param_sum_kernel adds serially, and passes the 2 additions of
            (r0 + r1) + (r2 + r3):  D_SUM = 16 + 3 + ceil(nwg / 4) + 2.  dgamma's terms carry the product's rounding and the
            roundings of x_hat = (z - mean) rstd as well.  With D_STAT = 8 CPL + 6 + 1 (a lane's serial additions, the
            butterfly, the division by N): mean is off by at most D_STAT 2^-24 mean|z|, the subtraction rounds once, rstd is
            off by (D_STAT + 3) / 2 + 2 roundings relative (the centred sum, eps, the square root and the division; a mean
            that is off by d moves the centred sum by N d^2 only), the product with rstd rounds once:
            D_XHAT = 1.5 D_STAT + 5.5 roundings of size 2^-24 (|z| + mean|z|) rstd.  So
                dbeta   S = sum_rows |dy|,                             depth D_SUM
                dgamma  S = sum_rows |dy| (|z| + mean|z|) rstd,        depth D_SUM + 1 + D_XHAT
            and extra = F32_ROUND |prefill| for an accumulating launch.  (gn_ref's own dgamma / dbeta bound carries
            sqrt(max(1024, rows)) of the same sums and is one to two orders wider.)

Scatter.  table[k] (+)= sum of dz[perm[j]] over the sorted positions j with key[j] == k, in fp64; key == skip_key and keys
outside [0, V) add nothing.  A row is the sum of `run` terms (the length of its run of keys) in a fixed order: row_ref.check
with depth = run (+ 1 for the addition onto the prefill).  With integer-valued dz (|v| <= 64) every fp32 sum of a run of up
to 2^17 terms is exact, so the kernel must equal the reference bit for bit.

Embeddings.  embed_ref.embed_reference gives y, dz, dgamma, dbeta in fp64 from the tables; the magnitudes come from the fp32
rows z = (word[id] + type[tt]) + pos[s] the kernels form, and the extras grow by the first-order effect of those two
roundings on each output (embed_reference_bounds)."""
import types

import torch

from tests import gn_ref, row_ref
from tests.embed_ref import embed_reference

TWO24 = gn_ref.TWO24
LN_ROWS = 4                 # rows (waves) per workgroup of the forward
LNB_RPW = 16                # rows per wave of the backward
LNB_WG_ROWS = 64            # rows per workgroup of the backward
# largest smallest-passing c of torch's fp32 F.layer_norm over the case table (tests/test_ln_ref_cpu.py measures it; the
# per-output values are in tests/golden/REPORT_text_rows.txt)
C_TORCH = 4.7
C_LN = 4.0 * C_TORCH

OUTPUTS = ("y", "dz", "dgamma", "dbeta")
f32 = gn_ref.f32


def cpl(N):
    """16-byte chunks per lane: the CPL instantiation a width runs on."""
    return (N // 8 + 63) // 64


def nwg_bwd(rows):
    return (rows + LNB_WG_ROWS - 1) // LNB_WG_ROWS


def d_sum(rows):
    return LNB_RPW + 3 + (nwg_bwd(rows) + 3) // 4 + 2


def d_xhat(N):
    d_stat = 8 * cpl(N) + 6 + 1
    return 1.5 * d_stat + 5.5


def pre_add(x, r):
    """The row the statistics see: x (+ r, added in fp32 as the kernel adds it), in fp64."""
    z = x.detach().float()
    if r is not None:
        z = z + r.detach().float()
    return z.double()


def reference(x, r, gamma, beta, eps, dy=None, prefill=None):
    """fp64 LayerNorm forward (and, with dy, backward) of the rows x (+ r) [rows, N] in any strides, with magnitudes.
    Returns a namespace: y, dz, dgamma, dbeta (fp64), o_mag / o_extra for y and dz (check with C_LN), o_S / o_depth / o_extra
    for dgamma and dbeta (row_ref.check).  prefill: (dgamma0, dbeta0) of an accumulating launch.  Also .rstd and .xhat [rows, 1 / N]."""
    rows, N = x.shape
    z = pre_add(x, r)
    g = gn_ref.reference(z.view(rows, 1, N), gamma, beta, 1, eps, False, dy=None if dy is None else dy.detach().double().view(rows, 1, N),
                         prefill=prefill)
    o = types.SimpleNamespace(rows=rows, N=N)
    o.y, o.y_mag, o.y_extra = g.y.view(rows, N), g.y_mag.view(rows, N), None
    rstd = o.rstd = g.rstd.view(rows, 1)
    o.xhat = (z - g.mean.view(rows, 1)) * rstd
    if dy is None:
        return o
    o.dz, o.dz_mag, o.dz_extra = g.dx.view(rows, N), g.dx_mag.view(rows, N), g.dx_extra.view(rows, N)
    xa = (z.abs() + z.abs().mean(1, keepdim=True)) * rstd
    dyd = dy.detach().double()
    o.dgamma, o.dbeta = g.dgamma, g.dbeta
    o.dgamma_S, o.dbeta_S = (dyd.abs() * xa).sum(0), dyd.abs().sum(0)
    o.dbeta_depth = d_sum(rows)
    o.dgamma_depth = d_sum(rows) + 1 + d_xhat(N)
    o.dgamma_extra, o.dbeta_extra = g.dgamma_extra, g.dbeta_extra
    return o


def out_dtype(name, xd, od):
    """The type an output is stored in: y in the launch's output type, dz in x's, the parameter gradients in fp32."""
    return {"y": od, "dz": xd}.get(name, torch.float32)


def check(got, o, name, dtype, what, c=C_LN):
    """One output of `reference` against its bound; returns the worst err / bound."""
    ref = getattr(o, name)
    if name in ("y", "dz"):
        return gn_ref.check(got, ref, getattr(o, name + "_mag"), dtype, f"{what} {name}", extra=getattr(o, name + "_extra"), c=c)
    return row_ref.check(got, ref, getattr(o, name + "_S"), torch.float32, f"{what} {name}", getattr(o, name + "_depth"),
                         extra=getattr(o, name + "_extra"))


def check_all(got, o, xd, od, what, names=None, c=C_LN):
    """check() for every output in `got` (name -> tensor): name -> worst err / bound."""
    return {n: check(got[n], o, n, out_dtype(n, xd, od), what, c=c) for n in (names or [n for n in OUTPUTS if n in got])}


def smallest_c(got, o, name, dtype):
    return gn_ref.smallest_c(got, getattr(o, name), getattr(o, name + "_mag"), dtype, extra=getattr(o, name + "_extra"))


# --------------------------------------------------------------------------------------------------------------- scatter
def scatter_reference(dz, key, perm, V, skip_key, prefill=None):
    """fp64 index_add over (key, perm): (ref [V, N], S = the same sum over |dz| (+ |prefill|), run [V, 1] = terms per row,
    named [V] = rows some live key names).  dz [*, N] in any row stride."""
    N = dz.shape[1]
    live = (key >= 0) & (key < V) & (key != skip_key)
    k, src = key[live], dz.detach().double()[perm[live]]
    ref = torch.zeros(V, N, dtype=torch.float64, device=dz.device).index_add_(0, k, src)
    S = torch.zeros_like(ref).index_add_(0, k, src.abs())
    run = torch.bincount(k, minlength=V).to(torch.float64).view(V, 1)
    if prefill is not None:
        p = prefill.detach().double()
        ref, S = ref + p, S + p.abs()
    return ref, S, run, run.view(-1) > 0


def check_scatter(got, ref, S, run, accumulate, what):
    """The random-valued comparison: depth = the row's run length (+ 1 onto the prefill)."""
    return row_ref.check(got, ref, S, torch.float32, what, (run + (1.0 if accumulate else 0.0)).expand_as(ref))


def sums_exactly_in_fp32(dz, run_max):
    """Integer-valued dz whose every partial sum of run_max terms is below 2^24: each fp32 summation order is exact."""
    d = dz.detach().double()
    return bool((d == d.round()).all()) and float(d.abs().max()) * run_max < 2.0 ** 24


# ------------------------------------------------------------------------------------------------------------ embeddings
def embed_rows(ids, tt, word, pos, typ):
    """The fp32 rows z = (word[id] + type[tt]) + pos[s] in the kernels' association [B * S, N], ids clamped into the tables,
    and the mask of the rows whose ids are inside them."""
    B, S = ids.shape
    V, T = word.shape[0], typ.shape[0]
    tt = torch.zeros_like(ids) if tt is None else tt
    valid = ((ids >= 0) & (ids < V) & (tt >= 0) & (tt < T)).reshape(-1)
    z = (word.float()[ids.clamp(0, V - 1)] + typ.float()[tt.clamp(0, T - 1)]) + pos.float()[:S][None]
    return z.reshape(B * S, -1), valid


def embed_reference_bounds(ids, tt, word, pos, typ, gamma, beta, eps, dy, prefill=None):
    """embed_ref.embed_reference's y, dz, gamma, beta as a namespace `check` takes; .valid = the mask of the rows inside the
    tables (the cotangent of the others is zeroed).  The magnitudes come from `reference` on the fp32 rows; the extras grow by
    what the rows' own two roundings can do to each output, to first order: d_i <= 2 2^-24 (|word| + |type| + |pos|)_i moves
        x_hat_i   by at most  e_i = rstd (d_i + mean d) + |x_hat_i| rstd mean(|x_hat| d)
        y_i       by |gamma_i| e_i
        dz_i      by rstd mean(|x_hat| d) |dz_i| + rstd (e_i |s2| + |x_hat_i| mean(|g| e))      (g = dy gamma)
        dgamma    by sum_rows |dy| e."""
    B, S = ids.shape
    V, T = word.shape[0], typ.shape[0]
    z, valid = embed_rows(ids, tt, word, pos, typ)
    cot = dy.detach().double() * valid[:, None].double()
    o = reference(z, None, gamma, beta, eps, dy=cot, prefill=prefill)
    t0 = torch.zeros_like(ids) if tt is None else tt
    A = (word.double().abs()[ids.clamp(0, V - 1)] + typ.double().abs()[t0.clamp(0, T - 1)] + pos.double().abs()[:S][None]).reshape(B * S, -1)
    d = 2.0 * TWO24 * A
    xa, rstd = o.xhat.abs(), o.rstd
    m = (xa * d).mean(1, keepdim=True)
    e = rstd * (d + d.mean(1, keepdim=True)) + xa * rstd * m
    gd = gamma.detach().double()
    g = cot * gd
    s2 = (g * o.xhat).mean(1, keepdim=True)
    o.y_extra = gd.abs() * e
    o.dz_extra = o.dz_extra + rstd * m * o.dz.abs() + rstd * (e * s2.abs() + xa * (g.abs() * e).mean(1, keepdim=True))
    ge = (cot.abs() * e).sum(0)
    o.dgamma_extra = ge if o.dgamma_extra is None else o.dgamma_extra + ge
    r = embed_reference(ids, tt, word, pos, typ, gamma, beta, f32(eps), 0, dy)
    o.y, o.dz, o.dgamma, o.dbeta = r["y"], r["dz"], r["gamma"], r["beta"]
    if prefill is not None:
        o.dgamma, o.dbeta = o.dgamma + prefill[0].double(), o.dbeta + prefill[1].double()
    o.valid = valid
    return o


def worst(table, key, ratio):
    table[key] = max(table.get(key, 0.0), float(ratio))
    return ratio

