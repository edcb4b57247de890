"""float64 references and derived error bounds for the row kernels of csrc/elementwise.hip: bilinear upsample (forward and
backward), psg_colsum, psg_sum_rows, psg_prep_weight, psg_epilogue_bwd and psg_dropout_apply (test infrastructure, not a
conftest).  tests/test_row_ref_cpu.py checks the references against torch and that each bound notices a subtly wrong result;
tests/test_row_kernels_gpu.py holds the kernels to them.

Every reference takes the operands the kernel really read (bf16 values widened exactly) and returns fp64 tensors on the
operands' own device.  Every bound is  r_out |ref| + depth 2^-24 S + A_FLOOR (+ extra)  with r_out the output rounding of
tests/gemm_ref.py (BF16_ROUND / F32_ROUND), S the sum of |term| over the terms of that element and `depth` the number of fp32
roundings a term can pass through in the kernel - derived per kernel below, never measured."""
import math

import numpy as np
import torch

from tests.gemm_ref import A_FLOOR, ACT_APPROX, BF16_ROUND, F32_ROUND
from tests import gemm_ref

U = 2.0 ** -24                 # unit roundoff of fp32 round-to-nearest
F32 = np.float32


# ----------------------------------------------------------------------------------------------------------- comparator
def check(got, ref, S, out_dtype, what, depth, extra=None, r_extra=0.0):
    """Assert |got - ref| <= r_out |ref| + depth 2^-24 S + extra + A_FLOOR element by element; return the worst err / bound.
    The sibling of gemm_ref.check for kernels that are no MFMA GEMM: `depth` (a number or a tensor of ref's shape) replaces
    c_acc(K).  The failure message is gemm_ref.check's."""
    r_out = (BF16_ROUND if out_dtype == torch.bfloat16 else F32_ROUND) + r_extra
    g = got.detach().to(device=ref.device, dtype=torch.float64)
    assert g.shape == ref.shape, f"{what}: shape {tuple(g.shape)} vs reference {tuple(ref.shape)}"
    bound = ref.abs() * r_out + S * depth * U + A_FLOOR
    if extra is not None:
        bound = bound + extra
    err = (g - ref).abs()
    ratio = err / bound
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)   # NaN in got: fails
    worst = float(ratio.max())
    if not worst <= 1.0:
        i = int(ratio.argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
        nbad = int((ratio > 1.0).sum())
        raise AssertionError(f"{what}: {nbad} of {ratio.numel()} elements out of bound; worst at {idx}: got {float(g.reshape(-1)[i]):.7g}, "
                             f"ref {float(ref.reshape(-1)[i]):.7g}, |err| {float(err.reshape(-1)[i]):.3g} > bound "
                             f"{float(bound.reshape(-1)[i]):.3g} (err/bound {worst:.3g}, depth {float(torch.as_tensor(depth).max()):g})")
    return worst


# ------------------------------------------------------------------------------------------------------------- upsample
def bilin_coord(n_in, n_out, ratio=None):
    """bilin_coord of elementwise.hip for every output index o, in numpy.float32 and in its order of operations:
    scale = fl(in / out); s = fl(fl(fl(o + 0.5) * scale) - 0.5) clamped at 0; i0 = min(int(s), in - 1); i1 = i0 + (i0 < in - 1);
    w1 = fl(s - i0).  ratio = (in', out'): take the scale from another axis (a planted mistake).  Returns (i0, i1, w1): int64,
    int64, float32 arrays [n_out].  (In exact arithmetic the coordinate differs from this one by about 1e-5 at 108 -> 215: a
    reference from the rational coordinate could not carry a useful bound.)"""
    o = np.arange(n_out, dtype=F32)
    scale = F32(n_in) / F32(n_out) if ratio is None else F32(ratio[0]) / F32(ratio[1])
    s = (o + F32(0.5)) * scale - F32(0.5)
    assert s.dtype == F32
    s = np.where(s < 0, F32(0), s)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    w1 = (s - i0.astype(F32)).astype(F32)
    return i0, i1, w1


def axis_weights(n_in, n_out, ratio=None):
    """The interpolation matrix of one axis, [n_out, n_in] fp64: row o holds 1 - w1 at i0 and w1 at i1 (added where i0 = i1),
    w1 the fp32 value of bilin_coord widened exactly; the subtraction 1 - w1 is taken in fp64."""
    i0, i1, w1 = bilin_coord(n_in, n_out, ratio)
    W = np.zeros((n_out, n_in), dtype=np.float64)
    o = np.arange(n_out)
    np.add.at(W, (o, i0), 1.0 - w1.astype(np.float64))
    np.add.at(W, (o, i1), w1.astype(np.float64))
    return W


def bwd_window(n_in, n_out):
    """The [lo, hi] window of output indices the backward kernels scan for every input index, restated in numpy.float32:
    lo = max(0, int(floorf(fl(fl(fl(fl(i - 1) + 0.5) * out) / in) - 0.5)) - 1), hi alike with i + 1, ceilf and + 1."""
    i = np.arange(n_in, dtype=F32)
    lo = np.floor((i - F32(1.0) + F32(0.5)) * F32(n_out) / F32(n_in) - F32(0.5)).astype(np.int64) - 1
    hi = np.ceil((i + F32(1.0) + F32(0.5)) * F32(n_out) / F32(n_in) - F32(0.5)).astype(np.int64) + 1
    return np.maximum(lo, 0), np.minimum(hi, n_out - 1)


def contributors(n_in, n_out):
    """Per input index the sorted output indices whose stencil touches it with a non-zero weight (what the backward sums)."""
    W = axis_weights(n_in, n_out)
    return [np.nonzero(W[:, i])[0] for i in range(n_in)]


def _t(W, like):
    return torch.from_numpy(W).to(like.device)


def upsample_fwd(x, Ho, Wo, Wh=None, Ww=None):
    """y[b, ho, wo, c] = sum_{hi, wi} Wh[ho, hi] Ww[wo, wi] x[b, hi, wi, c] in fp64, x [B, Hi, Wi, C] channels-last (any row
    stride).  Returns (y, S, n): S = the same sum over |x| (the weights are >= 0), n = 4, the terms the kernel adds.

    Bound (check(depth = n + 3)): the kernel forms a = fl(fl(1 - lh) * fl(1 - lw)) (3 roundings; the reference takes the same
    fp32 lh, lw but the product in fp64), then fl(v * a) per term and adds the 4 terms left to right: the first term passes
    through 1 + 3 = n roundings, so to first order |err| <= (n + 3) 2^-24 sum |a v| before the output rounding."""
    B, Hi, Wi, C = x.shape
    Wh = _t(axis_weights(Hi, Ho), x) if Wh is None else Wh
    Ww = _t(axis_weights(Wi, Wo), x) if Ww is None else Ww
    xd = x.detach().double()
    y = torch.einsum("oh,pw,bhwc->bopc", Wh, Ww, xd)
    S = torch.einsum("oh,pw,bhwc->bopc", Wh, Ww, xd.abs())
    return y, S, 4


def upsample_bwd(dy, Hi, Wi, Wh=None, Ww=None):
    """The transpose of upsample_fwd: dx[b, hi, wi, c] = sum_{ho, wo} Wh[ho, hi] Ww[wo, wi] dy[b, ho, wo, c] in fp64 (a scatter
    of the same weights).  Returns (dx, S, n): n [1, Hi, Wi, 1] = (contributing output rows) x (contributing output columns)
    of each input pixel, the number of terms the kernels add.

    Bound (check(depth = n + 3)): per term the kernel forms fl(wh * ww) with wh = fl(1 - lh) or lh (3 roundings at most, as in
    the forward; where i0 = i1 the kernel adds fl(fl(1 - l) + l), which the case table keeps exact, see
    tests/test_row_ref_cpu.py), fl(g * w), and adds the n terms in a fixed order: n + 3 roundings on the longest path."""
    B, Ho, Wo, C = dy.shape
    Wh = _t(axis_weights(Hi, Ho), dy) if Wh is None else Wh
    Ww = _t(axis_weights(Wi, Wo), dy) if Ww is None else Ww
    gd = dy.detach().double()
    dx = torch.einsum("oh,pw,bopc->bhwc", Wh, Ww, gd)
    S = torch.einsum("oh,pw,bopc->bhwc", Wh, Ww, gd.abs())
    n = ((Wh != 0).sum(0).reshape(1, Hi, 1, 1) * (Ww != 0).sum(0).reshape(1, 1, Wi, 1)).to(torch.float64)
    return dx, S, n


# --------------------------------------------------------------------------------------------------------------- colsum
def colsum_plan(R, groups, cols):
    """colsum_plan of elementwise.hip in integers: (splits, rows per split)."""
    cb = (cols + 63) // 64
    want = 2048 // (cb * groups)
    want = max(1, min(want, (R + 63) // 64, 256))
    rps = (R + want - 1) // want
    return (R + rps - 1) // rps, rps


def _tile_depth(n):
    """Longest chain of fp32 additions one input of an n-row colsum_tile passes through: row lane 0 holds m = ceil(n / 4) rows;
    m // 4 trips of the unrolled loop add one row each to a0..a3, the m % 4 left over go to a0, whose first row therefore
    passes m // 4 + m % 4 additions; then (a0 + a1) + (a2 + a3) and the LDS combine of the 4 row lanes, 2 each."""
    m = (n + 3) // 4
    return m // 4 + m % 4 + 4


def colsum_depth(R, splits, rps, accumulate=False):
    """`depth` of psg_colsum's fixed tree: one tile over R rows, or a stage-one tile over rps rows followed by a stage-two tile
    over the `splits` partials; + 1 for the addition onto the previous output.  (R 2^-24 S would be valid too, and useless: at
    R = 16 500 it is larger than one row.)"""
    d = _tile_depth(R) if splits == 1 else _tile_depth(rps) + _tile_depth(splits)
    return d + (1 if accumulate else 0)


def colsum(a, prev=None):
    """out[g, c] = sum_r a[g, r, c] (+ prev[g, c]) in fp64; S = sum |a| (+ |prev|).  a [groups, R, cols]."""
    ad = a.detach().double()
    ref, S = ad.sum(1), ad.abs().sum(1)
    if prev is not None:
        ref, S = ref + prev.double(), S + prev.double().abs()
    return ref, S


# ------------------------------------------------------------------------------------------------------------- sum_rows
def sum_rows_restated(a, b=None, c=None):
    """psg_sum_rows in torch on the CPU, bit for bit: the fp32 sum (a + b) + c rounded once to the operands' dtype; one
    source is a copy."""
    if b is None:
        return a.clone()
    v = a.float() + b.float()
    if c is not None:
        v = v + c.float()
    return v.to(a.dtype)


def sum_rows(a, b, c=None):
    """(ref, S) in fp64 of a + b (+ c); check(depth = 2): two fp32 additions."""
    ops = [t.detach().double() for t in (a, b, c) if t is not None]
    return sum(ops), sum(o.abs() for o in ops)


# ---------------------------------------------------------------------------------------------------------- prep_weight
def kpad(K, dtype):
    bk = 64 if dtype == torch.bfloat16 else 32
    return (K + bk - 1) // bk * bk


def prep_weight(w, dtype):
    """w: logical [O, I, k, k] (fp32 or bf16 values) -> (wf [O, kpad(taps I)], wd [I, kpad(taps O)]) in `dtype`, on the CPU:
    wf[o][tap * I + i] = wd[i][tap * O + o] = w[o, i, kh, kw] rounded once, tap = kh * k + kw, the K padding +0."""
    O, I, k, _ = w.shape
    q = w.to(dtype)
    wf = torch.zeros((O, kpad(k * k * I, dtype)), dtype=dtype)
    wd = torch.zeros((I, kpad(k * k * O, dtype)), dtype=dtype)
    wf[:, :k * k * I] = q.permute(0, 2, 3, 1).reshape(O, -1)
    wd[:, :k * k * O] = q.permute(1, 2, 3, 0).reshape(I, -1)
    return wf, wd


# -------------------------------------------------------------------------------------------- epilogue_bwd, dropout_apply
ACTS = {"none": 0, "silu": 1, "gelu": 2, "relu": 3, "tanh": 4, "quick_gelu": 5}       # enum psg_act
QUICK_GELU_C = gemm_ref.QUICK_GELU_C
# quick-GELU lives in tests/gemm_ref.py with the other activations (formula, derivative and its 2^-20 ACT_APPROX entry, which
# holds in dact_u's form - 4 ACT_APPROX relative + ACT_APPROX absolute; tests/test_row_ref_cpu.py evaluates the fp32 formula
# against fp64 over |u| <= 9); these names stay for the row tests.
ACT_APPROX_ROW = ACT_APPROX
act_grad = gemm_ref.act_grad


def p32(p):
    """The dropout rate the kernel sees: a C float."""
    return float(np.float32(p))


def keep_mask(seed, rows, cols, p):
    """Keep mask [rows, cols] of psg_dropout_apply / psg_epilogue_bwd: element (r, c) has index r * cols + c (the row stride
    does not enter)."""
    return gemm_ref.conv_keep_mask(seed, rows, cols, p32(p)) if p > 0 else torch.ones((rows, cols), dtype=torch.bool)


def keep_mask_rows(seed, rows_idx, cols, p):
    """keep_mask for the rows `rows_idx` (a 1-D integer tensor) of a wider launch: [len(rows_idx), cols]."""
    from tests.drop_ref import keep_flat
    idx = rows_idx.numpy().astype(np.uint64).reshape(-1, 1) * np.uint64(cols) + np.arange(cols, dtype=np.uint64).reshape(1, -1)
    return torch.from_numpy(keep_flat(seed, idx, p32(p)))


def epilogue_bwd(dy, u, kind, alpha, keep, p):
    """g = dy * alpha * keep / (1 - p) * act'(u) in fp64 (gemm_ref.epilogue_bwd, with quick-GELU and the C float p).
    Returns (ref, zero, depth, r_extra, extra) for check(S = |ref|): zero = the elements that are exactly 0 (dropped, or
    ReLU at u <= 0); depth = the fp32 roundings of a kept element: fl(dy * alpha), the scale fl(1 / fl(1 - p)) and its product
    when p > 0, the product with act'; r_extra / extra = dact_u's 4 ACT_APPROX relative and ACT_APPROX |dy alpha scale|
    absolute for the fp32 evaluation of act'."""
    p = p32(p)
    g0 = dy.detach().double() * alpha
    if p > 0:
        g0 = g0 * keep.to(g0.device).to(torch.float64) / (1.0 - p)
    ref = g0 if kind == "none" else g0 * act_grad(u.detach().double(), kind)
    zero = ~keep.to(g0.device) if p > 0 else torch.zeros_like(ref, dtype=torch.bool)
    if kind == "relu":
        zero = zero | (u <= 0)
    depth = 1 + (3 if p > 0 else 0) + (0 if kind == "none" else 1)
    A = ACT_APPROX_ROW[kind]
    return ref, zero, depth, 4.0 * A, A * g0.abs()


def dropout_apply(x, scale, keep):
    """y = keep ? fl(x * scale) : 0 -> (ref, depth = 1): one fp32 product before the output rounding; `scale` is a C float."""
    return x.detach().double() * float(np.float32(scale)) * keep.to(x.device).to(torch.float64), 1
