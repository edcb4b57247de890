"""float64 references for the GEMM-family launches (conv / Linear forward, data gradient, weight gradient) and an error
bound that is tight enough to notice a kernel that is subtly wrong (test infrastructure, not a conftest).

Every reference is a chunked im2col GEMM in float64 with torch on the tensors' own device, and returns the pair
(ref, S): the exact result of the operation on the operands it was given, and S = sum |a * b| over the same products
(|A| . |B|), which scales the accumulation error of the kernel under test.  Activations are channels-last
([B, H, W, C] or [..., C], any uniform row stride: concat-slot halves, ldx != Cin); weights are logical OIHW / [O, I]
whatever their memory order.  Inputs are used as they are: give the references the operands the kernel really read
(bf16 activations, bf16-representable weights), and nothing but the kernel's own arithmetic is left to bound.
"""
import math

import torch
import torch.nn.functional as F

# (samples per chunk) x (rows x K) of the largest fp64 im2col buffer; with its |.| twin and the products this keeps every
# fp64 buffer of a chunk below ~2 GB
CHUNK_BYTES = 1 << 29

BF16_ROUND = 2.0 ** -8        # |round(v) - v| <= 2^-8 |v| for bf16 round-to-nearest (8 significant bits)
F32_ROUND = 4 * 2.0 ** -24    # fp32 outputs: the final rounding plus the epilogue's own fp32 operations
A_FLOOR = 2.0 ** -126         # smallest normal fp32 / bf16: values below it carry no relative precision
# largest |d act / du| over the reals: what an accumulator error can become after the activation
# (quick-GELU x sigmoid(c x), c = 1.702, is SiLU on a scaled argument: d/dx = silu'(c x), the same largest slope; the second
# derivative is c silu''(c x), c times SiLU's curvature.)
QUICK_GELU_C = 1.702
ACT_SLOPE = {"none": 1.0, "silu": 1.0998, "gelu": 1.1289, "relu": 1.0, "tanh": 1.0, "quick_gelu": 1.0998}
# The kernels' activations are not the exact functions: bf16 launches use __expf / rcp SiLU and an erf by Abramowitz-Stegun
# 7.1.26 (|erf error| <= 1.5e-7).  Relative to the activation's value both stay below 2^-20, except GELU near its zero at
# u = 0 where the erf error enters as 0.5 |u| 1.5e-7; the bound adds ACT_APPROX * |u| for that.
# ReLU is fmaxf(x, 0): exact.  tanh is the math library's tanhf on both paths, specified to 5 ulp (OpenCL C 7.4; the HIP
# table lists 2): 5 * 2^-24 < 2^-21 relative to |tanh u| <= |u|; its derivative is 1 - t * t of that value (act_grad /
# act_both in psg_common.h), an absolute 2 |t| |dt| + 2^-24 <= 11 * 2^-24 < 2^-20.  tests/test_conv_ref_cpu.py evaluates
# the psg_common.h formulas in fp32 against fp64 and checks both against these entries.
# quick-GELU (psg_common.h quick_gelu_f / quick_gelu_grad: the exact-fp32 sigmoid of SiLU and one more fp32 product 1.702 x,
# whose rounding moves s by at most s (1 - s) |1.702 x| 2^-24) keeps SiLU's 2^-20 in every form
# (tests/test_row_ref_cpu.py::test_quick_gelu_act_approx_holds_for_the_fp32_formula and tests/test_conv_ref_cpu.py).
ACT_APPROX = {"none": 0.0, "silu": 2.0 ** -20, "gelu": 2.0 ** -20, "relu": 0.0, "tanh": 2.0 ** -21, "quick_gelu": 2.0 ** -20}
# largest |d^2 act / du^2| over the reals: what an accumulator error can become in a saved derivative act'(u).  (ReLU's
# derivative is a step: see saved_dact.)
ACT_CURV = {"none": 0.0, "silu": 0.5, "gelu": 0.7979, "relu": 0.0, "tanh": 0.7699, "quick_gelu": QUICK_GELU_C * 0.5}
# fp32 launches were not part of the measurement behind c_acc(): tests/test_conv_ref_cpu.py holds torch's own fp32 conv2d /
# conv_transpose2d / linear of every fp32 case of tests/conv_cases.py against check()'s bound, requires it to lie inside
# (else the bound would be widened for fp32 alone, by four times the factor torch needs) and writes the worst ratio it
# measured into tests/golden/REPORT_conv_routes.txt.  It lies inside, so fp32 cases use check() unwidened.


def c_acc(K):
    """Accumulation-error factor of an fp32-accumulating MFMA GEMM over K products: |err| <= c_acc(K) * sum|a*b|.

    Each 16x16xk MFMA step adds an exact-product block to an fp32 accumulator; a step's rounding is at most 2^-24 of the
    running sum, and the running sums are bounded by S.  Rounding errors of random sign add up like a random walk, so the
    observed error grows like sqrt(K): cdna_hip_programming.md ("FP32-input MFMA") measures max |err| ~ 1.5e-7 * S for
    K <= 1024 and 3.5e-7 * S at K = 4096, i.e. about 0.08 * 2^-24 * sqrt(K) * S.  We take 2^-24 * sqrt(K), floored at
    K = 1024: 12x the guide's figure at K <= 1024, 11x at 4096.  Measured on the bf16 kernels by the batch-256 table
    (tests/test_gemm_b256_gpu.py): the fp32 weight gradients, where this term is the whole bound, use at most 6 % of it
    (M = 256) and 0.1 % at M = 186 624 (split over fp32 partials); the bf16 outputs up to K = 23 040 reach 0.95-0.995 of
    their bound, nearly all of it their own rounding (2^-8 |ref|).  The bound stays meaningful: one 16-channel K slice
    missing at K = 11 520 is an error of ~4 sigma_a sigma_b per element while c_acc * S is ~0.05 sigma_a sigma_b
    (tests/test_gemm_ref_cpu.py)."""
    return 2.0 ** -24 * math.sqrt(max(1024.0, float(K)))


# ---------------------------------------------------------------------------------------------------------------- GEMMs
def _geom(H, W, ks, stride, pad=None):
    pad = ks // 2 if pad is None else pad
    return pad, (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1


def _nb(B, per_sample_elems):
    return max(1, min(B, CHUNK_BYTES // max(1, per_sample_elems * 8)))


def _cols(xb, ks, stride, pad):
    """[nb, C, H, W] fp64 -> im2col [nb, C*ks*ks, L] with k = (c, kh, kw): the order of OIHW weight.reshape(O, -1)."""
    if ks == 1 and stride == 1:
        return xb.reshape(xb.shape[0], xb.shape[1], -1)
    return F.unfold(xb, ks, padding=pad, stride=stride)


def conv_fwd(x, w, stride=1, pad=None):
    """y[b, ho, wo, o] = sum_{c, kh, kw} x[b, ho*s + kh - p, wo*s + kw - p, c] w[o, c, kh, kw]; pad None: ks // 2 (3x3 pad 1,
    1x1 pad 0), explicit for the 4x4 stride-2 convs (pad 1 or 2).  x [B, H, W, C] channels-last, any H x W, w [O, C, ks, ks].
    Returns (y, S) in fp64, [B, Ho, Wo, O]."""
    B, H, W_, C = x.shape
    O, ks = w.shape[0], w.shape[2]
    pad, Ho, Wo = _geom(H, W_, ks, stride, pad)
    wm = w.detach().double().reshape(O, -1)
    wa = wm.abs()
    y = torch.empty((B, Ho, Wo, O), dtype=torch.float64, device=x.device)
    S = torch.empty_like(y)
    nb = _nb(B, Ho * Wo * C * ks * ks)
    for b0 in range(0, B, nb):
        b1 = min(B, b0 + nb)
        cols = _cols(x[b0:b1].detach().permute(0, 3, 1, 2).double(), ks, stride, pad)
        y[b0:b1] = torch.matmul(wm, cols).transpose(1, 2).reshape(b1 - b0, Ho, Wo, O)
        S[b0:b1] = torch.matmul(wa, cols.abs()).transpose(1, 2).reshape(b1 - b0, Ho, Wo, O)
        del cols
    return y, S


def conv_dgrad(g, w, in_hw, stride=1, pad=None):
    """Data gradient dx = d(sum y * g)/dx of conv_fwd: the transposed conv of g [B, Ho, Wo, O] (any row stride) with
    w [O, C, ks, ks], onto the input grid in_hw = (H, W), square or not; 1x1 stride 2 leaves the odd positions zero.
    Returns (dx, S) in fp64, [B, H, W, C]."""
    B, Ho, Wo, O = g.shape
    C, ks = w.shape[1], w.shape[2]
    H, W_ = in_hw
    pad = ks // 2 if pad is None else pad
    assert (Ho, Wo) == _geom(H, W_, ks, stride, pad)[1:], "gradient grid inconsistent with the input grid"
    wt = w.detach().double().reshape(O, -1).t()
    wa = wt.abs()
    dx = torch.empty((B, H, W_, C), dtype=torch.float64, device=g.device)
    S = torch.empty_like(dx)
    nb = _nb(B, Ho * Wo * C * ks * ks)
    for b0 in range(0, B, nb):
        b1 = min(B, b0 + nb)
        gb = g[b0:b1].detach().double().reshape(b1 - b0, Ho * Wo, O).transpose(1, 2)      # [nb, O, L]
        for dst, a, gg in ((dx, wt, gb), (S, wa, gb.abs())):
            cols = torch.matmul(a, gg)                                                      # [nb, C*ks*ks, L]
            if ks == 1 and stride == 1:
                r = cols.reshape(b1 - b0, C, H, W_)
            else:
                r = F.fold(cols, (H, W_), ks, padding=pad, stride=stride)
            dst[b0:b1] = r.permute(0, 2, 3, 1)
            del cols, r
    return dx, S


def conv_wgrad(x, g, ks, stride=1):
    """Weight gradient dw[o, c, kh, kw] = sum_{b, ho, wo} g[b, ho, wo, o] x[b, ho*s + kh - p, wo*s + kw - p, c].
    x [B, H, W, C], g [B, Ho, Wo, O] (any row strides).  Returns (dw, S) in fp64, [O, C, ks, ks]."""
    B, H, W_, C = x.shape
    O = g.shape[-1]
    pad, Ho, Wo = _geom(H, W_, ks, stride)
    K = C * ks * ks
    dw = torch.zeros((O, K), dtype=torch.float64, device=x.device)
    S = torch.zeros_like(dw)
    nb = _nb(B, Ho * Wo * K)
    for b0 in range(0, B, nb):
        b1 = min(B, b0 + nb)
        cols = _cols(x[b0:b1].detach().permute(0, 3, 1, 2).double(), ks, stride, pad)      # [nb, K, L]
        cols = cols.transpose(1, 2).reshape(-1, K)                                          # [nb*L, K]
        gb = g[b0:b1].detach().double().reshape(-1, O)                                      # [nb*L, O]
        dw += gb.t() @ cols
        S += gb.abs().t() @ cols.abs()
        del cols, gb
    return dw.reshape(O, C, ks, ks), S.reshape(O, C, ks, ks)


def linear_fwd(x, w):
    """y = x . w^T over the rows of x [..., I] (any uniform row stride), w [O, I].  Returns (y, S) in fp64, [..., O]."""
    I, O = x.shape[-1], w.shape[0]
    xr = x.detach().reshape(-1, I)
    wt = w.detach().double().t()
    wa = wt.abs()
    y = torch.empty((xr.shape[0], O), dtype=torch.float64, device=x.device)
    S = torch.empty_like(y)
    n = _nb(xr.shape[0], max(I, O))
    for r0 in range(0, xr.shape[0], n):
        xb = xr[r0:r0 + n].double()
        y[r0:r0 + n] = xb @ wt
        S[r0:r0 + n] = xb.abs() @ wa
    return y.reshape(tuple(x.shape[:-1]) + (O,)), S.reshape(tuple(x.shape[:-1]) + (O,))


def linear_dgrad(g, w):
    """dx = g . w for g [..., O], w [O, I].  Returns (dx, S) in fp64, [..., I]."""
    return linear_fwd(g, w.detach().t())


def linear_wgrad(x, g):
    """dw = g^T . x summed over all rows: x [..., I], g [..., O].  Returns (dw, S) in fp64, [O, I]."""
    I, O = x.shape[-1], g.shape[-1]
    xr, gr = x.detach().reshape(-1, I), g.detach().reshape(-1, O)
    dw = torch.zeros((O, I), dtype=torch.float64, device=x.device)
    S = torch.zeros_like(dw)
    n = _nb(xr.shape[0], I + O)
    for r0 in range(0, xr.shape[0], n):
        xb, gb = xr[r0:r0 + n].double(), gr[r0:r0 + n].double()
        dw += gb.t() @ xb
        S += gb.abs().t() @ xb.abs()
    return dw, S


def bias_grad(g):
    """Column sums of g [..., O] over all rows: (db, S = sum |g|) in fp64, [O]."""
    gr = g.detach().reshape(-1, g.shape[-1]).double()
    return gr.sum(0), gr.abs().sum(0)


def rowadd_grad(g):
    """Per-sample column sums of g [B, ..., O]: the gradient of a per-sample row-add.  (dra, S) in fp64, [B, O]."""
    gr = g.detach().reshape(g.shape[0], -1, g.shape[-1]).double()
    return gr.sum(1), gr.abs().sum(1)


# ------------------------------------------------------------------------------------------------------------ epilogues
def _f64(t):
    return None if t is None else t.detach().double()


def act(u, kind):
    """The activation in fp64: none, SiLU, GELU in its erf form (nn.GELU()), ReLU, tanh or quick-GELU x sigmoid(1.702 x)."""
    if kind == "none":
        return u
    if kind == "relu":
        return torch.clamp(u, min=0.0)
    if kind == "tanh":
        return torch.tanh(u)
    if kind == "silu":
        return u * torch.sigmoid(u)
    if kind == "gelu":
        return 0.5 * u * (1.0 + torch.erf(u * (1.0 / math.sqrt(2.0))))
    if kind == "quick_gelu":
        return u * torch.sigmoid(QUICK_GELU_C * u)
    raise ValueError(kind)


def act_grad(u, kind):
    """d act / du in fp64 (ReLU: 1 for u > 0, else 0, as the kernels define it at 0)."""
    if kind == "none":
        return torch.ones_like(u)
    if kind == "relu":
        return (u > 0).to(u.dtype)
    if kind == "tanh":
        return 1.0 - torch.tanh(u) ** 2
    if kind == "silu":
        s = torch.sigmoid(u)
        return s * (1.0 + u * (1.0 - s))
    if kind == "gelu":
        return 0.5 * (1.0 + torch.erf(u * (1.0 / math.sqrt(2.0)))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    if kind == "quick_gelu":
        s = torch.sigmoid(QUICK_GELU_C * u)
        return s * (1.0 + QUICK_GELU_C * u * (1.0 - s))
    raise ValueError(kind)


def epilogue(acc, S, bias=None, rowadd=None, residual=None, kind="none", alpha=1.0, keep=None, p=0.0):
    """y = residual + alpha * drop(act(acc + bias + rowadd[b])) in fp64 - the fused forward epilogue of psg_conv_fwd.

    acc, S: a reference GEMM's (result, sum |a*b|), [B, ..., O]; bias [O]; rowadd [B, O] (one row per sample); residual of
    acc's shape; keep: the dropout keep mask (bool, acc's shape) with rate p, kept values scaled by 1 / (1 - p).
    Returns (y, S_y, A_y): S_y carries what an accumulator or epilogue rounding can become at the output (the activation's
    largest slope, the dropout scale, alpha, plus |bias|, |rowadd| and |residual|, whose fp32 additions round like the
    accumulator's); A_y = ACT_APPROX * |u| * ... for the activation approximation (see check's `extra`)."""
    u = acc.clone()
    Su = S.clone()
    if bias is not None:
        b = _f64(bias)
        u += b
        Su += b.abs()
    if rowadd is not None:
        ra = _f64(rowadd)
        shape = (ra.shape[0],) + (1,) * (acc.dim() - 2) + (ra.shape[1],)
        u += ra.reshape(shape)
        Su += ra.abs().reshape(shape)
    y = act(u, kind)
    slope = ACT_SLOPE[kind]
    A = ACT_APPROX[kind] * (y.abs() + u.abs())
    if keep is not None:
        sc = 1.0 / (1.0 - p)
        m = keep.to(torch.float64) * sc
        y, A = y * m, A * m
        Sy = Su * (slope * m)
    else:
        Sy = Su * slope
    y, Sy, A = y * alpha, Sy * abs(alpha), A * abs(alpha)
    if residual is not None:
        r = _f64(residual)
        y = y + r
        Sy = Sy + r.abs()
    return y, Sy, A


def epilogue_bwd(dy, u, kind="none", alpha=1.0, keep=None, p=0.0):
    """The gradient at the accumulator of an epilogue: g = dy * alpha * drop'(.) * act'(u) in fp64 (psg_epilogue_bwd).
    With u = None the activation's factor is 1."""
    g = _f64(dy) * alpha
    if keep is not None:
        g = g * keep.to(torch.float64) / (1.0 - p)
    if u is not None and kind != "none":
        g = g * act_grad(_f64(u), kind)
    return g


def dact_mul(acc, S, dact):
    """The FFN's DACT_MUL data-gradient form (ops.py, _FFNFn.backward): the accumulator times the saved derivative
    (gelu'(u) * keep / (1 - p), one value per element).  Returns (ref, S): an accumulator error is scaled by |dact| too."""
    d = _f64(dact)
    return acc * d, S * d.abs()


def dact_u(acc, S, u, kind):
    """The backward form without DACT_MUL: the accumulator times act'(saved u), u as the kernel read it (bf16 or fp32, used
    exactly).  Returns (ref, S, r_extra): the kernel evaluates act' in fp32 by the psg_common.h formulas, a relative
    4 ACT_APPROX of a derivative that is not near zero - and an absolute ACT_APPROX |acc| where it is (tanh' and GELU'
    cancel there), which the caller adds as `extra` = ACT_APPROX[kind] * |acc|."""
    d = act_grad(_f64(u), kind)
    return acc * d, S * d.abs(), 4.0 * ACT_APPROX[kind]


def saved_dact(u, Su, kind, keep=None, p=0.0):
    """What PSG_CONV_SAVE_DACT stores in `preact`: act'(u) * keep / (1 - p) in fp64, u = acc + bias + rowadd.  Returns
    (ref, S, extra) for check(): an accumulator error moves act'(u) by at most ACT_CURV times itself, the approximation of
    act' is absolute ((|u| + 1) ACT_APPROX, as for GELU in the batch-256 table).  ReLU's derivative is a step at 0: an
    element whose |u| lies within its own accumulator bound may take either side, so it gets extra = 1 there
    (tests/test_conv_ref_cpu.py::test_relu_and_tanh_cases_exercise_the_activation bounds their number per case)."""
    sc = 1.0 if keep is None else 1.0 / (1.0 - p)
    m = sc if keep is None else keep.to(torch.float64) * sc
    ref = act_grad(u, kind) * m
    extra = (u.abs() + 1.0) * ACT_APPROX[kind] * m
    if kind == "relu":
        extra = extra + (u.abs() <= Su * 2.0 ** -19).to(torch.float64) * m
    return ref, Su * ACT_CURV[kind] * m, extra


def conv_keep_mask(seed, M, N, p):
    """Keep mask [M, N] (bool tensor) of a psg_conv_fwd epilogue: element (m, n) has index m * N + n with m the ROW OF y
    (not of the tile, the class or the parity grid) and N = Cout; tests/drop_ref.py restates the hash in integers."""
    import numpy as np
    from tests.drop_ref import keep_flat
    idx = np.arange(M, dtype=np.uint64).reshape(M, 1) * np.uint64(N) + np.arange(N, dtype=np.uint64).reshape(1, N)
    return torch.from_numpy(keep_flat(seed, idx, p))


# ----------------------------------------------------------------------------------------------------------- comparator
def check(got, ref, S, out_dtype, what, K, extra=None, r_extra=0.0):
    """Assert |got - ref| <= r_out |ref| + c_acc(K) S + extra + A_FLOOR element by element; return the worst err / bound.

    r_out   rounding of the output: 2^-8 for bf16 outputs (round to nearest, 8 significant bits), 4 fp32 ulps for fp32
            outputs (the final rounding plus the epilogue's fp32 operations); `r_extra` adds a relative term, e.g. for a
            saved activation derivative the kernel rounded to bf16 before using it.
    c_acc   fp32 accumulation over K products, times S = sum |a*b| (see c_acc()).  Callers fold epilogue slopes, |bias|,
            |rowadd| and |residual| into S (epilogue()).
    extra   an absolute per-element term the caller derives, e.g. the activation approximation (epilogue()'s A).
    A_FLOOR the smallest normal float: below it nothing is relative.
    On failure the message names the worst element: its index, got, ref and bound, and how many elements failed."""
    r_out = (BF16_ROUND if out_dtype == torch.bfloat16 else F32_ROUND) + r_extra
    g = got.detach().to(device=ref.device, dtype=torch.float64)
    assert g.shape == ref.shape, f"{what}: shape {tuple(g.shape)} vs reference {tuple(ref.shape)}"
    bound = ref.abs() * r_out + S * c_acc(K) + A_FLOOR
    if extra is not None:
        bound += extra
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
                             f"{float(bound.reshape(-1)[i]):.3g} (err/bound {worst:.3g}, K {K})")
    return worst
