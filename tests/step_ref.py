"""References and derived error bounds for the streaming and reduction kernels of csrc/elementwise.hip that start and end a
train step: noise, layout, pooling, time features, the losses, the reparameterisation, the sampler updates, the gradient norm,
the clip and the single-tensor AdamW (test infrastructure, not a conftest).  tests/test_step_ref_cpu.py checks the references
against torch and that each bound notices a planted mistake; tests/test_step_kernels_gpu.py holds the kernels to them.

Two kinds of reference:
  * bit-exact entries (the kernels use __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn): numpy float32, one operation at a time
    in the kernel's documented order; compared with same_bits (the bits, NaN positions equal);
  * everything else: torch fp64 of the fp32 values the kernel read, widened exactly (scalars as fp64(fp32(value))), on the
    operands' own device, held to row_ref.check's bound  r_out |ref| + depth 2^-24 S + A_FLOOR (+ extra).  The library is built
    with -ffp-contract=off, so every fp32 operation of a kernel is one rounding; `depth` counts them per kernel below.

Every elementwise reference takes dtype (fp64; fp32 = the kernel's own arithmetic restated in torch, which must sit inside the
bound) and `mistake` (a planted error, for the CPU suite)."""
import math

import numpy as np
import torch

from tests.row_ref import U, check  # noqa: F401  (check: the comparator of every bounded entry)

F32 = np.float32
F64 = torch.float64
# HIP documentation, "HIP math API", table "Single precision mathematical functions": expf, powf, sinf and cosf are listed with
# a maximum error of 1 ULP.  One ULP of an fp32 value is at most 2^-23 of its magnitude.
EXPF_REL = 2.0 ** -23
POWF_REL = 2.0 ** -23
SIN_BAR = {torch.float32: 2e-6, torch.bfloat16: 4e-3}      # the absolute bars of test_kernels_gpu.test_layout_pool_sinusoid

FLAG_NOISY_BAD, FLAG_T_RANGE, FLAG_PRED_BAD, FLAG_LOSS_BAD, FLAG_FALLBACK, FLAG_INPUT_BAD = 1, 2, 4, 8, 16, 32   # enum psg_flag

# grid caps of the launchers (elements one launch covers in a single trip of its grid-stride loop)
GRID_CAP = 2048 * 256              # grid_for's default: the streaming kernels
RED_CAP = 1024 * 256               # RED_BLOCKS x RED_THREADS: smooth_l1, recon_loss
SUMSQ_CAP = 4 * RED_CAP            # sumsq_kernel reads float4
SCALAR_CAP = 4096 * 256            # adamw_kernel, clip_scale_kernel
RED_BLOCKS, RED_THREADS = 1024, 256


def f32(x):
    """The C float a scalar argument becomes, as a Python float."""
    return float(F32(x))


def same_bits(got, want):
    """fp32 / bf16 / integer arrays or tensors: equal bits wherever `want` is not NaN, NaN exactly where `want` is NaN."""
    g, w = (torch.as_tensor(np.asarray(t)) if not torch.is_tensor(t) else t.detach().cpu() for t in (got, want))
    if g.shape != w.shape or g.dtype != w.dtype:
        return False
    if not g.dtype.is_floating_point:
        return bool(torch.equal(g, w))
    nan = torch.isnan(w)
    if not torch.equal(torch.isnan(g), nan):
        return False
    iv = torch.int16 if g.element_size() == 2 else torch.int32
    return bool(torch.equal(g.contiguous().view(iv)[~nan], w.contiguous().view(iv)[~nan]))


# ---------------------------------------------------------------------------------------------------- bit-exact entries
def clamp3(x):
    """clamp3 of elementwise.hip: torch.clamp(x, -3, 3) with NaN kept."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), x, np.minimum(np.maximum(x, F32(-3)), F32(3))).astype(F32)


def _bad(r):
    return bool((np.isnan(r) | np.isinf(r)).any())


def noise_add(x0, noise, t, tabA, tabB, do_clamp):
    """psg_noise_add_f32: out[b, i] = fl(fl(a x) + fl(c noise)), a = tabA[clamped t[b]].  x0, noise float32 [B, chw]; returns
    (out, flag bits: T_RANGE for a t outside the table, FALLBACK for a non-finite output)."""
    num_t = len(tabA)
    flag = FLAG_T_RANGE if bool(((t < 0) | (t >= num_t)).any()) else 0
    tc = np.clip(t, 0, num_t - 1)
    a, c = tabA[tc].astype(F32)[:, None], tabB[tc].astype(F32)[:, None]
    x = clamp3(x0) if do_clamp else x0
    with np.errstate(all="ignore"):
        r = (a * x).astype(F32) + (c * noise).astype(F32)
    assert r.dtype == F32
    return r, flag | (FLAG_FALLBACK if _bad(r) else 0)


def noise_fallback(x0, noise, do_clamp):
    """psg_noise_fallback_f32 with the fallback bit set: fl(x + fl(0.1f noise)); (out, NOISY_BAD or 0)."""
    x = clamp3(x0) if do_clamp else x0
    with np.errstate(all="ignore"):
        r = x + (F32(0.1) * noise).astype(F32)
    assert r.dtype == F32
    return r, FLAG_NOISY_BAD if _bad(r) else 0


def ddpm_update(x, eps, z, c1, c2, sg, t):
    """psg_ddpm_update_f32: fl(c1 fl(x - fl(c2 eps))) [+ fl(sg z) when t > 0], the scalars read at index t."""
    r = F32(c1[t]) * (x - (F32(c2[t]) * eps).astype(F32)).astype(F32)
    if t > 0:
        r = r.astype(F32) + (F32(sg[t]) * z).astype(F32)
    return r.astype(F32)


def sampler_update(x, eps, z, mode, c0, c1, c2, c3, mistake=None):
    """psg_sampler_update_f32, modes 1..3 in the kernel's order.  mistake "div_first": mode 1 as c1 (eps / c2)."""
    c0, c1, c2, c3 = F32(c0), F32(c1), F32(c2), F32(c3)
    if mode == 1:
        q = (c1 * (eps / c2).astype(F32)).astype(F32) if mistake == "div_first" else ((c1 * eps).astype(F32) / c2).astype(F32)
        r = (c0 * (x - q).astype(F32)).astype(F32)
        if z is not None:
            r = r + (c3 * z).astype(F32)
    elif mode == 2:
        r = x - eps
    else:
        r = ((x - (c0 * eps).astype(F32)).astype(F32) / c1).astype(F32)
        if z is not None:
            r = (c2 * r).astype(F32) + (c3 * z).astype(F32)
    assert r.dtype == F32
    return r


def nchw_to_nhwc(src, dtype):
    """[B, C, HW] fp32 -> [B * HW, C] in dtype: one rounding of the fp32 value."""
    return src.permute(0, 2, 1).reshape(-1, src.shape[1]).to(dtype)


def nhwc_to_nchw(rows, B, C, HW):
    """[B * HW, C] in any dtype -> [B, C, HW] fp32, widened exactly."""
    return rows.float().reshape(B, HW, C).permute(0, 2, 1).contiguous()


# --------------------------------------------------------------------------------------------------- reparameterisation
def reparam(mu, logvar, eps, dtype=F64, mistake=None):
    """out = mu + eps exp(0.5 logvar) -> (ref, S, depth, extra).  The kernel: fl(0.5 logvar) (exact), expf (its own term:
    EXPF_REL |eps e|), fl(eps e), fl(mu + .): the product term passes 2 roundings -> depth 2, S = |mu| + |eps e|."""
    mu, lv, ep = (t.detach().to(dtype) for t in (mu, logvar, eps))
    e = torch.exp(lv if mistake == "exp_logvar" else 0.5 * lv)
    prod = ep * e
    return mu + prod, mu.abs() + prod.abs(), 2, EXPF_REL * prod.abs()


def reparam_bwd(dlat, logvar, eps, prev_mu=None, prev_lv=None, dtype=F64, mistake=None):
    """dmu = dlat (+ prev), dlogvar = dlat eps 0.5 exp(0.5 logvar) (+ prev) -> ((dmu, S, depth), (dlogvar, S, depth, extra)).
    dmu: a copy (depth 0: bits) or one addition (depth 1).  dlogvar: fl(d eps), fl(0.5 e) (exact), their product: 2
    roundings, + 1 for the addition onto prev; expf's own term EXPF_REL |v|."""
    d, lv, ep = (t.detach().to(dtype) for t in (dlat, logvar, eps))
    v = (d * ep) * (0.5 * torch.exp(lv if mistake == "exp_logvar" else 0.5 * lv))
    if prev_mu is None:
        dm = (d, d.abs(), 0)
    else:
        dm = (prev_mu.to(dtype) + d, prev_mu.to(dtype).abs() + d.abs(), 1)
    if prev_lv is None:
        dl = (v, v.abs(), 2, EXPF_REL * v.abs())
    else:
        dl = (prev_lv.to(dtype) + v, prev_lv.to(dtype).abs() + v.abs(), 3, EXPF_REL * v.abs())
    return dm, dl


# ---------------------------------------------------------------------------------------------------------------- losses
def red_trips(n, per_trip=RED_BLOCKS * RED_THREADS):
    """T: the trips of one lane's serial accumulation when `per_trip` elements (items) are covered per trip of the grid."""
    return -(-n // per_trip)


def red_tree(blocks):
    """c: the roundings of the fixed tree behind the lanes' accumulators, read off wave_sum / block_sum (psg_common.h) and the
    finish kernels: 6 shuffle levels of wave_sum, 4 additions over the block's 4 waves (256 lanes; the first onto 0), the
    finish kernel's ceil(blocks / 256) serial trips over the partials, its own 6 + 4, the rounding of 1 / n and the product
    with it."""
    return (6 + 4) + -(-blocks // 256) + (6 + 4) + 2


def red_blocks(items):
    return max(1, min(RED_BLOCKS, -(-items // RED_THREADS)))


def red_depth(n, per_term, items=None):
    """depth of a sum of non-negative terms: T + c + the roundings inside one term; S = ref."""
    items = n if items is None else items
    return red_trips(items) + red_tree(red_blocks(items)) + per_term


def _drop_trip(terms, n, cap):
    """A planted mistake: the second trip of the grid-stride loop (elements cap .. 2 cap - 1) never added."""
    t = terms.clone()
    t[cap:2 * cap] = 0
    return t


def smooth_l1(pred, target, beta, grad_scale, dtype=F64, mistake=None):
    """SmoothL1Loss(beta), mean, and its gradient times grad_scale -> (loss, depth_loss, grad, S_grad, depth_grad), all on
    flat tensors.
    grad: fl(p - t), / beta, the rounding of 1 / n, the products with it and with grad_scale: depth 5 on S = |grad| (the
    linear branch has fewer).  Where fl(d) and d fall on different sides of beta both branches give |g| = 1 to one rounding.
    loss: a term is fl(fl(fl(0.5 d) d) / beta) - d twice (2), 0.5 d exact, product, quotient: 4 roundings - or
    fl(|d| - fl(0.5 beta)): the rounding of d is 2^-24 |d| <= 2 x 2^-24 term (term >= |d| / 2), the subtraction one more: 3.
    per_term = 4."""
    p, t = pred.detach().to(dtype).reshape(-1), target.detach().to(dtype).reshape(-1)
    n = p.numel()
    beta, gs = f32(beta), f32(grad_scale)
    d = p - t
    ad = d.abs()
    quad = 0.5 * d * d if mistake == "no_div_beta" else 0.5 * d * d / beta
    terms = torch.where(ad < beta, quad, ad - 0.5 * beta)
    if mistake == "drop_trip":
        terms = _drop_trip(terms, n, RED_CAP)
    inv_n = 1.0 / (n - 1) if mistake == "n_minus_1" else (1.0 / n if dtype == F64 else float(F32(1.0) / F32(n)))
    loss = terms.sum() * inv_n
    gq = d if mistake == "no_div_beta" else d / beta
    g = torch.where(ad < beta, gq, torch.where(d > 0, 1.0, -1.0).to(dtype)) * inv_n * gs
    return loss, red_depth(n, 4), g, g.abs(), 5


def recon_loss(pred, target, w_l1, w_mse, dtype=F64, mistake=None):
    """out3 = {w_l1 l1 + w_mse mse, l1 = mean |d|, mse = mean d^2} and grad = (w_l1 sign(d) + 2 w_mse d) / n ->
    (out3 [3], depth [3], grad, S_grad, depth_grad).
    l1: a term is |fl(p - t)|: per_term 1.  mse: fl(d d), d twice: per_term 3.  out3[0]: two products and one addition of
    non-negative values on top of the deeper of the two: + 3, S = ref.
    grad: fl(p - t), w_l1 sign and 2 w_mse exact, fl(2 w_mse d), the addition, the rounding of 1 / n and the product with it:
    depth 5 on S = (|w_l1 sign| + |2 w_mse d|) / n.  sign(fl(d)) = sign(d): a difference of two floats never rounds to 0."""
    p, t = pred.detach().to(dtype).reshape(-1), target.detach().to(dtype).reshape(-1)
    n = p.numel()
    w1, w2 = f32(w_l1), f32(w_mse)
    d = p - t
    a1, a2 = d.abs(), d * d
    if mistake == "drop_trip":
        a1, a2 = _drop_trip(a1, n, RED_CAP), _drop_trip(a2, n, RED_CAP)
    inv_n = 1.0 / (n - 1) if mistake == "n_minus_1" else (1.0 / n if dtype == F64 else float(F32(1.0) / F32(n)))
    l1, mse = a1.sum() * inv_n, a2.sum() * inv_n
    out3 = torch.stack([w1 * l1 + w2 * mse, l1, mse])
    d1, d2 = red_depth(n, 1), red_depth(n, 3)
    sign = torch.sign(d) if mistake != "sign0_is_1" else torch.where(d >= 0, 1.0, -1.0).to(dtype)
    k = w2 if mistake == "mse_no_2" else 2.0 * w2
    g = (w1 * sign + k * d) * inv_n
    S = (abs(w1) * sign.abs() + abs(2.0 * w2) * d.abs()) * inv_n
    return out3, [max(d1, d2) + 3, d1, d2], g, S, 5


def sumsq(g, prev=None, dtype=F64, mistake=None):
    """sum g^2 (+ prev >= 0) -> (ref, depth).  A lane adds fl(fl(fl(v0^2 + v1^2) + v2^2) + v3^2) per float4: the first square
    passes its own rounding and 3 additions, per_term 4; T counts float4s; + 1 for the n % 4 tail element added to a lane of
    block 0; the finish kernel's product with 1.0f is exact but stays counted in red_tree; + 1 for the addition onto prev."""
    x = g.detach().to(dtype).reshape(-1)
    n = x.numel()
    t = x * x
    if mistake == "drop_trip":
        t = _drop_trip(t, n, SUMSQ_CAP)
    if mistake == "tail_twice":
        t = torch.cat([t, t[n - n % 4:]])
    ref = t.sum()
    if prev is not None:
        ref = ref + float(prev)
    return ref, red_depth(n, 4, items=(n + 3) // 4) + (1 if n % 4 else 0) + (1 if prev is not None else 0)


# ------------------------------------------------------------------------------------------------------- clip and AdamW
CLIP_EPS = f32(1e-6)


def clip_coef(normsq, max_norm, dtype=F64, mistake=None):
    """min(1, max_norm / (sqrt(normsq) + 1e-6f)) as a Python float: sqrtf, the addition, the division - 3 roundings."""
    if normsq is None:
        return 1.0
    eps = 0.0 if mistake == "clip_no_eps" else CLIP_EPS
    if dtype == F64:
        return min(1.0, f32(max_norm) / (math.sqrt(f32(normsq)) + eps))
    return float(min(F32(1.0), F32(max_norm) / (np.sqrt(F32(normsq)) + F32(eps))))


CLIP_DEPTH = 3


def clip_scale(g, normsq, max_norm, dtype=F64, mistake=None):
    """g min(1, coef) -> (ref, S = |ref|, depth 4: the coefficient's 3 roundings and the product).  A coefficient >= 1 leaves
    every bit as it was: the caller checks that where the norm is clearly below max_norm."""
    ref = g.detach().to(dtype) * clip_coef(normsq, max_norm, dtype, mistake)
    return ref, ref.abs(), CLIP_DEPTH + 1


def adamw(p, g, m, v, step, lr, beta1, beta2, eps, wd, normsq=None, max_norm=0.0, dtype=F64, mistake=None):
    """torch.optim.AdamW's decoupled update after clip_grad_norm_, step 1-based, the bias corrections from the beta1 given:
        gi = g coef;  m' = b1 m + (1 - b1) gi;  v' = b2 v + (1 - b2) gi^2
        p' = p (1 - lr wd) - (lr / (1 - b1^step)) m' / (sqrt(v') / sqrt(1 - b2^step) + eps)
    -> {"p": (ref, S), "m": (ref, S, depth), "v": (ref, S, depth)}; p's S is already weighted (check it with depth 1).

    Roundings, with dc = 3 when a norm is given (clip_coef) and 0 otherwise:
      m': the gradient term passes coef (dc), fl(g coef), fl(1 - b1), their product and the addition: depth dc + 4 on
          S = |b1 m| + |(1 - b1) gi|.
      v': gi twice (2 (dc + 1)), fl(1 - b2), two products, the addition: depth 2 (dc + 1) + 4 on S = v' (no cancellation).
      p': A = p (1 - lr wd): fl(lr wd), fl(1 - .), the product: 3 |A|.
          B = step_size (m' / denom), relative roundings in units of 2^-24:
            step_size = lr / bc1, bc1 = fl(1 - powf(b1, step)): powf's accuracy amplified by b1^step / (1 - b1^step)
              (2 amp1 units), the subtraction and the division: 2 amp1 + 2;
            denom = sqrtf(v') / bc2_sqrt + eps: half of v's depth and sqrtf (1); bc2_sqrt: half of (2 amp2 + 1) and sqrtf (1);
              the division and the addition (2);
            the quotient m' / denom and the product with step_size (2);
          and m's own absolute error depth_m 2^-24 S_m scaled by step_size / denom.
          S_p = 3 |A| + |B| (rel_step + rel_denom + 2) + step_size / denom depth_m S_m; the final subtraction is r_out."""
    P, G, M, V = (t.detach().to(dtype) for t in (p, g, m, v))
    lr, b1, b2, eps, wd = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(wd)
    dc = CLIP_DEPTH if normsq is not None else 0
    coef = clip_coef(normsq, max_norm, dtype, mistake)
    s_bc = step - 1 if mistake == "bc_step_minus_1" else step
    if dtype == F64:
        pw1, pw2 = b1 ** s_bc, b2 ** s_bc
        bc1, bc2s = 1.0 - pw1, math.sqrt(1.0 - pw2)
        one_b1, one_b2, keep, ss = 1.0 - b1, 1.0 - b2, 1.0 - lr * wd, None
    else:
        with np.errstate(all="ignore"):
            pw1, pw2 = float(np.power(F32(b1), F32(s_bc))), float(np.power(F32(b2), F32(s_bc)))
            bc1, bc2s = float(F32(1) - F32(pw1)), float(np.sqrt(F32(1) - F32(pw2)))
            one_b1, one_b2, keep = float(F32(1) - F32(b1)), float(F32(1) - F32(b2)), float(F32(1) - F32(lr) * F32(wd))
            ss = float(F32(lr) / F32(bc1))
    gi = G * coef
    if mistake == "wd_on_grad":
        gi, keep = gi + wd * P, 1.0
    mi = b1 * M + one_b1 * gi
    vi = b2 * V + one_b2 * gi * gi
    denom = torch.sqrt(vi + eps) / bc2s if mistake == "eps_in_sqrt" else torch.sqrt(vi) / bc2s + eps
    step_size = ss if ss is not None else (lr / bc1 if bc1 != 0 else math.inf)
    A = P * keep
    B = step_size * (mi / denom)
    S_m = (b1 * M).abs() + (one_b1 * gi).abs()
    depth_m, depth_v = dc + 4, 2 * (dc + 1) + 4
    amp1 = pw1 / (1.0 - pw1) if pw1 < 1 else math.inf
    amp2 = pw2 / (1.0 - pw2) if pw2 < 1 else math.inf
    unit = POWF_REL / U                                  # powf's accuracy in units of 2^-24
    rel_step = unit * amp1 + 2
    rel_denom = (depth_v / 2 + 1) + ((unit * amp2 + 1) / 2 + 1) + 2
    S_p = 3 * A.abs() + B.abs() * (rel_step + rel_denom + 2) + (step_size / denom).abs() * depth_m * S_m
    return {"p": (A - B, S_p), "m": (mi, S_m, depth_m), "v": (vi, vi.abs(), depth_v)}


# ------------------------------------------------------------------------------------------------- text_pool, sinusoid
def text_pool(text, dtype=F64):
    """pooled[b, d] = mean_s text[b, s, d] -> (ref, S, depth): S - 1 serial additions (the first onto 0 is exact) and the
    division by (float)S: depth S on S = sum |text| / S."""
    x = text.detach().to(dtype)
    Sn = x.shape[1]
    if dtype == F64:
        return x.mean(1), x.abs().mean(1), Sn
    acc = torch.zeros_like(x[:, 0])
    for s in range(Sn):
        acc = acc + x[:, s]
    return acc / Sn, x.abs().mean(1), Sn


def sinusoid_coeff(half):
    """unet.py's emb_coeff: exp(arange(half) * -(log(10000) / (half - 1))), fp32."""
    return torch.exp(torch.arange(half) * -(math.log(10000) / (half - 1))).float()


def sinusoid(t, coeff):
    """[sin(e), cos(e)], e = fl((float)t coeff) in fp32 (the kernel's __fmul_rn) widened exactly; fp64 sin / cos.  [B, 2 half]."""
    e = (t.float().unsqueeze(-1) * coeff.float().unsqueeze(0)).double()
    return torch.cat([torch.sin(e), torch.cos(e)], dim=-1)


# ---------------------------------------------------------------------------------------------------------- comparators
def check_scalar(got, ref, depth, what):
    """One reduction output against (ref, depth): a sum of non-negative terms, S = ref."""
    r = torch.as_tensor(ref, dtype=F64).detach().cpu().reshape(1)
    return check(torch.as_tensor(got).detach().cpu().reshape(1), r, r.abs(), torch.float32, what, depth)


def check_adamw(got, ref, what):
    """got: {"p", "m", "v"} tensors; ref: adamw()'s result -> the worst err / bound of each."""
    return {"p": check(got["p"], ref["p"][0], ref["p"][1], torch.float32, what + " p", 1),
            "m": check(got["m"], ref["m"][0], ref["m"][1], torch.float32, what + " m", ref["m"][2]),
            "v": check(got["v"], ref["v"][0], ref["v"][1], torch.float32, what + " v", ref["v"][2])}
