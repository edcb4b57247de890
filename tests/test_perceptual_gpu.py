"""-m gpu: the stage-1 loss.  Kernel level through the C ABI, element by element (max-pool, image preprocessing, feature L1,
KL); module level per case of tests/vgg_ref.py against its fp64 restatement, at bars that come from the torch CPU error in the
same precision (vgg_ref.BASELINE_ERR, recorded by tests/test_vgg_ref_cpu.py) times 4 - never from this code's own output.
Every test prints `RATIO <what> <err / bound>` before it asserts."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import vgg_ref as R
from tests.gemm_ref import A_FLOOR, BF16_ROUND, F32_ROUND, c_acc
from tests.util import h

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
PREC = {torch.float32: "fp32", torch.bfloat16: "bf16"}
TWO24 = 2.0 ** -24
INV_STD_MIN = 1.0 / 0.229           # the largest normalisation factor: what an fp32 rounding of v - mean is scaled by


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    return _lib.init(0)


def _api():
    from pokemon_sprite_generator_amd import _lib
    return _lib


def _ratio(what, err, bound):
    r = float(err) / float(bound)
    print(f"RATIO {what} {r:.3g}")
    return r


def _worst(what, got, ref, bound):
    """Element-wise |got - ref| <= bound; returns (and prints) the worst err / bound.  A NaN in got fails."""
    err = (got.detach().double().cpu() - ref).abs()
    ratio = err / bound
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    w = float(ratio.max())
    print(f"RATIO {what} {w:.3g}")
    assert w <= 1.0, f"{what}: worst err / bound {w:.3g} at flat index {int(ratio.argmax())}"
    return w


def _strided(t, pad):
    """The same values in rows `pad` elements longer: a row-strided operand."""
    buf = torch.empty(tuple(t.shape[:-1]) + (t.shape[-1] + pad,), dtype=t.dtype, device=t.device)
    buf[..., :t.shape[-1]] = t
    return buf[..., :t.shape[-1]], buf.stride(-2)


# ---------------------------------------------------------------------------------------------------------------- max-pool
@pytest.mark.parametrize("hw", [(2, 2), (5, 7), (23, 21), (16, 24)], ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("Cc", [8, 64, 72])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: PREC[d])
def test_maxpool_bit_exact(lib, dtype, Cc, hw):
    L = _api()
    B, (Hi, Wi) = 2, hw
    Ho, Wo = Hi // 2, Wi // 2
    # five levels (-0.0 among them): most windows hold a repeated maximum
    x = (torch.round(h((B, Hi, Wi, Cc), f"mp.x.{Hi}.{Cc}") * 2.0) / 2.0).to(dtype)
    dy = h((B, Ho, Wo, Cc), f"mp.dy.{Hi}.{Cc}").to(dtype)
    xn = x.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    yr, ir = F.max_pool2d(xn, 2, 2, return_indices=True)
    yr.backward(dy.float().permute(0, 3, 1, 2))
    ih, iw = ir // Wi, ir % Wi
    ho = torch.arange(Ho).view(1, 1, Ho, 1)
    wo = torch.arange(Wo).view(1, 1, 1, Wo)
    tap_ref = ((ih - 2 * ho) * 2 + (iw - 2 * wo)).permute(0, 2, 3, 1).to(torch.uint8)
    assert int((tap_ref > 0).sum()) > 0 and int(tap_ref.max()) <= 3
    ties = (F.max_pool2d(xn.detach(), 2, 2).unsqueeze(-1) == F.unfold(xn.detach().reshape(B * Cc, 1, Hi, Wi), 2, stride=2)
            .reshape(B, Cc, 4, Ho, Wo).permute(0, 1, 3, 4, 2)).sum(-1)
    assert int((ties > 1).sum()) > 0, "the input must hold ties"

    xs, ldx = _strided(x.to(DEV), 8)
    y = torch.full((B, Ho, Wo, Cc), float("nan"), dtype=dtype, device=DEV)
    tap = torch.full((B, Ho, Wo, Cc), 255, dtype=torch.uint8, device=DEV)
    code = L.dtype_code(dtype)
    L.check(lib.psg_maxpool2x2_fwd(L.ptr(xs), ldx, L.ptr(y), Cc, L.ptr(tap), B, Hi, Wi, Cc, code, L.stream_ptr()), "maxpool fwd")
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    want_y = yr.detach().permute(0, 2, 3, 1).contiguous().to(dtype)
    assert torch.equal(y.cpu().view(bits), want_y.view(bits)), "y differs from torch.max_pool2d in its bits"
    assert torch.equal(tap.cpu(), tap_ref), "recorded taps differ from torch's indices (first tap wins on ties)"
    y2 = torch.empty_like(y)
    L.check(lib.psg_maxpool2x2_fwd(L.ptr(xs), ldx, L.ptr(y2), Cc, None, B, Hi, Wi, Cc, code, L.stream_ptr()), "maxpool fwd, no taps")
    assert torch.equal(y2.view(bits), y.view(bits))

    dys, lddy = _strided(dy.to(DEV), 16)
    dx = torch.full((B, Hi, Wi, Cc), float("nan"), dtype=dtype, device=DEV)      # poison: every element must be written
    L.check(lib.psg_maxpool2x2_bwd(L.ptr(dys), lddy, L.ptr(tap), L.ptr(dx), Cc, B, Hi, Wi, Cc, code, L.stream_ptr()), "maxpool bwd")
    want_dx = xn.grad.permute(0, 2, 3, 1).contiguous()
    got = dx.float().cpu()
    assert not bool(torch.isnan(got).any()), "an element of dx was not written"
    assert torch.equal(got, want_dx), "dx differs from torch's backward"
    if Hi % 2:
        assert float(got[:, Hi - 1].abs().max()) == 0.0
    if Wi % 2:
        assert float(got[:, :, Wi - 1].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------- image preprocessing
def _prep_f64(img, a, b, size):
    x = img.double().requires_grad_(True)
    v = torch.clamp(a * x + b, 0, 1)
    if size is not None:
        v = F.interpolate(v, size=size, mode="bilinear", align_corners=False)
    mean = torch.tensor(R.MEAN, dtype=torch.float32).double().view(1, 3, 1, 1)
    std = torch.tensor(R.STD, dtype=torch.float32).double().view(1, 3, 1, 1)
    return x, (v - mean) / std


@pytest.mark.parametrize("ab", [(1.0, 0.0), (0.5, 0.5)], ids=["unit", "half"])
@pytest.mark.parametrize("size", [None, (32, 29), (8, 6)], ids=["same", "resize", "shrink"])
def test_image_prep(lib, size, ab):
    """Forward: fp32 within 4 * 2^-24 * (|ref| + 1 / std_min) of fp64 per element - the roundings of a x + b, of the (at most
    four-term, convex) interpolation, of v - mean (absolute 2^-24, scaled by up to 1 / std_min) and of the product; bf16 within
    one bf16 rounding of the fp32 launch's result; padding channels exactly 0.
    Backward: exactly 0 outside the clamp, the planted edge pixels inside, and the same relative bound: |got - ref| <=
    4 * 2^-24 * M with M the same gradient taken with |dy| (the sum of the terms' magnitudes), in every form - same size,
    up-sampling (23x21 -> 32x29) and down-sampling (-> 8x6, where some input pixels lie under no stencil and get exactly 0).
    A bf16 launch reads a bf16 dy (given exactly to the reference) and writes fp32: the same bound."""
    from pokemon_sprite_generator_amd import ops
    a, b = ab
    img, _ = R.images("odd", unit=(ab == (1.0, 0.0)))
    u = a * img + b
    assert int((u == 0).sum()) > 50 and int((u == 1).sum()) > 50 and float(u.min()) < 0 and float(u.max()) > 1
    x64, ref = _prep_f64(img, a, b, size)
    B, _, Ho, Wo = ref.shape
    ref_cl = ref.detach().permute(0, 2, 3, 1)
    outs = {}
    for dtype in DTYPES:
        g = img.to(DEV).requires_grad_(True)
        y = ops.image_prep(g, a, b, size, dtype)
        assert tuple(y.shape) == (B, Ho, Wo, 8) and y.dtype == dtype
        assert float(y.detach()[..., 3:].float().abs().max()) == 0.0, "padding channels must be exactly 0"
        outs[dtype] = y.detach().float().cpu()[..., :3].double()
        if dtype == torch.float32:
            _worst(f"image_prep fwd fp32 {size} {ab}", outs[dtype], ref_cl, 4 * TWO24 * (ref_cl.abs() + INV_STD_MIN))
        else:
            f32 = outs[torch.float32]
            _worst(f"image_prep fwd bf16 {size} {ab}", outs[dtype], f32, BF16_ROUND * f32.abs() + A_FLOOR)
        dy = h((B, Ho, Wo, 8), f"prep.dy.{size}").to(dtype)
        y.backward(dy.to(DEV))
        dy64 = dy.double()[..., :3].permute(0, 3, 1, 2)
        gref, = torch.autograd.grad(ref, x64, dy64, retain_graph=True)
        gmag, = torch.autograd.grad(ref, x64, dy64.abs(), retain_graph=True)
        got = g.grad.cpu()
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(img.shape)
        outside = (u < 0) | (u > 1)
        assert float(got[outside].abs().max()) == 0.0, "gradient outside the clamp must be exactly 0"
        edge = (u == 0) | (u == 1)
        assert int((gmag[edge] > 0).sum()) > 50 and bool(((got[edge] != 0) == (gref[edge] != 0)).all()), "the clamp's edges are inside"
        if size == (8, 6):
            assert int((gmag[~outside] == 0).sum()) > 0 and float(got[gmag == 0].abs().max()) == 0.0    # pixels under no stencil
        _worst(f"image_prep bwd {PREC[dtype]} {size} {ab}", got, gref, 4 * TWO24 * gmag + A_FLOOR)


# ------------------------------------------------------------------------------------------------------------- feature L1
@pytest.mark.parametrize("shape", [(37, 72), (214, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: PREC[d])
def test_feat_l1(lib, dtype, shape):
    L = _api()
    rows, cols = shape
    n = rows * cols
    scale = 0.7
    # post-ReLU maps: zero in many places, and equal to the other map (zero or not) in many
    a = torch.relu(h((rows, cols), "fl.a")).to(dtype)
    b = torch.relu(h((rows, cols), "fl.b")).to(dtype)
    same = h((rows, cols), "fl.same") > 0.3
    b = torch.where(same, a, b)
    d = a.double() - b.double()
    assert int((d == 0).sum()) > n // 4 and int((d > 0).sum()) > n // 8 and int((d < 0).sum()) > n // 8
    ad, lda = _strided(a.to(DEV), 8)
    bd, ldb = _strided(b.to(DEV), 16)
    code = L.dtype_code(dtype)
    need = lib.psg_feat_l1_workspace_bytes()
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def run(with_grad):
        grad = torch.full((rows, cols), float("nan"), dtype=dtype, device=DEV) if with_grad else None
        out2 = torch.full((2,), float("nan"), dtype=torch.float32, device=DEV)
        L.check(lib.psg_feat_l1(L.ptr(ad), lda, L.ptr(bd), ldb, L.ptr(grad), cols, L.ptr(out2), rows, cols, scale, code, L.ptr(ws), need,
                                L.stream_ptr()), "feat_l1")
        return out2.cpu(), (grad.cpu() if with_grad else None)

    out2, grad = run(True)
    gval = (np.float32(scale) / np.float32(n)).item()
    want = (torch.sign(d) * gval).float().to(dtype)
    assert torch.equal(grad, want), "gradient is not exactly scale * sign / n rounded to the dtype (sign(0) = 0)"
    assert float(grad[d == 0].float().abs().max()) == 0.0
    ref = float(d.abs().mean())
    # fp32 accumulation of n non-negative terms in a fixed tree, then one product with 1 / n: c_acc(n) of the sum, plus the
    # output's roundings
    bound = (c_acc(n) + F32_ROUND) * ref
    assert _ratio(f"feat_l1 loss {PREC[dtype]} {shape}", abs(float(out2[0]) - ref), bound) <= 1.0
    assert _ratio(f"feat_l1 scaled loss {PREC[dtype]} {shape}", abs(float(out2[1]) - scale * ref), bound * scale + TWO24 * scale * ref) <= 1.0
    again, grad2 = run(True)
    assert torch.equal(again.view(torch.int32), out2.view(torch.int32)) and torch.equal(grad2, grad), "two runs differ"
    nograd, _ = run(False)
    assert torch.equal(nograd.view(torch.int32), out2.view(torch.int32)), "the loss without a gradient pointer differs"


# --------------------------------------------------------------------------------------------------------------------- KL
@pytest.mark.parametrize("n", [8 * 27 * 27, 7])
def test_kl(lib, n):
    L = _api()
    mu, lv = h((n,), "kl.mu", 1.5), h((n,), "kl.lv", 2.0)
    md, ld = mu.double().requires_grad_(True), lv.double().requires_grad_(True)
    ref = R.kl(md, ld)
    ref.backward()
    need = lib.psg_kl_workspace_bytes()
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    m_, l_ = mu.to(DEV), lv.to(DEV)

    def run(want_mu, want_lv):
        dmu = torch.full((n,), float("nan"), device=DEV) if want_mu else None
        dlv = torch.full((n,), float("nan"), device=DEV) if want_lv else None
        out = torch.full((1,), float("nan"), device=DEV)
        L.check(lib.psg_kl_f32(L.ptr(m_), L.ptr(l_), L.ptr(dmu), L.ptr(dlv), L.ptr(out), n, L.ptr(ws), need, L.stream_ptr()), "kl")
        return out.cpu(), (dmu.cpu() if want_mu else None), (dlv.cpu() if want_lv else None)

    out, dmu, dlv = run(True, True)
    r = 8 * TWO24
    assert _ratio(f"kl loss n={n}", abs(float(out[0]) - float(ref.detach())), r * abs(float(ref.detach()))) <= 1.0
    _worst(f"kl dmu n={n}", dmu, md.grad, r * md.grad.abs() + A_FLOOR)
    _worst(f"kl dlogvar n={n}", dlv, ld.grad, r * ld.grad.abs() + A_FLOOR)
    for wm, wl in ((False, True), (True, False), (False, False)):
        o2, g1, g2 = run(wm, wl)
        assert torch.equal(o2.view(torch.int32), out.view(torch.int32)), "a null gradient pointer changed the loss"
        assert (g1 is None or torch.equal(g1, dmu)) and (g2 is None or torch.equal(g2, dlv))


# ----------------------------------------------------------------------------------------------------------------- modules
@functools.lru_cache(maxsize=None)
def _f64(case):
    g, t = R.images(case)
    return R.perceptual(g, t, R.vgg_state_dict(), case, torch.float64)


@functools.lru_cache(maxsize=None)
def _module(case, dtype):
    import pokemon_sprite_generator_amd as psg
    c = R.CASES[case]
    return psg.VGGPerceptualLoss(feature_layers=list(c["feature_layers"]), weights=list(c["weights"]), state_dict=R.vgg_state_dict(),
                                 compute_dtype=dtype, min_size=c["min_size"], resize_to=c["resize_to"]).to(DEV)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: PREC[d])
@pytest.mark.parametrize("case", list(R.CASES))
def test_perceptual_loss_against_fp64(lib, case, dtype):
    prec = PREC[dtype]
    m = _module(case, dtype)
    gen, tgt = R.images(case)
    ref_loss, ref_grad = _f64(case)

    def run():
        g = gen.to(DEV).requires_grad_(True)
        t = tgt.to(DEV).requires_grad_(True)
        loss = m(g, t)
        assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
        loss.backward()
        assert t.grad is None, "the target is a constant"
        return loss.detach().cpu(), g.grad.cpu()

    loss, grad = run()
    assert all(p.grad is None for p in m.parameters()), "no VGG parameter gets a gradient"
    el, eg = R.rel(loss, ref_loss), R.rel(grad, ref_grad)
    rl = _ratio(f"perceptual {case} {prec} loss (err {el:.3e})", el, R.bar(case, prec, "loss"))
    rg = _ratio(f"perceptual {case} {prec} grad (err {eg:.3e})", eg, R.bar(case, prec, "grad"))
    assert rl <= 1.0, f"{case} {prec}: loss relative error {el:.3e} > bar {R.bar(case, prec, 'loss'):.3e}"
    assert rg <= 1.0, f"{case} {prec}: gradient rel-L2 {eg:.3e} > bar {R.bar(case, prec, 'grad'):.3e}"
    loss2, grad2 = run()
    assert torch.equal(loss2.view(torch.int32), loss.view(torch.int32)) and torch.equal(grad2, grad), "two runs differ"
    with torch.no_grad():
        val = m(gen.to(DEV), tgt.to(DEV)).cpu()
    assert torch.equal(val.view(torch.int32), loss.view(torch.int32)), "the no_grad (validation) loss differs from the grad-mode loss"


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: PREC[d])
def test_extract_features_layout(lib, dtype):
    m = _module("odd", dtype)
    gen, _ = R.images("odd")
    feats = m.extract_features(gen.to(DEV))
    assert [tuple(f.shape) for f in feats] == [(2, 128, 11, 10), (2, 256, 5, 5)] and all(f.dtype == torch.float32 for f in feats)
    x = R._prep(gen.double(), 1.0, 0.0, 0, 224, torch.float64)
    ref = R.feature_maps(x, R.vgg_state_dict(), (8, 15), torch.float64)
    for f, r in zip(feats, ref):
        assert R.rel(f, r) <= (1e-5 if dtype == torch.float32 else 3e-2)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: PREC[d])
def test_combined_loss(lib, dtype):
    import pokemon_sprite_generator_amd as psg
    prec = PREC[dtype]
    sd = {"perceptual_loss." + k: v for k, v in R.vgg_state_dict().items()}
    m = psg.CombinedLoss(state_dict=sd, compute_dtype=dtype).to(DEV)
    m.perceptual_loss.min_size = R.CASES[R.COMBINED_CASE]["min_size"]
    gen, tgt = R.images(R.COMBINED_CASE, unit=False)
    mu, lv = R.latents()
    ref = R.combined(gen, tgt, mu, lv, R.vgg_state_dict())
    g, mu_d, lv_d = (v.to(DEV).requires_grad_(True) for v in (gen, mu, lv))
    t = tgt.to(DEV)
    total, parts = m.forward_tensors(g, t, mu_d, lv_d)
    assert parts.dtype == torch.float32 and tuple(parts.shape) == (4,) and parts.is_cuda and not parts.requires_grad
    total.backward()
    got = dict(zip(("total", "reconstruction", "perceptual", "kl"), parts.cpu()))
    got.update(grad=g.grad.cpu(), dmu=mu_d.grad.cpu(), dlogvar=lv_d.grad.cpu())
    assert float(total.detach()) == float(got["total"])
    worst = {}
    for name, v in got.items():
        e = R.rel(v, ref[name])
        worst[name] = _ratio(f"combined {prec} {name} (err {e:.3e})", e, R.bar("combined", prec, name))
    assert all(r <= 1.0 for r in worst.values()), worst
    with torch.no_grad():
        total2, d = m(g, t, mu_d, lv_d)
    assert list(d) == ["total_loss", "reconstruction_loss", "perceptual_loss", "kl_loss"] and all(isinstance(v, float) for v in d.values())
    assert [d[k] for k in d] == parts.tolist() and float(total2) == d["total_loss"], "forward and forward_tensors disagree"


def test_combined_forward_tensors_is_capturable(lib):
    """forward_tensors does no host synchronisation: it runs inside a graph capture (a synchronising call would abort the capture)
    and the replay reproduces the eager values."""
    import pokemon_sprite_generator_amd as psg
    L = _api()
    sd = {"perceptual_loss." + k: v for k, v in R.vgg_state_dict().items()}
    m = psg.CombinedLoss(state_dict=sd, compute_dtype=torch.bfloat16).to(DEV)
    m.perceptual_loss.min_size = 0
    gen, tgt = R.images("even", unit=False)
    mu, lv = R.latents()
    g, t, mu_d, lv_d = (v.to(DEV) for v in (gen, tgt, mu, lv))
    g.requires_grad_(True)
    dev = torch.device(DEV, torch.cuda.current_device())
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    hold = None
    try:
        with torch.cuda.stream(side):
            eager = m.forward_tensors(g, t, mu_d, lv_d)[1].clone()          # warm-up on the capture stream: caches, scratch
            torch.cuda.synchronize(dev)
            graph = torch.cuda.CUDAGraph()
            L.freeze_workspaces(True)
            try:
                with torch.cuda.graph(graph, stream=side):
                    total, parts = m.forward_tensors(g, t, mu_d, lv_d)
            finally:
                L.freeze_workspaces(False)
            hold = L.hold_workspace(dev)
            parts.zero_()
            graph.replay()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        assert torch.equal(parts.view(torch.int32), eager.view(torch.int32)) and float(eager[0]) > 0
    finally:
        L.drop_workspace(hold)
