"""CPU checks of tests/gemm_ref.py: the float64 references equal torch's conv / linear and their autograd gradients, and
the comparator accepts an fp32-accumulated, bf16-rounded result while rejecting subtly wrong ones at the widths where a
max-relative bar of 3e-2 would not."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_ref as R


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _bf(t):
    """bf16-representable values, kept in fp32 (the operands the bf16 kernels read)."""
    return t.bfloat16().float()


def _close(a, b, what):
    a, b = a.double(), b.double()
    err = float((a - b).abs().max() / (b.abs().max() + 1e-300))
    assert err < 1e-12, f"{what}: {err:.3g}"


# ------------------------------------------------------------------------------------------------------ reference == torch
@pytest.mark.parametrize("B,H,Cin,Cout,ks,stride", [(2, 27, 5, 7, 3, 1), (3, 7, 6, 4, 3, 2), (2, 5, 9, 3, 3, 1), (2, 4, 8, 6, 3, 2),
                                                    (2, 27, 4, 6, 3, 2), (3, 5, 7, 5, 1, 1), (1, 4, 16, 8, 1, 1)])
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
def test_conv_reference_matches_torch(B, H, Cin, Cout, ks, stride, strided):
    g = _g(B * 1000 + H * 10 + Cin)
    pad = ks // 2
    xb = torch.randn(B, H, H, Cin + 3, dtype=torch.float64, generator=g)
    x = xb[..., 1:Cin + 1] if strided else xb[..., :Cin].contiguous()          # ldx != Cin: a concat-slot half
    w = torch.randn(Cout, Cin, ks, ks, dtype=torch.float64, generator=g)
    xn = x.permute(0, 3, 1, 2).detach().clone().requires_grad_(True)
    wn = w.clone().requires_grad_(True)
    y = F.conv2d(xn, wn, stride=stride, padding=pad)
    Ho = y.shape[2]
    gyb = torch.randn(B, Ho, Ho, Cout + 5, dtype=torch.float64, generator=g)
    gy = gyb[..., 2:Cout + 2] if strided else gyb[..., :Cout].contiguous()      # ldy != Cout: a slot's gradient
    y.backward(gy.permute(0, 3, 1, 2))
    ref, S = R.conv_fwd(x, w, stride)
    _close(ref.permute(0, 3, 1, 2), y.detach(), "forward")
    _, S2 = R.conv_fwd(x.abs(), w.abs(), stride)
    assert torch.equal(S, S2) or _close(S, S2, "S") is None
    dx, Sd = R.conv_dgrad(gy, w, (H, H), stride)
    _close(dx.permute(0, 3, 1, 2), xn.grad, "data gradient")
    _close(Sd, R.conv_dgrad(gy.abs(), w.abs(), (H, H), stride)[0], "S of the data gradient")
    dw, Sw = R.conv_wgrad(x, gy, ks, stride)
    _close(dw, wn.grad, "weight gradient")
    _close(Sw, R.conv_wgrad(x.abs(), gy.abs(), ks, stride)[0], "S of the weight gradient")
    db, Sb = R.bias_grad(gy)
    _close(db, gy.sum((0, 1, 2)), "bias gradient")
    dra, _ = R.rowadd_grad(gy)
    _close(dra, gy.sum((1, 2)), "row-add gradient")


def test_conv_reference_chunks_over_samples(monkeypatch):
    """A chunk of one sample gives the same result as one chunk (the chunking is only a memory bound)."""
    g = _g(3)
    x = torch.randn(5, 7, 7, 6, dtype=torch.float64, generator=g)
    w = torch.randn(4, 6, 3, 3, dtype=torch.float64, generator=g)
    gy = torch.randn(5, 4, 4, 4, dtype=torch.float64, generator=g)
    full = R.conv_fwd(x, w, 2)[0], R.conv_dgrad(gy, w, (7, 7), 2)[0], R.conv_wgrad(x, gy, 3, 2)[0]
    monkeypatch.setattr(R, "CHUNK_BYTES", 8)
    small = R.conv_fwd(x, w, 2)[0], R.conv_dgrad(gy, w, (7, 7), 2)[0], R.conv_wgrad(x, gy, 3, 2)[0]
    for a, b, what in zip(full, small, ("fwd", "dgrad", "wgrad")):
        _close(a, b, what)


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
def test_linear_reference_matches_torch(strided):
    g = _g(11)
    xb = torch.randn(3, 10, 24, dtype=torch.float64, generator=g)
    x = xb[..., 4:20] if strided else xb[..., :16].contiguous()
    w = torch.randn(12, 16, dtype=torch.float64, generator=g)
    xn, wn = x.detach().clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.linear(xn, wn)
    gy = torch.randn(3, 10, 12, dtype=torch.float64, generator=g)
    y.backward(gy)
    ref, S = R.linear_fwd(x, w)
    _close(ref, y.detach(), "forward")
    _close(S, x.abs() @ w.abs().t(), "S")
    _close(R.linear_dgrad(gy, w)[0], xn.grad, "data gradient")
    _close(R.linear_wgrad(x, gy)[0], wn.grad, "weight gradient")


@pytest.mark.parametrize("kind", ["none", "silu", "gelu"])
@pytest.mark.parametrize("form", ["bias", "rowadd", "residual_alpha", "dropout"])
def test_epilogue_forms_match_autograd(kind, form):
    """epilogue() and epilogue_bwd() against torch autograd in fp64 for every activation and epilogue form."""
    g = _g(7)
    B, H, C, O = 3, 5, 6, 8
    x = torch.randn(B, H, H, C, dtype=torch.float64, generator=g)
    w = torch.randn(O, C, 3, 3, dtype=torch.float64, generator=g)
    b = torch.randn(O, dtype=torch.float64, generator=g)
    ra = torch.randn(B, O, dtype=torch.float64, generator=g) if form == "rowadd" else None
    res = torch.randn(B, H, H, O, dtype=torch.float64, generator=g) if form == "residual_alpha" else None
    alpha = 0.7 if form == "residual_alpha" else 1.0
    p = 0.3 if form == "dropout" else 0.0
    keep = (torch.rand(B, H, H, O, generator=g) >= p) if form == "dropout" else None
    un = (F.conv2d(x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1) + b).requires_grad_(True)
    u = un + ra[:, None, None, :] if ra is not None else un
    a = {"none": u, "silu": F.silu(u), "gelu": F.gelu(u)}[kind]
    if keep is not None:
        a = a * keep / (1.0 - p)
    y = alpha * a + (res if res is not None else 0.0)
    gy = torch.randn(y.shape, dtype=torch.float64, generator=g)
    y.backward(gy)
    acc, S = R.conv_fwd(x, w)
    ref, Sy, A = R.epilogue(acc, S, bias=b, rowadd=ra, residual=res, kind=kind, alpha=alpha, keep=keep, p=p)
    _close(ref, y.detach(), "epilogue")
    assert bool((Sy >= 0).all()) and bool((A >= 0).all())
    gu = R.epilogue_bwd(gy, u.detach(), kind=kind, alpha=alpha, keep=keep, p=p)
    _close(gu, un.grad, "epilogue gradient")


def test_dact_mul_is_the_ffn_data_gradient():
    """The FFN's DACT_MUL form: (g2 . W2) * gelu'(u) * keep / (1 - p) is the gradient at u of drop(gelu(u)) . W2^T."""
    g = _g(9)
    M, C, Hd, p = 20, 8, 16, 0.25
    u = torch.randn(M, Hd, dtype=torch.float64, generator=g).requires_grad_(True)
    w2 = torch.randn(C, Hd, dtype=torch.float64, generator=g)
    keep = torch.rand(M, Hd, generator=g) >= p
    y = F.linear(F.gelu(u) * keep / (1 - p), w2)
    g2 = torch.randn(M, C, dtype=torch.float64, generator=g)
    y.backward(g2)
    acc, S = R.linear_dgrad(g2, w2)
    ref, _ = R.dact_mul(acc, S, R.act_grad(u.detach(), "gelu") * keep / (1 - p))
    _close(ref, u.grad, "DACT_MUL")


# ------------------------------------------------------------------------------------------------------------ sensitivity
def _sim_conv(x, w, stride=1, bias=None, residual=None, alpha=1.0):
    """What a correct bf16 kernel returns: fp32 accumulation of the bf16 operands, fp32 epilogue, one bf16 rounding."""
    y = F.conv2d(x.permute(0, 3, 1, 2), w, stride=stride, padding=w.shape[2] // 2).permute(0, 2, 3, 1)
    if bias is not None:
        y = y + bias
    y = y * alpha
    if residual is not None:
        y = y + residual
    return y.bfloat16()


def _operands(B, H, Cin, Cout, seed):
    g = _g(seed)
    x = _bf(torch.randn(B, H, H, Cin, generator=g))
    w = _bf(torch.randn(Cout, Cin, 3, 3, generator=g) * math.sqrt(1.0 / (9 * Cin)))
    return x, w, g


def _ratio(got, ref, S, K, extra=None):
    return R.check(got, ref, S, torch.bfloat16, "case", K, extra=extra)


def test_comparator_accepts_a_correct_result_and_reports_headroom():
    x, w, _ = _operands(2, 7, 1280, 32, 1)
    ref, S = R.conv_fwd(x, w)
    r = _ratio(_sim_conv(x, w), ref, S, 9 * 1280)
    assert 0.0 < r < 1.0


def test_comparator_names_the_worst_element():
    x, w, _ = _operands(1, 5, 64, 16, 2)
    ref, S = R.conv_fwd(x, w)
    got = _sim_conv(x, w).float()
    got[0, 3, 1, 9] += 1.0
    with pytest.raises(AssertionError, match=r"1 of 400 elements out of bound; worst at \(0, 3, 1, 9\)"):
        _ratio(got, ref, S, 9 * 64)
    got[0, 3, 1, 9] = float("nan")
    with pytest.raises(AssertionError, match=r"worst at \(0, 3, 1, 9\): got nan"):
        _ratio(got, ref, S, 9 * 64)


def test_rejects_one_missing_tap():
    x, w, _ = _operands(2, 14, 320, 32, 3)
    ref, S = R.conv_fwd(x, w)
    _ratio(_sim_conv(x, w), ref, S, 9 * 320)
    wb = w.clone()
    wb[:, :, 2, 0] = 0.0                        # tap (kh, kw) = (2, 0) never gathered
    with pytest.raises(AssertionError, match="out of bound"):
        _ratio(_sim_conv(x, wb), ref, S, 9 * 320)


@pytest.mark.parametrize("Cin", [1280, 2560])
def test_rejects_one_missing_k_slice(Cin):
    """One 16-channel slice of one tap out of K = 11 520 / 23 040 (the 7x7 1280- and 2560-channel layers): an error of
    sqrt(16 / K) of the output's spread, ~2.6-3.7 %, which a max-relative bar of 3e-2 lets through."""
    x, w, _ = _operands(2, 7, Cin, 32, 4)
    K = 9 * Cin
    ref, S = R.conv_fwd(x, w)
    _ratio(_sim_conv(x, w), ref, S, K)
    wb = w.clone()
    wb[:, 1008:1024, 1, 1] = 0.0
    bad = _sim_conv(x, wb)
    spread = float((bad.double() - ref).abs().max() / ref.abs().max())
    assert spread < 0.1                          # (the size of the slip, for scale: the same order as 3e-2)
    with pytest.raises(AssertionError, match="out of bound"):
        _ratio(bad, ref, S, K)


def test_rejects_two_swapped_output_channels():
    x, w, _ = _operands(2, 7, 640, 32, 5)
    ref, S = R.conv_fwd(x, w)
    got = _sim_conv(x, w)
    got[..., [21, 22]] = got[..., [22, 21]]     # adjacent columns inside the 16-column block 16..31
    with pytest.raises(AssertionError, match="out of bound"):
        _ratio(got, ref, S, 9 * 640)


def test_rejects_a_shifted_partial_last_tile():
    """M = 2 * 7 * 7 = 98 rows in tiles of 64: the rows of the last, partial tile (64..97) land one row off."""
    x, w, _ = _operands(2, 7, 640, 32, 6)
    ref, S = R.conv_fwd(x, w)
    good = _sim_conv(x, w).reshape(-1, 32)
    got = good.clone()
    got[65:98] = good[64:97]
    with pytest.raises(AssertionError, match="out of bound"):
        _ratio(got.reshape(ref.shape), ref, S, 9 * 640)


def test_rejects_a_missing_bias_channel():
    x, w, g = _operands(2, 7, 640, 32, 7)
    bias = torch.randn(32, generator=g) * 0.3
    acc, S = R.conv_fwd(x, w)
    ref, Sy, A = R.epilogue(acc, S, bias=bias)
    _ratio(_sim_conv(x, w, bias=bias), ref, Sy, 9 * 640, extra=A)
    bb = bias.clone()
    bb[13] = 0.0
    with pytest.raises(AssertionError, match="out of bound"):
        _ratio(_sim_conv(x, w, bias=bb), ref, Sy, 9 * 640, extra=A)


def test_rejects_alpha_off_by_one_percent():
    x, w, g = _operands(2, 7, 1280, 32, 8)
    bias = torch.randn(32, generator=g) * 0.3
    res = _bf(torch.randn(2, 7, 7, 32, generator=g))
    acc, S = R.conv_fwd(x, w)
    ref, Sy, A = R.epilogue(acc, S, bias=bias, residual=res, alpha=0.7)
    _ratio(_sim_conv(x, w, bias=bias, residual=res, alpha=0.7), ref, Sy, 9 * 1280, extra=A)
    with pytest.raises(AssertionError, match="out of bound"):
        _ratio(_sim_conv(x, w, bias=bias, residual=res, alpha=0.707), ref, Sy, 9 * 1280, extra=A)
