"""-m gpu: the CLIP kernels (csrc/clip.hip) and the quick-GELU epilogue against the float64 restatement of tests/clip_ref.py:
psg_clip_prep_fwd / _bwd, psg_attn_fwd_causal, psg_cosine_loss, ops.linear(act=ACT_QUICK_GELU).  Every bound is `clip_ref.bar`:
four times the error of torch on the CPU in the same precision on the same case, floored at 1e-6."""
import pytest
import torch
import torch.nn.functional as F

from tests import clip_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from pokemon_sprite_generator_amd import _lib, ops as o
    _lib.init(0)
    return o


def _check(got, key, prec):
    errs = R.errors(got, key)
    bars = {n: R.bar(key + (prec,), n) for n in errs}
    print(f"{key} {prec}: " + ", ".join(f"{n} {errs[n]:.3e} (bar {bars[n]:.3e})" for n in errs))
    for n in errs:
        assert errs[n] <= bars[n], f"{key} {prec} {n}: {errs[n]:.3e} > {bars[n]:.3e}"


@pytest.mark.parametrize("prec", list(R.PRECISIONS))
@pytest.mark.parametrize("B", R.PREP_BATCHES)
@pytest.mark.parametrize("Hi,S,P", R.PREP_CASES)
def test_prep_forward_and_backward(ops, Hi, S, P, B, prec):
    dt = R.PRECISIONS[prec]
    img, dy = R.prep_inputs(Hi, S, P, B)
    x = img.to(DEV).requires_grad_(True)
    rows = ops.clip_prep(x, S, P, 0.5, 0.5, dt)
    G = S // P
    assert rows.dtype == dt and tuple(rows.shape) == (B, G * G, 3 * P * P)
    (rows.float() * dy.to(DEV)).sum().backward()
    assert x.grad.dtype == torch.float32 and x.grad.shape == x.shape
    _check(dict(fwd=rows, bwd=x.grad), ("prep", Hi, S, P, B), prec)
    # layout and resize without the restatement: the kernel's rows against F.unfold of torch's own antialiased resize in float64
    v = 0.5 * img.double() + 0.5
    if Hi != S:
        v = F.interpolate(v, size=(S, S), mode="bicubic", align_corners=False, antialias=True)
    pv = (v - torch.tensor(R.MEAN, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(R.STD, dtype=torch.float64).view(1, 3, 1, 1)
    assert R.rel(rows, F.unfold(pv, P, stride=P).transpose(1, 2)) <= R.bar(("prep", Hi, S, P, B, prec), "fwd")
    r, c, ky, kx = G + 1 if G > 1 else 0, 2, P - 3, 1                  # one element by hand: patch r, column c P^2 + ky P + kx
    want = float(pv[B - 1, c, (r // G) * P + ky, (r % G) * P + kx])
    got = float(rows.detach()[B - 1, r, c * P * P + ky * P + kx])
    assert abs(got - want) <= (2 ** -7 if prec == "bf16" else 1e-5) * max(1.0, abs(want))


def test_prep_same_size_does_no_resampling(ops):
    """Hi == S: every output is (0.5 x + 0.5 - mean) * inv_std of ONE pixel and every gradient one dy times 0.5 * inv_std."""
    img = R.image("same", 1, 16).to(DEV).requires_grad_(True)
    rows = ops.clip_prep(img, 16, 8)
    pv = F.fold(rows.transpose(1, 2), (16, 16), 8, stride=8)
    mean = torch.tensor(R.MEAN, device=DEV).view(1, 3, 1, 1)
    inv = (1.0 / torch.tensor(R.STD, device=DEV)).view(1, 3, 1, 1)
    assert torch.equal(pv, ((0.5 * img.detach() + 0.5) - mean) * inv)
    rows.sum().backward()
    assert torch.equal(img.grad, (0.5 * inv).expand_as(img) * 1.0)


def test_prep_rejects_what_it_does_not_compute(ops):
    from pokemon_sprite_generator_amd import _lib
    lib = _lib.init(0)
    y = torch.empty(4 * 192 * 2, device=DEV)
    img = torch.zeros(1, 3, 17, 17, device=DEV)
    f = lib.psg_clip_prep_fwd
    assert f(_lib.ptr(img), _lib.ptr(y), 192, 1, 17, 17, 16, 8, 0.5, 0.5, 0, None) == -1          # Hi > S
    assert f(_lib.ptr(img), _lib.ptr(y), 192, 1, 8, 9, 16, 8, 0.5, 0.5, 0, None) == -1            # Hi != Wi
    assert f(_lib.ptr(img), _lib.ptr(y), 192, 1, 8, 8, 18, 8, 0.5, 0.5, 0, None) == -1            # S % P != 0
    with pytest.raises(_lib.PsgError, match="square"):
        ops.clip_prep(torch.zeros(1, 3, 8, 9, device=DEV), 16, 8)
    with pytest.raises(_lib.PsgError):
        ops.clip_prep(torch.zeros(1, 3, 17, 17, device=DEV), 16, 8)


@pytest.mark.parametrize("prec", list(R.PRECISIONS))
@pytest.mark.parametrize("L,d", R.CAUSAL_CASES)
def test_causal_attention(ops, L, d, prec):
    dt = R.PRECISIONS[prec]
    qkv = R.causal_inputs(L, d).to(DEV).to(dt)
    with torch.no_grad():
        o = ops.attention_causal(qkv, 2)
    assert o.dtype == dt and tuple(o.shape) == (2, L, 2 * d)
    _check(dict(out=o), ("causal", L, d), prec)
    assert torch.equal(o[:, 0], qkv[:, 0, 4 * d:])                    # query 0 sees key 0 alone: the row is v[0], to the bit
    with pytest.raises(RuntimeError):
        ops.attention_causal(qkv.clone().requires_grad_(True), 2)     # forward only


def test_causal_attention_ignores_later_keys(ops):
    """Changing token s changes no output row before s (and the log-sum-exp the entry can write matches the masked softmax)."""
    from pokemon_sprite_generator_amd import _lib
    lib = _lib.init(0)
    L, d = 17, 16
    qkv = R.causal_inputs(L, d).to(DEV)
    with torch.no_grad():
        a = ops.attention_causal(qkv, 2)
        other = qkv.clone()
        other[:, 9:] = 3.0
        b = ops.attention_causal(other, 2)
    assert torch.equal(a[:, :9], b[:, :9]) and not torch.equal(a[:, 9:], b[:, 9:])
    o = torch.empty(2, L, 2 * d, device=DEV)
    lse = torch.empty(2, 2, L, device=DEV)
    p = qkv.data_ptr()
    _lib.check(lib.psg_attn_fwd_causal(p, 96, p + 4 * 32, 96, p + 4 * 64, 96, _lib.ptr(o), 32, _lib.ptr(lse), 2, 2, L, L, d, d ** -0.5, 0.0, 0, 0,
                                       _lib.stream_ptr()), "psg_attn_fwd_causal")
    q, k, _ = (t.view(2, L, 2, d).transpose(1, 2).double() for t in qkv.split(32, -1))
    s = (q @ k.transpose(-1, -2) * d ** -0.5).masked_fill(torch.ones(L, L, dtype=torch.bool, device=DEV).triu(1), float("-inf"))
    assert torch.equal(o, a) and R.rel(lse, torch.logsumexp(s, -1)) < 1e-6


@pytest.mark.parametrize("prec", list(R.PRECISIONS))
@pytest.mark.parametrize("B,D,zero", R.COSINE_CASES)
def test_cosine_loss(ops, B, D, zero, prec):
    dt = R.PRECISIONS[prec]
    x, v = R.cosine_inputs(B, D, zero)
    xs = x.to(DEV).to(dt).requires_grad_(True)
    vs = v.to(DEV).to(dt).requires_grad_(True)                         # the text side is a constant even when it asks
    out = ops.cosine_loss(xs, vs)
    assert out.dtype == torch.float32 and out.dim() == 0
    out.backward()
    assert xs.grad.dtype == dt and vs.grad is None
    _check(dict(loss=out.detach(), du=xs.grad), ("cosine", B, D, zero), prec)
    with torch.no_grad():                                              # no gradient asked: the same value
        assert torch.equal(ops.cosine_loss(xs.detach(), v.to(DEV).to(dt)), out.detach())


@pytest.mark.parametrize("prec", list(R.PRECISIONS))
def test_quick_gelu_through_linear(ops, prec):
    dt = R.PRECISIONS[prec]
    x, w, b, dy = R.qgelu_inputs()
    xs = x.to(DEV).to(dt).requires_grad_(True)
    ws, bs = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    y = ops.linear(xs, ws, bs, act=ops.ACT_QUICK_GELU)
    (y.float() * dy.to(DEV)).sum().backward()
    _check(dict(fwd=y, dx=xs.grad, dw=ws.grad, db=bs.grad), ("qgelu",), prec)
