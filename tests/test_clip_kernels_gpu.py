"""-m gpu: the CLIP kernels (csrc/clip.hip) and the quick-GELU epilogue against the float64 restatement of tests/clip_ref.py:
psg_clip_prep_fwd / _bwd, psg_attn_fwd_causal, psg_cosine_loss, ops.linear(act=ACT_QUICK_GELU).  Every bound is `clip_ref.bar`:
four times the error of torch on the CPU in the same precision on the same case, floored at 1e-6.

Below them the same kernels through the C ABI on the cases of tests/clip_cases.py, element by element: guarded NaN-filled
buffers on the least alignment and with the row strides the header allows, every element within the derived bound of the fp64
reference of the operands the kernel read (tests/clip_ref.py, tests/attn_ref.py), guards and unwritten columns untouched,
identical bits from identical launches and with or without the optional output.  Every comparison prints
`RATIO <what> <err / bound>` before it asserts (0 = a bit comparison).  A device error ends the run."""
import os

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


# ---- element by element, through the C ABI (tests/clip_cases.py) -----------------------------------------------------------
from tests import clip_cases as KC  # noqa: E402

REPORT = os.environ.get("PSG_CLIP_REPORT")           # optional: append each case's worst err / bound to this file


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    return _lib.init(0)


def _ratio(what, ratios):
    line = f"{what} " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items())
    print("RATIO " + line)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write("gpu " + line + "\n")


def _run(rc, what):
    from pokemon_sprite_generator_amd import _lib
    _lib.check(rc, what)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                          # a device error: nothing more runs on this GPU
        pytest.exit(f"{what}: {e}", returncode=3)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _least_aligned(pair, what):
    """The view starts on a 4-element boundary and not on the next larger one (bf16: 8 bytes, not 16; fp32: 16, not 32)."""
    n = 4 * pair[1].element_size()
    assert pair[1].data_ptr() % (2 * n) == n, f"{what}: base {pair[1].data_ptr():#x}"


@pytest.mark.parametrize("name", [c["name"] for c in KC.CAUSAL])
def test_causal_elementwise(lib, name):
    from pokemon_sprite_generator_amd import _lib
    c = KC.CAUSAL_BY_NAME[name]
    dt, code = KC.DTYPES[c["dtype"]], KC.DTYPE_CODE[c["dtype"]]
    B, L, H, d = c["B"], c["L"], c["heads"], c["d"]
    E, ld = H * d, KC.causal_ld(c)
    ops = KC.causal_operands(name)
    src = {n: KC.filled(t.reshape(B * L, E), ld[n], dt, DEV) for n, t in zip("qkv", ops)}
    outs = []
    for with_lse in (True, False, True):
        ob = KC.alloc(B * L, ld["o"], dt, DEV)
        lb = KC.alloc(1, B * H * L, torch.float32, DEV) if with_lse else None
        for n, pair in list(src.items()) + [("o", ob)]:
            _least_aligned(pair, f"{name} {n}")
        _run(lib.psg_attn_fwd_causal(src["q"][1].data_ptr(), ld["q"], src["k"][1].data_ptr(), ld["k"], src["v"][1].data_ptr(), ld["v"],
                                     ob[1].data_ptr(), ld["o"], lb[1].data_ptr() if lb else None, B, H, L, L, d, c["scale"], 0.0, 0, code,
                                     _lib.stream_ptr()), "psg_attn_fwd_causal " + name)
        KC.guards_ok(ob, E, f"{name} o")
        if lb:
            KC.guards_ok(lb, B * H * L, f"{name} lse")
        outs.append((ob, lb))
    (ob, lb), (ob_nolse, _), (ob2, lb2) = outs
    o = ob[1][:, :E].reshape(B, L, E)
    _ratio(f"causal {name}", KC.causal_check(o, lb[1].view(B, H, L), name, name))
    assert torch.equal(_bits(ob[0]), _bits(ob_nolse[0])), f"{name}: o depends on whether lse is asked for"
    assert torch.equal(_bits(ob[0]), _bits(ob2[0])) and torch.equal(_bits(lb[0]), _bits(lb2[0])), f"{name}: two identical launches differ"
    assert torch.equal(_bits(o[:, 0].contiguous()), _bits(ops[2][:, 0].to(DEV, dt).contiguous())), f"{name}: row 0 is not v[0] to the bit"


def _prep_fwd(lib, img_pair, B, Hi, S, P, a, b, extra, dt, what):
    from pokemon_sprite_generator_amd import _lib
    G = S // P
    yb = KC.alloc(B * G * G, 3 * P * P + extra, dt, DEV)
    _run(lib.psg_clip_prep_fwd(img_pair[1].data_ptr(), yb[1].data_ptr(), 3 * P * P + extra, B, Hi, Hi, S, P, a, b, _lib.dtype_code(dt),
                               _lib.stream_ptr()), what)
    KC.guards_ok(yb, 3 * P * P, what)
    return yb


def _prep_bwd(lib, dy_pair, B, Hi, S, P, a, dt, what):
    from pokemon_sprite_generator_amd import _lib
    gb = KC.alloc(1, B * 3 * Hi * Hi, torch.float32, DEV)               # NaN-poisoned: every element must be written
    _run(lib.psg_clip_prep_bwd(dy_pair[1].data_ptr(), dy_pair[1].shape[1], gb[1].data_ptr(), B, Hi, Hi, S, P, a, _lib.dtype_code(dt),
                               _lib.stream_ptr()), what)
    KC.guards_ok(gb, B * 3 * Hi * Hi, what)
    return gb


@pytest.mark.parametrize("dn", list(KC.DTYPES))
@pytest.mark.parametrize("B", KC.PREP_BATCHES)
@pytest.mark.parametrize("Hi,S,P", KC.PREP_SHAPES)
def test_prep_elementwise(lib, Hi, S, P, B, dn):
    """Every (a, b) and row stride of the table.  fp32: each element within K_PREP 2^-24 Mag of the fp64 reference.  bf16: the
    kernel stores (bf16_t)v, round to nearest even (psg_common.h Elem<bf16_t>::st), so the launch must equal the fp32 launch's
    result converted with .to(torch.bfloat16) bit for bit.  The backward reads the bf16-representable dy exactly in both."""
    dt = KC.DTYPES[dn]
    img, dy = KC.prep_operands(Hi, S, P, B)
    imgb = KC.filled(img.reshape(1, -1), img.numel(), torch.float32, DEV)
    worst = {"fwd": 0.0, "bwd": 0.0}
    for a, b in KC.PREP_AB:
        ref, mag = R.prep_fwd_ref(img, S, P, a, b)
        g, M = R.prep_bwd_ref(dy, B, Hi, S, P, a)
        for extra in KC.PREP_LD_EXTRA:
            what = f"prep {Hi}->{S} P{P} B{B} {dn} a{a} b{b} ld+{extra}"
            y32 = _prep_fwd(lib, imgb, B, Hi, S, P, a, b, extra, torch.float32, what + " fwd")
            if dn == "f32":
                worst["fwd"] = max(worst["fwd"], R.check_bound(y32[1][:, :3 * P * P], ref, R.prep_fwd_bound(mag), what + " fwd"))
                again = _prep_fwd(lib, imgb, B, Hi, S, P, a, b, extra, torch.float32, what + " fwd")
                assert torch.equal(_bits(y32[0]), _bits(again[0])), f"{what}: two identical launches differ"
            else:
                y16 = _prep_fwd(lib, imgb, B, Hi, S, P, a, b, extra, dt, what + " fwd")
                assert torch.equal(_bits(y16[1][:, :3 * P * P].contiguous()), _bits(y32[1][:, :3 * P * P].to(dt).contiguous())), \
                    f"{what}: the bf16 launch is not the fp32 launch rounded to nearest even"
            dyb = KC.filled(dy, 3 * P * P + extra, dt, DEV)
            gb = _prep_bwd(lib, dyb, B, Hi, S, P, a, dt, what + " bwd")
            worst["bwd"] = max(worst["bwd"], R.check_bound(gb[1].view(B, 3, Hi, Hi), g, R.prep_bwd_bound(M), what + " bwd"))
            assert torch.equal(_bits(gb[0]), _bits(_prep_bwd(lib, dyb, B, Hi, S, P, a, dt, what + " bwd")[0])), f"{what}: two identical launches differ"
    _ratio(f"prep {Hi}->{S} P{P} B{B} {dn}", worst)


def test_prep_same_size_through_the_abi_with_a_stride(lib):
    """test_prep_same_size_does_no_resampling on strided rows: Hi == S, every output ((a x + b) - mean) * inv_std of ONE pixel and
    every gradient one dy times inv_std times a, to the bit."""
    B, S, P, extra = 3, 16, 4, 8
    img, dy = KC.prep_operands(S, S, P, B)
    imgb = KC.filled(img.reshape(1, -1), img.numel(), torch.float32, DEV)
    mean = torch.tensor(R.MEAN, device=DEV).view(1, 3, 1, 1)
    inv = (1.0 / torch.tensor(R.STD, device=DEV)).view(1, 3, 1, 1)
    x = img.to(DEV)
    for a, b in KC.PREP_AB:
        yb = _prep_fwd(lib, imgb, B, S, S, P, a, b, extra, torch.float32, "prep same-size fwd")
        want = R.rows_of(((a * x + b) - mean) * inv, P)
        assert torch.equal(yb[1][:, :3 * P * P], want), (a, b)
        dyb = KC.filled(dy, 3 * P * P + extra, torch.float32, DEV)
        gb = _prep_bwd(lib, dyb, B, S, S, P, a, torch.float32, "prep same-size bwd")
        assert torch.equal(gb[1].view(B, 3, S, S), R.pixels_of(dy.to(DEV), B, S, P) * inv * a), (a, b)
    _ratio("prep same-size strided", {"fwd": 0.0, "bwd": 0.0})


@pytest.mark.parametrize("dn", list(KC.DTYPES))
@pytest.mark.parametrize("D", KC.COS_D)
@pytest.mark.parametrize("B", KC.COS_B)
def test_cosine_elementwise(lib, B, D, dn):
    from pokemon_sprite_generator_amd import _lib
    dt, code, ld = KC.DTYPES[dn], KC.DTYPE_CODE[dn], KC.cosine_ld(D)
    worst = {}
    for kind in KC.COS_KINDS if B > 1 else ("none",):
        what = f"cosine B{B} D{D} {dn} {kind}"
        u, v = KC.cosine_operands(B, D, kind, dn)
        ub, vb = KC.filled(u, ld["u"], dt, DEV), KC.filled(v, ld["v"], dt, DEV)
        outs = []
        for with_du in (True, False, True):
            db = KC.alloc(B, ld["du"], dt, DEV) if with_du else None
            sb = KC.alloc(1, 1, torch.float32, DEV)
            for n, pair in (("u", ub), ("v", vb)) + ((("du", db),) if db else ()):
                _least_aligned(pair, f"{what} {n}")
            _run(lib.psg_cosine_loss(ub[1].data_ptr(), ld["u"], vb[1].data_ptr(), ld["v"], db[1].data_ptr() if db else None, ld["du"] if db else 0,
                                     sb[1].data_ptr(), B, D, code, _lib.stream_ptr()), "psg_cosine_loss " + what)
            KC.guards_ok(sb, 1, what + " out")
            if db:
                KC.guards_ok(db, D, what + " du")
            outs.append((sb, db))
        (sb, db), (sb_nodu, _), (sb2, db2) = outs
        for k, w in KC.cosine_check(sb[1].reshape(()), db[1][:, :D], B, D, kind, dn, what).items():
            worst[k] = max(worst.get(k, 0.0), w)
        assert torch.equal(_bits(sb[0]), _bits(sb_nodu[0])), f"{what}: the loss depends on whether du is asked for"
        assert torch.equal(_bits(sb[0]), _bits(sb2[0])) and torch.equal(_bits(db[0]), _bits(db2[0])), f"{what}: two identical launches differ"
    _ratio(f"cosine B{B} D{D} {dn}", worst)
