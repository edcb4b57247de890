"""Every GEMM launch form of the bf16 train step at batch 256 (BASELINE configs[2]) against a float64 reference.

One case per distinct launch form: the U-Net's 3x3 / 1x1 / stride-2 convs, attention Linears, the FFN, the ProjGroup and
time-MLP Linears, each through the public ops with the U-Net's own epilogue (bias, row-add, residual, alpha, GELU / SiLU,
dropout, concat-slot output).  Forward, data gradient, weight / bias / row-add gradients are checked element by element
with tests/gemm_ref.check (fp64 reference, bound from the output rounding and the fp32 accumulation over K).  Where a
launch reads an intermediate the op made itself (an activation's backward gradient, the FFN's hidden activation and
saved derivative), the intermediate is checked against its own fp64 value and the next GEMM against the operand it read.

test_table_covers_every_gemm_launch_of_the_b256_train_step records the launch keys of one real train step and fails,
naming the missing keys, if the table stops covering one.  PSG_GEMM_B256_REPORT=path appends each case's worst
err / bound ratios and its fp64 time as JSON lines."""
import json
import math
import os
import time

import pytest
import torch
import torch.nn as nn

from tests import gemm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 256
BF = torch.bfloat16
P = 0.05                 # unet.ATTN_DROPOUT
TEXT_S = 32              # text tokens of the benchmark batch
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from pokemon_sprite_generator_amd import _lib, ops as o
    _lib.init(0)
    return o


# ------------------------------------------------------------------------------------------------------------ launches
class _Launches:
    """Wraps ops._conv_launch / ops._wgrad_launch (as tools/layer_table.py does): the distinct launch keys, which of them
    took a split-K workspace, the border-class order or the persistent pointwise kernel, and (keep=True) every launch's
    operands, which stay alive for the references."""

    def __init__(self, monkeypatch, keep=False):
        from pokemon_sprite_generator_amd import _lib, ops
        self.keep, self.keys, self.calls = keep, {}, []
        lib = _lib.init(0)
        counters = lambda: (ops.SplitKStats.launches, int(lib.psg_conv_tapclass_launches()), int(lib.psg_conv_pw_launches()))
        oc, ow = ops._conv_launch, ops._wgrad_launch

        def note(key, before, operands):
            after = counters()
            took = tuple(a > b for a, b in zip(after, before))
            old = self.keys.get(key, (False, False, False))
            self.keys[key] = tuple(o or t for o, t in zip(old, took))
            if self.keep:
                self.calls.append((key[0], operands))

        def conv(lib_, dtype, x, ldx, w, ldw, y, ldy, geom, Cin, Cout, transposed=False, bias=None, rowadd=None, residual=None,
                 ld_res=0, preact=None, dact_u=None, ld_dact=0, act=0, alpha=1.0, drop_p=0.0, seed=0, flags=0):
            key = ("dgrad" if transposed else "fwd", tuple(geom), Cin, Cout, ldx != Cin, ldy != Cout, int(act), bias is not None,
                   rowadd is not None, residual is not None, preact is not None, dact_u is not None, int(flags), drop_p > 0,
                   alpha != 1.0)
            before = counters()
            oc(lib_, dtype, x, ldx, w, ldw, y, ldy, geom, Cin, Cout, transposed=transposed, bias=bias, rowadd=rowadd,
               residual=residual, ld_res=ld_res, preact=preact, dact_u=dact_u, ld_dact=ld_dact, act=act, alpha=alpha, drop_p=drop_p,
               seed=seed, flags=flags)
            note(key, before, dict(x=x, y=y, preact=preact, dact_u=dact_u))

        def wgrad(lib_, dtype, x, ldx, dy, lddy, dw, geom, Cin, Cout, accumulate=False, dbias=None, accumulate_bias=False, scale=1.0):
            key = ("wgrad", tuple(geom), Cin, Cout, ldx != Cin, lddy != Cout, ops.weight_layout(dw), bool(accumulate),
                   dbias is not None, scale != 1.0)
            before = counters()
            ow(lib_, dtype, x, ldx, dy, lddy, dw, geom, Cin, Cout, accumulate=accumulate, dbias=dbias,
               accumulate_bias=accumulate_bias, scale=scale)
            note(key, before, dict(x=x, dy=dy))

        monkeypatch.setattr(ops, "_conv_launch", conv)
        monkeypatch.setattr(ops, "_wgrad_launch", wgrad)

    def operand(self, kind, name, i=0):
        """The `name` operand of the i-th recorded launch of `kind` (fwd / dgrad / wgrad)."""
        return [c for k, c in self.calls if k == kind][i][name]


# ------------------------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _act(shape, g, scale=1.0):
    return (torch.randn(shape, device=DEV, generator=g) * scale).to(BF)


def _weight(shape, g, conv):
    """fp32 Parameter holding bf16-representable values (the kernels read its bf16 copy), OHWI for a conv weight (the
    parameter arena's order, as in test_conv_ohwi_master_weights)."""
    K = 1
    for n in shape[1:]:
        K *= n
    w = (torch.randn(shape, device=DEV, generator=g) * math.sqrt(1.0 / K)).to(BF).float()
    if conv:
        w = w.contiguous(memory_format=torch.channels_last)
    return nn.Parameter(w)


def _bias(n, g):
    return nn.Parameter(torch.randn(n, device=DEV, generator=g) * 0.3)


def _slot(ops, shape, C1, g):
    """A decoder concat slot whose whole buffer is NaN: the op under test writes buf[..., :C1]."""
    skip = _act(tuple(shape[:-1]) + (shape[-1] - C1,), g)
    s = ops.ConcatSlot(skip, C1)
    s.buf.fill_(NAN)
    return s, skip


def _check_slot(s, C1):
    assert not bool(torch.isnan(s.buf[..., :C1]).any()), "a store is missing inside the slot"
    assert bool(torch.isnan(s.buf[..., C1:]).all()), "a store landed outside the slot"


def _sync_time():
    torch.cuda.synchronize()
    return time.perf_counter()


def _report(case, ratios, secs):
    path = os.environ.get("PSG_GEMM_B256_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": case, "ratios": ratios, "fp64_s": round(secs, 3)}) + "\n")


def _scaled(refS, s):
    return refS[0] * s, refS[1] * abs(s)


def _free():
    from pokemon_sprite_generator_amd import ops
    ops.WeightCache.clear()                 # (it keeps every parameter it prepared alive)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- cases
def _conv_case(ops, mp, fp64, H, Cin, Cout, ks=3, stride=1, rowadd=False, residual=False, slot=False, dx=True,
               strided_grad=False, seed=0):
    """ops.conv2d with the U-Net's epilogue forms; `slot`: the result goes into a concat slot and its gradient comes back
    with row stride 2 Cout; `strided_grad`: only the gradient does (the residual branch of a conv that writes a slot)."""
    g = _gen(seed)
    pad = ks // 2
    Ho = (H + 2 * pad - ks) // stride + 1
    x = _act((B, H, H, Cin), g).requires_grad_(dx)
    w, b = _weight((Cout, Cin, ks, ks), g, True), _bias(Cout, g)
    ra_full = _act((B, 2 * Cout), g, 0.5).requires_grad_(True) if rowadd else None
    ra = ra_full[:, Cout:] if rowadd else None                  # a column slice, like the ProjGroup's per-block views
    res = _act((B, Ho, Ho, Cout), g).requires_grad_(True) if residual else None
    rec = _Launches(mp, keep=fp64)
    s, skip = _slot(ops, (B, Ho, Ho, 2 * Cout), Cout, g) if slot else (None, None)
    y = ops.conv2d(x, w, b, stride=stride, rowadd=ra, residual=res, out=s.out if slot else None)
    if slot:
        _check_slot(s, Cout)
        top = s.cat(y, skip)
        dtop = _act(tuple(top.shape), g)
        dy = dtop[..., :Cout]                                   # the slot's gradient: row stride 2 * Cout
    elif strided_grad:
        top = y
        dtop = dy = _act((B, Ho, Ho, 2 * Cout), g)[..., Cout:]
    else:
        top = y
        dtop = dy = _act(tuple(y.shape), g)
    top.backward(dtop)
    if not fp64:
        return rec.keys
    t0 = _sync_time()
    r = {}
    acc, S = R.conv_fwd(x, w, stride)
    ref, Sy, A = R.epilogue(acc, S, bias=b, rowadd=ra, residual=res)
    del acc, S
    r["fwd"] = R.check(y, ref, Sy, BF, "forward", Cin * ks * ks, extra=A)
    del ref, Sy, A
    if dx:
        ref, S = R.conv_dgrad(dy, w, (H, H), stride)
        r["dgrad"] = R.check(x.grad, ref, S, BF, "data gradient", Cout * ks * ks)
        del ref, S
    M = B * Ho * Ho
    ref, S = R.conv_wgrad(x, dy, ks, stride)
    assert w.grad.stride() == w.stride(), "the weight gradient must keep the parameter's memory order"
    r["wgrad"] = R.check(w.grad, ref, S, torch.float32, "weight gradient", M)
    del ref, S
    r["dbias"] = R.check(b.grad, *R.bias_grad(dy), torch.float32, "bias gradient", M)
    if rowadd:
        r["drowadd"] = R.check(ra_full.grad[:, Cout:], *R.rowadd_grad(dy), BF, "row-add gradient", Ho * Ho)
        assert bool((ra_full.grad[:, :Cout] == 0).all())
    if residual:
        assert torch.equal(res.grad, dy), "residual gradient"
    return r, _sync_time() - t0


ACTS = {"none": 0, "silu": 1, "gelu": 2}


def _linear_case(ops, mp, fp64, lead, Cin, Cout, kind="none", residual=False, alpha=1.0, dx=True, seed=0):
    """ops.linear(x, w, b, residual, act, alpha) on x [*lead, Cin]; the U-Net's Linears have no dropout outside the FFN."""
    g = _gen(seed)
    x = _act(tuple(lead) + (Cin,), g).requires_grad_(dx)
    w, b = _weight((Cout, Cin), g, False), _bias(Cout, g)
    res = _act(tuple(lead) + (Cout,), g).requires_grad_(True) if residual else None
    from pokemon_sprite_generator_amd import _lib
    code = {"none": _lib.ACT_NONE, "silu": _lib.ACT_SILU, "gelu": _lib.ACT_GELU}[kind]
    rec = _Launches(mp, keep=fp64)
    y = ops.linear(x, w, b, residual=res, act=code, alpha=alpha)
    dy = _act(tuple(y.shape), g)
    y.backward(dy)
    if not fp64:
        return rec.keys
    t0 = _sync_time()
    r = {}
    acc, S = R.linear_fwd(x, w)
    ref, Sy, A = R.epilogue(acc, S, bias=b, residual=res, kind=kind, alpha=alpha)
    r["fwd"] = R.check(y, ref, Sy, BF, "forward", Cin, extra=A)
    M = y.numel() // Cout
    if kind != "none":
        # the pre-activation the forward saved, and the accumulator gradient backward made from it (psg_epilogue_bwd)
        pre = rec.operand("fwd", "preact")
        u, Su, _ = R.epilogue(acc, S, bias=b)
        r["preact"] = R.check(pre, u, Su, BF, "saved pre-activation", Cin)
        gk = rec.operand("wgrad", "dy")
        gref = R.epilogue_bwd(dy, pre, kind=kind, alpha=alpha)
        r["g"] = R.check(gk, gref.reshape(gk.shape), torch.zeros_like(gref).reshape(gk.shape), BF, "epilogue gradient", 1,
                         extra=gref.abs().reshape(gk.shape) * R.ACT_APPROX[kind] * 4)
        gate = 1.0
    else:
        gk, gate = dy, alpha                                    # g = dy; alpha rides in the dgrad epilogue and the wgrad scale
    del acc, S, ref, Sy, A
    if dx:
        r["dgrad"] = R.check(x.grad, *_scaled(R.linear_dgrad(gk, w), gate), BF, "data gradient", Cout)
    r["wgrad"] = R.check(w.grad, *_scaled(R.linear_wgrad(x, gk), gate), torch.float32, "weight gradient", M)
    r["dbias"] = R.check(b.grad, *_scaled(R.bias_grad(gk), gate), torch.float32, "bias gradient", M)
    if residual:
        assert torch.equal(res.grad, dy), "residual gradient"
    return r, _sync_time() - t0


def _cross_case(ops, mp, fp64, L, C, seed=0):
    """ops.cross_in_proj: q = xn W[:C]^T + b[:C] at M = 256 L, kv = tp W[C:]^T + b[C:] at M = 256 * 32, one packed parameter."""
    g = _gen(seed)
    xn = _act((B, L, C), g).requires_grad_(True)
    tp = _act((B, TEXT_S, C), g).requires_grad_(True)
    w, b = _weight((3 * C, C), g, False), _bias(3 * C, g)
    rec = _Launches(mp)
    q, kv = ops.cross_in_proj(xn, tp, w, b)
    dq, dkv = _act(tuple(q.shape), g), _act(tuple(kv.shape), g)
    torch.autograd.backward([q, kv], [dq, dkv])
    if not fp64:
        return rec.keys
    t0 = _sync_time()
    r = {}
    wq, wkv = w.detach()[:C], w.detach()[C:]
    for nm, src, wp, bp, out, d in (("q", xn, wq, b.detach()[:C], q, dq), ("kv", tp, wkv, b.detach()[C:], kv, dkv)):
        acc, S = R.linear_fwd(src, wp)
        ref, Sy, A = R.epilogue(acc, S, bias=bp)
        r[nm + ".fwd"] = R.check(out, ref, Sy, BF, nm + " forward", C, extra=A)
        r[nm + ".dgrad"] = R.check(src.grad, *R.linear_dgrad(d, wp), BF, nm + " data gradient", wp.shape[0])
    r["wgrad"] = R.check(w.grad, *[torch.cat(p) for p in zip(R.linear_wgrad(xn, dq), R.linear_wgrad(tp, dkv))],
                         torch.float32, "weight gradient", B * max(L, TEXT_S))
    r["dbias"] = R.check(b.grad, *[torch.cat(p) for p in zip(R.bias_grad(dq), R.bias_grad(dkv))], torch.float32, "bias gradient",
                         B * max(L, TEXT_S))
    return r, _sync_time() - t0


def _drop_masks(ops, M, C, Hd, s1, s2):
    """The two keep masks of the FFN's dropouts, read off probe launches (the mask is a function of seed and element index
    only), as test_ffn_gelu_dropout_backward does."""
    with torch.no_grad():
        z1 = ops.linear(torch.zeros(M, C, device=DEV, dtype=BF), torch.zeros(Hd, C, device=DEV), torch.ones(Hd, device=DEV),
                        act=ops.ACT_GELU, drop_p=P, seed=s1)
        z2 = ops.linear(torch.zeros(M, Hd, device=DEV, dtype=BF), torch.zeros(C, Hd, device=DEV), torch.ones(C, device=DEV),
                        drop_p=P, seed=s2)
    m1, m2 = z1 > 0, z2 > 0
    for m in (m1, m2):
        assert abs(float(m.float().mean()) - (1 - P)) < 0.01
    return m1, m2


def _ffn_case(ops, mp, fp64, L, C, slot=False, seed=0):
    """ops.ffn in train mode: y = x + 0.6 drop2(W2 drop1(gelu(W1 x + b1)) + b2), p = 0.05, SAVE_DACT forward, DACT_MUL
    data gradient, residual gradient in the epilogue; with `slot` the result goes into a concat slot (middle / decoder
    block 0) and its gradient arrives with row stride 2C."""
    g = _gen(seed)
    Hd, alpha, s1, s2 = 2 * C, 0.6, 1000 + seed, 2000 + seed
    M = B * L
    m1, m2 = _drop_masks(ops, M, C, Hd, s1, s2) if fp64 else (None, None)
    x = _act((B, L, C), g).requires_grad_(True)
    w1, b1 = _weight((Hd, C), g, False), _bias(Hd, g)
    w2, b2 = _weight((C, Hd), g, False), _bias(C, g)
    rec = _Launches(mp, keep=fp64)
    s, skip = _slot(ops, (B, L, 2 * C), C, g) if slot else (None, None)
    y = ops.ffn(x, w1, b1, w2, b2, alpha, drop_p=P, seed1=s1, seed2=s2, out=s.out if slot else None)
    if slot:
        _check_slot(s, C)
        top = s.cat(y, skip)
        dtop = _act(tuple(top.shape), g)
        dy = dtop[..., :C]
    else:
        top = y
        dtop = dy = _act(tuple(y.shape), g)
    top.backward(dtop)
    if not fp64:
        return rec.keys
    t0 = _sync_time()
    r = {}
    hmid, dact = rec.operand("fwd", "y", 0), rec.operand("fwd", "preact", 0)
    assert rec.operand("fwd", "x", 1).data_ptr() == hmid.data_ptr()
    g2 = rec.operand("dgrad", "x", 0)                            # psg_epilogue_bwd's result, read by the DACT_MUL launch
    gu = rec.operand("dgrad", "y", 0)
    assert rec.operand("dgrad", "x", 1).data_ptr() == gu.data_ptr()
    k1, k2 = m1.reshape(M, Hd), m2.reshape(M, C)
    # first Linear: hidden activation and the saved derivative gelu'(u) keep / (1 - p)
    acc, S = R.linear_fwd(x, w1)
    acc, S = acc.reshape(M, Hd), S.reshape(M, Hd)
    ref, Sy, A = R.epilogue(acc, S, bias=b1, kind="gelu", keep=k1, p=P)
    r["hidden"] = R.check(hmid, ref, Sy, BF, "hidden activation", C, extra=A)
    u, Su, _ = R.epilogue(acc, S, bias=b1)
    sc = k1.double() / (1 - P)
    # |gelu''| <= 0.7979: an accumulator error moves the derivative by at most that times itself
    r["dact"] = R.check(dact, R.act_grad(u, "gelu") * sc, Su * 0.7979 * sc, BF, "saved GELU derivative", C,
                        extra=(u.abs() + 1.0) * sc * R.ACT_APPROX["gelu"])
    del acc, S, ref, Sy, A, u, Su
    # second Linear on the kernel's hidden activation
    acc, S = R.linear_fwd(hmid, w2)
    ref, Sy, A = R.epilogue(acc, S, bias=b2, residual=x.detach().reshape(M, C), alpha=alpha, keep=k2, p=P)
    r["fwd"] = R.check(y.reshape(M, C), ref, Sy, BF, "output", Hd, extra=A)
    del acc, S, ref, Sy, A
    # backward
    dyr = dy.reshape(M, C)
    g2ref = R.epilogue_bwd(dyr, None, alpha=alpha, keep=k2, p=P)
    r["g2"] = R.check(g2, g2ref, torch.zeros_like(g2ref), BF, "second Linear's accumulator gradient", 1)
    r["gu"] = R.check(gu, *R.dact_mul(*R.linear_dgrad(g2, w2), dact), BF, "DACT_MUL data gradient", C, r_extra=0.0)
    acc, S = R.linear_dgrad(gu, w1)
    r["dx"] = R.check(x.grad.reshape(M, C), acc + dyr.double(), S + dyr.double().abs(), BF, "data gradient + residual", Hd)
    del acc, S
    r["dw2"] = R.check(w2.grad, *R.linear_wgrad(hmid, g2), torch.float32, "W2 gradient", M)
    r["db2"] = R.check(b2.grad, *R.bias_grad(g2), torch.float32, "b2 gradient", M)
    r["dw1"] = R.check(w1.grad, *R.linear_wgrad(x, gu), torch.float32, "W1 gradient", M)
    r["db1"] = R.check(b1.grad, *R.bias_grad(gu), torch.float32, "b1 gradient", M)
    return r, _sync_time() - t0


PROJ_W = 15360           # sum of the 17 ResBlocks' out_channels: the ProjGroup's [sum Cout, K] operands
CASES = [
    # 3x3 stride 1, level 27x27 (no attention); ResBlock conv1 carries the row-add, conv2 the residual
    ("conv27_init_8_320", _conv_case, dict(H=27, Cin=8, Cout=320, dx=False)),
    ("conv27_320_320_rowadd", _conv_case, dict(H=27, Cin=320, Cout=320, rowadd=True)),
    ("conv27_320_320_res", _conv_case, dict(H=27, Cin=320, Cout=320, residual=True)),
    ("conv27_320_320_res_slot", _conv_case, dict(H=27, Cin=320, Cout=320, residual=True, slot=True)),
    ("conv27_640_320_rowadd", _conv_case, dict(H=27, Cin=640, Cout=320, rowadd=True)),
    ("conv27_up_640_320_slot", _conv_case, dict(H=27, Cin=640, Cout=320, slot=True)),
    ("conv27_final_320_8", _conv_case, dict(H=27, Cin=320, Cout=8)),
    ("skip27_640_320", _conv_case, dict(H=27, Cin=640, Cout=320, ks=1)),
    ("skip27_640_320_slotgrad", _conv_case, dict(H=27, Cin=640, Cout=320, ks=1, strided_grad=True)),
    ("down27_320_640", _conv_case, dict(H=27, Cin=320, Cout=640, stride=2)),
    # 14x14
    ("conv14_640_640_rowadd", _conv_case, dict(H=14, Cin=640, Cout=640, rowadd=True)),
    ("conv14_640_640_res", _conv_case, dict(H=14, Cin=640, Cout=640, residual=True)),
    ("conv14_1280_640_rowadd", _conv_case, dict(H=14, Cin=1280, Cout=640, rowadd=True)),
    ("conv14_up_1280_640_slot", _conv_case, dict(H=14, Cin=1280, Cout=640, slot=True)),
    ("skip14_1280_640", _conv_case, dict(H=14, Cin=1280, Cout=640, ks=1)),
    ("down14_640_1280", _conv_case, dict(H=14, Cin=640, Cout=1280, stride=2)),
    # 7x7
    ("conv7_1280_1280_rowadd", _conv_case, dict(H=7, Cin=1280, Cout=1280, rowadd=True)),
    ("conv7_1280_1280_res", _conv_case, dict(H=7, Cin=1280, Cout=1280, residual=True)),
    ("conv7_2560_1280_rowadd", _conv_case, dict(H=7, Cin=2560, Cout=1280, rowadd=True)),
    ("conv7_up_1280_1280_slot", _conv_case, dict(H=7, Cin=1280, Cout=1280, slot=True)),
    ("skip7_2560_1280", _conv_case, dict(H=7, Cin=2560, Cout=1280, ks=1)),
    ("down7_1280_1280", _conv_case, dict(H=7, Cin=1280, Cout=1280, stride=2)),
    # 4x4
    ("conv4_1280_1280_rowadd", _conv_case, dict(H=4, Cin=1280, Cout=1280, rowadd=True)),
    ("conv4_1280_1280_res", _conv_case, dict(H=4, Cin=1280, Cout=1280, residual=True)),
    ("conv4_2560_1280_rowadd", _conv_case, dict(H=4, Cin=2560, Cout=1280, rowadd=True)),
    ("skip4_2560_1280", _conv_case, dict(H=4, Cin=2560, Cout=1280, ks=1)),
    # attention Linears at M = 256 L: self in-projection, out-projections (residual, alpha 0.7 / 0.8), text projection,
    # cross in-projection (q at M = 256 L, kv at M = 256 * 32)
    ("qkv196_640", _linear_case, dict(lead=(B, 196), Cin=640, Cout=1920)),
    ("qkv49_1280", _linear_case, dict(lead=(B, 49), Cin=1280, Cout=3840)),
    ("qkv16_1280", _linear_case, dict(lead=(B, 16), Cin=1280, Cout=3840)),
    ("outproj196_640", _linear_case, dict(lead=(B, 196), Cin=640, Cout=640, residual=True, alpha=0.7)),
    ("outproj49_1280", _linear_case, dict(lead=(B, 49), Cin=1280, Cout=1280, residual=True, alpha=0.8)),
    ("outproj16_1280", _linear_case, dict(lead=(B, 16), Cin=1280, Cout=1280, residual=True, alpha=0.7)),
    ("textproj_256_640", _linear_case, dict(lead=(B, TEXT_S), Cin=256, Cout=640, dx=False)),
    ("textproj_256_1280", _linear_case, dict(lead=(B, TEXT_S), Cin=256, Cout=1280, dx=False)),
    ("cross196_640", _cross_case, dict(L=196, C=640)),
    ("cross49_1280", _cross_case, dict(L=49, C=1280)),
    ("cross16_1280", _cross_case, dict(L=16, C=1280)),
    # FFN C -> 2C -> C, GELU, dropout 0.05; the middle and decoder block 0 write theirs into a concat slot
    ("ffn196_640", _ffn_case, dict(L=196, C=640)),
    ("ffn196_640_slot", _ffn_case, dict(L=196, C=640, slot=True)),
    ("ffn49_1280", _ffn_case, dict(L=49, C=1280)),
    ("ffn49_1280_slot", _ffn_case, dict(L=49, C=1280, slot=True)),
    ("ffn16_1280", _ffn_case, dict(L=16, C=1280)),
    ("ffn16_1280_slot", _ffn_case, dict(L=16, C=1280, slot=True)),
    # ProjGroup (time / text projections of the 17 ResBlocks, one Linear each; pooled text has no gradient) and time MLP
    ("projgroup_time", _linear_case, dict(lead=(B,), Cin=128, Cout=PROJ_W)),
    ("projgroup_text", _linear_case, dict(lead=(B,), Cin=256, Cout=PROJ_W, residual=True, dx=False)),
    ("time_mlp1", _linear_case, dict(lead=(B,), Cin=128, Cout=512, kind="silu", dx=False)),
    ("time_mlp2", _linear_case, dict(lead=(B,), Cin=512, Cout=512, kind="silu")),
    ("time_mlp3", _linear_case, dict(lead=(B,), Cin=512, Cout=128)),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gemm_b256_against_fp64(ops, monkeypatch, case):
    name, fn, kw = case
    r, secs = fn(ops, monkeypatch, True, seed=len(name) * 131 + sum(map(ord, name)), **kw)
    _report(name, r, secs)
    _free()


def _train_step_launches(monkeypatch):
    """The launch keys of one bf16 DiffusionStepper.train_step at batch 256, train mode (set up as
    test_gradient_batch_linearity_b256)."""
    import pokemon_sprite_generator_amd as psg
    dev = torch.device(DEV, 0)
    torch.manual_seed(0)
    unet = psg.UNet(compute_dtype=BF).to(dev)
    st = psg.DiffusionStepper(unet, psg.NoiseScheduler(), distributed=False)
    g = _gen(5)
    lat = torch.randn(B, 8, 27, 27, device=dev, generator=g)
    txt = torch.randn(B, TEXT_S, 256, device=dev, generator=g)
    t = torch.randint(0, 1000, (B,), device=dev, generator=g)
    rec = _Launches(monkeypatch)
    st.train_step(lat, txt, t)
    torch.cuda.synchronize()
    monkeypatch.undo()
    st.close()
    del st, unet
    _free()
    return rec.keys


def test_table_covers_every_gemm_launch_of_the_b256_train_step(ops, monkeypatch):
    """Every distinct GEMM launch key of the benchmark's train step appears among the table's cases, and the table takes
    the split-K workspace, the border-class order and the persistent pointwise kernel wherever the step does."""
    step = _train_step_launches(monkeypatch)
    table = {}
    for name, fn, kw in CASES:
        with monkeypatch.context() as mp:
            for k, f in fn(ops, mp, False, **kw).items():
                old = table.get(k, (False, False, False))
                table[k] = tuple(a or b for a, b in zip(old, f))
    missing = [k for k in step if k not in table]
    assert not missing, "launch keys of the train step no case covers:\n" + "\n".join(map(str, missing))
    paths = ("split-K", "border-class order", "persistent pointwise")
    lost = [(k, paths[i]) for k, f in step.items() for i in range(3) if f[i] and not table[k][i]]
    assert not lost, "the step takes these paths, the table's launch does not:\n" + "\n".join(map(str, lost))
    counts = [sum(f[i] for f in step.values()) for i in range(3)]
    print("train step: %d distinct GEMM launch keys; split-K on %d, border-class on %d, persistent on %d" % (len(step), *counts))
    for k, f in step.items():
        if f[0]:
            print("split-K:", k)
    _free()
