"""-m gpu: the streaming and reduction kernels of csrc/elementwise.hip that start and end a train step, through the C ABI, on
the cases of tests/step_cases.py against the references and derived bounds of tests/step_ref.py: noise_add / noise_fallback,
ddpm_update / sampler_update, the two layout conversions, text_pool, timestep_sinusoid, reparam and its backward, smooth_l1,
recon_loss, sumsq, clip_scale and the single-tensor AdamW (host-step and device-step entries).

Every entry runs once well below its grid cap (a ragged last block) and once at 2 x cap + 333 elements (two and three trips of
the grid-stride loop).  Every device buffer sits between guard words that must keep their bits; outputs start as NaN; inputs
must keep their bits.  Bit-exact entries are compared on the bits, the others element by element within their bound; every
comparison prints `RATIO <what> <err / bound>` before it asserts (0 = a bit comparison).  A device error ends the run."""
import os
import time

import numpy as np
import pytest
import torch

from tests import step_cases as K
from tests import step_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
REPORT = os.environ.get("PSG_STEP_REPORT")     # optional: write the worst err / bound per kernel to this file
_WORST, _T = {}, {"t0": None, "n": 0}


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    lib = _lib.init(0)
    _T["t0"] = time.perf_counter()
    yield lib
    if REPORT:
        with open(REPORT, "w") as f:
            f.write("Step kernels (tests/test_step_kernels_gpu.py): worst |err| / bound per kernel over the cases of tests/step_cases.py;\n"
                    "bounds derived in tests/step_ref.py.  0 = bit-exact comparison.\n\n")
            for k in sorted(_WORST):
                f.write(f"{k:<44s} {_WORST[k]:.3g}\n")
            f.write(f"\ncomparisons {_T['n']}, wall time of the file {time.perf_counter() - _T['t0']:.1f} s\n")


def _api():
    from pokemon_sprite_generator_amd import _lib
    return _lib


def _stream():
    return _api().stream_ptr()


def _note(key, what, ratio):
    print(f"RATIO {what} {float(ratio):.3g}")
    _T["n"] += 1
    _WORST[key] = max(_WORST.get(key, 0.0), float(ratio))


def _sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                   # a device error: nothing more runs on this GPU
        pytest.exit(f"{what}: {e}", returncode=3)


def _run(rc, what):
    _api().check(rc, what)
    _sync(what)


def _bits(t):
    if not t.dtype.is_floating_point:
        return t
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _tensor(v):
    return torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v.detach().cpu().contiguous()


class Dev:
    """n elements on the device between GUARD guard words (`off` more in front: a base off the 16-byte boundary).  values: an
    input, whose bits kept() compares later; None: an output, NaN (floats) or 0x5A5A5A5A (integers) everywhere."""

    def __init__(self, values=None, n=None, dtype=F32, off=0):
        src = None if values is None else _tensor(values).reshape(-1)
        if src is not None:
            n, dtype = src.numel(), src.dtype
        self.flat = torch.empty(n + 2 * K.GUARD + off, dtype=dtype, device=DEV)
        self.flat.fill_(float("nan") if dtype.is_floating_point else 0x5A5A5A5A)
        lo = K.GUARD + off
        self.v = self.flat[lo:lo + n]
        self.src = src
        if src is not None:
            self.v.copy_(src)
        self._outside = [self.flat[:lo], self.flat[lo + n:]]
        self._saved = [_bits(t).clone() for t in self._outside]

    def ptr(self):
        return self.v.data_ptr()

    def intact(self):
        return all(torch.equal(_bits(t), s) for t, s in zip(self._outside, self._saved))

    def kept(self):
        return self.intact() and torch.equal(_bits(self.v.cpu()), _bits(self.src))

    def cpu(self):
        return self.v.cpu()

    def np(self):
        return self.v.cpu().numpy()


def _i32(v):
    return Dev(np.array([v], dtype=np.int32))


def _f1(v):
    return Dev(np.array([v], dtype=np.float32))


def _all_ok(bufs, what):
    for name, b in bufs.items():
        ok = b.kept() if b.src is not None else b.intact()
        assert ok, f"{what}: {'input' if b.src is not None else 'guards of'} {name} changed"


def _bitcheck(key, what, got, want):
    _note(key, what, 0.0)
    assert R.same_bits(got, want), f"{what}: not bit-equal to the restated fp32 arithmetic"


def _check(key, what, got, ref, S, depth, dt=F32, extra=None):
    try:
        r = R.check(got, ref, S, dt, what, depth, extra=extra)
    except AssertionError as e:
        print(f"RATIO {what} out of bound: {e}")
        raise
    _note(key, what, r)
    return r


def _check_scalar(key, what, got, ref, depth):
    r = torch.as_tensor(ref, dtype=torch.float64).detach().cpu().reshape(1)
    return _check(key, what, torch.as_tensor(got).detach().cpu().reshape(1), r, r.abs(), depth)


# ---------------------------------------------------------------------------------------------- noise_add, noise_fallback
@pytest.mark.parametrize("t_range", [False, True], ids=["t-in-range", "t-out-of-range"])
@pytest.mark.parametrize("do_clamp", [0, 1], ids=["raw", "clamp"])
@pytest.mark.parametrize("shape", K.NOISE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_noise_add(lib, shape, do_clamp, t_range):
    B, chw = shape
    what = f"noise_add {B}x{chw} clamp={do_clamp} t_range={t_range}"
    tabA, tabB = K.noise_tables()
    x0, noise, t = K.noise_inputs(B, chw, t_range)
    want, wflag = R.noise_add(x0, noise, t, tabA, tabB, do_clamp)
    assert bool(wflag & R.FLAG_T_RANGE) == t_range and wflag & R.FLAG_FALLBACK          # the NaN x0 stays NaN and raises the fallback bit
    b = dict(x0=Dev(x0), noise=Dev(noise), t=Dev(t), tabA=Dev(tabA), tabB=Dev(tabB), out=Dev(n=B * chw), flag=_i32(0))
    _run(lib.psg_noise_add_f32(b["x0"].ptr(), b["noise"].ptr(), b["t"].ptr(), b["tabA"].ptr(), b["tabB"].ptr(), b["out"].ptr(), b["flag"].ptr(),
                               B, chw, K.NUM_T, do_clamp, _stream()), what)
    fb = b.pop("flag")
    flag = int(fb.cpu()[0])
    assert fb.intact()
    _all_ok(b, what)
    _bitcheck("noise_add", what, b["out"].np().reshape(B, chw), want)
    assert flag == wflag, f"{what}: flag word {flag}, restated {wflag}"


@pytest.mark.parametrize("state", ["clear", "set", "set-still-bad"])
@pytest.mark.parametrize("do_clamp", [0, 1], ids=["raw", "clamp"])
@pytest.mark.parametrize("n", K.STREAM_N)
def test_noise_fallback(lib, n, do_clamp, state):
    what = f"noise_fallback n={n} clamp={do_clamp} {state}"
    x0, noise = K.fallback_inputs(n, state == "set-still-bad")
    word = 0 if state == "clear" else R.FLAG_FALLBACK
    b = dict(x0=Dev(x0), noise=Dev(noise), out=Dev(n=n))
    flag = _i32(word)
    _run(lib.psg_noise_fallback_f32(b["x0"].ptr(), b["noise"].ptr(), b["out"].ptr(), flag.ptr(), n, do_clamp, _stream()), what)
    _all_ok(b, what)
    assert flag.intact()
    got = int(flag.cpu()[0])
    if state == "clear":
        assert got == 0 and bool(torch.isnan(b["out"].v).all()), f"{what}: the flag was clear, yet the output or the flag was written"
        _note("noise_fallback", what, 0.0)
        return
    want, bad = R.noise_fallback(x0, noise, do_clamp)
    assert bool(bad) == (state == "set-still-bad")
    _bitcheck("noise_fallback", what, b["out"].np(), want)
    assert got == R.FLAG_FALLBACK | bad, f"{what}: flag word {got}, restated {R.FLAG_FALLBACK | bad}"


# ------------------------------------------------------------------------------------------- ddpm_update, sampler_update
@pytest.mark.parametrize("t", K.DDPM_T)
@pytest.mark.parametrize("n", K.STREAM_N)
def test_ddpm_update(lib, n, t):
    what = f"ddpm_update n={n} t={t}"
    x, e, z = K.xez(n, "ddpm")
    c1, c2, sg = K.ddpm_tables()
    b = dict(eps=Dev(e), z=Dev(z), c1=Dev(c1), c2=Dev(c2), sg=Dev(sg), t=_i32(t))
    xb = Dev(x)
    _run(lib.psg_ddpm_update_f32(xb.ptr(), b["eps"].ptr(), b["z"].ptr(), b["c1"].ptr(), b["c2"].ptr(), b["sg"].ptr(), b["t"].ptr(), n, _stream()), what)
    _all_ok(b, what)
    assert xb.intact()
    _bitcheck("ddpm_update", what, xb.np(), R.ddpm_update(x, e, z, c1, c2, sg, t))


@pytest.mark.parametrize("mode_z", K.SAMPLER, ids=lambda m: f"mode{m[0]}{'-z' if m[1] else ''}")
@pytest.mark.parametrize("n", K.STREAM_N)
def test_sampler_update(lib, n, mode_z):
    mode, with_z = mode_z
    what = f"sampler_update n={n} mode={mode} z={with_z}"
    x, e, z = K.xez(n, "samp")
    b = dict(eps=Dev(e), z=Dev(z))
    xb = Dev(x)
    _run(lib.psg_sampler_update_f32(xb.ptr(), b["eps"].ptr(), b["z"].ptr() if with_z else None, mode, *K.SAMPLER_C, n, _stream()), what)
    _all_ok(b, what)
    assert xb.intact()
    _bitcheck(f"sampler_update mode {mode}", what, xb.np(), R.sampler_update(x, e, z if with_z else None, mode, *K.SAMPLER_C))


# --------------------------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("extra", K.LD_EXTRA, ids=lambda e: f"ld+{e}")
@pytest.mark.parametrize("dname", list(K.DTYPES))
@pytest.mark.parametrize("shape", K.LAYOUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layout(lib, shape, dname, extra):
    """nchw_to_nhwc into rows of stride C + extra (the padding columns poisoned), then nhwc_to_nchw from those rows."""
    B, C, HW = shape
    dt, code, ld = K.DTYPES[dname], K.DTYPE_CODE[dname], C + extra
    what = f"layout {B}x{C}x{HW} {dname} ld={ld}"
    src = K.h((B, C, HW), f"step.lay.{HW}", 2.0)
    sb, rows = Dev(src), Dev(n=B * HW * ld, dtype=dt)
    _run(lib.psg_nchw_to_nhwc(sb.ptr(), rows.ptr(), ld, B, C, HW, code, _stream()), what)
    assert sb.kept() and rows.intact(), f"{what}: the source or the guards changed"
    got = rows.cpu().view(B * HW, ld)
    assert bool(torch.isnan(got[:, C:]).all()), f"{what}: the padding columns were written"
    want = R.nchw_to_nhwc(src, dt)
    _bitcheck(f"nchw_to_nhwc {dname}", what, got[:, :C].contiguous(), want)
    back = Dev(n=B * C * HW)
    keep = _bits(rows.v).clone()
    _run(lib.psg_nhwc_to_nchw(rows.ptr(), ld, back.ptr(), B, C, HW, code, _stream()), what)
    assert torch.equal(_bits(rows.v), keep) and rows.intact() and back.intact(), f"{what}: the rows or the guards changed"
    _bitcheck(f"nhwc_to_nchw {dname}", what + " back", back.cpu().view(B, C, HW), R.nhwc_to_nchw(want, B, C, HW))


# ---------------------------------------------------------------------------------------------------- text_pool, sinusoid
@pytest.mark.parametrize("SD", K.TEXT_POOL, ids=lambda c: f"S{c[0]}-D{c[1]}")
def test_text_pool(lib, SD):
    S, D = SD
    B = K.TEXT_B
    text = K.h((B, S, D), f"step.pool.{S}.{D}", 1.5)
    ref, Sabs, depth = R.text_pool(text)
    tb = Dev(text)
    for dname, dt in K.DTYPES.items():
        for extra in K.LD_EXTRA:
            for with_cast in (False, True):
                ld = D + extra
                what = f"text_pool S={S} D={D} {dname} ld={ld} cast={with_cast}"
                pooled, cast = Dev(n=B * ld, dtype=dt), Dev(n=B * S * D, dtype=dt)
                _run(lib.psg_text_pool(tb.ptr(), pooled.ptr(), ld, cast.ptr() if with_cast else None, B, S, D, K.DTYPE_CODE[dname], _stream()), what)
                assert tb.kept() and pooled.intact() and cast.intact(), f"{what}: the input or the guards changed"
                got = pooled.cpu().view(B, ld)
                assert bool(torch.isnan(got[:, D:]).all()), f"{what}: the padding columns were written"
                _check(f"text_pool {dname}", what, got[:, :D], ref, Sabs, depth, dt)
                if with_cast:
                    _bitcheck(f"text_pool cast {dname}", what + " cast", cast.cpu().view(B, S, D), text.to(dt))
                else:
                    assert bool(torch.isnan(cast.v).all())


@pytest.mark.parametrize("half", K.SIN_HALF)
def test_timestep_sinusoid(lib, half):
    """The absolute bars of test_layout_pool_sinusoid (2e-6 fp32, 4e-3 bf16) against fp64 sin / cos of the fp32 product."""
    B = K.SIN_B
    t, coeff = torch.tensor(K.SIN_T), R.sinusoid_coeff(half)
    ref = R.sinusoid(t, coeff)
    tb, cb = Dev(t), Dev(coeff)
    for dname, dt in K.DTYPES.items():
        for extra in K.LD_EXTRA:
            ld = 2 * half + extra
            what = f"sinusoid half={half} {dname} ld={ld}"
            out = Dev(n=B * ld, dtype=dt)
            _run(lib.psg_timestep_sinusoid(tb.ptr(), cb.ptr(), out.ptr(), ld, B, half, K.DTYPE_CODE[dname], _stream()), what)
            assert tb.kept() and cb.kept() and out.intact(), f"{what}: an input or the guards changed"
            got = out.cpu().view(B, ld)
            assert bool(torch.isnan(got[:, 2 * half:]).all()), f"{what}: the padding columns were written"
            err = float((got[:, :2 * half].double() - ref).abs().max())
            _note(f"sinusoid {dname}", what, err / R.SIN_BAR[dt])
            assert err <= R.SIN_BAR[dt], f"{what}: |err| {err:.3g} above the bar {R.SIN_BAR[dt]:g}"


# ------------------------------------------------------------------------------------------------------------- reparam
@pytest.mark.parametrize("n", K.STREAM_N)
def test_reparam(lib, n):
    what = f"reparam n={n}"
    mu, lv, ep = K.reparam_inputs(n)
    b = dict(mu=Dev(mu), logvar=Dev(lv), eps=Dev(ep), out=Dev(n=n))
    _run(lib.psg_reparam_f32(b["mu"].ptr(), b["logvar"].ptr(), b["eps"].ptr(), b["out"].ptr(), n, _stream()), what)
    _all_ok(b, what)
    ref, S, depth, extra = R.reparam(mu, lv, ep)
    _check("reparam", what, b["out"].cpu(), ref, S, depth, extra=extra)


@pytest.mark.parametrize("accumulate", [0, 1], ids=["write", "accumulate"])
@pytest.mark.parametrize("outs", ["both", "dmu", "dlogvar"])
@pytest.mark.parametrize("n", K.STREAM_N)
def test_reparam_bwd(lib, n, outs, accumulate):
    what = f"reparam_bwd n={n} {outs} accumulate={accumulate}"
    _, lv, ep = K.reparam_inputs(n)
    d = K.h((n,), f"step.rp.d.{n}", 1.0)
    pm, pl = K.h((n,), f"step.rp.pm.{n}", 0.77), K.h((n,), f"step.rp.pl.{n}", 0.77)
    b = dict(d=Dev(d), logvar=Dev(lv), eps=Dev(ep))
    dmu = (Dev(pm) if accumulate else Dev(n=n)) if outs != "dlogvar" else None
    dlv = (Dev(pl) if accumulate else Dev(n=n)) if outs != "dmu" else None
    # without dlogvar the kernel reads neither logvar nor eps: NULL is legal for them then
    pl_, pe_ = (b["logvar"].ptr(), b["eps"].ptr()) if dlv is not None else (None, None)
    _run(lib.psg_reparam_bwd_f32(b["d"].ptr(), pl_, pe_, dmu.ptr() if dmu else None, dlv.ptr() if dlv else None, accumulate, n, _stream()), what)
    _all_ok(b, what)
    (rm, Sm, dm), (rl, Sl, dl, xl) = R.reparam_bwd(d, lv, ep, pm if accumulate else None, pl if accumulate else None)
    if dmu is not None:
        assert dmu.intact()
        if accumulate:
            _check("reparam_bwd dmu", what + " dmu", dmu.cpu(), rm, Sm, dm)
        else:
            _bitcheck("reparam_bwd dmu", what + " dmu", dmu.cpu(), d)
    if dlv is not None:
        assert dlv.intact()
        _check("reparam_bwd dlogvar", what + " dlogvar", dlv.cpu(), rl, Sl, dl, extra=xl)


# --------------------------------------------------------------------------------------------------------------- losses
def _ws(lib, nbytes):
    return Dev(n=int(nbytes) // 4)                     # exactly the bytes the library asks for, guards behind


@pytest.mark.parametrize("n", K.RED_N)
def test_smooth_l1(lib, n):
    what = f"smooth_l1 n={n}"
    pred, target = K.smooth_l1_inputs(n)
    loss_ref, dl, g_ref, S, dg = R.smooth_l1(pred, target, K.SL1_BETA, K.SL1_SCALE)
    b = dict(pred=Dev(pred), target=Dev(target))
    runs = []
    for with_grad, with_flag in ((True, True), (True, True), (False, False)):
        grad, loss, flag, ws = Dev(n=n), Dev(n=1), _i32(0), _ws(lib, lib.psg_reduce_workspace_bytes())
        _run(lib.psg_smooth_l1_f32(b["pred"].ptr(), b["target"].ptr(), grad.ptr() if with_grad else None, loss.ptr(), flag.ptr() if with_flag else None,
                                   K.SL1_BETA, K.SL1_SCALE, n, ws.ptr(), _stream()), what)
        _all_ok(b, what)
        assert grad.intact() and loss.intact() and flag.intact() and ws.intact(), f"{what}: a store outside an output or behind the workspace"
        assert int(flag.cpu()[0]) == 0
        if not with_grad:
            assert bool(torch.isnan(grad.v).all())
        runs.append((loss.cpu().clone(), grad.cpu().clone()))
    assert R.same_bits(runs[0][0], runs[1][0]) and R.same_bits(runs[0][1], runs[1][1]), f"{what}: a second identical launch gives other bits"
    assert R.same_bits(runs[0][0], runs[2][0]), f"{what}: grad = NULL changes the loss"
    _check_scalar("smooth_l1 loss", what + " loss", runs[0][0], loss_ref, dl)
    _check("smooth_l1 grad", what + " grad", runs[0][1], g_ref, S, dg)


@pytest.mark.parametrize("case", ["nan-pred", "inf-pred", "inf-target", "nan-pred-no-flag"])
def test_smooth_l1_flags(lib, case):
    """PRED_BAD for a NaN or an infinity in pred, LOSS_BAD for a non-finite loss (an infinite target alone leaves pred good);
    nan_flag = NULL is legal."""
    n = K.N_SMALL
    pred, target = K.smooth_l1_inputs(n)
    if case == "inf-target":
        target[n - 1] = float("inf")
    else:
        pred[n // 2] = float("inf") if case == "inf-pred" else float("nan")
    want = R.FLAG_LOSS_BAD | (0 if case == "inf-target" else R.FLAG_PRED_BAD)
    pb, tb, grad, loss, flag, ws = Dev(pred), Dev(target), Dev(n=n), Dev(n=1), _i32(R.FLAG_FALLBACK), _ws(lib, lib.psg_reduce_workspace_bytes())
    _run(lib.psg_smooth_l1_f32(pb.ptr(), tb.ptr(), grad.ptr(), loss.ptr(), None if case.endswith("no-flag") else flag.ptr(), K.SL1_BETA, 1.0, n,
                               ws.ptr(), _stream()), case)
    assert all(x.intact() for x in (pb, tb, grad, loss, flag, ws))
    assert not bool(torch.isfinite(loss.v).any())
    got = int(flag.cpu()[0])
    assert got == (R.FLAG_FALLBACK if case.endswith("no-flag") else R.FLAG_FALLBACK | want), f"{case}: flag word {got}"
    _note("smooth_l1 flags", f"smooth_l1 {case}", 0.0)


@pytest.mark.parametrize("w", K.RECON_W, ids=lambda w: f"l1={w[0]}-mse={w[1]}")
@pytest.mark.parametrize("n", K.RED_N)
def test_recon_loss(lib, n, w):
    what = f"recon_loss n={n} w={w}"
    pred, target = K.recon_inputs(n)
    out_ref, d3, g_ref, S, dg = R.recon_loss(pred, target, *w)
    b = dict(pred=Dev(pred), target=Dev(target))
    runs = []
    for with_grad in (True, True, False):
        grad, out3, ws = Dev(n=n), Dev(n=3), _ws(lib, lib.psg_recon_loss_workspace_bytes())
        _run(lib.psg_recon_loss_f32(b["pred"].ptr(), b["target"].ptr(), grad.ptr() if with_grad else None, out3.ptr(), n, w[0], w[1], ws.ptr(), _stream()), what)
        _all_ok(b, what)
        assert grad.intact() and out3.intact() and ws.intact(), f"{what}: a store outside an output or behind the workspace"
        if not with_grad:
            assert bool(torch.isnan(grad.v).all())
        runs.append((out3.cpu().clone(), grad.cpu().clone()))
    assert R.same_bits(runs[0][0], runs[1][0]) and R.same_bits(runs[0][1], runs[1][1]), f"{what}: a second identical launch gives other bits"
    assert R.same_bits(runs[0][0], runs[2][0]), f"{what}: grad = NULL changes the three scalars"
    for i, name in enumerate(("total", "l1", "mse")):
        _check_scalar(f"recon_loss {name}", f"{what} {name}", runs[0][0][i], out_ref[i], d3[i])
    g = runs[0][1]
    _check("recon_loss grad", what + " grad", g, g_ref, S, dg)
    zero = (pred == target)
    assert int(zero.sum()) >= 8 and bool((g[zero] == 0).all()), f"{what}: sign(0) is not 0"


@pytest.mark.parametrize("accumulate", [0, 1], ids=["write", "accumulate"])
@pytest.mark.parametrize("n", K.SUMSQ_N)
def test_sumsq(lib, n, accumulate):
    what = f"sumsq n={n} accumulate={accumulate}"
    g = K.h((n,), f"step.sumsq.{n}", 1.0)
    ref, depth = R.sumsq(g, K.SUMSQ_PREV if accumulate else None)
    gb = Dev(g)
    runs = []
    for _ in range(2):
        out, ws = (_f1(K.SUMSQ_PREV) if accumulate else Dev(n=1)), _ws(lib, lib.psg_reduce_workspace_bytes())
        _run(lib.psg_sumsq_f32(gb.ptr(), n, out.ptr(), accumulate, ws.ptr(), _stream()), what)
        assert gb.kept() and out.intact() and ws.intact(), f"{what}: the input or the guards changed"
        runs.append(out.cpu().clone())
    assert R.same_bits(runs[0], runs[1]), f"{what}: a second identical launch gives other bits"
    _check_scalar("sumsq", what, runs[0], ref, depth)


# ------------------------------------------------------------------------------------------------------------ clip_scale
@pytest.mark.parametrize("name", list(K.CLIP))
@pytest.mark.parametrize("n", K.CLIP_N)
def test_clip_scale(lib, n, name):
    nsq, mx = K.CLIP[name]
    what = f"clip_scale n={n} norm {name}"
    g = K.h((n,), f"step.clip.g.{n}", 1.0)
    gb, nb = Dev(g), _f1(nsq)
    _run(lib.psg_clip_scale_f32(gb.ptr(), n, nb.ptr(), mx, _stream()), what)
    assert gb.intact() and nb.kept(), f"{what}: the norm or the guards changed"
    if name == "below":
        _bitcheck("clip_scale", what, gb.cpu(), g)
    else:
        ref, S, depth = R.clip_scale(g, nsq, mx)
        _check("clip_scale", what, gb.cpu(), ref, S, depth)
        if name == "above":
            assert not torch.equal(gb.cpu(), g)


# ----------------------------------------------------------------------------------------------------------------- AdamW
class Adam:
    """p, g, m, v (and optionally a bf16 shadow) of one case on the device, `off` floats off the 16-byte boundary."""

    def __init__(self, n, off=0, shadow=False):
        self.n = n
        self.host = K.adam_inputs(n)
        self.p, self.g, self.m, self.v = (Dev(t, off=off) for t in self.host)
        self.shadow = Dev(n=n, dtype=BF16) if shadow else None

    def state(self):
        return {"p": self.p.cpu(), "m": self.m.cpu(), "v": self.v.cpu()}

    def intact(self):
        return self.g.kept() and all(x.intact() for x in (self.p, self.m, self.v)) and (self.shadow is None or self.shadow.intact())

    def launch(self, lib, entry, step, kw, norm=None, skip=None, what="adamw", tables=None, step_dev=None, expect=0):
        """entry "host": psg_adamw_f32 with `step`; "dev": psg_adamw_dev_f32 with *step_dev = step - 1 and one-entry tables (or
        `tables` = (lr, beta1) device buffers and a given step_dev)."""
        nb = _f1(norm[0]) if norm is not None else None
        mx = norm[1] if norm is not None else 0.0
        sh = self.shadow.ptr() if self.shadow is not None else None
        ptrs = (self.p.ptr(), self.g.ptr(), self.m.ptr(), self.v.ptr())
        if entry == "host":
            rc = lib.psg_adamw_f32(*ptrs, self.n, kw["lr"], kw["beta1"], kw["beta2"], kw["eps"], kw["wd"], step, nb.ptr() if nb else None, mx,
                                   skip.ptr() if skip else None, sh, _stream())
            sd = None
        else:
            sd = step_dev if step_dev is not None else _i32(step - 1)
            lrt, b1t, length = tables if tables is not None else (_f1(kw["lr"]), None, 1)
            rc = lib.psg_adamw_dev_f32(*ptrs, self.n, lrt.ptr(), b1t.ptr() if b1t is not None else None, length, kw["beta1"], kw["beta2"], kw["eps"],
                                       kw["wd"], sd.ptr(), nb.ptr() if nb else None, mx, skip.ptr() if skip else None, sh, _stream())
        assert rc == expect, f"{what}: return code {rc}, expected {expect}: {lib.psg_last_error().decode()}"
        _sync(what)
        assert self.intact() and (nb is None or nb.kept()) and (sd is None or sd.intact()), f"{what}: the gradient, the norm or a guard changed"
        return sd


def _adam_ref(host, step, kw, norm):
    nsq, mx = norm if norm is not None else (None, 0.0)
    return R.adamw(*host, step, lr=kw["lr"], beta1=kw["beta1"], beta2=kw["beta2"], eps=kw["eps"], wd=kw["wd"], normsq=nsq, max_norm=mx)


def _adam_check(key, what, got, ref):
    try:
        ratios = R.check_adamw(got, ref, what)
    except AssertionError as e:
        print(f"RATIO {what} out of bound: {e}")
        raise
    for name, r in ratios.items():
        _note(f"{key} {name}", f"{what} {name}", r)


@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("cid", list(K.ADAM_CASES))
def test_adamw(lib, cid, entry):
    n, step, norm, over = K.ADAM_CASES[cid]
    kw = K.adam_kw(over)
    what = f"adamw {cid} {entry}"
    a = Adam(n)
    sd = a.launch(lib, entry, step, kw, norm, what=what)
    if sd is not None:
        assert int(sd.cpu()[0]) == step, f"{what}: *step_dev {int(sd.cpu()[0])} after the call, expected {step}"
    _adam_check("adamw " + ("float4" if n % 4 == 0 else "scalar"), what, a.state(), _adam_ref(a.host, step, kw, norm))


@pytest.mark.parametrize("entry", ["host", "dev"])
def test_adamw_off_the_boundary_is_the_float4_kernel_bitwise(lib, entry):
    """n % 4 == 0 with p, g, m, v one float off the 16-byte boundary takes the scalar kernel: the same bits as the float4 one."""
    n, step, norm, over = K.ADAM_CASES["vec-step2"]
    kw = K.adam_kw(over)
    vec, sca = Adam(n), Adam(n, off=1)
    assert vec.p.ptr() % 16 == 0 and sca.p.ptr() % 16 == 4 and sca.g.ptr() % 16 == 4 and sca.m.ptr() % 16 == 4 and sca.v.ptr() % 16 == 4
    vec.launch(lib, entry, step, kw, norm, what="aligned")
    sca.launch(lib, entry, step, kw, norm, what="one float off")
    for name, x in vec.state().items():
        _bitcheck("adamw scalar vs float4", f"adamw {entry} one float off, {name}", sca.state()[name], x)
    _adam_check("adamw scalar", f"adamw {entry} one float off", sca.state(), _adam_ref(sca.host, step, kw, norm))


@pytest.mark.parametrize("entry", ["host", "dev"])
def test_adamw_shadow(lib, entry):
    """The bf16 shadow is the rounding of the p just written, bit for bit; on the scalar path it is refused with PSG_ERR_ALIGN
    before anything is written."""
    n, step, norm, over = K.ADAM_CASES["vec-step2"]
    kw = K.adam_kw(over)
    a = Adam(n, shadow=True)
    a.launch(lib, entry, step, kw, norm, what="shadow")
    _adam_check("adamw float4", f"adamw {entry} with shadow", a.state(), _adam_ref(a.host, step, kw, norm))
    _bitcheck("adamw shadow", f"adamw {entry} shadow", a.shadow.cpu(), a.p.cpu().to(BF16))
    for bad in (Adam(n, off=1, shadow=True), Adam(n + 1, shadow=True)):
        sd = bad.launch(lib, entry, step, kw, norm, what="shadow refused", expect=_api().ERR_ALIGN)
        assert b"bf16 shadow" in lib.psg_last_error()
        for name, x in bad.state().items():
            assert R.same_bits(x, bad.host["pgmv".index(name)]), f"refused launch wrote {name}"
        assert bool(torch.isnan(bad.shadow.v).all()) and (sd is None or int(sd.cpu()[0]) == step - 1)
    _note("adamw shadow", f"adamw {entry} shadow refused off the float4 path", 0.0)


def test_adamw_dev_schedule_tables(lib):
    """lr_table / beta1_table of length 4 with *step_dev running 0..5: entries 0, 1, 2, 3, 3, 3; beta1 from the table in the
    moment and in the bias correction.  Each call is held to the reference from the state it started from."""
    n, kw = 1000, K.adam_kw({})
    a = Adam(n)
    lrt, b1t = Dev(np.array(K.SCHED_LR, dtype=np.float32)), Dev(np.array(K.SCHED_B1, dtype=np.float32))
    sd = _i32(0)
    for call in range(K.SCHED_CALLS):
        k = min(call, len(K.SCHED_LR) - 1)
        before = a.state()
        a.launch(lib, "dev", None, dict(kw, beta1=0.5), K.NORM_ABOVE, what=f"schedule call {call}", tables=(lrt, b1t, len(K.SCHED_LR)), step_dev=sd)
        assert int(sd.cpu()[0]) == call + 1 and lrt.kept() and b1t.kept()
        ref = _adam_ref((before["p"], a.host[1], before["m"], before["v"]), call + 1, dict(kw, lr=K.SCHED_LR[k], beta1=K.SCHED_B1[k]), K.NORM_ABOVE)
        _adam_check("adamw_dev tables", f"adamw_dev tables call {call} entry {k}", a.state(), ref)


@pytest.mark.parametrize("entry", ["host", "dev"])
def test_adamw_skip_word(lib, entry):
    """Each single bit of PSG_FLAG_SKIP_MASK leaves p, m, v, the shadow and *step_dev as they were; 16 and 64 alone do not skip
    and give the bits of a launch without a flag word."""
    n, step, norm, over = K.ADAM_CASES["vec-step2"]
    kw = K.adam_kw(over)
    plain = Adam(n, shadow=True)
    plain.launch(lib, entry, step, kw, norm, what="no flag word")
    for bit in K.SKIP_BITS + K.NO_SKIP_BITS:
        a, word = Adam(n, shadow=True), _i32(bit)
        sd = a.launch(lib, entry, step, kw, norm, skip=word, what=f"skip word {bit}")
        assert word.kept()
        skipped = bit in K.SKIP_BITS
        want = dict(zip("pmv", (a.host[0], a.host[2], a.host[3]))) if skipped else plain.state()
        for name, x in a.state().items():
            assert R.same_bits(x, want[name]), f"skip word {bit}: {name} {'changed' if skipped else 'differs from the launch without a flag'}"
        assert bool(torch.isnan(a.shadow.v).all()) if skipped else R.same_bits(a.shadow.cpu(), plain.shadow.cpu())
        if sd is not None:
            assert int(sd.cpu()[0]) == (step - 1 if skipped else step), f"skip word {bit}: *step_dev {int(sd.cpu()[0])}"
        _note("adamw skip word", f"adamw {entry} skip word {bit}", 0.0)
