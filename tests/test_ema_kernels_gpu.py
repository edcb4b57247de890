"""-m gpu: psg_adamw_dev_ema_f32 and psg_swap_f32 through the C ABI, on the AdamW inputs of tests/step_cases.py plus a hashed
EMA buffer, against tests/ema_ref.py.

The optimizer side (p, m, v, the bf16 shadow, *step_dev) must have the bits psg_adamw_dev_f32 gives on copies of the same
inputs; the EMA must have the bits of the fp32 restatement applied to the kernel's own p', and lie within the fp64 bound.  The
device buffers, their guard words and the comparison helpers are those of tests/test_step_kernels_gpu.py (imported, not
copied).  Every comparison prints `RATIO <what> <err / bound>` before it asserts (0 = a bit comparison)."""
import numpy as np
import pytest
import torch

from tests import ema_ref as E
from tests import step_cases as K
from tests import step_ref as R
from tests import test_step_kernels_gpu as T
from tests.test_step_kernels_gpu import lib  # noqa: F401  (the module-scoped library fixture)

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

# id: n, *step_dev, ema_warmup, ema_decay, (normsq, max_norm) or None, beta1 table, bf16 shadow.  Not the full product: every
# size, step, warm-up flag, decay and option appears on the float4 path (n % 4 == 0; 1004 = 251 float4s: the last has no
# pair) and on the scalar path (1001; N_SCALAR: past the grid cap, two and three trips).  The shadow exists on the float4 path only.
CASES = {
    "vec-8-step0-warm-0.9": (8, 0, 1, 0.9, K.NORM_ABOVE, False, False),
    "vec-1000-step1-warm-0.9999-b1-shadow": (1000, 1, 1, 0.9999, K.NORM_ABOVE, True, True),
    "vec-1004-step8-warm-0.9-shadow": (1004, 8, 1, 0.9, None, False, True),
    "vec-1000-step999-warm-0.9999": (1000, 999, 1, 0.9999, K.NORM_ABOVE, False, False),
    "vec-1000-step999-fixed-0.9-b1": (1000, 999, 0, 0.9, None, True, False),
    "vec-1004-step0-fixed-0.0-shadow": (1004, 0, 0, 0.0, K.NORM_ABOVE, False, True),
    "vec-8-step8-fixed-0.9999": (8, 8, 0, 0.9999, None, False, False),
    "vec-1000-step1-warm-0.0": (1000, 1, 1, 0.0, K.NORM_BELOW, False, False),
    "scalar-1001-step0-warm-0.9": (1001, 0, 1, 0.9, K.NORM_ABOVE, False, False),
    "scalar-1001-step1-fixed-0.0-b1": (1001, 1, 0, 0.0, None, True, False),
    "scalar-1001-step8-warm-0.9999-b1": (1001, 8, 1, 0.9999, K.NORM_ABOVE, True, False),
    "scalar-1001-step999-warm-0.9": (1001, 999, 1, 0.9, None, False, False),
    "scalar-past-cap-step999-warm-0.9999": (K.N_SCALAR, 999, 1, 0.9999, K.NORM_ABOVE, False, False),
    "scalar-past-cap-step0-fixed-0.9": (K.N_SCALAR, 0, 0, 0.9, None, False, False),
    "scalar-1001-step8-fixed-0.9999": (1001, 8, 0, 0.9999, K.NORM_ABOVE, False, False),
}


def ema_input(n):
    return K.hn(n, f"ema.kernel.ema.{n}", 1.0)


class Run:
    """One launch of either entry on fresh copies of the case's inputs."""

    def __init__(self, n, step_dev, norm, b1_table, shadow, off=0, ema=True, ema_off=None):
        self.a = T.Adam(n, off=off, shadow=shadow)
        self.n, self.norm = n, norm
        self.sd = T._i32(step_dev)
        if b1_table:
            self.lrt, self.b1t, self.len = T.Dev(np.array(K.SCHED_LR, dtype=np.float32)), T.Dev(np.array(K.SCHED_B1, dtype=np.float32)), len(K.SCHED_LR)
        else:
            self.lrt, self.b1t, self.len = T._f1(K.ADAM["lr"]), None, 1
        self.nb = T._f1(norm[0]) if norm is not None else None
        self.ema0 = ema_input(n) if ema else None
        self.ema = T.Dev(self.ema0, off=off if ema_off is None else ema_off) if ema else None

    def launch(self, lib, decay=None, warmup=0, skip=None, kw=None, expect=0, what="adamw_dev_ema", ema_ptr="own", sync=True):
        kw = kw or K.ADAM
        a = self.a
        head = (a.p.ptr(), a.g.ptr(), a.m.ptr(), a.v.ptr(), self.n, self.lrt.ptr(), self.b1t.ptr() if self.b1t is not None else None, self.len,
                kw["beta1"], kw["beta2"], kw["eps"], kw["wd"], self.sd.ptr(), self.nb.ptr() if self.nb else None,
                self.norm[1] if self.norm is not None else 0.0, skip.ptr() if skip else None, a.shadow.ptr() if a.shadow is not None else None)
        if decay is None:
            rc = lib.psg_adamw_dev_f32(*head, T._stream())
        else:
            eptr = (self.ema.ptr() if self.ema is not None else None) if ema_ptr == "own" else ema_ptr
            rc = lib.psg_adamw_dev_ema_f32(*head, eptr, decay, warmup, T._stream())
        assert rc == expect, f"{what}: return code {rc}, expected {expect}: {lib.psg_last_error().decode()}"
        if sync:
            T._sync(what)
            self.check_guards(what)

    def check_guards(self, what):
        a = self.a
        assert a.intact() and self.sd.intact() and self.lrt.kept() and (self.b1t is None or self.b1t.kept()) and (self.nb is None or self.nb.kept()) \
            and (self.ema is None or self.ema.intact()), f"{what}: the gradient, a table, the norm or a guard changed"

    def state(self):
        s = dict(self.a.state(), step=self.sd.cpu())
        if self.a.shadow is not None:
            s["shadow"] = self.a.shadow.cpu()
        return s

    def untouched(self):
        h = self.a.host
        ok = all(R.same_bits(x, h["pgmv".index(name)]) for name, x in self.a.state().items())
        ok = ok and (self.a.shadow is None or bool(torch.isnan(self.a.shadow.v).all()))
        return ok and (self.ema is None or self.ema.kept())


def _ema_checks(key, what, run, decay, warmup, k):
    """The EMA against the restatement on the kernel's own p' (bits) and against the fp64 bound."""
    p_new = run.a.p.np()
    T._bitcheck(key + " bits", what + " ema vs restatement", run.ema.cpu(), torch.from_numpy(E.ema_f32(run.ema0, p_new, decay, warmup, k)))
    try:
        r = E.check_ema(run.ema.cpu(), run.ema0, p_new, decay, warmup, k, what + " ema")
    except AssertionError as e:
        print(f"RATIO {what} ema out of bound: {e}")
        raise
    T._note(key + " bound", what + " ema vs fp64", r)


@pytest.mark.parametrize("cid", list(CASES))
def test_adamw_dev_ema(lib, cid):
    n, step_dev, warmup, decay, norm, b1_table, shadow = CASES[cid]
    plain, fused = Run(n, step_dev, norm, b1_table, shadow, ema=False), Run(n, step_dev, norm, b1_table, shadow)
    assert (fused.ema.ptr() % 16 == 0) and (fused.a.p.ptr() % 16 == 0)
    plain.launch(lib, what=f"{cid} adamw_dev")
    fused.launch(lib, decay, warmup, what=f"{cid} adamw_dev_ema")
    key = "adamw_dev_ema " + ("float4" if n % 4 == 0 else "scalar")
    want = plain.state()
    assert int(want["step"][0]) == step_dev + 1
    for name, x in fused.state().items():
        T._bitcheck(key + " optimizer side", f"{cid} {name} vs adamw_dev", x, want[name])
    assert not R.same_bits(fused.a.p.cpu(), fused.a.host[0]), "the step did not move p"
    _ema_checks(key, cid, fused, decay, warmup, step_dev + 1)


def test_ema_off_the_boundary_is_the_float4_kernel_bitwise(lib):
    """n % 4 == 0 with every buffer one float off the 16-byte boundary, or with the EMA alone off it, takes the scalar kernel:
    the same bits as the float4 one."""
    n, step_dev, warmup, decay, norm = 1000, 8, 1, 0.9999, K.NORM_ABOVE
    vec = Run(n, step_dev, norm, False, False)
    vec.launch(lib, decay, warmup, what="aligned")
    for name, off, ema_off in (("all one float off", 1, None), ("the EMA one float off", 0, 1)):
        sca = Run(n, step_dev, norm, False, False, off=off, ema_off=ema_off)
        assert sca.ema.ptr() % 16 == 4 and sca.a.p.ptr() % 16 == (4 if off else 0)
        sca.launch(lib, decay, warmup, what=name)
        for what, x in vec.state().items():
            T._bitcheck("adamw_dev_ema scalar vs float4", f"{name}: {what}", sca.state()[what], x)
        T._bitcheck("adamw_dev_ema scalar vs float4", f"{name}: ema", sca.ema.cpu(), vec.ema.cpu())
    bad = Run(n, step_dev, norm, False, True, ema_off=1)                 # the shadow needs the float4 path: refused, nothing written
    bad.launch(lib, decay, warmup, expect=T._api().ERR_ALIGN, what="shadow with the EMA off the boundary")
    assert b"bf16 shadow" in lib.psg_last_error() and bad.untouched() and int(bad.sd.cpu()[0]) == step_dev


@pytest.mark.parametrize("n", [1000, 1001], ids=["float4", "scalar"])
def test_ema_skip_word(lib, n):
    """Each single bit of PSG_FLAG_SKIP_MASK leaves p, m, v, the shadow, the EMA and *step_dev as they were; 16 and 64 alone do
    not skip and give the bits of a launch without a flag word."""
    step_dev, warmup, decay, norm, shadow = 1, 1, 0.9, K.NORM_ABOVE, n % 4 == 0
    plain = Run(n, step_dev, norm, False, shadow)
    plain.launch(lib, decay, warmup, what="no flag word")
    for bit in K.SKIP_BITS + K.NO_SKIP_BITS:
        r, word = Run(n, step_dev, norm, False, shadow), T._i32(bit)
        r.launch(lib, decay, warmup, skip=word, what=f"skip word {bit}")
        assert word.kept()
        if bit in K.SKIP_BITS:
            assert r.untouched() and int(r.sd.cpu()[0]) == step_dev, f"skip word {bit}: something was written"
        else:
            for name, x in plain.state().items():
                assert R.same_bits(r.state()[name], x), f"skip word {bit}: {name} differs from the launch without a flag"
            assert R.same_bits(r.ema.cpu(), plain.ema.cpu()) and not r.ema.kept(), f"skip word {bit}: the EMA differs from the launch without a flag"
        T._note("adamw_dev_ema skip word", f"n {n} skip word {bit}", 0.0)


def test_ema_drift_over_200_calls(lib):
    """200 calls with an lr table of zeros and no weight decay: p' stays p bit for bit, the EMA walks towards it under the
    warm-up's d_k (decay 0.9) and stays within the geometrically summed per-step bound of the fp64 recursion."""
    n, calls, decay = 1000, 200, 0.9
    r = Run(n, 0, None, False, False)
    r.lrt = T._f1(0.0)
    kw = K.adam_kw({"wd": 0.0})
    for _ in range(calls):
        r.launch(lib, decay, 1, kw=kw, what="drift", sync=False)
    T._sync("drift")
    r.check_guards("drift")
    assert int(r.sd.cpu()[0]) == calls
    assert R.same_bits(r.a.p.cpu(), r.a.host[0]), "lr = 0 and wd = 0 moved p"
    ref, bound = E.drift(r.ema0, r.a.host[0], decay, 1, calls)
    err = (r.ema.cpu().double() - ref).abs()
    ratio = float((err / bound).max())
    T._note("adamw_dev_ema drift", f"drift over {calls} calls", ratio)
    assert ratio <= 1.0, f"drift: worst err / bound {ratio:.3g}"
    T._bitcheck("adamw_dev_ema drift", "drift vs the restatement folded", r.ema.cpu(), torch.from_numpy(E.fold(r.ema0, [r.a.host[0].numpy()] * calls, decay, 1)))


@pytest.mark.parametrize("n,off", [(1, 0), (7, 0), (1000, 0), (1001, 0), (1000, 1)], ids=["1", "7", "1000-float4", "1001", "1000-one-float-off"])
def test_swap(lib, n, off):
    a0, b0 = K.hn(n, f"ema.swap.a.{n}", 1.0), K.hn(n, f"ema.swap.b.{n}", 2.0)
    a, b = T.Dev(a0, off=off), T.Dev(b0, off=off)
    assert a.ptr() % 16 == 4 * off and b.ptr() % 16 == 4 * off
    T._run(lib.psg_swap_f32(a.ptr(), b.ptr(), n, T._stream()), "swap")
    assert a.intact() and b.intact(), "swap: a guard changed"
    T._bitcheck("swap", f"swap n {n} off {off}: a", a.cpu(), torch.from_numpy(b0))
    T._bitcheck("swap", f"swap n {n} off {off}: b", b.cpu(), torch.from_numpy(a0))
    T._run(lib.psg_swap_f32(a.ptr(), b.ptr(), n, T._stream()), "swap back")
    assert a.kept() and b.kept(), "swap twice is not the identity"


def test_argument_errors_write_nothing(lib):
    api = T._api()
    n = 1000
    r = Run(n, 3, K.NORM_ABOVE, False, True)
    r.launch(lib, 0.9, 1, expect=api.ERR_ARG, ema_ptr=None, what="null ema")
    assert b"null" in lib.psg_last_error() and r.untouched() and int(r.sd.cpu()[0]) == 3
    for bad in (1.0, -0.5, float("nan")):
        r.launch(lib, bad, 1, expect=api.ERR_SHAPE, what=f"ema_decay {bad}")
        assert b"ema_decay" in lib.psg_last_error() and r.untouched() and int(r.sd.cpu()[0]) == 3
    buf = T.Dev(K.hn(64, "ema.swap.overlap", 1.0))
    p = buf.ptr()
    assert lib.psg_swap_f32(p, p + 16, 8, T._stream()) == api.ERR_ARG and b"overlap" in lib.psg_last_error()
    assert lib.psg_swap_f32(p, None, 8, T._stream()) == api.ERR_ARG
    assert lib.psg_swap_f32(p, p, 8, T._stream()) == api.OK and lib.psg_swap_f32(p, p + 128, 0, T._stream()) == api.OK
    T._sync("swap refusals")
    assert buf.kept()
    T._note("adamw_dev_ema refusals", "null ema, ema_decay out of range, swap overlap", 0.0)
