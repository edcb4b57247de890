"""CPU suite for the EMA tests: the fp32 restatement of tests/ema_ref.py lies inside the fp64 bound, each planted mistake lies
outside it, the warm-up table matches its closed form and saturates where the arithmetic says, the drift bound holds for the
restatement iterated - and the host-only refusals of psg_adamw_dev_ema_f32 / psg_swap_f32 with their codes (nothing here launches
a kernel)."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import ema_ref as E
from tests import step_cases as K

FAKE = 0x7F0000000000          # a 16-byte aligned address nothing dereferences: every call below returns before a launch
N = 1000
DECAYS = [0.0, 0.9, 0.999, 0.9999]
STEPS = [1, 2, 9, 80, 1000]


def _inputs():
    return K.hn(N, "ema.ref.ema", 1.0), K.hn(N, "ema.ref.p", 1.0)


@pytest.mark.parametrize("warmup", [0, 1])
@pytest.mark.parametrize("decay", DECAYS)
def test_restatement_lies_within_the_bound(decay, warmup):
    ema, p = _inputs()
    for k in STEPS:
        got = E.ema_f32(ema, p, decay, warmup, k)
        r = E.check_ema(got, ema, p, decay, warmup, k, f"ema decay {decay} warmup {warmup} k {k}")
        assert r <= 1.0


def test_torch_form_of_the_restatement_has_the_numpy_forms_bits():
    ema, p = _inputs()
    for decay, warmup, k in [(0.9, 1, 1), (0.9999, 1, 1000), (0.999, 0, 3), (0.0, 1, 2)]:
        a = E.ema_f32(ema, p, decay, warmup, k)
        b = E.ema_f32(torch.from_numpy(ema), torch.from_numpy(p), decay, warmup, k)
        assert b.dtype == torch.float32 and np.array_equal(a.view(np.int32), b.numpy().view(np.int32))
    a, b = E.fold(ema, [p, ema, p], 0.999, 1), E.fold(torch.from_numpy(ema), [torch.from_numpy(x) for x in (p, ema, p)], 0.999, 1)
    assert np.array_equal(a.view(np.int32), b.numpy().view(np.int32))


@pytest.mark.parametrize("mistake", E.MISTAKES)
def test_planted_mistakes_exceed_the_bound(mistake):
    """k off by one where the warm-up is in use (also at k = 1000, where the quotient moves by 9e-6), d and 1 - d swapped with
    and without the warm-up."""
    ema, p = _inputs()
    cases = [(0.9999, 1, 1), (0.9999, 1, 9), (0.9999, 1, 1000)] if mistake == "k_off_by_one" else [(0.9, 0, 5), (0.9999, 1, 9), (0.9999, 0, 1000)]
    for decay, warmup, k in cases:
        wrong, _, _, _ = E.ema_f64(ema, p, decay, warmup, k, mistake=mistake)
        with pytest.raises(AssertionError, match="out of bound"):
            E.check_ema(wrong.float(), ema, p, decay, warmup, k, f"{mistake} decay {decay} k {k}")


def test_k_off_by_one_is_invisible_only_where_the_decay_saturates():
    """decay 0.9 at k = 200: both k and k - 1 give min = 0.9, the planted mistake changes nothing - the kernel cases that are to
    notice it must sit in the warm-up (tests/test_ema_kernels_gpu.py: *step_dev 0, 1, 8 with 0.9; all four with 0.9999)."""
    ema, p = _inputs()
    a = E.ema_f64(ema, p, 0.9, 1, 200)[0]
    b = E.ema_f64(ema, p, 0.9, 1, 200, mistake="k_off_by_one")[0]
    assert torch.equal(a, b)


def test_warmup_table_matches_the_closed_form_and_saturates():
    for k in range(1, 2001):
        w = E.warmup_f32(k)
        exact = Fraction(1 + k, 10 + k)
        assert abs(Fraction(float(w)) - exact) <= exact * Fraction(1, 2 ** 24), f"k = {k}: the quotient is not the rounded (1 + k) / (10 + k)"
        for decay in (0.9, 0.999, 0.9999):
            d, omd = E.decay_f32(decay, 1, k)
            dx, quotient = E.decay_exact(decay, 1, k)
            assert d == min(np.float32(decay), w) and omd == np.float32(1) - d
            assert quotient == (exact < Fraction(float(np.float32(decay))))
            assert abs(float(d) - dx) <= dx * E.U
    # (1 + k) / (10 + k) >= D  <=>  k >= (10 D - 1) / (1 - D), D the fp32 value of the decay (0.9f is just below 0.9, 0.999f just
    # above 0.999, 0.9999f below 0.9999): the first saturated step is 80, 8991 and 89 976
    for decay in (0.9, 0.999, 0.9999):
        D = Fraction(float(np.float32(decay)))
        first = -((1 - 10 * D) // (1 - D))                  # ceil((10 D - 1) / (1 - D))
        first = int(first)
        assert E.decay_exact(decay, 1, first) == (float(D), False) and E.decay_exact(decay, 1, first - 1)[1]
        assert E.decay_f32(decay, 1, first + 1)[0] == np.float32(decay)
    firsts = [int(-((1 - 10 * Fraction(float(np.float32(d)))) // (1 - Fraction(float(np.float32(d)))))) for d in (0.9, 0.999, 0.9999)]
    assert firsts == [80, 8991, 89976]
    assert E.decay_f32(0.999, 1, 2000)[0] < np.float32(0.999) and E.decay_f32(0.9999, 1, 2000)[0] < np.float32(0.9999)     # not yet
    assert E.decay_f32(0.9, 1, 2000)[0] == np.float32(0.9)
    assert E.decay_f32(0.999, 1, 9000)[0] == np.float32(0.999) and E.decay_f32(0.9999, 1, 90000)[0] == np.float32(0.9999)
    assert E.decay_f32(0.9999, 0, 1) == (np.float32(0.9999), np.float32(1) - np.float32(0.9999))


def test_drift_bound_admits_the_restatement_iterated():
    ema, p = _inputs()
    ref, bound = E.drift(ema, p, 0.9, 1, 200)
    got = E.fold(ema, [p] * 200, 0.9, 1)
    err = (torch.from_numpy(got).double() - ref).abs()
    assert bool((err <= bound).all())
    assert float(bound.max()) < 1e-5                        # a bound, not a licence: 200 steps stay within ~100 ulps of |p| <= 1
    # the whole warm-up one step late: after 200 steps the start is forgotten (prod d_k ~ 1e-17), after 5 it is not
    ref5, bound5 = E.drift(ema, p, 0.9, 1, 5)
    assert bool(((torch.from_numpy(E.fold(ema, [p] * 5, 0.9, 1)).double() - ref5).abs() <= bound5).all())
    assert bool(((torch.from_numpy(E.fold(ema, [p] * 5, 0.9, 1, k0=2)).double() - ref5).abs() > bound5).any())


# ------------------------------------------------------------------------------------------------ host-only refusals
@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def _ema_call(lib, ema=FAKE, decay=0.9, n=8, p=FAKE, step_dev=FAKE, sched_len=1):
    return lib.psg_adamw_dev_ema_f32(p, FAKE, FAKE, FAKE, n, FAKE, None, sched_len, 0.9, 0.999, 1e-6, 0.01, step_dev, None, 0.0, None, None,
                                     ema, decay, 1, None)


def test_adamw_dev_ema_refusals(lib):
    from pokemon_sprite_generator_amd import _lib
    assert _ema_call(lib, ema=None) == _lib.ERR_ARG and b"null" in lib.psg_last_error()
    assert _ema_call(lib, p=None) == _lib.ERR_ARG and _ema_call(lib, step_dev=None) == _lib.ERR_ARG
    for bad in (1.0, 1.5, -0.1, float("nan")):
        assert _ema_call(lib, decay=bad) == _lib.ERR_SHAPE, f"ema_decay {bad}"
        assert b"ema_decay" in lib.psg_last_error()
    assert _ema_call(lib, n=0) == _lib.ERR_SHAPE and _ema_call(lib, sched_len=0) == _lib.ERR_SHAPE
    # the bf16 shadow needs the float4 path, and an EMA off the 16-byte boundary leaves it
    rc = lib.psg_adamw_dev_ema_f32(FAKE, FAKE, FAKE, FAKE, 8, FAKE, None, 1, 0.9, 0.999, 1e-6, 0.01, FAKE, None, 0.0, None, FAKE, FAKE + 4, 0.9, 1, None)
    assert rc == _lib.ERR_ALIGN and b"bf16 shadow" in lib.psg_last_error()


def test_swap_refusals(lib):
    from pokemon_sprite_generator_amd import _lib
    assert lib.psg_swap_f32(None, FAKE, 8, None) == _lib.ERR_ARG and lib.psg_swap_f32(FAKE, None, 8, None) == _lib.ERR_ARG
    assert b"null" in lib.psg_last_error()
    assert lib.psg_swap_f32(FAKE, FAKE + 4096, 0, None) == _lib.OK and lib.psg_swap_f32(FAKE, FAKE + 4096, -3, None) == _lib.OK
    assert lib.psg_swap_f32(FAKE, FAKE, 8, None) == _lib.OK                                   # a == b: nothing to do, nothing launched
    assert lib.psg_swap_f32(FAKE, FAKE + 16, 8, None) == _lib.ERR_ARG and lib.psg_swap_f32(FAKE + 28, FAKE, 8, None) == _lib.ERR_ARG
    assert b"overlap" in lib.psg_last_error()
