"""-m gpu: psg_guided_update_f32, psg_cfg_combine_f32 and psg_text_cond_drop_f32 through the C ABI, on the bits against the
float32 restatements of tests/guided_ref.py.  Every device buffer sits between guard words that must keep their bits; inputs
must keep theirs.

Sizes: 1, 3, 4, 7 (scalar path, one float4, a ragged tail), 5832 = 8 x 27 x 27 (one latent batch, float4 path), 2 x 5832 + 1 (odd:
x_copy = x + n is then off the 16-byte boundary) and 4 x GRID_CAP + 5 (more than one trip of the capped grid)."""
import itertools

import numpy as np
import pytest
import torch

from tests import guided_ref as G
from tests import step_ref as R
from tests.test_step_kernels_gpu import Dev, _all_ok, _i32, _run, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
NS = [1, 3, 4, 7, 5832, 2 * 5832 + 1, R.GRID_CAP * 4 + 5]
WS = [0.0, 1.0, 7.5, -1.0]
CLIPS = [0.0, 3.0, 0.25]
K_STEPS = 7
JS = [0, K_STEPS // 2, K_STEPS - 1, -1, K_STEPS]


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    return _lib.init(0)


@pytest.fixture(scope="module")
def tab():
    """[5, 7] fp32: the cosine-clipped schedule at eta = 0.7, from the restatement (test_guided_ref_cpu holds the package's to it)."""
    import pokemon_sprite_generator_amd as psg
    abar = psg.NoiseScheduler().alphas_cumprod.cpu().numpy().astype(np.float32)
    return G.ddim_tables(abar, G.ddim_timesteps(1000, K_STEPS), 0.7)


_INPUTS = {}


def _inputs(n):
    """x0 targets by index % 3: 0 -> 0.5 <= |v| <= 2 (clamped at clip 0.25 only), 1 -> |v| < 0.2 (never), 2 -> 3.5 <= |v| <= 6
    (always), so the unguided x = S0 x0 + S1 eps_c clamps some elements and not others at every step; eps_u is independent of
    eps_c, so guided launches move x0 about.  Shared among the tests and never written."""
    if n not in _INPUTS:
        rng = np.random.default_rng(n)
        kind = np.arange(n) % 3
        mag = np.where(kind == 0, rng.uniform(0.5, 2.0, n), np.where(kind == 1, rng.uniform(0.0, 0.2, n), rng.uniform(3.5, 6.0, n)))
        x0 = (mag * rng.choice([-1.0, 1.0], n)).astype(np.float32)
        ec, eu, z = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
        _INPUTS[n] = (x0, ec, eu, z)
    return _INPUTS[n]


def _combos(n):
    """(has_u, has_z, j, w, clip): the full cross for the small sizes; for the two latent sizes every value of j, w and clip with
    every (has_u, has_z), each at least once; the multi-trip size is about the grid, two launches per (has_u, has_z)."""
    uz = list(itertools.product([False, True], repeat=2))
    if n <= 7:
        return [(u, z, j, w, c) for (u, z) in uz for j in JS for w in WS for c in CLIPS]
    out = []
    for a, (u, z) in enumerate(uz):
        for i in range(len(JS) if n < 100000 else 2):
            out.append((u, z, JS[i], WS[(i + a) % len(WS)], CLIPS[(i + a) % len(CLIPS)]))
    return out


@pytest.mark.parametrize("copy", ["none", "adjacent", "separate"])
@pytest.mark.parametrize("n", NS)
def test_guided_update(lib, tab, n, copy):
    x0, ec, eu, z = _inputs(n)
    tb, ecb, eub, zb = Dev(tab), Dev(ec), Dev(eu), Dev(z)
    clamped = total = 0
    for has_u, has_z, j, w, clip in _combos(n):
        what = f"guided_update n={n} copy={copy} u={has_u} z={has_z} j={j} w={w} clip={clip}"
        jc = min(max(j, 0), K_STEPS - 1)
        x = (tab[0, jc] * x0 + tab[1, jc] * ec).astype(np.float32)
        want, acted = G.guided_update(x, ec, eu if has_u else None, z if has_z else None, tab, j, w, clip, want_mask=True)
        if clip > 0:
            clamped, total = clamped + int(acted.sum()), total + n
        if copy == "adjacent":                                   # the 2n input buffer: x_copy = x + n, unaligned for odd n
            xb = Dev(np.concatenate([x, np.full(n, 77.0, dtype=np.float32)]))
            xp, cp = xb.ptr(), xb.ptr() + 4 * n
        else:
            xb = Dev(x)
            cb = Dev(np.full(n, 77.0, dtype=np.float32)) if copy == "separate" else None
            xp, cp = xb.ptr(), (cb.ptr() if cb is not None else None)
        sb = _i32(j)
        _run(lib.psg_guided_update_f32(xp, cp, ecb.ptr(), eub.ptr() if has_u else None, zb.ptr() if has_z else None, tb.ptr(), K_STEPS,
                                       sb.ptr(), w, clip, n, _stream()), what)
        _all_ok(dict(tab=tb, eps_c=ecb, eps_u=eub, z=zb, step=sb), what)
        assert xb.intact(), what
        got = xb.np()
        assert R.same_bits(got[:n], want), f"{what}: x is not the restated fp32 arithmetic on the bits"
        if copy == "adjacent":
            assert R.same_bits(got[n:], want), f"{what}: x_copy"
        elif copy == "separate":
            assert cb.intact() and R.same_bits(cb.np(), want), f"{what}: x_copy"
    share = clamped / total
    print(f"CLAMPED SHARE guided_update n={n} copy={copy}: {share:.3f} of {total} elements over the launches with clip > 0")
    assert 0.0 < share < 1.0


@pytest.mark.parametrize("n", [7, 5832])
def test_guided_update_nan_stays_where_it_is(lib, tab, n):
    x0, ec, eu, z = _inputs(n)
    ec = ec.copy()
    at = n // 2
    ec[at] = np.nan
    x = (tab[0, 3] * x0 + tab[1, 3] * np.nan_to_num(ec)).astype(np.float32)
    for clip in (0.0, 3.0):
        for has_u in (False, True):
            xb, sb = Dev(np.concatenate([x, x])), _i32(3)
            b = dict(tab=Dev(tab), eps_c=Dev(ec), eps_u=Dev(eu), z=Dev(z), step=sb)
            _run(lib.psg_guided_update_f32(xb.ptr(), xb.ptr() + 4 * n, b["eps_c"].ptr(), b["eps_u"].ptr() if has_u else None, b["z"].ptr(),
                                           b["tab"].ptr(), K_STEPS, sb.ptr(), 2.0, clip, n, _stream()), f"guided_update NaN n={n}")
            got = xb.np()
            want = G.guided_update(x, ec, eu if has_u else None, z, tab, 3, 2.0, clip)
            nan = np.isnan(got[:n])
            assert nan[at] and int(nan.sum()) == 1 and R.same_bits(got[:n], want) and R.same_bits(got[n:], want)
            assert xb.intact()
            # (same_bits compares the NaN of eps_c by position; the other inputs keep their bits)
            assert all(v.intact() for v in b.values()) and b["eps_u"].kept() and b["z"].kept() and b["tab"].kept()


def test_guided_update_refusals(lib):
    from pokemon_sprite_generator_amd import _lib
    P = 4096

    def err():
        return lib.psg_last_error().decode()
    call = lambda a, k=3, clip=3.0, n=8: lib.psg_guided_update_f32(a[0], P, a[1], P, P, a[2], k, a[3], 1.0, clip, n, None)   # noqa: E731
    for i in range(4):                                             # x, eps_c, tab, step_dev
        a = [P] * 4
        a[i] = None
        assert call(a) == _lib.ERR_ARG and err() == "guided_update: null pointer"
    assert call([P] * 4, clip=-0.5) == _lib.ERR_ARG and err().startswith("guided_update: clip=-0.5")
    assert call([P] * 4, clip=float("nan")) == _lib.ERR_ARG
    for k in (0, -2):
        assert call([P] * 4, k=k) == _lib.ERR_ARG and err().endswith(f"k={k}")
    for n in (0, -5):
        assert call([P] * 4, n=n) == _lib.OK                       # nothing launched: the fake pointers are never read
        assert lib.psg_cfg_combine_f32(P, P, 1.0, P, n, None) == _lib.OK
    for i in range(3):
        a = [P] * 3
        a[i] = None
        assert lib.psg_cfg_combine_f32(a[0], a[1], 1.0, a[2], 8, None) == _lib.ERR_ARG and err() == "cfg_combine: null pointer"
    for i in range(3):
        a = [P, 2 * P, 3 * P]
        a[i] = None
        assert lib.psg_text_cond_drop_f32(a[0], a[1], a[2], None, 2, 8, 0.5, 1, None) == _lib.ERR_ARG and err() == "text_cond_drop: null pointer"
    assert lib.psg_text_cond_drop_f32(P, 2 * P, P, None, 2, 8, 0.5, 1, None) == _lib.ERR_ARG and err() == "text_cond_drop: out aliases text"
    for p in (1.0, -0.1, 1.5, float("nan")):
        assert lib.psg_text_cond_drop_f32(P, 2 * P, 3 * P, None, 2, 8, p, 1, None) == _lib.ERR_ARG and err().startswith("text_cond_drop: p=")
    assert lib.psg_text_cond_drop_f32(P, 2 * P, 3 * P, None, 0, 8, 0.5, 1, None) == _lib.OK          # an empty batch
    for B, row in ((-1, 8), (2, 0)):
        assert lib.psg_text_cond_drop_f32(P, 2 * P, 3 * P, None, B, row, 0.5, 1, None) == _lib.ERR_SHAPE


# ---------------------------------------------------------------------------------------------------------- cfg_combine
@pytest.mark.parametrize("alias", [False, True], ids=["out", "in-place"])
@pytest.mark.parametrize("n", NS)
def test_cfg_combine(lib, n, alias):
    _, ec, eu, _ = _inputs(n)
    ub = Dev(eu)
    for w in WS:
        what = f"cfg_combine n={n} w={w} alias={alias}"
        cb = Dev(ec)
        ob = cb if alias else Dev(n=n)
        _run(lib.psg_cfg_combine_f32(cb.ptr(), ub.ptr(), w, ob.ptr(), n, _stream()), what)
        assert ub.kept() and ob.intact() and (alias or cb.kept()), what
        assert R.same_bits(ob.np(), G.cfg_combine(ec, eu, w)), what
    if n >= 4:                                                     # a base off the 16-byte boundary: the element-by-element path
        cb, u1, ob = Dev(ec, off=1), Dev(eu, off=2), Dev(n=n, off=3)
        _run(lib.psg_cfg_combine_f32(cb.ptr(), u1.ptr(), 7.5, ob.ptr(), n, _stream()), "cfg_combine unaligned")
        assert cb.kept() and u1.kept() and ob.intact() and R.same_bits(ob.np(), G.cfg_combine(ec, eu, 7.5))


# ------------------------------------------------------------------------------------------------------- text_cond_drop
SHAPES = [(1, 1), (5, 3), (8, 32 * 256), (64, 20 * 256 + 4), (3, 5)]
_TEXT = {}


def _text(B, row):
    if (B, row) not in _TEXT:
        rng = np.random.default_rng(B * 100003 + row)
        _TEXT[(B, row)] = (rng.standard_normal((B, row)).astype(np.float32), rng.standard_normal(row).astype(np.float32))
    return _TEXT[(B, row)]


def _drop_case(lib, B, row, p, seed, word, off=0):
    """One launch; `word`: the value of the device seed word, or None for none set by this test (one left by an earlier test is
    read and added, as the launch does)."""
    from pokemon_sprite_generator_amd import ops
    dev = torch.device(DEV, 0)
    text, null = _text(B, row)
    was_on = ops.SeedSource.enabled()
    old = int(ops.SeedSource._t.item()) if was_on else None
    try:
        if word is not None:
            ops.SeedSource.enable(dev).fill_(word)
        add = int(ops.SeedSource._t.item()) if ops.SeedSource.enabled() else 0
        eff = (seed + add) & 0xFFFFFFFFFFFFFFFF
        what = f"text_cond_drop B={B} row={row} p={p} seed={seed} word={word} off={off}"
        b = dict(text=Dev(text, off=off), null=Dev(null))
        ob, db = Dev(n=B * row, off=off), Dev(n=B, dtype=torch.int32)
        _run(lib.psg_text_cond_drop_f32(b["text"].ptr(), b["null"].ptr(), ob.ptr(), db.ptr(), B, row, p, seed, _stream()), what)
        _all_ok(b, what)
        assert ob.intact() and db.intact(), what
        want, dropped = G.text_cond_drop(text, null, eff, p)
        got, gd = ob.np().reshape(B, row), db.np()
        assert np.array_equal(gd, dropped), f"{what}: dropped {gd.tolist()}, restated {dropped.tolist()}"
        keep = dropped == 0
        assert R.same_bits(got[keep], text[keep]) and R.same_bits(got[~keep], np.broadcast_to(null, (int((~keep).sum()), row)).copy()), what
        assert R.same_bits(got, want)
        # dropped == NULL: the same rows
        o2 = Dev(n=B * row, off=off)
        _run(lib.psg_text_cond_drop_f32(b["text"].ptr(), b["null"].ptr(), o2.ptr(), None, B, row, p, seed, _stream()), what + " no mask out")
        assert o2.intact() and R.same_bits(o2.np().reshape(B, row), want)
        return dropped
    finally:
        if was_on:
            ops.SeedSource._t.fill_(old)
        else:
            ops.SeedSource.disable()


@pytest.mark.parametrize("word", [None, 1 << 40], ids=["no-word", "word"])            # (the word reaches the seed's high half)
@pytest.mark.parametrize("seed", [1234, 99])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_text_cond_drop(lib, shape, p, seed, word):
    B, row = shape
    dropped = _drop_case(lib, B, row, p, seed, word)
    if p == 0:
        assert not dropped.any()
    elif B >= 8:
        assert 0 < int(dropped.sum()) < B, "both kinds of sample must occur"


def test_text_cond_drop_counts_and_unaligned_base(lib):
    assert int(_drop_case(lib, 8, 32 * 256, 0.5, 1234, 0).sum()) == 3          # (word 0: the figures are those of the plain seed)
    assert int(_drop_case(lib, 64, 20 * 256 + 4, 0.1, 1234, 0).sum()) == 7
    _drop_case(lib, 8, 32 * 256, 0.5, 1234, None, off=1)          # row % 4 == 0 but text / out off the 16-byte boundary
