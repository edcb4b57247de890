"""-m gpu: the row kernels of csrc/elementwise.hip on every route, through the C ABI (psg_upsample_bilinear_fwd / _bwd,
psg_colsum, psg_sum_rows, psg_prep_weight, psg_epilogue_bwd, psg_dropout_apply), element by element against the fp64 references
and derived bounds of tests/row_ref.py on the cases of tests/row_cases.py.

Per launch: the route or plan is the one the table stores (psg_upsample_route, psg_prep_weight_route,
psg_colsum_workspace_bytes; asserted before the launch); operands sit inside wider NaN-filled row buffers with guard elements
before and after; outputs pre-filled with NaN hold none afterwards; the padding columns, the guards and every input keep
their bits; a second identical launch gives identical bits; and every element lies within its bound of the reference (copies
and weight layouts: bit for bit).  A device error ends the run."""
import os
import time

import numpy as np
import pytest
import torch

from tests import row_cases as K
from tests import row_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
REPORT = os.environ.get("PSG_ROW_REPORT")      # optional: write the worst err / bound per kernel, dtype and route to this file
_WORST, _T = {}, {"t0": None, "n": 0}


def _note(key, ratio):
    _T["n"] += 1
    _WORST[key] = max(_WORST.get(key, 0.0), float(ratio))


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    lib = _lib.init(0)
    _T["t0"] = time.perf_counter()
    yield lib
    if REPORT:
        with open(REPORT, "w") as f:
            f.write("Row kernels (tests/test_row_kernels_gpu.py): worst |err| / bound per kernel, dtype and route over the cases of\n"
                    "tests/row_cases.py; bounds derived in tests/row_ref.py.  0 = bit-exact comparison.\n\n")
            for k in sorted(_WORST):
                f.write(f"{k:<52s} {_WORST[k]:.3g}\n")
            f.write(f"\ncomparisons {_T['n']}, wall time of the file {time.perf_counter() - _T['t0']:.1f} s\n")


def _sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                   # a device error: nothing more runs on this GPU
        pytest.exit(f"{what}: {e}", returncode=3)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


class Buf:
    """A [rows, cols] operand at column `off` of a [rows, ld] row buffer with GUARD elements before and after, all NaN (or
    `pad_values` [rows, ld]) outside the operand.  values: what an input holds (restored by reset()); None: an output, NaN."""

    def __init__(self, rows, cols, ld, off, dtype, values=None, pad_values=None):
        assert off + cols <= ld
        self.flat = torch.full((2 * K.GUARD + rows * ld,), NAN, dtype=dtype, device=DEV)
        self.rows2d = self.flat[K.GUARD:K.GUARD + rows * ld].view(rows, ld)
        if pad_values is not None:
            self.rows2d.copy_(pad_values)
        self.view = self.rows2d[:, off:off + cols]
        self.values = None if values is None else values.to(DEV, dtype)
        self.ld = ld
        self.reset()
        self._outside = [self.flat[:K.GUARD], self.flat[-K.GUARD:], self.rows2d[:, :off], self.rows2d[:, off + cols:]]
        self._saved = [_bits(t).clone() for t in self._outside]

    def reset(self):
        if self.values is None:
            self.view.fill_(NAN)
        else:
            self.view.copy_(self.values)

    def ptr(self):
        return self.view.data_ptr()

    def outside_intact(self):
        return all(torch.equal(_bits(t), s) for t, s in zip(self._outside, self._saved))

    def unchanged(self):
        return self.outside_intact() and torch.equal(_bits(self.view), _bits(self.values))


def _launch_twice(call, outs, what):
    """Run `call` twice on freshly reset outputs; assert the return code, no NaN left, identical bits; return the first results."""
    from pokemon_sprite_generator_amd import _lib
    runs = []
    for _ in range(2):
        for o in outs:
            o.reset()
        _lib.check(call(), what)
        _sync(what)
        runs.append([o.view.clone() for o in outs])
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b)), f"{what}: a second identical launch gives other bits"
    return runs[0]


def _stream():
    from pokemon_sprite_generator_amd import _lib
    return _lib.stream_ptr()


def _hash01(n, mul):
    """n fp32 values in [0, 1) on the device, a multiplicative hash of the element index (inputs of the grid-stride cases)."""
    i = torch.arange(n, device=DEV, dtype=torch.int64)
    return (((i * mul) & 0xFFFFFFFF).double() / 4294967296.0).float()


# ------------------------------------------------------------------------------------------------------------- upsample
def _upsample(lib, layout_name, dname, C, rd, wr, B, Hi, Wi, Ho, Wo, backward, src, want_route, ref_fn):
    dt, code = K.DTYPES[dname], K.DTYPE_CODE[dname]
    rows_rd, rows_wr = (B * Ho * Wo, B * Hi * Wi) if backward else (B * Hi * Wi, B * Ho * Wo)
    rdb = Buf(rows_rd, C, rd[0], rd[1], dt, values=src.reshape(rows_rd, C))
    wrb = Buf(rows_wr, C, wr[0], wr[1], dt)
    what = f"upsample_{'bwd' if backward else 'fwd'} {layout_name} {Hi}x{Wi}->{Ho}x{Wo}"
    rc, got = K.query_upsample_route(lib, backward, dname, rdb.ptr(), rd[0], wrb.ptr(), wr[0], B, Hi, Wi, Ho, Wo, C)
    assert rc == 0 and got == want_route, f"{what}: route {got} (rc {rc}), table {want_route}"
    fn = lib.psg_upsample_bilinear_bwd if backward else lib.psg_upsample_bilinear_fwd
    out, = _launch_twice(lambda: fn(rdb.ptr(), rd[0], wrb.ptr(), wr[0], B, Hi, Wi, Ho, Wo, C, code, _stream()), [wrb], what)
    assert rdb.unchanged(), f"{what}: the launch wrote into its input"
    assert wrb.outside_intact(), f"{what}: the launch wrote into the padding columns or the guards"
    assert not bool(torch.isnan(out).any()), f"{what}: the output still holds NaN"
    ref, S, n = ref_fn()
    ratio = R.check(out.to(ref.device).reshape(ref.shape), ref, S, dt, what, n + 3)
    _note(f"upsample_{'bwd' if backward else 'fwd'} {dname} {'8-channel' if want_route else '4-channel'}", ratio)


@pytest.mark.parametrize("layout", list(K.UP_LAYOUTS))
@pytest.mark.parametrize("geom", K.UP_GEOMS, ids=K.up_ids())
def test_upsample(lib, geom, layout):
    dname, C, rd, wr, _ = K.UP_LAYOUTS[layout]
    (Hi, Wi), (Ho, Wo), _ = geom
    x, dy = K.up_operands(layout, geom)
    _upsample(lib, layout, dname, C, rd, wr, K.UP_B, Hi, Wi, Ho, Wo, 0, x, K.up_expected_route(layout, geom, 0), lambda: R.upsample_fwd(x, Ho, Wo))
    _upsample(lib, layout, dname, C, rd, wr, K.UP_B, Hi, Wi, Ho, Wo, 1, dy, K.up_expected_route(layout, geom, 1), lambda: R.upsample_bwd(dy, Hi, Wi))


def test_upsample_grid_stride(lib):
    """fp32, B = 4, 54 -> 108, C = 256: more four-channel items than the generic forward's 8192 x 256 lanes, so every lane loops.
    The fp64 reference is taken on the device, over every element."""
    g = K.UP_GRID_STRIDE
    B, Hi, Wi, Ho, Wo, C = (g[k] for k in ("B", "Hi", "Wi", "Ho", "Wo", "C"))
    dy = (_hash01(B * Ho * Wo * C, 2654435761) * 3.0 - 1.5).reshape(B, Ho, Wo, C)
    x = dy[:, :Hi, :Wi, :].contiguous() * 0.9
    _upsample(lib, "grid-stride", "f32", C, (C, 0), (C, 0), B, Hi, Wi, Ho, Wo, 0, x, 0, lambda: R.upsample_fwd(x, Ho, Wo))
    _upsample(lib, "grid-stride", "f32", C, (C, 0), (C, 0), B, Hi, Wi, Ho, Wo, 1, dy, 0, lambda: R.upsample_bwd(dy, Hi, Wi))


# --------------------------------------------------------------------------------------------------------------- colsum
@pytest.mark.parametrize("v", K.colsum_variants(), ids=K.colsum_id)
def test_colsum(lib, v):
    R_, groups, cols, lda, (splits, rps, last), di, do, acc, ldo = v
    dti, dto = K.DTYPES[di], K.DTYPES[do]
    what = "colsum " + K.colsum_id(v)
    a, prev = K.colsum_operands(R_, groups, cols, di)
    nbytes = int(lib.psg_colsum_workspace_bytes(R_, groups, cols))
    assert nbytes == groups * splits * cols * 4 and R.colsum_plan(R_, groups, cols) == (splits, rps) and R_ - (splits - 1) * rps == last, \
        f"{what}: plan {nbytes // (groups * cols * 4)} splits, table {splits}"
    ab = Buf(groups * R_, cols, lda, 0, dti, values=a.reshape(-1, cols))
    ob = Buf(groups, cols, ldo, 0, dto, values=prev if acc else None)
    ws = Buf(1, nbytes // 4, nbytes // 4, 0, torch.float32)                 # exactly the bytes asked for, NaN-filled, a guard behind
    out, part = _launch_twice(lambda: lib.psg_colsum(ab.ptr(), lda, ob.ptr(), ldo, R_, groups, cols, K.DTYPE_CODE[di], K.DTYPE_CODE[do], acc,
                                                     ws.ptr(), nbytes, _stream()), [ob, ws], what)
    assert ab.unchanged(), f"{what}: the launch wrote into its input"
    assert ob.outside_intact() and ws.outside_intact(), f"{what}: a store outside the output or behind the workspace"
    assert not bool(torch.isnan(out).any()), f"{what}: the output still holds NaN"
    assert bool(torch.isnan(part).all()) if splits == 1 else not bool(torch.isnan(part).any()), f"{what}: workspace use does not match {splits} splits"
    ref, S = R.colsum(a, prev if acc else None)
    ratio = R.check(out.cpu(), ref, S, dto, what, R.colsum_depth(R_, splits, rps, acc))
    _note(f"colsum {di}->{do} {'single pass' if splits == 1 else 'two-stage'}{' accumulate' if acc else ''}", ratio)


# ------------------------------------------------------------------------------------------------------------- sum_rows
@pytest.mark.parametrize("nsrc", [1, 2, 3])
@pytest.mark.parametrize("case", K.SUM_ROWS, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_sum_rows(lib, case, nsrc):
    dname, rows, cols = case
    dt = K.DTYPES[dname]
    what = f"sum_rows {dname} {rows}x{cols} {nsrc} source(s)"
    a, b, c, left = K.sum_rows_operands(dname, rows, cols)
    if nsrc == 1:                                              # a copy moves bits: -0.0, infinities, a NaN payload, subnormals
        sp = K.special_values(dname)
        a.reshape(-1)[:sp.numel()] = sp
    lay = K.sum_rows_layout(dname, cols)
    srcs = [Buf(rows, cols, *lay[n], dt, values=t) for n, t in zip("abc", (a, b, c))][:nsrc]
    ldy, C1 = lay["y"]
    pad = torch.full((rows, ldy), NAN, dtype=dt)
    pad[:, :C1] = left                                         # the other half of the concat buffer: it must survive
    yb = Buf(rows, cols, ldy, C1, dt, pad_values=pad)
    p = [(s.ptr(), s.ld) for s in srcs] + [(None, 0)] * (3 - nsrc)
    out, = _launch_twice(lambda: lib.psg_sum_rows(p[0][0], p[0][1], p[1][0], p[1][1], p[2][0], p[2][1], yb.ptr(), ldy, rows, cols,
                                                  K.DTYPE_CODE[dname], _stream()), [yb], what)
    assert all(s.unchanged() for s in srcs), f"{what}: the launch wrote into an input"
    assert yb.outside_intact(), f"{what}: the launch wrote into the neighbouring half, the padding or the guards"
    want = R.sum_rows_restated(*(a, b, c)[:nsrc])
    assert torch.equal(_bits(out.cpu()), _bits(want)), f"{what}: not bit-equal to the fp32 sum rounded once"
    ratio = 0.0
    if nsrc > 1:
        assert not bool(torch.isnan(out).any()), f"{what}: the output still holds NaN"
        ref, S = R.sum_rows(*(a, b, c)[:nsrc])
        ratio = R.check(out.cpu(), ref, S, dt, what, 2)
    _note(f"sum_rows {dname} {nsrc} source(s)", ratio)


def test_sum_rows_copy_beyond_the_grid_cap(lib):
    """bf16, 131 073 x 1024: more 16-byte chunks than 65 536 blocks of 256 lanes, so the lanes loop.  Random bits, compared on
    the device."""
    g = K.SUM_ROWS_BIG
    rows, cols = g["rows"], g["cols"]
    assert rows * (cols // 8) > 65536 * 256
    gen = torch.Generator(device=DEV).manual_seed(1234)
    src = torch.randint(-32768, 32767, (rows, cols), dtype=torch.int16, device=DEV, generator=gen).view(torch.bfloat16)
    keep = _bits(src).clone()
    yb = Buf(rows, cols, cols + 8, 0, torch.bfloat16)
    what = "sum_rows copy beyond the grid cap"
    from pokemon_sprite_generator_amd import _lib
    for _ in range(2):
        yb.reset()
        _lib.check(lib.psg_sum_rows(src.data_ptr(), cols, None, 0, None, 0, yb.ptr(), yb.ld, rows, cols, 1, _stream()), what)
        _sync(what)
        assert torch.equal(_bits(yb.view), keep), f"{what}: the copy differs from its source"
    assert torch.equal(_bits(src), keep) and yb.outside_intact(), f"{what}: a store into the source, the padding or the guards"
    _note("sum_rows bf16 copy, grid-stride", 0.0)


# ---------------------------------------------------------------------------------------------------------- prep_weight
@pytest.mark.parametrize("v", K.prep_variants(), ids=K.prep_id)
def test_prep_weight(lib, v):
    sd, lay, O, I, ks, td, kern = v
    dt = K.DTYPES[td]
    w, mem = K.prep_source(sd, lay, O, I, ks)
    wf_ref, wd_ref = R.prep_weight(w, dt)
    assert wf_ref.shape[1] == int(lib.psg_kpad(ks * ks * I, K.DTYPE_CODE[td])) and wd_ref.shape[1] == int(lib.psg_kpad(ks * ks * O, K.DTYPE_CODE[td]))
    src = Buf(1, mem.numel(), mem.numel(), 0, K.DTYPES[sd], values=mem.reshape(1, -1))
    for req, kname in zip(K.PREP_REQUESTS, kern):
        what = f"prep_weight {K.prep_id(v)} request {req}"
        wfb = Buf(O, wf_ref.shape[1], wf_ref.shape[1], 0, dt) if "f" in req else None       # dense rows
        wdb = Buf(I, wd_ref.shape[1], wd_ref.shape[1], 0, dt) if "d" in req else None
        pf, pd = wfb.ptr() if wfb else 0, wdb.ptr() if wdb else 0
        rc, got = K.query_prep_route(lib, src.ptr(), sd, lay, pf, pd, O, I, ks, td)
        assert rc == 0 and got == K.PREP_KERNELS[kname], f"{what}: kernel {got} (rc {rc}), table {kname}"
        outs = [b for b in (wfb, wdb) if b]
        res = _launch_twice(lambda: lib.psg_prep_weight(src.ptr(), K.DTYPE_CODE[sd], 1 if lay == "ohwi" else 0, pf or None, pd or None, O, I, ks,
                                                        K.DTYPE_CODE[td], _stream()), outs, what)
        assert src.unchanged(), f"{what}: the launch wrote into the source"
        for b, r, ref, name in zip(outs, res, [t for t, o in ((wf_ref, wfb), (wd_ref, wdb)) if o], [n for n, o in (("wf", wfb), ("wd", wdb)) if o]):
            assert b.outside_intact(), f"{what}: a store outside {name}"
            assert not bool(torch.isnan(r).any()), f"{what}: {name} still holds NaN"
            assert torch.equal(_bits(r.cpu()), _bits(ref)), f"{what}: {name} is not the permuted, once-rounded weight with +0 padding"
        _note(f"prep_weight {kname} {sd}->{td}", 0.0)


# -------------------------------------------------------------------------------------------- epilogue_bwd, dropout_apply
def _eff_seed(seed):
    """The seed a launch hashes: its argument plus the device word of psg_set_seed_source, if an earlier test left one set."""
    from pokemon_sprite_generator_amd import ops
    return (seed + (int(ops.SeedSource._t.item()) if ops.SeedSource.enabled() else 0)) & 0xFFFFFFFFFFFFFFFF


def _epilogue(lib, what, dname, kind, p, alpha, seed, dyb, ub, gb, rows, cols, dy, u, keep, sel=None):
    dt = K.DTYPES[dname]
    out, = _launch_twice(lambda: lib.psg_epilogue_bwd(dyb.ptr(), dyb.ld, ub.ptr() if kind != "none" else None, ub.ld, gb.ptr(), gb.ld, rows, cols,
                                                      R.ACTS[kind], alpha, p, seed, K.DTYPE_CODE[dname], _stream()), [gb], what)
    assert dyb.unchanged() and ub.unchanged(), f"{what}: the launch wrote into an input"
    assert gb.outside_intact(), f"{what}: the launch wrote into the padding columns or the guards"
    assert not bool(torch.isnan(out).any()), f"{what}: the output still holds NaN"
    got = (out if sel is None else out[sel.to(DEV)]).cpu()
    ref, zero, depth, r_extra, extra = R.epilogue_bwd(dy, u, kind, alpha, keep, p)
    assert torch.equal(got == 0, zero), f"{what}: the zero pattern is not the restated mask ({int(((got == 0) != zero).sum())} elements differ)"
    return R.check(got, ref, ref.abs(), dt, what, depth, extra=extra, r_extra=r_extra)


@pytest.mark.parametrize("kind", K.EPI_ACTS)
@pytest.mark.parametrize("dname", list(K.DTYPES))
@pytest.mark.parametrize("shape", K.EPI_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_epilogue_bwd(lib, shape, dname, kind):
    rows, cols = shape
    dt = K.DTYPES[dname]
    dy, u = K.epi_operands(rows, cols, dname)
    lay = K.epi_layout(cols)
    dyb, ub, gb = Buf(rows, cols, *lay["dy"], dt, values=dy), Buf(rows, cols, *lay["u"], dt, values=u), Buf(rows, cols, *lay["g"], dt)
    for p in K.EPI_P:
        for alpha in K.EPI_ALPHA:
            seed = 7700 + rows + int(alpha * 10)
            keep = R.keep_mask(_eff_seed(seed), rows, cols, p)
            what = f"epilogue_bwd {rows}x{cols} {dname} {kind} p={p} alpha={alpha}"
            ratio = _epilogue(lib, what, dname, kind, p, alpha, seed, dyb, ub, gb, rows, cols, dy, u, keep)
            _note(f"epilogue_bwd {dname} {kind}", ratio)


def _big_inputs(rows, cols):
    d = _hash01(rows * cols, 2654435761) * 2.0 - 1.0
    v = _hash01(rows * cols, 2246822519) * 2.0 - 1.0
    dy = torch.where(d >= 0, 0.25 + d, -0.25 + d).reshape(rows, cols)
    u = torch.where(v >= 0, 0.02 + 2.98 * v, -0.02 + 2.98 * v).reshape(rows, cols)
    return dy, u


def test_epilogue_bwd_grid_stride(lib):
    """fp32, 8200 x 1024: more four-element items than 8192 x 256 lanes.  The reference covers 64 fixed rows, the first and the
    last included; the NaN, guard and input checks cover everything."""
    rows, cols = K.EPI_GRID_STRIDE
    assert rows * cols // 4 > 8192 * 256
    dy, u = _big_inputs(rows, cols)
    sel = K.fixed_rows(rows)
    assert int(sel[0]) == 0 and int(sel[-1]) == rows - 1
    dyb, ub, gb = Buf(rows, cols, cols, 0, torch.float32, values=dy), Buf(rows, cols, cols, 0, torch.float32, values=u), Buf(rows, cols, cols, 0, torch.float32)
    seed, p = 424242, 0.1
    keep = R.keep_mask_rows(_eff_seed(seed), sel, cols, p)
    ratio = _epilogue(lib, "epilogue_bwd grid-stride", "f32", "silu", p, 0.5, seed, dyb, ub, gb, rows, cols, dy[sel.to(DEV)].cpu(), u[sel.to(DEV)].cpu(), keep, sel)
    _note("epilogue_bwd f32 silu, grid-stride", ratio)


def _dropout(lib, what, dname, rows, cols, p, seed, xb, yb, x, keep, sel=None):
    dt = K.DTYPES[dname]
    scale = float(np.float32(1.0 / (1.0 - p)))
    out, = _launch_twice(lambda: lib.psg_dropout_apply(xb.ptr(), xb.ld, yb.ptr(), yb.ld, rows, cols, p, seed, scale, K.DTYPE_CODE[dname], _stream()),
                         [yb], what)
    assert xb is yb or xb.unchanged(), f"{what}: the launch wrote into its input"
    assert yb.outside_intact(), f"{what}: the launch wrote into the padding columns or the guards"
    assert not bool(torch.isnan(out).any()), f"{what}: the output still holds NaN"
    got = (out if sel is None else out[sel.to(DEV)]).cpu()
    ref, depth = R.dropout_apply(x, scale, keep)
    assert torch.equal(got == 0, ~keep), f"{what}: the zero pattern is not the restated mask"
    return R.check(got, ref, ref.abs(), dt, what, depth)


@pytest.mark.parametrize("inplace", [0, 1], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("dname", list(K.DTYPES))
@pytest.mark.parametrize("shape", K.EPI_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_dropout_apply(lib, shape, dname, inplace):
    rows, cols = shape
    dt = K.DTYPES[dname]
    x, _ = K.epi_operands(rows, cols, dname)                   # no element is zero: every zero of the output is a dropped one
    lay = K.epi_layout(cols)
    xb = Buf(rows, cols, *lay["dy"], dt, values=x)
    yb = xb if inplace else Buf(rows, cols, *lay["g"], dt)
    for p in K.DROP_P:
        seed = 9100 + cols + int(p * 10)
        keep = R.keep_mask(_eff_seed(seed), rows, cols, p)
        ratio = _dropout(lib, f"dropout_apply {rows}x{cols} {dname} p={p} {'in place' if inplace else ''}", dname, rows, cols, p, seed, xb, yb, x, keep)
        _note(f"dropout_apply {dname} {'in place' if inplace else 'out of place'}", ratio)


def test_dropout_apply_grid_stride(lib):
    """fp32, 8200 x 1024, as test_epilogue_bwd_grid_stride."""
    rows, cols = K.EPI_GRID_STRIDE
    x, _ = _big_inputs(rows, cols)
    sel = K.fixed_rows(rows)
    xb, yb = Buf(rows, cols, cols, 0, torch.float32, values=x), Buf(rows, cols, cols, 0, torch.float32)
    seed, p = 515151, 0.5
    keep = R.keep_mask_rows(_eff_seed(seed), sel, cols, p)
    ratio = _dropout(lib, "dropout_apply grid-stride", "f32", rows, cols, p, seed, xb, yb, x[sel.to(DEV)].cpu(), keep, sel)
    _note("dropout_apply f32, grid-stride", ratio)
