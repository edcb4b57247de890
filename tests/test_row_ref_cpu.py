"""CPU suite for the row-kernel tests: the references and bounds of tests/row_ref.py are right and tight (against torch, and
against planted mistakes), the tables of tests/row_cases.py agree with the library's host-only answers
(psg_upsample_route, psg_prep_weight_route, psg_colsum_workspace_bytes), and the host-only refusals of the row launchers -
nothing here launches a kernel."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import row_cases as K
from tests import row_ref as R

FAKE = 0x7F0000000000          # a 16-byte aligned address nothing dereferences: every call below is refused or host-only


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------------------- upsample
_GEOMS = [(g[0], g[1]) for g in K.UP_GEOMS] + [((54, 54), (108, 108))]         # every case shape, the grid-stride case included


@pytest.mark.parametrize("geom", _GEOMS, ids=lambda g: f"{g[0][0]}x{g[0][1]}-{g[1][0]}x{g[1][1]}")
def test_upsample_restatement_agrees_with_interpolate(geom):
    """(a) F.interpolate(bilinear, align_corners=False) on fp32 CPU tensors, forward and backward, lies within the bound of the
    restatement: the restated fp32 coordinates are torch's, and the bound admits a correct fp32 implementation.

    One allowance, for this comparison only: torch's CPU build contracts the coordinate's multiply-add, the kernels (built with
    -ffp-contract=off) and the restatement round the product first - at 2 -> 6, o = 1 torch's weight is 1.5e-8 where theirs is
    0.  A coordinate then differs by at most 2^-24 (s + 0.5) <= 2^-24 n_in per axis, which moves a forward value by at most
    |dy/dl| = |(1 - lw)(v10 - v00) + lw (v11 - v01)| <= 2 max |x| times that, and each of the n weights of a backward sum by
    at most that: extra = 2^-24 (Hi + Wi) 2 max |x|, respectively 2^-24 (Hi + Wi) n max |dy|."""
    (Hi, Wi), (Ho, Wo) = geom
    x = K.h((2, Hi, Wi, 4), "row.up.cpu.x", 1.5)
    dy = K.h((2, Ho, Wo, 4), "row.up.cpu.dy", 1.5)
    xt = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    yt = F.interpolate(xt, size=(Ho, Wo), mode="bilinear", align_corners=False)
    yt.backward(dy.permute(0, 3, 1, 2).contiguous())
    coord = R.U * (Hi + Wi)
    y, S, n = R.upsample_fwd(x, Ho, Wo)
    R.check(yt.detach().permute(0, 2, 3, 1), y, S, torch.float32, f"interpolate forward {geom}", n + 3, extra=coord * 2 * float(x.abs().max()))
    dx, S, n = R.upsample_bwd(dy, Hi, Wi)
    R.check(xt.grad.permute(0, 2, 3, 1), dx, S, torch.float32, f"interpolate backward {geom}", n + 3, extra=coord * n * float(dy.abs().max()))


def _contrib_counts(n_in, n_out):
    i0, i1, w1 = R.bilin_coord(n_in, n_out)
    assert bool((w1 < 1).all()) and bool((w1 >= 0).all())          # 1 - w1 is never zero: i0 always contributes
    second = (w1 != 0) & (i1 != i0)
    return np.bincount(i0, minlength=n_in) + np.bincount(i1[second], minlength=n_in), i0, i1, second


def test_upsample_bwd8_keeps_enough_columns_up_to_3x():
    """(b) upsample_bwd8_kernel keeps 6 contributing output columns per input column and drops a seventh silently; the
    predicate sends Wo <= 3 Wi there.  For every 1 <= Wi <= 256 and Wi <= Wo <= 3 Wi no input column has more than 6 (the VAE
    decoder's 108 -> 215 is inside), the count reaches exactly 6, and 7 -> 28 has 8."""
    worst = 0
    for Wi in range(1, 257):
        for Wo in range(Wi, 3 * Wi + 1):
            c = int(_contrib_counts(Wi, Wo)[0].max())
            assert c <= 6, (Wi, Wo, c)
            worst = max(worst, c)
    assert worst == 6
    assert int(_contrib_counts(7, 28)[0].max()) == 8
    assert [len(c) for c in R.contributors(7, 28)] == list(_contrib_counts(7, 28)[0])


def test_upsample_bwd_window_contains_every_contributor():
    """(b) the [lo, hi] window of output indices both backward kernels scan, restated in fp32, contains every contributing
    output index, for Wi <= 64 and Wo up to 8 Wi."""
    for Wi in range(1, 65):
        for Wo in range(Wi, 8 * Wi + 1):
            _, i0, i1, second = _contrib_counts(Wi, Wo)
            o = np.arange(Wo)
            first, last = np.full(Wi, Wo), np.full(Wi, -1)
            np.minimum.at(first, i0, o); np.maximum.at(last, i0, o)
            np.minimum.at(first, i1[second], o[second]); np.maximum.at(last, i1[second], o[second])
            lo, hi = R.bwd_window(Wi, Wo)
            used = last >= 0
            assert bool((lo[used] <= first[used]).all()) and bool((hi[used] >= last[used]).all()), (Wi, Wo)


def test_upsample_clamped_weights_are_exact_in_the_case_table():
    """Where i0 = i1 with a non-zero w1 (one input pixel along the axis) the backward adds fl(fl(1 - l) + l): two roundings where
    the bound counts one.  The table's cases of that kind have weights for which both operations are exact."""
    seen = 0
    for (Hi, Wi), (Ho, Wo), _ in K.UP_GEOMS:
        for n_in, n_out in ((Hi, Ho), (Wi, Wo)):
            i0, i1, w1 = R.bilin_coord(n_in, n_out)
            m = (i0 == i1) & (w1 != 0)
            seen += int(m.sum())
            one_minus = (np.float32(1.0) - w1[m]).astype(np.float32)
            assert bool((one_minus.astype(np.float64) == 1.0 - w1[m].astype(np.float64)).all())
            assert bool(((one_minus + w1[m]).astype(np.float32) == 1.0).all())
    assert seen > 0


def _ulp_off(ref, dtype):
    """ref rounded to dtype, with one element moved one bf16 ulp away from its reference: an element in the lower half of its
    binade, where an ulp (2^-7 of the binade's base) clearly exceeds the rounding allowance 2^-8 |ref|."""
    got = ref.to(dtype).double().reshape(-1)
    r = ref.reshape(-1)
    mant = r.abs() / 2.0 ** torch.floor(torch.log2(r.abs().clamp_min(1e-30)))
    ok = (r.abs() > 0.05) & (mant > 1.05) & (mant < 1.4)
    assert bool(ok.any())
    i = int(torch.nonzero(ok)[0])
    ulp = 2.0 ** (math.floor(math.log2(float(r[i].abs()))) - 7)
    got[i] = got[i] + (ulp if got[i] >= r[i] else -ulp)
    return got.reshape(ref.shape)


@pytest.mark.parametrize("layout", ["bf16-c8", "f32-c4"])
@pytest.mark.parametrize("geom", K.UP_GEOMS, ids=K.up_ids())
def test_upsample_bound_notices_planted_mistakes(geom, layout):
    """(c) one contribution dropped, the H and W coordinates exchanged (where the two ratios differ), and one bf16 ulp on one
    element: each lands outside the bound, forward and backward, at every case - and the unmodified result inside."""
    (Hi, Wi), (Ho, Wo), _ = geom
    dname = K.UP_LAYOUTS[layout][0]
    dt = K.DTYPES[dname]
    x, dy = K.up_operands(layout, geom)
    Wh, Ww = R.axis_weights(Hi, Ho), R.axis_weights(Wi, Wo)
    tw = torch.from_numpy
    y, Sy, ny = R.upsample_fwd(x, Ho, Wo)
    dx, Sx, nx = R.upsample_bwd(dy, Hi, Wi)
    R.check(y.to(dt), y, Sy, dt, "forward", ny + 3)
    R.check(dx.to(dt), dx, Sx, dt, "backward", nx + 3)
    # one contribution dropped: the largest single term of the backward, the largest of the forward
    terms = torch.einsum("oh,pw,bopc->bopchw", tw(Wh), tw(Ww), dy.double())              # term of dx[b,h,w,c] from (o,p)
    i = int(terms.abs().argmax())
    b, o, p, c, hh, ww = (int(v) for v in torch.unravel_index(torch.tensor(i), terms.shape))
    bad = dx.clone(); bad[b, hh, ww, c] -= terms[b, o, p, c, hh, ww]
    assert _fails(lambda: R.check(bad.to(dt), dx, Sx, dt, "backward", nx + 3)), "a dropped backward contribution passes"
    terms = torch.einsum("oh,pw,bhwc->bopchw", tw(Wh), tw(Ww), x.double())
    i = int(terms.abs().argmax())
    b, o, p, c, hh, ww = (int(v) for v in torch.unravel_index(torch.tensor(i), terms.shape))
    bad = y.clone(); bad[b, o, p, c] -= terms[b, o, p, c, hh, ww]
    assert _fails(lambda: R.check(bad.to(dt), y, Sy, dt, "forward", ny + 3)), "a dropped forward contribution passes"
    # H and W exchanged: each axis interpolated with the other axis's ratio (visible only where the ratios differ)
    if Hi * Wo != Wi * Ho:
        Whs, Wws = tw(R.axis_weights(Hi, Ho, ratio=(Wi, Wo))), tw(R.axis_weights(Wi, Wo, ratio=(Hi, Ho)))
        ys = R.upsample_fwd(x, Ho, Wo, Whs, Wws)[0]
        dxs = R.upsample_bwd(dy, Hi, Wi, Whs, Wws)[0]
        assert _fails(lambda: R.check(ys.to(dt), y, Sy, dt, "forward", ny + 3)), "exchanged axes pass (forward)"
        assert _fails(lambda: R.check(dxs.to(dt), dx, Sx, dt, "backward", nx + 3)), "exchanged axes pass (backward)"
    # one bf16 ulp on one element
    assert _fails(lambda: R.check(_ulp_off(y, dt), y, Sy, dt, "forward", ny + 3)), "one bf16 ulp passes (forward)"
    assert _fails(lambda: R.check(_ulp_off(dx, dt), dx, Sx, dt, "backward", nx + 3)), "one bf16 ulp passes (backward)"


def test_upsample_route_table(lib):
    """The stored routes are psg_upsample_route's answers for pointers of the stored alignment (host only)."""
    for layout, (dname, C, (ldr, offr), (ldw, offw), _) in K.UP_LAYOUTS.items():
        es = 2 if dname == "bf16" else 4
        for geom in K.UP_GEOMS:
            (Hi, Wi), (Ho, Wo), _ = geom
            for backward in (0, 1):
                rc, got = K.query_upsample_route(lib, backward, dname, FAKE + offr * es, ldr, FAKE + 0x100000 + offw * es, ldw, K.UP_B, Hi, Wi, Ho, Wo, C)
                assert rc == 0 and got == K.up_expected_route(layout, geom, backward), (layout, geom, backward, rc, got)
    g = K.UP_GRID_STRIDE
    rc, got = K.query_upsample_route(lib, 0, "f32", FAKE, g["C"], FAKE, g["C"], g["B"], g["Hi"], g["Wi"], g["Ho"], g["Wo"], g["C"])
    assert (rc, got) == (0, 0) and g["B"] * g["Ho"] * g["Wo"] * g["C"] // 4 > 8192 * 256        # the forward's lanes loop
    # the launches' own refusals, with their codes
    assert K.query_upsample_route(lib, 0, "bf16", FAKE, 8, FAKE, 8, 2, 4, 4, 3, 8, 8)[0] == -1          # Ho < Hi
    assert K.query_upsample_route(lib, 1, "bf16", FAKE, 6, FAKE, 8, 2, 4, 4, 8, 8, 8)[0] == -1          # ld < C
    assert K.query_upsample_route(lib, 1, "bf16", 0, 8, FAKE, 8, 2, 4, 4, 8, 8, 8)[0] == -6             # null pointer
    assert lib.psg_upsample_bilinear_fwd(FAKE, 8, FAKE, 8, 2, 4, 4, 3, 8, 8, 1, None) == -1 and b"upsample_fwd" in lib.psg_last_error()
    assert lib.psg_upsample_bilinear_bwd(FAKE, 8, None, 8, 2, 4, 4, 8, 8, 8, 1, None) == -6 and b"upsample_bwd" in lib.psg_last_error()


# --------------------------------------------------------------------------------------------------------------- colsum
def test_colsum_plans(lib):
    """The stored (splits, rows per split, last split) are colsum_plan's, by its restatement and by the library
    (splits = psg_colsum_workspace_bytes / (groups * cols * 4)); the rows hit what they are in the table for."""
    for R_, groups, cols, lda, plan in K.COLSUM:
        splits, rps = R.colsum_plan(R_, groups, cols)
        assert (splits, rps, R_ - (splits - 1) * rps) == plan, (R_, groups, cols, splits, rps)
        assert int(lib.psg_colsum_workspace_bytes(R_, groups, cols)) == groups * splits * cols * 4
        assert lda >= cols
    plans = {c[0]: c[4] for c in K.COLSUM}
    assert plans[64][0] == 1 and plans[65][0] == 2 and plans[70][0] == 1 and plans[16500][0] < 256 < (16500 + 63) // 64
    assert plans[4097][2] == 1 and R._tile_depth(17) == 1 + 1 + 4 and R._tile_depth(1) == 5 and R._tile_depth(64) == 4 + 0 + 4


@pytest.mark.parametrize("v", K.colsum_variants(), ids=K.colsum_id)
def test_colsum_bound_notices_planted_mistakes(v):
    """A dropped row, a row counted twice, and the rows of the last split read from the next group each land outside the bound,
    at every launch of the table; the fp64 sum rounded to the output dtype lies inside."""
    R_, groups, cols, lda, (splits, rps, last), di, do, acc, ldo = v
    a, prev = K.colsum_operands(R_, groups, cols, di, extra_groups=1)
    nxt, a = a[1:], a[:groups]
    dt = K.DTYPES[do]
    ref, S = R.colsum(a, prev if acc else None)
    depth = R.colsum_depth(R_, splits, rps, acc)
    R.check(ref.to(dt), ref, S, dt, "colsum", depth)
    g, r = groups - 1, R_ // 2
    for what, bad in (("a dropped row", ref[g] - a[g, r].double()), ("a row counted twice", ref[g] + a[g, r].double()),
                      ("the next group's rows in the last split", ref[g] - a[g, R_ - last:].double().sum(0) + nxt[g, R_ - last:].double().sum(0))):
        m = ref.clone(); m[g] = bad
        assert _fails(lambda: R.check(m.to(dt), ref, S, dt, "colsum", depth)), f"{what} passes at {K.colsum_id(v)}"


def test_colsum_refusals(lib):
    """Host-only: a workspace one byte short, and accumulate onto a bf16 output."""
    need = int(lib.psg_colsum_workspace_bytes(130, 3, 100))
    assert lib.psg_colsum(FAKE, 104, FAKE, 100, 130, 3, 100, 1, 0, 0, FAKE, need - 1, None) == -4 and b"workspace" in lib.psg_last_error()
    assert lib.psg_colsum(FAKE, 104, FAKE, 100, 130, 3, 100, 1, 1, 1, FAKE, need, None) == -6 and b"accumulate" in lib.psg_last_error()


# ------------------------------------------------------------------------------------------------------------- sum_rows
@pytest.mark.parametrize("case", K.SUM_ROWS, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_sum_rows_restatement_within_the_fp64_bound(case):
    dname, rows, cols = case
    dt = K.DTYPES[dname]
    a, b, c, _ = K.sum_rows_operands(dname, rows, cols)
    for ops in ((a, b), (a, b, c)):
        ref, S = R.sum_rows(*ops)
        got = R.sum_rows_restated(*ops)
        assert got.dtype == dt
        R.check(got, ref, S, dt, f"sum_rows {len(ops)} sources", 2)
        assert _fails(lambda: R.check(_ulp_off(ref, dt), ref, S, dt, "sum_rows", 2))
    sp = K.special_values(dname)
    assert torch.equal(R.sum_rows_restated(sp).view(torch.int16 if dname == "bf16" else torch.int32), sp.view(torch.int16 if dname == "bf16" else torch.int32))
    assert bool(torch.isnan(sp[3])) and float(sp[0]) == 0.0 and bool(torch.isinf(sp[1:3]).all()) and 0 < float(sp[4].double()) < 2.0 ** -126


def test_sum_rows_refusals(lib):
    """Host-only: c without b, cols not a multiple of the chunk, a pointer off by 8 bytes."""
    assert lib.psg_sum_rows(FAKE, 8, None, 0, FAKE, 8, FAKE, 8, 4, 8, 1, None) == -6 and b"c needs b" in lib.psg_last_error()
    assert lib.psg_sum_rows(FAKE, 16, None, 0, None, 0, FAKE, 16, 4, 12, 1, None) == -1          # bf16: 12 % 8
    assert lib.psg_sum_rows(FAKE, 8, None, 0, None, 0, FAKE, 8, 4, 6, 0, None) == -1             # fp32: 6 % 4
    for k in range(4):
        p = [FAKE, FAKE, FAKE, FAKE]
        p[k] += 8
        assert lib.psg_sum_rows(p[0], 8, p[1], 8, p[2], 8, p[3], 8, 4, 8, 1, None) == -3 and b"alignment" in lib.psg_last_error()


# ---------------------------------------------------------------------------------------------------------- prep_weight
def test_prep_weight_route_table(lib):
    """The stored kernels are psg_prep_weight_route's (host only), every kernel is reached with and without K padding, and the
    table holds the tile-edge shapes."""
    npad = {}
    for v in K.prep_variants():
        sd, lay, O, I, ks, td, kern = v
        for req, kname in zip(K.PREP_REQUESTS, kern):
            rc, got = K.query_prep_route(lib, FAKE, sd, lay, FAKE + 0x100000 if "f" in req else 0, FAKE + 0x200000 if "d" in req else 0, O, I, ks, td)
            assert rc == 0 and got == K.PREP_KERNELS[kname], (K.prep_id(v), req, rc, got)
            dt = K.DTYPES[td]
            for asked, k in (("f", ks * ks * I), ("d", ks * ks * O)):
                if asked in req:
                    npad.setdefault(kname, set()).add(R.kpad(k, dt) == k)
    assert npad == {k: {True, False} for k in K.PREP_KERNELS}, npad
    # a bf16 source the OHWI kernels cannot take, and a bf16 source for fp32 weights: refused as by the launcher
    assert K.query_prep_route(lib, FAKE, "bf16", "oihw", FAKE, 0, 8, 8, 3, "bf16")[0] == -6
    assert K.query_prep_route(lib, FAKE, "bf16", "ohwi", FAKE, 0, 8, 8, 3, "f32")[0] == -2


def test_prep_weight_refuses_misaligned_4x4_outputs(lib):
    """ksize 4 runs on the OHWI kernels only (prep_weight_kernel's LDS tile holds 9 taps per input channel): a wf or wd that is
    not 16-byte aligned used to fall through to it.  Now PSG_ERR_ARG, from the launcher and the route query alike, before any
    launch."""
    from pokemon_sprite_generator_amd import _lib
    for wf, wd in ((FAKE + 8, FAKE), (FAKE, FAKE + 8), (FAKE + 4, 0), (0, FAKE + 8)):
        for td in (0, 1):
            assert lib.psg_prep_weight(FAKE, 0, 1, wf, wd, 8, 8, 4, td, None) == _lib.ERR_ARG
            assert b"4x4" in lib.psg_last_error() and b"aligned wf and wd" in lib.psg_last_error()
            assert K.query_prep_route(lib, FAKE, "f32", "ohwi", wf, wd, 8, 8, 4, "bf16" if td else "f32")[0] == _lib.ERR_ARG
    assert K.query_prep_route(lib, FAKE, "f32", "ohwi", FAKE, FAKE, 8, 8, 4, "f32") == (0, K.PREP_KERNELS["ohwi_f32"])
    assert K.query_prep_route(lib, FAKE, "f32", "ohwi", FAKE + 8, 0, 8, 8, 3, "f32") == (0, K.PREP_KERNELS["generic"])   # 3x3: the generic kernel takes it


@pytest.mark.parametrize("v", K.prep_variants(), ids=K.prep_id)
def test_prep_weight_reference_layouts(v):
    """The reference's two layouts index the same rounded weight; a wd written at tap * I instead of tap * O differs."""
    sd, lay, O, I, ks, td, _ = v
    dt = K.DTYPES[td]
    w, mem = K.prep_source(sd, lay, O, I, ks)
    assert torch.equal((mem.float().permute(0, 3, 1, 2) if lay == "ohwi" else mem.float()), w)
    wf, wd = R.prep_weight(w, dt)
    taps = ks * ks
    for o, i, t in ((0, 0, 0), (O - 1, I - 1, taps - 1), (O // 2, I // 3, taps // 2)):
        want = w[o, i, t // ks, t % ks].to(dt)
        assert wf[o, t * I + i] == want and wd[i, t * O + o] == want
    assert not bool(wf[:, taps * I:].any()) and not bool(wd[:, taps * O:].any())
    if taps > 1 and O != I:
        bad = torch.zeros((I, max(wd.shape[1], taps * max(O, I))), dtype=dt)
        q = w.to(dt)
        for t in range(taps):
            bad[:, t * I:t * I + O] = q[:, :, t // ks, t % ks].t()
        assert not torch.equal(bad[:, :wd.shape[1]], wd)


# -------------------------------------------------------------------------------------------- epilogue_bwd, dropout_apply
def test_quick_gelu_act_approx_holds_for_the_fp32_formula():
    """psg_common.h quick_gelu_grad, s (1 + 1.702 x (1 - s)) with s = sigmoid(1.702 x), in fp32 with torch against fp64: within
    4 ACT_APPROX relative + ACT_APPROX absolute (the form epilogue_bwd's bound uses), with room to spare."""
    u32 = torch.cat([torch.linspace(-9, 9, 200001), torch.logspace(-6, 1, 20001), -torch.logspace(-6, 1, 20001)]).float()
    s = torch.sigmoid(torch.tensor(1.702) * u32)
    d32 = (s * (1.0 + torch.tensor(1.702) * u32 * (1.0 - s))).double()
    d = R.act_grad(u32.double(), "quick_gelu")
    A = R.ACT_APPROX_ROW["quick_gelu"]
    assert float(((d32 - d).abs() / (4.0 * A * d.abs() + A)).max()) <= 0.5
    x = torch.linspace(-6, 6, 4001, dtype=torch.float64, requires_grad=True)
    (x * torch.sigmoid(1.702 * x)).sum().backward()
    assert torch.allclose(R.act_grad(x.detach(), "quick_gelu"), x.grad, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("kind", K.EPI_ACTS)
def test_epilogue_bwd_reference_and_bound(kind):
    """The reference equals gemm_ref.epilogue_bwd where that knows the activation; only ReLU has kept zeros; a result with one
    element kept that should be dropped, the derivative left out, or alpha forgotten lands outside the bound."""
    from tests import gemm_ref
    rows, cols = 77, 36
    dy, u = K.epi_operands(rows, cols, "bf16")
    keep = R.keep_mask(99, rows, cols, 0.1)
    assert 0.8 < float(keep.float().mean()) < 0.97
    ref, zero, depth, r_extra, extra = R.epilogue_bwd(dy, u, kind, 0.5, keep, 0.1)
    if kind != "quick_gelu":
        assert torch.allclose(ref, gemm_ref.epilogue_bwd(dy, u, kind, 0.5, keep, R.p32(0.1)), rtol=1e-13, atol=0)
    assert torch.equal(ref == 0, zero) and (kind == "relu" or torch.equal(zero, ~keep))
    dt = torch.bfloat16
    chk = lambda got: R.check(got, ref, ref.abs(), dt, kind, depth, extra=extra, r_extra=r_extra)
    chk(ref.to(dt))
    assert _fails(lambda: chk((ref / 0.5).to(dt))), "alpha forgotten passes"
    if kind not in ("none",):
        assert _fails(lambda: chk((dy.double() * 0.5 * keep / (1 - R.p32(0.1))).to(dt))), "the derivative left out passes"
    assert _fails(lambda: chk((ref * (1 - R.p32(0.1))).to(dt))), "the dropout scale forgotten passes"
