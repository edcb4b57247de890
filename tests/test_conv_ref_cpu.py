"""Host-side proofs behind the conv route tests (no GPU: psg_conv_route plans on the host).

(a) the routes stored in tests/golden/conv_routes.json are the library's, for every case of tests/conv_cases.py under its own
    settings, and the query leaves the launch counters and the settings alone;
(b) a sweep of shapes, dtypes, geometries, workspace states and settings reaches no launch variant (dtype, tile, mode, split,
    class order, pointwise, staged epilogue) that the table does not launch, and the table holds none the sweep cannot reach;
    every epilogue kind and staging sub-path, every pointwise instantiation and every parity-class shape is in the table;
(c) the extended references of tests/gemm_ref.py equal torch autograd in fp64 on the new geometries, the new activation
    entries hold for the psg_common.h formulas evaluated in fp32, and torch's own fp32 conv of every fp32 case lies within
    gemm_ref.check's bound (so the bound measured on the bf16 kernels is not too tight for the fp32 ones);
(d) the comparator (conv_cases.verify) accepts a plain fp32 emulation of a launch and rejects each of a list of injected
    defects at the table's own shapes.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_cases as K
from tests import gemm_ref as R
from tests.drop_ref import keep_flat


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    return _lib.load()


def _report(line):
    path = os.environ.get("PSG_CONV_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


# ----------------------------------------------------------------------------------------------------- (a) table vs library
def test_table_routes_are_the_librarys(lib):
    pw0, tc0 = int(lib.psg_conv_pw_launches()), int(lib.psg_conv_tapclass_launches())
    bad = []
    for c in K.CASES:
        rc, got = K.query_route(lib, c)
        assert rc == 0, f"{c['name']}: psg_conv_route returned {rc}: {lib.psg_last_error()}"
        want = K.expected_route(c["name"])
        if got != want:
            bad.append(f"{c['name']}: library {[dict(zip(K.ROUTE_FIELDS, l)) for l in got]}, table {[dict(zip(K.ROUTE_FIELDS, l)) for l in want]}")
    assert not bad, "\n".join(bad)
    assert (int(lib.psg_conv_pw_launches()), int(lib.psg_conv_tapclass_launches())) == (pw0, tc0), "the route query moved a launch counter"


def test_route_query_checks_what_the_launch_checks(lib):
    c = dict(K.BY_NAME["epi.staged.plain"])
    out = (C.c_int32 * (1 + 4 * K.NF))()
    o = C.cast(out, C.c_void_p)
    d = K.make_desc(c, K.FAKE_PTRS)
    assert lib.psg_conv_route(C.byref(d), None) == -6                                # PSG_ERR_ARG
    assert lib.psg_conv_route(None, o) == -6
    d.Cin = 60
    assert lib.psg_conv_route(C.byref(d), o) == -1                                   # PSG_ERR_SHAPE
    d = K.make_desc(c, K.FAKE_PTRS); d.dtype = 7
    assert lib.psg_conv_route(C.byref(d), o) == -2                                   # PSG_ERR_DTYPE
    d = K.make_desc(c, dict(K.FAKE_PTRS, x=0x10008))
    assert lib.psg_conv_route(C.byref(d), o) == -3                                   # PSG_ERR_ALIGN
    d = K.make_desc(c, K.FAKE_PTRS); d.Ho = 4
    assert lib.psg_conv_route(C.byref(d), o) == -1
    # a pinned 160-wide tile: an error for fp32 and for parity-class launches, nothing else changes
    for name in ("epi.f32.plain", "g.bf16.3x3s2.dgrad.7x7"):
        cc = dict(K.BY_NAME[name], tile=3)
        assert K.query_route(lib, cc)[0] == -6, name
    assert K.query_route(lib, dict(c, tile=3))[1][0][:2] == (128, 160)
    # a pinned tile is never split, and the setter takes the choice back with -1
    cc = K.BY_NAME["split.bf16.pinned"]
    assert K.query_route(lib, cc)[1][0][3] == 1 and K.query_route(lib, dict(cc, tile=-1, ws="ok"))[1][0][3] > 1


def test_workspace_query_is_the_split_of_the_route(lib):
    """psg_conv_fwd_workspace_bytes and psg_conv_route plan through the same entry: with a workspace of any size offered, every
    case (under its own settings) is routed with splits x M x N x 4 bytes of it when the route splits, and asks for 0 otherwise."""
    bad = []
    for c in K.CASES:
        with K.settings(lib, c):
            need = int(lib.psg_conv_fwd_workspace_bytes(C.byref(K.make_desc(c, K.FAKE_PTRS))))
            rc, launches = K.route_of(lib, K.make_desc(c, K.FAKE_PTRS, 0x900000, 1 << 40))
        assert rc == 0, c["name"]
        L = [dict(zip(K.ROUTE_FIELDS, l)) for l in launches]
        want = L[0]["splits"] * L[0]["M"] * c["Cout"] * 4 if L[0]["splits"] > 1 else 0
        if need != want or any(l["splits"] != 1 for l in L[1:]) or (c["tile"] >= 0 and need):
            bad.append(f"{c['name']}: workspace query {need}, route {[(l['splits'], l['M']) for l in L]} x Cout {c['Cout']}")
    assert not bad, "\n".join(bad)
    d = K.make_desc(K.CASES[0], K.FAKE_PTRS); d.Cin = 60
    assert int(lib.psg_conv_fwd_workspace_bytes(C.byref(d))) == -1


def test_combinations_without_a_kernel_are_an_error_of_the_plan(lib):
    """No fp32 tile is 160 wide and no parity-class kernel is (candidates 3 and 4): pinned there, psg_conv_route returns PSG_ERR_ARG
    in every gather mode, not a route.  There is no fp32 border-class kernel either: with psg_conv_set_tapclass(2) an fp32 launch
    keeps the plain order - the setting forces the form only where it applies.  Smallest shapes of the mat.* cases."""
    modes = {0: dict(H=3, W=5), 1: dict(H=3, W=5, tr=1), 2: dict(H=3, W=5), 3: dict(H=5, W=8, stride=2, tr=1)}
    mk = lambda dn, mode, **kw: K._mk("nokernel", None, dtype=dn, B=3, Cin={"bf16": (64, 24), "f32": (32, 12)}[dn][mode == 2], Cout=12, ks=3,
                                      **modes[mode], **kw)
    for tile in (3, 4):
        for mode in modes:
            assert K.query_route(lib, mk("f32", mode, tile=tile))[0] == -6, (tile, mode)
        assert K.query_route(lib, mk("bf16", 3, tile=tile))[0] == -6, tile
        with K.settings(lib, mk("f32", 0, tile=tile)):             # (a pinned launch is never split: nothing to ask for)
            assert int(lib.psg_conv_fwd_workspace_bytes(C.byref(K.make_desc(mk("f32", 0), K.FAKE_PTRS)))) == 0
    for tile in (-1, 0, 1, 2):
        for mode in (0, 1):
            rc, launches = K.query_route(lib, mk("f32", mode, tile=tile, tapcls=2))
            L = dict(zip(K.ROUTE_FIELDS, launches[0]))
            assert rc == 0 and (L["mode"], L["tapcls"]) == (mode, 0), (tile, mode, L)
            assert dict(zip(K.ROUTE_FIELDS, K.query_route(lib, mk("bf16", mode, tile=tile, tapcls=2))[1][0]))["tapcls"] == 1


def test_case_shapes_are_tiny():
    for c in K.CASES:
        g = K.geom(c)
        assert g["M"] <= 4096 and g["Min"] <= 4096 and c["Cin"] <= 320 and c["Cout"] <= 640, c["name"]


# ---------------------------------------------------------------------------------------------------- (b) reachability
def _table_keys():
    keys = {}
    for c in K.CASES:
        for l in K.expected_route(c["name"]):
            keys.setdefault(K.route_key(c["dtype"], l), c["name"])
    return keys


def _sweep(lib):
    """Every (dtype, BM, BN, mode, split, tapcls, pw, epi_lds) some legal small launch takes.  The tile pin is part of the sweep:
    it is a supported setting, and the only way to some (tile, mode) pairs at these sizes."""
    seen = {}
    out = (C.c_int32 * (1 + 4 * K.NF))()
    o = C.cast(out, C.c_void_p)
    geoms = [(1, 1, 0, 0), (1, 1, 0, 1), (1, 2, 0, 0), (1, 2, 0, 1), (3, 1, 1, 0), (3, 1, 1, 1), (3, 2, 1, 0), (3, 2, 1, 1), (4, 2, 1, 0), (4, 2, 2, 0)]
    grids = [(1, 1, 1), (3, 3, 3), (3, 4, 4), (5, 5, 7), (37, 3, 3), (83, 5, 5), (20, 14, 14), (768, 1, 1), (700, 1, 1), (2048, 1, 1)]
    try:
        for dn in ("bf16", "f32"):
            cins = (8, 24, 64, 192, 200, 320) if dn == "bf16" else (4, 12, 32, 96, 100, 320)
            for (ks, st, pad, tr) in geoms:
                for (B, H, W) in grids:
                    if ks > 1 and H == 1 and B > 100:
                        continue
                    for Cin in cins:
                        for Cout in (4, 8, 72, 136, 320, 512, 640):
                            for ldpre in (0, 4):
                                c = K._mk("sweep", None, dtype=dn, B=B, H=H, W=W, Cin=Cin, Cout=Cout, ks=ks, stride=st, pad=pad, tr=tr,
                                          preact=bool(ldpre), ldpre=ldpre)
                                if K.geom(c)["Hi"] < 1 or K.geom(c)["Wi"] < 1 or K.geom(c)["Ho"] < 1 or K.geom(c)["Wo"] < 1:
                                    continue
                                d0 = K.make_desc(c, K.FAKE_PTRS)
                                d1 = K.make_desc(c, K.FAKE_PTRS, 0x900000, 1 << 30)
                                for cus in (8, 0):
                                    lib.psg_set_available_cus(cus)
                                    for tile in (-1, 0, 1, 2, 3, 4):
                                        lib.psg_conv_set_tile(tile)
                                        for tcls in (0, 1, 2):
                                            lib.psg_conv_set_tapclass(tcls)
                                            for pw in (1, 0):
                                                lib.psg_conv_set_pw(pw)
                                                for d in (d0, d1):
                                                    if lib.psg_conv_route(C.byref(d), o) != 0:
                                                        continue
                                                    for i in range(out[0]):
                                                        l = tuple(out[1 + i * K.NF: 1 + (i + 1) * K.NF])
                                                        seen.setdefault(K.route_key(dn, l), (c, cus, tile, tcls, pw, d is d1))
    finally:
        lib.psg_conv_set_tile(-1); lib.psg_conv_set_tapclass(1); lib.psg_conv_set_pw(1); lib.psg_set_available_cus(0)
    return seen


def test_table_reaches_what_the_sweep_reaches_and_nothing_else(lib):
    table, seen = _table_keys(), _sweep(lib)
    _report(f"sweep reached {len(seen)} route tuples, table holds {len(table)}")
    missing = {k: v for k, v in seen.items() if k not in table}
    fmt = lambda k, v: f"{k} e.g. B={v[0]['B']} {v[0]['H']}x{v[0]['W']} Cin={v[0]['Cin']} Cout={v[0]['Cout']} ks={v[0]['ks']} s={v[0]['stride']} " \
                       f"tr={v[0]['tr']} ldpre={v[0]['ldpre']} cus={v[1]} tile={v[2]} tapcls={v[3]} pw={v[4]} ws={v[5]}"
    assert not missing, "route tuples (dtype, BM, BN, mode, split, tapcls, pw, epi_lds) a legal launch takes but no case of the table:\n" + \
        "\n".join(fmt(k, v) for k, v in sorted(missing.items()))
    extra = {k: v for k, v in table.items() if k not in seen}
    assert not extra, f"route tuples in the table that the sweep cannot reach (a case's stored route is stale, or the sweep too narrow): {extra}"


def test_table_reaches_every_epilogue_form_and_shape_class():
    forms, pw_inst, parity, cls_forms = set(), set(), set(), set()
    for c in K.CASES:
        for l in K.expected_route(c["name"]):
            L = dict(zip(K.ROUTE_FIELDS, l))
            f = K.epi_form(c, l)
            forms.add(f)
            if L["pw"]:
                pw_inst.add((f, bool(c["residual"] or c["dact"]), bool(c["preact"])))
            if L["mode"] == 3:
                parity.add((L["sub_nH"] > 0, L["ntap"]))
            if L["tapcls"] and f.startswith("lds"):
                cls_forms.add((f.split(":")[2], L["BN"] == 160))
    want = {"split", "f32", "direct"} | {f"lds:{ek}:two_pass" for ek in ("PLAIN", "DROP", "GELU", "GELU_DROP", "DMUL", "GENERIC")} \
        | {f"lds:{ek}:stage_aux" for ek in ("PLAIN", "DROP", "DMUL")} | {f"lds:{ek}:stage_both" for ek in ("PLAIN", "DROP", "GELU", "GELU_DROP", "GENERIC")} \
        | {f"pw:{ek}" for ek in ("PLAIN", "DROP", "GELU", "GELU_DROP", "DMUL")}
    assert not want - forms, f"epilogue forms no case runs: {sorted(want - forms)}"
    # conv_pw.hip PSG_PW_FOR_ALL: (kind, aux, preact)
    inst = {("pw:PLAIN", False, False), ("pw:PLAIN", True, False), ("pw:DROP", False, False), ("pw:DROP", True, False), ("pw:GELU", False, False),
            ("pw:GELU", False, True), ("pw:GELU_DROP", False, False), ("pw:GELU_DROP", False, True), ("pw:DMUL", True, False)}
    assert pw_inst == inst, f"pointwise instantiations: missing {inst - pw_inst}, unexpected {pw_inst - inst}"
    assert {n for _, n in parity} == {1, 2, 4}
    assert cls_forms >= {("stage_aux", False), ("stage_both", False), ("two_pass", False), ("two_pass", True), ("stage_aux", True)}, cls_forms
    # every data gradient of a stride-2 3x3 conv on a 1-pixel grid has empty classes: fewer than four launches
    assert len(K.expected_route("g.bf16.3x3s2.dgrad.1x1")) == 1 and len(K.expected_route("g.bf16.3x3s2.dgrad.2x2")) == 4
    assert len(K.expected_route("g.bf16.3x3s2.dgrad.1x4")) == 2 and len(K.expected_route("g.bf16.3x3s2.dgrad.2x1")) == 2


def test_unpinned_cases_reach_every_tile_through_the_plan():
    """Each of the 8 (dtype, tile) pairs is chosen by the plan itself in some case that pins nothing - from the stored routes,
    which test_table_routes_are_the_librarys holds to the library: a planning change that strands a tile fails here."""
    got = {(c["dtype"], l[0], l[1]) for c in K.CASES if c["tile"] == -1 for l in K.expected_route(c["name"])}
    want = {(dn, BM, BN) for dn in ("bf16", "f32") for BM, BN in K.TILES if dn == "bf16" or BN != 160}
    assert got >= want, f"tiles no unpinned case reaches: {sorted(want - got)}"
    unsplit = {(c["dtype"], l[0], l[1]) for c in K.CASES if c["tile"] == -1 for l in K.expected_route(c["name"]) if l[3] == 1}
    assert unsplit >= want, f"tiles no unpinned, unsplit case reaches: {sorted(want - unsplit)}"


def test_relu_and_tanh_cases_exercise_the_activation():
    """ReLU must clamp and pass a sizeable share of every case's elements, tanh must stay off saturation, on every epilogue
    path that runs them; the ReLU-derivative elements that may take either side of the step (gemm_ref.saved_dact) stay rare."""
    paths = {"relu": set(), "tanh": set()}
    for c in K.CASES:
        if c["act"] not in paths:
            continue
        o = K.operands(c)
        ref = K.reference(c, o)
        u = torch.as_tensor(o["dact"]).double() if c["dact"] == "u" else ref["u"]
        n = u.numel()
        form = {K.epi_form(c, l).split(":")[0] for l in K.expected_route(c["name"])}
        if c["act"] == "relu":
            neg, pos = float((u < 0).double().mean()), float((u > 0).double().mean())
            if n >= 256:
                assert neg >= 0.1 and pos >= 0.1, f"{c['name']}: ReLU sees {neg:.3f} negative / {pos:.3f} positive pre-activations"
                paths["relu"] |= form
            if c["save_dact"]:
                amb = int((ref["preact"][2] >= 1.0).sum())
                assert amb <= max(2, n // 1000), f"{c['name']}: {amb} of {n} saved ReLU derivatives may take either side of the step"
        else:
            live = float((R.act_grad(u, "tanh") > 0.2).double().mean())
            if n >= 256:
                assert live >= 0.8, f"{c['name']}: tanh' > 0.2 on only {live:.3f} of the elements (saturated)"
                paths["tanh"] |= form
    for kind in paths:
        assert paths[kind] >= {"lds", "direct", "f32", "split"}, f"{kind}: epilogue paths with a case of >= 256 elements: {sorted(paths[kind])}"


def test_table_holds_the_raster_and_split_edges():
    """The places the issue names: grids and M-tile counts that are no multiples of 8 with two N tiles, class-order grids with
    mtiles & 7 != 0, a split whose last share is shorter and one whose kt0 lies inside a tap group, in modes 0, 1 and 2."""
    ragged, cls_ragged, short_last, mid_tap, split_modes = set(), False, set(), set(), set()
    for c in K.CASES:
        for l in K.expected_route(c["name"]):
            L = dict(zip(K.ROUTE_FIELDS, l))
            if L["grid"] % 8 and L["mtiles"] % 8 and L["ntiles"] >= 2 and not L["pw"] and L["splits"] == 1:
                ragged.add((c["dtype"], L["BM"], L["BN"]))
            if L["tapcls"] and L["mtiles"] % 8 and L["mtiles"] > 8:
                cls_ragged = True
            if L["splits"] > 1:
                split_modes.add(L["mode"])
                if L["KT"] % L["kt_per_split"]:
                    short_last.add(L["mode"])
                if L["mode"] in (0, 1) and L["kt_per_split"] % 9:
                    mid_tap.add(L["mode"])
    tiles = {(dn, BM, BN) for dn in ("bf16", "f32") for BM, BN in K.TILES if dn == "bf16" or BN != 160}
    assert ragged == tiles, tiles - ragged
    assert cls_ragged and split_modes == {0, 1, 2} and short_last == {0, 1, 2} and mid_tap == {0, 1}


# ------------------------------------------------------------------------------------------------------ (c) references
@pytest.mark.parametrize("ks,stride,pad,H,W", [(4, 2, 1, 6, 8), (4, 2, 2, 6, 8), (4, 2, 2, 5, 7), (3, 1, 1, 3, 5), (3, 2, 1, 5, 8), (1, 2, 0, 5, 7),
                                               (1, 2, 0, 4, 6), (3, 2, 1, 1, 4), (3, 1, 1, 1, 6), (3, 2, 1, 2, 1)])
def test_extended_conv_references_equal_autograd(ks, stride, pad, H, W):
    g = torch.Generator().manual_seed(ks * 100 + H * 10 + W)
    x = torch.randn(2, H, W, 5, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(7, 5, ks, ks, generator=g, dtype=torch.float64)
    y = F.conv2d(x.permute(0, 3, 1, 2), w, stride=stride, padding=pad).permute(0, 2, 3, 1)
    ref, S = R.conv_fwd(x, w, stride, pad)
    assert torch.allclose(ref, y.detach(), rtol=1e-12, atol=1e-12) and bool((S >= ref.abs() - 1e-12).all())
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    dx, Sd = R.conv_dgrad(gy, w, (H, W), stride, pad)
    assert torch.allclose(dx, x.grad, rtol=1e-12, atol=1e-12) and bool((Sd >= dx.abs() - 1e-12).all())


@pytest.mark.parametrize("kind", ["relu", "tanh", "silu", "gelu", "quick_gelu"])
def test_activation_references_equal_autograd(kind):
    u = torch.linspace(-6, 6, 4001, dtype=torch.float64, requires_grad=True)
    fn = {"relu": torch.relu, "tanh": torch.tanh, "silu": F.silu, "gelu": F.gelu, "quick_gelu": lambda t: t * torch.sigmoid(1.702 * t)}[kind]
    y = fn(u)
    y.sum().backward()
    assert torch.allclose(R.act(u.detach(), kind), y.detach(), rtol=1e-13, atol=1e-15)
    assert torch.allclose(R.act_grad(u.detach(), kind), u.grad, rtol=1e-12, atol=1e-15)
    # the constants: largest slope and curvature over the reals
    uu = torch.linspace(-8, 8, 160001, dtype=torch.float64)
    assert float(R.act_grad(uu, kind).abs().max()) <= R.ACT_SLOPE[kind] + 1e-4
    d = R.act_grad(uu, kind)
    curv = ((d[2:] - d[:-2]) / (uu[2:] - uu[:-2])).abs()
    if kind != "relu":
        assert float(curv.max()) <= R.ACT_CURV[kind] + 1e-3


def test_new_act_approx_entries_hold_for_the_fp32_formulas():
    """psg_common.h: ReLU is fmaxf(x, 0) and its derivative x > 0; tanh is tanhf(x) and its derivative 1 - t * t.  Evaluated in
    fp32 with torch against fp64: the value within ACT_APPROX (|y| + |u|) as epilogue() uses it, the derivative within
    (|u| + 1) ACT_APPROX as saved_dact() uses it, and within 4 ACT_APPROX relative + ACT_APPROX absolute as dact_u() does."""
    u32 = torch.cat([torch.linspace(-9, 9, 200001), torch.logspace(-6, 1, 20001), -torch.logspace(-6, 1, 20001)]).float()
    u = u32.double()
    assert torch.equal(torch.clamp(u32, min=0.0).double(), R.act(u, "relu")) and R.ACT_APPROX["relu"] == 0.0
    assert torch.equal((u32 > 0).double(), R.act_grad(u, "relu"))
    t32 = torch.tanh(u32)
    y = R.act(u, "tanh")
    worst_v = float(((t32.double() - y).abs() / (R.ACT_APPROX["tanh"] * (y.abs() + u.abs()) + R.A_FLOOR)).max())
    d32 = (1.0 - t32 * t32).double()
    d = R.act_grad(u, "tanh")
    worst_d = float(((d32 - d).abs() / ((u.abs() + 1.0) * R.ACT_APPROX["tanh"])).max())
    worst_r = float(((d32 - d).abs() / (4.0 * R.ACT_APPROX["tanh"] * d.abs() + R.ACT_APPROX["tanh"])).max())
    _report(f"act_approx tanh value {worst_v:.3f} derivative {worst_d:.3f} relative-form {worst_r:.3f} (fp32 torch vs fp64, ratio to the bound)")
    assert worst_v <= 0.5 and worst_d <= 0.5 and worst_r <= 0.5, (worst_v, worst_d, worst_r)
    # quick-GELU, psg_common.h quick_gelu_f / quick_gelu_grad / act_both: s = 1 / (1 + exp(-(1.702f x))), y = x s,
    # dy = s (1 + 1.702f x (1 - s)), every operation in fp32
    c32 = torch.tensor(1.702)
    s32 = 1.0 / (1.0 + torch.exp(-(c32 * u32)))
    y32, d32 = (u32 * s32).double(), (s32 * (1.0 + c32 * u32 * (1.0 - s32))).double()
    y, d, A = R.act(u, "quick_gelu"), R.act_grad(u, "quick_gelu"), R.ACT_APPROX["quick_gelu"]
    worst_v = float(((y32 - y).abs() / (A * (y.abs() + u.abs()) + R.A_FLOOR)).max())
    worst_d = float(((d32 - d).abs() / ((u.abs() + 1.0) * A)).max())
    worst_r = float(((d32 - d).abs() / (4.0 * A * d.abs() + A)).max())
    _report(f"act_approx quick_gelu value {worst_v:.3f} derivative {worst_d:.3f} relative-form {worst_r:.3f} (fp32 torch vs fp64, ratio to the bound)")
    assert worst_v <= 0.5 and worst_d <= 0.5 and worst_r <= 0.5, (worst_v, worst_d, worst_r)


def test_quick_gelu_cases_reach_every_epilogue_form():
    """The forms the quick-GELU cases run, from the stored routes: the staged bf16 epilogue, the direct one, fp32, the split-K
    finishing kernel, a parity-class launch and the CLIP MLP's whole-tile pointwise class; value alone, value + saved
    derivative, value under dropout, derivative of a saved pre-activation on each of staged / direct / fp32."""
    forms = {}
    for c in K.CASES:
        if c["act"] != "quick_gelu":
            continue
        assert c["recipe"] in K.QGELU_RECIPES
        for l in K.expected_route(c["name"]):
            f = K.epi_form(c, l).split(":")[0]
            forms.setdefault(f, set()).add(c["recipe"])
            if c["name"].startswith("g.bf16.3x3s2.dgrad"):
                assert dict(zip(K.ROUTE_FIELDS, l))["mode"] == 3
    assert set(forms) >= {"lds", "direct", "f32", "split"}, forms
    for f in ("lds", "direct", "f32"):
        assert forms[f] >= set(K.QGELU_RECIPES), (f, forms[f])
    assert {c["dtype"] for c in K.CASES if c["act"] == "quick_gelu" and K.expected_route(c["name"])[0][3] > 1} == {"bf16", "f32"}
    # the MLP's class: unsplit whole tiles, more workgroups than resident slots; quick-GELU has no per-kind copy, so the staged
    # epilogue is the generic one and the persistent pointwise kernel (which has none) must not take the launch
    c = K.BY_NAME["pw.qgelu.plan"]
    (l,) = K.expected_route(c["name"])
    L = dict(zip(K.ROUTE_FIELDS, l))
    assert L["splits"] == 1 and L["M"] % L["BM"] == 0 and c["Cout"] % L["BN"] == 0 and L["mtiles"] * L["ntiles"] > 16
    assert K.epi_form(c, l) == ("pw:GENERIC" if L["pw"] else "lds:GENERIC:two_pass")
    assert L["pw"] == 0, "the persistent pointwise kernel has no generic (quick-GELU) instantiation"


def _torch_f32(c, o):
    """torch's own fp32 result of a case's GEMM (no epilogue): conv2d / conv_transpose2d / linear of the same operands."""
    x = o["x"].permute(0, 3, 1, 2).contiguous()
    if c["ks"] == 1 and c["stride"] == 1:
        w2 = o["wl"].reshape(o["wl"].shape[0], o["wl"].shape[1])
        return F.linear(o["x"], w2.t().contiguous() if c["tr"] else w2)
    if c["tr"]:
        g = K.geom(c)
        oph = c["H"] - ((g["Hi"] - 1) * c["stride"] - 2 * c["pad"] + c["ks"])
        opw = c["W"] - ((g["Wi"] - 1) * c["stride"] - 2 * c["pad"] + c["ks"])
        y = F.conv_transpose2d(x, o["wl"], stride=c["stride"], padding=c["pad"], output_padding=(oph, opw))
    else:
        y = F.conv2d(x, o["wl"], stride=c["stride"], padding=c["pad"])
    return y.permute(0, 2, 3, 1)


def test_torch_fp32_gemm_of_every_fp32_case_is_within_the_bound():
    """check() and c_acc() were measured on the bf16 kernels.  For the fp32 launches: torch's fp32 conv2d / conv_transpose2d /
    linear of the same operands must lie within the same bound of the fp64 reference, or the bound would have to be widened
    for fp32 (by four times the factor torch needs).  The worst ratio goes into the report."""
    worst, at = 0.0, None
    for c in K.CASES:
        if c["dtype"] != "f32":
            continue
        o = K.operands(c)
        got = _torch_f32(c, o)
        if c["tr"]:
            ref, S = R.conv_dgrad(o["x"], o["wl"], (c["H"], c["W"]), c["stride"], c["pad"])
        else:
            ref, S = R.conv_fwd(o["x"], o["wl"], c["stride"], c["pad"])
        r = R.check(got.reshape(ref.shape), ref, S, torch.float32, c["name"] + " torch fp32", K.gemm_K(c))
        if r > worst:
            worst, at = r, c["name"]
    _report(f"torch_f32_vs_bound worst {worst:.4f} at {at}")
    # (torch's blocking differs from host to host: the figure is recorded, the requirement is the bound itself)
    assert worst <= 1.0, f"torch's fp32 result is outside check()'s bound ({worst:.4f} at {at}): the fp32 bound needs its own factor, 4 x {worst:.3f}"


def test_keep_mask_is_the_per_element_hash_of_the_y_row():
    seed, M, N, p = 0x0123456789ABCDEF, 37, 24, 0.5
    k = R.conv_keep_mask(seed, M, N, p).numpy()
    flat = keep_flat(seed, np.arange(M * N, dtype=np.uint64), p).reshape(M, N)
    assert (k == flat).all() and 0.4 < k.mean() < 0.6
    assert R.conv_keep_mask(seed, M, N, 0.05).float().mean() > 0.9


# -------------------------------------------------------------------------------------------- (d) emulation and defects
def _gather(c):
    """src [taps, M]: the input row each tap of each y row reads (-1: padding), and (b, ho, wo) of the rows."""
    g = K.geom(c)
    B, Hi, Wi, Ho, Wo, ks, s, p = c["B"], g["Hi"], g["Wi"], g["Ho"], g["Wo"], c["ks"], c["stride"], c["pad"]
    m = torch.arange(g["M"])
    b, ho, wo = m // (Ho * Wo), (m // Wo) % Ho, m % Wo
    src = torch.full((ks * ks, g["M"]), -1, dtype=torch.int64)
    pos = []
    for kh in range(ks):
        for kw in range(ks):
            if not c["tr"]:
                hi, wi = ho * s + kh - p, wo * s + kw - p
                ok = (hi >= 0) & (hi < Hi) & (wi >= 0) & (wi < Wi)
            else:
                th, tw = ho + p - kh, wo + p - kw
                hi, wi = th // s, tw // s
                ok = (th % s == 0) & (tw % s == 0) & (hi >= 0) & (hi < Hi) & (wi >= 0) & (wi < Wi)
            src[kh * ks + kw] = torch.where(ok, (b * Hi + hi) * Wi + wi, torch.full_like(m, -1))
            pos.append((hi, wi, ok))
    return src, (b, ho, wo), pos


def _tile_rows(c, launches):
    """GEMM row (the kernel's tile pixel index, launch by launch) of every y row: class order for a border-class launch,
    the parity grid's own row-major order for a parity-class launch, m itself otherwise."""
    g = K.geom(c)
    B, Ho, Wo = c["B"], g["Ho"], g["Wo"]
    m = torch.arange(g["M"])
    b, ho, wo = m // (Ho * Wo), (m // Wo) % Ho, m % Wo
    L = dict(zip(K.ROUTE_FIELDS, launches[0]))
    if L["tapcls"]:
        BM, rows, t0 = L["BM"], torch.zeros_like(m), 0
        hcs = [1, 0, 2, 1, 1, 0, 0, 2, 2]            # conv_gemm_kernel.h tapcls_hc / tapcls_wc: interior, top, bottom, left, right, corners
        wcs = [1, 1, 1, 0, 2, 0, 2, 0, 2]
        cls_of = lambda v, n: torch.where(v == 0, 0, torch.where(v == n - 1, 2, 1))
        for hc, wc in zip(hcs, wcs):
            nh, nw = (Ho - 2 if hc == 1 else 1), (Wo - 2 if wc == 1 else 1)
            h0, w0 = (0, 1, Ho - 1)[hc], (0, 1, Wo - 1)[wc]
            sel = (cls_of(ho, Ho) == hc) & (cls_of(wo, Wo) == wc)
            rows[sel] = (t0 * BM + (b * nh + (ho - h0)) * nw + (wo - w0))[sel]
            t0 += -(-(B * nh * nw) // BM)
        return rows
    if L["mode"] == 3:
        rows = torch.zeros_like(m)
        for l in launches:
            L = dict(zip(K.ROUTE_FIELDS, l))
            sel = (ho % 2 == L["sub_h0"]) & (wo % 2 == L["sub_w0"])
            rows[sel] = ((b * L["sub_nH"] + (ho - L["sub_h0"]) // 2) * L["sub_nW"] + (wo - L["sub_w0"]) // 2)[sel]
        return rows
    return m


def _ksteps(c, L):
    """The K steps of a launch in the kernel's order, each the list of (tap, channel range) pieces it covers."""
    step = 64 if c["dtype"] == "bf16" else 32
    taps, Cin = c["ks"] ** 2, c["Cin"]
    if L["mode"] in (0, 1):                          # taps innermost per channel slice
        return [[(t, c0, c0 + step)] for c0 in range(0, Cin, step) for t in range(taps)]
    steps = []                                       # mode 2: k = (tap, ci) flattened, a step may cross taps
    for k0 in range(0, taps * Cin, step):
        pieces, k = [], k0
        while k < min(k0 + step, taps * Cin):
            t, ci = divmod(k, Cin)
            e = min(Cin, ci + (k0 + step - k))
            pieces.append((t, ci, e))
            k += e - ci
        steps.append(pieces)
    return steps


def emulate(c, o, launches, defect=None):
    """A plain fp32 emulation of psg_conv_fwd on the operands o (fp32 matmul over the gathered taps, the epilogue in the order of
    conv_value, one rounding to the output dtype), into guarded NaN buffers as the GPU test allocates them - with one defect
    injected.  Returns (ybuf, prebuf) for conv_cases.verify."""
    g = K.geom(c)
    M, N, Cin, taps = g["M"], c["Cout"], c["Cin"], c["ks"] ** 2
    dt = K.DTYPES[c["dtype"]]
    L = dict(zip(K.ROUTE_FIELDS, launches[0]))
    src, (b, ho, wo), pos = _gather(c)
    x2 = o["x"].reshape(-1, Cin)
    if defect == "left_border_wrap":                 # the pad read left of column 0 lands on the previous row's last pixel
        for t in range(taps):
            hi, wi, ok = pos[t]
            wrap = (wi == -1) & (hi >= 0) & (hi < g["Hi"]) & ((b * g["Hi"] + hi) * g["Wi"] + wi >= 0)
            src[t] = torch.where(wrap, (b * g["Hi"] + hi) * g["Wi"] + wi, src[t])
    if defect == "parity_tap_off_by_one":            # one tap of a parity class reads the next gradient column
        t = 0
        hi, wi, ok = pos[t]
        src[t] = torch.where(ok & (wi + 1 < g["Wi"]), src[t] + 1, src[t])
    A = torch.zeros(M, taps, Cin)
    for t in range(taps):
        ok = src[t] >= 0
        A[ok, t] = x2[src[t][ok]]
    wl = o["wl"]
    Wt = (wl.permute(1, 2, 3, 0) if c["tr"] else wl.permute(0, 2, 3, 1)).reshape(N, taps, Cin).clone()      # [N, tap, c]
    if defect == "missing_tap_corner":               # the corner position (0, 0) of sample 0 loses one of its valid taps
        t = int((src[:, 0] >= 0).nonzero()[-1])
        A[0, t] = 0
    if defect == "drop_last_kstep":
        for t, c0, c1 in _ksteps(c, L)[-1]:
            A[:, t, c0:c1] = 0
    if defect == "last_split_missing":
        for pieces in _ksteps(c, L)[L["kt_per_split"] * (L["splits"] - 1):]:
            for t, c0, c1 in pieces:
                A[:, t, c0:c1] = 0
    acc = A.reshape(M, -1) @ Wt.reshape(N, -1).t()
    if defect == "zero_slice":                       # tile (0, 0) loses 16 channels of its first K step
        rows = (_tile_rows(c, launches) < L["BM"]).nonzero().flatten()
        t0 = int((src[:, rows[0]] >= 0).nonzero()[0])
        acc[rows[:, None], torch.arange(min(N, L["BN"]))[None, :]] -= A[rows, t0, 16:32] @ Wt[:min(N, L["BN"]), t0, 16:32].t()
    v = acc.clone()
    if o["bias"] is not None:
        v += o["bias"]
    if o["rowadd"] is not None:
        v += o["rowadd"][(b + 1) % c["B"] if defect == "rowadd_neighbour" else b]
    pre = v.clone()
    d = torch.ones_like(v)
    kind = {"act_as_gelu_erf": "gelu", "act_as_silu": "silu"}.get(defect, c["act"])     # another activation's code taken
    if c["dact"] == "mul":
        v = v * o["dact"]
    elif c["dact"] == "u":
        v = v * R.act_grad(o["dact"].double(), kind).float()
    elif c["act"] != "none":
        d = R.act_grad(v.double(), kind).float()
        if defect != "act_as_identity":               # (a ReLU that clamps nothing, a tanh that is not applied)
            v = R.act(v.double(), kind).float()
        if defect == "dact_constant_one":
            d = torch.ones_like(d)
    if defect == "preact_post_activation":
        pre = v.clone()
    if c["drop_p"] > 0:
        rows = torch.arange(M)
        if defect == "mask_by_tile_row":
            rows = _tile_rows(c, launches)
        idx = (rows.numpy().astype(np.uint64)[:, None] * np.uint64(N) + np.arange(N, dtype=np.uint64)[None, :])
        if defect == "pair_halves_swapped":
            idx = idx ^ np.uint64(1)
        keep = torch.from_numpy(keep_flat(K.drop_seed(c), idx, c["drop_p"])).float()
        sc = float(np.float32(1.0) / (np.float32(1.0) - np.float32(c["drop_p"])))
        v = v * keep * sc
        d = d * keep * (1.0 if defect == "save_dact_unscaled" else sc)
    if c["save_dact"]:
        pre = d
    v = v * c["alpha"]
    ybuf = K.alloc(M, g["ldy"], dt)
    if c["residual"]:
        res = o["residual"]
        if defect == "residual_with_ldy":            # the residual rows addressed with y's stride
            rb = torch.zeros(M * max(g["ldres"], g["ldy"]) + N)
            rb[:M * g["ldres"]].view(M, g["ldres"])[:, :N] = res
            res = torch.stack([rb[m * g["ldy"]: m * g["ldy"] + N] for m in range(M)])
        v = v + res
    ybuf[1][:, :N] = v.to(dt)
    if defect == "store_past_M":                     # one row too many
        n = min(N, K.GUARD)
        ybuf[0][K.GUARD + M * g["ldy"]: K.GUARD + M * g["ldy"] + n] = v[-1, :n].to(dt)
    prebuf = None
    if c["preact"]:
        prebuf = K.alloc(M, g["ldpre"], dt)
        prebuf[1][:, :N] = pre.to(dt)
    return ybuf, prebuf


# defect -> the cases that must reject it
DEFECTS = {
    "missing_tap_corner": ("g.bf16.3x3.3x3", "g.f32.3x3.3x5", "g.bf16.3x3.dgrad.2x2", "k.bf16.3x3.cin24", "cls.3x3.b37.fwd.t2"),
    "left_border_wrap": ("g.bf16.3x3.3x5", "g.f32.3x3.5x7", "k.bf16.3x3.cin8", "cls.3x5.b21.fwd.t0", "g.bf16.3x3s2.5x8"),
    "parity_tap_off_by_one": ("g.bf16.3x3s2.dgrad.7x7", "g.bf16.3x3s2.dgrad.5x8", "g.f32.3x3s2.dgrad.7x7"),
    "drop_last_kstep": ("tile.bf16.128x128.m128.n12", "tile.f32.64x64.m64.n12", "tile.bf16.64x160.m65.n156", "k.bf16.3x3.cin40", "k.f32.3x3.cin20",
                        "g.bf16.3x3.5x7"),
    "zero_slice": ("tile.bf16.128x64.mt9", "tile.f32.128x128.mt17", "g.bf16.3x3.14x14", "cls.7x7.b37.fwd.t0", "pw.plain.on"),
    "mask_by_tile_row": ("cls.7x7.b37.fwd.t2", "cls.3x5.b21.dgrad.t0", "cls.3x3.b37.fwd.t3", "g.bf16.3x3s2.dgrad.7x7", "ld.mode3.all"),
    "pair_halves_swapped": ("epi.staged.drop", "epi.direct.drop", "epi.f32.drop", "pw.drop.on", "split.bf16.drop", "epi.staged.gelu_drop_save"),
    "rowadd_neighbour": ("split.bf16.all", "split.f32.all", "epi.staged.rowadd", "g.bf16.3x3s2.7x7", "tile.bf16.128x128.m128.n12", "g.bf16.3x3s2.dgrad.14x14"),
    "residual_with_ldy": ("ld.staged.all", "ld.f32.all", "ld.mode3.all", "pw.res_ld.on"),
    "preact_post_activation": ("epi.staged.gelu_pre", "epi.direct.gelu_pre", "epi.f32.all", "pw.gelu_pre.on", "split.bf16.gelu_pre"),
    "save_dact_unscaled": ("epi.staged.gelu_drop_save", "epi.staged.p50", "pw.gelu_drop_save.on", "split.bf16.gelu_drop_save"),
    "last_split_missing": ("split.bf16.res", "split.bf16.rowadd", "split.bf16.mode2", "split.f32.mode2", "split.bf16.gelu_pre"),
    "act_as_identity": ("epi.staged.relu_save", "epi.direct.relu_save", "epi.f32.relu_save", "split.bf16.relu_save", "split.f32.relu_save",
                        "epi.staged.tanh", "epi.direct.tanh", "epi.f32.tanh", "split.bf16.tanh", "split.bf16.128x128.mode2"),
    "dact_constant_one": ("epi.staged.relu_save", "epi.direct.relu_save", "epi.f32.relu_save", "split.bf16.relu_save", "split.f32.relu_save",
                          "epi.staged.gelu_drop_save", "split.bf16.silu_save_res"),
    "act_as_gelu_erf": tuple(c["name"] for c in K.CASES if c["act"] == "quick_gelu"),
    "act_as_silu": tuple(c["name"] for c in K.CASES if c["act"] == "quick_gelu"),
    "store_past_M": ("tile.bf16.64x64.m63.n8", "tile.f32.128x64.m259.n64", "epi.staged.plain", "ld.staged.all"),
}


def _clean_and_ref(name, cache={}):
    if name not in cache:
        c = K.BY_NAME[name]
        o = K.operands(c)
        cache[name] = (c, o, K.expected_route(name), K.reference(c, o))
    return cache[name]


ACCEPT = sorted({n for v in DEFECTS.values() for n in v} | {c["name"] for i, c in enumerate(K.CASES) if i % 4 == 0 and K.geom(c)["M"] <= 1200})


@pytest.mark.parametrize("name", ACCEPT)
def test_comparator_accepts_the_plain_emulation(name):
    c, o, launches, ref = _clean_and_ref(name)
    ybuf, prebuf = emulate(c, o, launches)
    worst = K.verify(c, launches, ref, ybuf, prebuf)
    assert all(0.0 <= w <= 1.0 for w in worst.values())


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_comparator_rejects_injected_defect(defect):
    for name in DEFECTS[defect]:
        c, o, launches, ref = _clean_and_ref(name)
        clean = emulate(c, o, launches)
        K.verify(c, launches, ref, *clean)
        bad = emulate(c, o, launches, defect)
        same = torch.equal(torch.nan_to_num(bad[0][0].float(), nan=-7.0), torch.nan_to_num(clean[0][0].float(), nan=-7.0)) and \
            (bad[1] is None or torch.equal(torch.nan_to_num(bad[1][0].float(), nan=-7.0), torch.nan_to_num(clean[1][0].float(), nan=-7.0)))
        assert not same, f"{defect} changes nothing at {name}: the case does not exercise it"
        with pytest.raises(AssertionError):
            K.verify(c, launches, ref, *bad)
        _report(f"defect {defect} rejected at {name}")
