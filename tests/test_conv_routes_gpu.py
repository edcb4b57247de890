"""-m gpu: every conv forward / data-gradient route and kernel variant, through the C ABI (psg_prep_weight, psg_conv_fwd), element
by element against the fp64 reference and bound of tests/gemm_ref.py on the cases of tests/conv_cases.py.

Per case: the route is the one the table stores (psg_conv_route, asserted before the launch) and the launch counters
(persistent pointwise, border-class order) and the split-K workspace agree with it afterwards; y and preact, pre-filled with
NaN inside guard regions and with NaN in the unwritten columns of strided rows, hold no NaN inside and only NaN outside;
every element is within gemm_ref.check's bound of the fp64 reference of the operands the kernel read (the unread columns of
strided inputs and of the wider prepared weight hold NaN, so a read outside the operand shows too); preact and the saved
derivative are held to their own fp64 values; the dropout zero pattern equals the integer restatement of tests/drop_ref.py
exactly; and a second identical launch gives identical bits.  Every shape is legal per conv_setup; a workspace that is too
small is a supported path."""
import ctypes
import json
import os
import time

import pytest
import torch

from tests import conv_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPORT = os.environ.get("PSG_CONV_REPORT")     # optional: append each case's worst err / bound (JSON lines) to this file
_T = {"t0": None, "n": 0, "slowest": ("", 0.0)}


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    lib = _lib.init(0)
    _T["t0"] = time.perf_counter()
    yield lib
    lib.psg_conv_set_tile(-1); lib.psg_conv_set_tapclass(1); lib.psg_conv_set_pw(1); lib.psg_set_available_cus(0); lib.psg_set_reserve_rounds(0)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(json.dumps({"wall_s": time.perf_counter() - _T["t0"], "tests": _T["n"], "slowest": _T["slowest"][0],
                                "slowest_s": _T["slowest"][1]}) + "\n")


def _rows(values, ld, dtype, fill=K.NAN):
    """[rows, C] values inside a guarded [rows, ld] buffer on the device; everything else `fill`."""
    flat, view = K.alloc(values.shape[0], ld, dtype, DEV, fill)
    view[:, :values.shape[1]] = values.to(DEV, dtype)
    return flat, view


def _prep_weight(lib, c, o, g):
    """The prepared weight the launch reads: psg_prep_weight's [N][Kpad] (forward operand, or the data-gradient operand of the
    logical conv weight), placed at column woff of a NaN-filled [N][ldw] buffer."""
    from pokemon_sprite_generator_amd import _lib
    dt, code = K.DTYPES[c["dtype"]], K.DTYPE_CODE[c["dtype"]]
    wl = o["wl"].to(DEV).contiguous()
    O, I = wl.shape[0], wl.shape[1]
    layout = 0                                                  # PSG_W_OIHW
    if c["ks"] == 4:                                            # (4x4 master weights are accepted in OHWI order only)
        wl, layout = wl.permute(0, 2, 3, 1).contiguous(), 1
    N, Kpad = c["Cout"], g["Kpad"]
    assert int(lib.psg_kpad(g["K"], code)) == Kpad
    dense = torch.full((N, Kpad), K.NAN, dtype=dt, device=DEV)
    wf, wd = (None, dense) if c["tr"] else (dense, None)
    _lib.check(lib.psg_prep_weight(_lib.ptr(wl), _lib.PSG_F32, layout, _lib.ptr(wf), _lib.ptr(wd), O, I, c["ks"], code, _lib.stream_ptr()), "psg_prep_weight")
    flat, view = K.alloc(N, g["ldw"], dt, DEV)
    view[:, c["woff"]:c["woff"] + Kpad] = dense
    return flat, view[:, c["woff"]:]


@pytest.mark.parametrize("name", K.case_ids())
def test_conv_route(lib, name):
    from pokemon_sprite_generator_amd import _lib
    t_start = time.perf_counter()
    c = K.BY_NAME[name]
    g = K.geom(c)
    dt = K.DTYPES[c["dtype"]]
    M, N = g["M"], c["Cout"]
    o = K.operands(c)
    ref = K.reference(c, o)
    want = K.expected_route(name)

    keep = []                                                   # buffers stay alive until the launches are done
    xb = _rows(o["x"].reshape(-1, c["Cin"]), g["ldx"], dt); keep.append(xb)
    wb, wview = _prep_weight(lib, c, o, g); keep.append(wb)
    ptrs = dict(x=xb[1].data_ptr(), w=wview.data_ptr(), bias=0, rowadd=0, residual=0, preact=0, dact_u=0)
    if c["bias"]:
        bias = o["bias"].to(DEV, torch.float32).contiguous(); keep.append(bias)
        ptrs["bias"] = bias.data_ptr()
    if c["rowadd"]:
        ra = o["rowadd"].to(DEV, dt).contiguous(); keep.append(ra)
        ptrs["rowadd"] = ra.data_ptr()
    if c["dact"] is not None:
        db = _rows(o["dact"], g["lddact"], dt); keep.append(db)
        ptrs["dact_u"] = db[1].data_ptr()
    resb = None
    if c["residual"] and not c["alias"]:
        resb = _rows(o["residual"], g["ldres"], dt); keep.append(resb)
        ptrs["residual"] = resb[1].data_ptr()

    def fresh_outputs():
        yb = K.alloc(M, g["ldy"], dt, DEV)
        if c["alias"]:                                          # the residual IS y: the launch reads it before it writes
            yb[1][:, :N] = o["residual"].to(DEV, dt)
        pb = K.alloc(M, g["ldpre"], dt, DEV) if c["preact"] else None
        return yb, pb

    with K.settings(lib, c):
        ws_ptr, ws_bytes, wsb = 0, 0, None
        if c["ws"] != "none":
            _, ws_bytes = K.ws_for(lib, c, dict(ptrs, y=0x10000, preact=0x20000), 0x900000)
            wsb = torch.full((ws_bytes // 4 + K.GUARD,), K.NAN, dtype=torch.float32, device=DEV)
            ws_ptr = wsb.data_ptr()
        outs = []
        for rep in range(2):
            yb, pb = fresh_outputs()
            p = dict(ptrs, y=yb[1].data_ptr(), preact=pb[1].data_ptr() if pb else 0)
            if c["alias"]:
                p["residual"] = p["y"]
            d = K.make_desc(c, p, ws_ptr, ws_bytes)
            rc, got = K.route_of(lib, d)
            assert rc == 0 and got == want, f"{name}: route {got}, table {want}"
            pw0, tc0 = int(lib.psg_conv_pw_launches()), int(lib.psg_conv_tapclass_launches())
            _lib.check(lib.psg_conv_fwd(ctypes.byref(d), _lib.stream_ptr()), "psg_conv_fwd " + name)     # (a refusal fails this test only)
            try:
                torch.cuda.synchronize()
            except RuntimeError as e:                           # a device error: nothing more runs on this GPU
                pytest.exit(f"{name}: {e}", returncode=3)
            assert int(lib.psg_conv_pw_launches()) - pw0 == sum(l[6] for l in want), f"{name}: persistent pointwise launches"
            assert int(lib.psg_conv_tapclass_launches()) - tc0 == sum(l[5] for l in want), f"{name}: border-class launches"
            outs.append((yb, pb))
        if wsb is not None:
            L = dict(zip(K.ROUTE_FIELDS, want[0]))
            used = L["splits"] * M * N if L["splits"] > 1 else 0
            assert used * 4 <= ws_bytes
            assert not bool(torch.isnan(wsb[:used]).any()), f"{name}: split-K partials missing in the workspace"
            assert bool(torch.isnan(wsb[used:]).all()), f"{name}: a store behind the split-K partials (splits {L['splits']})"

    (yb, pb), (yb2, pb2) = outs
    worst = K.verify(c, want, ref, yb, pb)
    bits = lambda t: t.view(torch.int16 if t.element_size() == 2 else torch.int32)
    assert torch.equal(bits(yb[0]), bits(yb2[0])), f"{name}: y differs between two identical launches"
    if pb:
        assert torch.equal(bits(pb[0]), bits(pb2[0])), f"{name}: preact differs between two identical launches"
    secs = time.perf_counter() - t_start
    _T["n"] += 1
    if secs > _T["slowest"][1]:
        _T["slowest"] = (name, secs)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(json.dumps({"case": name, "keys": [list(K.route_key(c["dtype"], l)) for l in want],
                                "forms": [K.epi_form(c, l) for l in want], "ratios": worst, "s": round(secs, 3)}) + "\n")
