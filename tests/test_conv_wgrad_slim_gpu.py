"""-m gpu: psg_conv_wgrad_slim (csrc/conv_wgrad_slim.hip) through the C ABI, element-wise against the fp64 weight gradient of
the bf16-rounded operands, under the bound tests/test_wgrad_routes_gpu.py applies to bf16 operands with fp32 accumulation
(tests/gemm_ref.check, K = M).  Shapes: tests/wgrad_slim_cases.py - every Cout / Cin / kernel-size corner on a 5 x 7 grid with
batch 3 and wide rows, two cases whose images span several tiles, slab pins 1 and 3 with accumulate and dbias on and off in
both dw layouts, and one 2 x 215 x 215 launch on the plan's own slab count.

Per launch: x and dy are slices of NaN-filled buffers, dw, dbias and the workspace sit inside NaN guards; nothing is written
outside the results or behind the workspace the query reports; a second identical launch gives identical bits.  Contract
violations return their codes and leave dw untouched.  A device error ends the run."""
import ctypes

import pytest
import torch

from tests import gemm_ref as R
from tests import wgrad_cases as W
from tests import wgrad_slim_cases as SC
from tests.conv_cases import GUARD, NAN, alloc
from tests.util import h

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    lib = _lib.init(0)
    yield lib
    lib.psg_conv_wgrad_slim_set_splits(0)


def _guarded(n, fill_values=None):
    flat = torch.full((n + 2 * GUARD,), NAN, dtype=torch.float32, device=DEV)
    view = flat[GUARD:GUARD + n]
    if fill_values is not None:
        view.copy_(fill_values.reshape(-1).to(DEV))
    return flat, view


def _operands(c):
    """(x, dy) bf16-exact fp32 on the CPU, their guarded device buffers, and the fp64 references."""
    g = W.geom(c)
    name = c["name"]
    x = (0.3 + 0.8 * h((c["B"], c["H"], c["W"], c["Cin"]), name + ".x")).to(BF16).float()
    dy = (0.2 + h((c["B"], g["Ho"], g["Wo"], c["Cout"]), name + ".dy")).to(BF16).float()
    xb = alloc(c["B"] * c["H"] * c["W"], g["ldx"], BF16, DEV)
    xb[1][:, :c["Cin"]] = x.reshape(-1, c["Cin"]).to(DEV, BF16)
    yb = alloc(g["M"], g["lddy"], BF16, DEV)
    yb[1][:, :c["Cout"]] = dy.reshape(-1, c["Cout"]).to(DEV, BF16)
    dev = DEV if g["M"] > 4096 else "cpu"
    ref, S = R.linear_wgrad(x.to(dev), dy.to(dev)) if c["ks"] == 1 else R.conv_wgrad(x.to(dev), dy.to(dev), c["ks"], 1)
    shape = (c["Cout"], c["Cin"], c["ks"], c["ks"])
    bref, bS = R.bias_grad(dy)
    return xb, yb, ref.reshape(shape).cpu(), S.reshape(shape).cpu(), bref, bS


def _launch(lib, c, xb, yb, dw0, db0):
    """One guarded launch: ((dw flat, dw view), (dbias flat, view) or None)."""
    from pokemon_sprite_generator_amd import _lib
    g = W.geom(c)
    probe = W.make_desc(c, "bf16")
    need = int(lib.psg_conv_wgrad_slim_workspace_bytes(ctypes.byref(probe)))
    assert need > 0 and need % 4 == 0, lib.psg_last_error()
    dwb = _guarded(c["Cout"] * g["Q"], dw0)
    dbb = _guarded(c["Cout"], db0) if c["dbias"] else None
    wsb = torch.full((need // 4 + GUARD,), NAN, dtype=torch.float32, device=DEV)
    ptrs = dict(x=xb[1].data_ptr(), dy=yb[1].data_ptr(), dw=dwb[1].data_ptr(), dbias=dbb[1].data_ptr() if dbb else 0)
    d = W.make_desc(c, "bf16", ptrs, wsb.data_ptr(), need)
    _lib.check(lib.psg_conv_wgrad_slim(ctypes.byref(d), _lib.stream_ptr()), "psg_conv_wgrad_slim " + c["name"])
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                           # a device error: nothing more runs on this GPU
        pytest.exit(f"{c['name']}: {e}", returncode=3)
    used = need // 4 if c["dbias"] else need // 4 - (need // 4) // (c["Cout"] * g["Q"] + c["Cout"]) * c["Cout"]
    assert not bool(torch.isnan(wsb[:used]).any()), f"{c['name']}: partials missing in the workspace"
    assert bool(torch.isnan(wsb[need // 4:]).all()), f"{c['name']}: a store behind the workspace the query reports"
    return dwb, dbb


def _verify(c, tag, dwb, dbb, ref, S, bref, bS, dw0, db0):
    g = W.geom(c)
    Cout, Cin, ks = c["Cout"], c["Cin"], c["ks"]
    for what, (flat, view) in (("dw", dwb), ("dbias", dbb)) if dbb else (("dw", dwb),):
        f = flat.cpu()
        assert bool(torch.isnan(f[:GUARD]).all()) and bool(torch.isnan(f[-GUARD:]).all()), f"{tag} {what}: a store outside the result (guard)"
        assert not bool(torch.isnan(view).any()), f"{tag} {what}: elements never stored (or NaN)"
    got = dwb[1].cpu()
    got = got.view(Cout, ks, ks, Cin).permute(0, 3, 1, 2) if c["layout"] == "ohwi" else got.view(Cout, Cin, ks, ks)
    if c["acc"]:
        a = dw0.double()
        a = a.view(Cout, ks, ks, Cin).permute(0, 3, 1, 2) if c["layout"] == "ohwi" else a.view(Cout, Cin, ks, ks)
        ref, S = ref + a, S + a.abs()
    worst = R.check(got, ref, S, torch.float32, tag + " dw", g["M"])
    if dbb:
        if c["acc"]:
            bref, bS = bref + db0.double(), bS + db0.double().abs()
        worst = max(worst, R.check(dbb[1].cpu(), bref, bS, torch.float32, tag + " dbias", g["M"]))
    return worst


@pytest.mark.parametrize("base", SC.SMALL, ids=[c["name"] for c in SC.SMALL])
def test_small_shapes_every_configuration(lib, base):
    xb, yb, ref, S, bref, bS = _operands(base)
    g = W.geom(base)
    worst = 0.0
    try:
        for i, (splits, acc, dbias, layout) in enumerate(SC.CONFIGS):
            c = dict(base, acc=acc, dbias=dbias, layout=layout)
            assert lib.psg_conv_wgrad_slim_set_splits(splits) == 0
            slabs = min(splits, SC.ntiles(c))
            slabs = -(-SC.ntiles(c) // -(-SC.ntiles(c) // slabs))
            probe = W.make_desc(c, "bf16")
            assert lib.psg_conv_wgrad_slim_workspace_bytes(ctypes.byref(probe)) == slabs * (c["Cout"] * g["Q"] + c["Cout"]) * 4
            dw0 = 0.5 * h((c["Cout"] * g["Q"],), c["name"] + ".dw0") if acc else None
            db0 = 0.5 * h((c["Cout"],), c["name"] + ".db0") if acc and dbias else None
            tag = f"{c['name']} [slabs {slabs} acc {int(acc)} dbias {int(dbias)} {layout}]"
            dwb, dbb = _launch(lib, c, xb, yb, dw0, db0)
            worst = max(worst, _verify(c, tag, dwb, dbb, ref, S, bref, bS, dw0, db0))
            if i % 4 == 2:                               # accumulate + dbias: the second launch must give the same bits
                dwb2, dbb2 = _launch(lib, c, xb, yb, dw0, db0)
                assert torch.equal(dwb[0].view(torch.int32), dwb2[0].view(torch.int32)), f"{tag}: dw differs between two identical launches"
                assert torch.equal(dbb[0].view(torch.int32), dbb2[0].view(torch.int32)), f"{tag}: dbias differs between two identical launches"
    finally:
        lib.psg_conv_wgrad_slim_set_splits(0)
    print(f"{base['name']}: worst err / bound {worst:.3f}")


def test_large_m_on_the_plans_own_slab_count(lib):
    c = SC.LARGE
    g = W.geom(c)
    assert g["M"] > 1 << 16
    lib.psg_conv_wgrad_slim_set_splits(0)
    probe = W.make_desc(c, "bf16")
    need = int(lib.psg_conv_wgrad_slim_workspace_bytes(ctypes.byref(probe)))
    slabs = need // ((c["Cout"] * g["Q"] + c["Cout"]) * 4)
    assert 256 < slabs <= SC.ntiles(c), slabs              # follows M and the CUs: beyond psg_conv_wgrad's cap of 256
    xb, yb, ref, S, bref, bS = _operands(c)
    tag = f"{c['name']} [slabs {slabs}]"
    dwb, dbb = _launch(lib, c, xb, yb, None, None)
    worst = _verify(c, tag, dwb, dbb, ref, S, bref, bS, None, None)
    dwb2, dbb2 = _launch(lib, c, xb, yb, None, None)
    assert torch.equal(dwb[0].view(torch.int32), dwb2[0].view(torch.int32)) and torch.equal(dbb[0].view(torch.int32), dbb2[0].view(torch.int32))
    print(f"{tag}: worst err / bound {worst:.3f}")


def test_contract_violations_launch_nothing(lib):
    from pokemon_sprite_generator_amd._lib import ERR_ALIGN, ERR_DTYPE, ERR_SHAPE
    base = SC.mk("v", B=1, H=5, W=7, Cin=32, Cout=32, ks=3, dbias=True)
    g = W.geom(base)
    xb, yb = alloc(35, 160, BF16, DEV, fill=1.0), alloc(35, 160, BF16, DEV, fill=1.0)      # wide enough for every variation below
    dwb, dbb = _guarded(96 * 9 * 136), _guarded(96)
    ws = torch.full((1 << 20,), NAN, dtype=torch.float32, device=DEV)
    ptrs = dict(x=xb[1].data_ptr(), dy=yb[1].data_ptr(), dw=dwb[1].data_ptr(), dbias=dbb[1].data_ptr())

    def run(c, dn="bf16", **over):
        d = W.make_desc(c, dn, dict(ptrs, **over), ws.data_ptr(), ws.numel() * 4)
        return lib.psg_conv_wgrad_slim(ctypes.byref(d), None)

    assert run(base, "f32") == ERR_DTYPE and b"bf16 only" in lib.psg_last_error()
    assert run(dict(base, stride=2)) == ERR_SHAPE and b"stride" in lib.psg_last_error()
    assert run(dict(base, Cout=96)) == ERR_SHAPE and b"Cout=96" in lib.psg_last_error()
    assert run(dict(base, Cin=136)) == ERR_SHAPE and b"Cin=136" in lib.psg_last_error()
    assert run(base, x=ptrs["x"] + 2) == ERR_ALIGN and run(base, dy=ptrs["dy"] + 8) == ERR_ALIGN
    torch.cuda.synchronize()
    assert bool(torch.isnan(dwb[0]).all()) and bool(torch.isnan(dbb[0]).all()) and bool(torch.isnan(ws).all())
    assert run(base) == 0                                   # the same descriptor inside the contract does launch
    torch.cuda.synchronize()
    assert not bool(torch.isnan(dwb[1][:32 * g["Q"]]).any()) and not bool(torch.isnan(dbb[1][:32]).any())
