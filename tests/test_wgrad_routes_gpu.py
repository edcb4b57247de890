"""-m gpu: every row of the weight-gradient variant table (csrc/wgrad.hip) through the C ABI (psg_conv_wgrad), at the smallest
shapes that still have a tail in every direction (tests/wgrad_cases.py SMALL), each in its finishing configurations: tiles
straight into dw, the sum kernel with the folded bias, the reduce kernel plus the bias-sum kernel, and accumulation into a
pre-filled dw / dbias.

Per case: the route is asserted before the launch (family, geometry, split count, finishing kernels); x is a slice of a wider
NaN-filled buffer, dw, dbias and the workspace sit inside NaN guards; every element of dw and dbias is within gemm_ref.check's
bound of the fp64 reference; nothing is written outside the results or behind the workspace the plan reports; and a second
identical launch gives identical bits.  A device error ends the run."""
import ctypes

import pytest
import torch

from tests import gemm_ref as R
from tests import wgrad_cases as W
from tests.conv_cases import GUARD, NAN, alloc
from tests.util import h

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
IDS = [f"{c['name']}.{dn}" if len(c["dtypes"]) > 1 else c["name"] for c in W.SMALL for dn in c["dtypes"]]
PARAMS = [(c, dn) for c in W.SMALL for dn in c["dtypes"]]


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    lib = _lib.init(0)
    yield lib
    lib.psg_conv_wgrad_set_variant(-1); lib.psg_conv_wgrad_set_splits(0); lib.psg_set_available_cus(0); lib.psg_set_reserve_rounds(0)


def _guarded(n, fill_values=None):
    """n fp32 values inside NaN guards: (flat, view)."""
    flat = torch.full((n + 2 * GUARD,), NAN, dtype=torch.float32, device=DEV)
    view = flat[GUARD:GUARD + n]
    if fill_values is not None:
        view.copy_(fill_values.reshape(-1).to(DEV))
    return flat, view


@pytest.mark.parametrize("c,dn", PARAMS, ids=IDS)
def test_wgrad_route(lib, c, dn):
    from pokemon_sprite_generator_amd import _lib
    g = W.geom(c)
    dt = DTYPES[dn]
    name = c["name"]
    B, H, Cin, Cout, ks, M, Q = c["B"], c["H"], c["Cin"], c["Cout"], c["ks"], g["M"], g["Q"]
    x = (0.3 + 0.8 * h((B, H, c["W"], Cin), name + ".x")).to(dt).float()
    dy = (0.2 + h((B, g["Ho"], g["Wo"], Cout), name + ".dy")).to(dt).float()
    dw0 = 0.5 * h((Cout * Q,), name + ".dw0") if c["acc"] else None
    db0 = 0.5 * h((Cout,), name + ".db0") if c["acc"] and c["dbias"] else None

    ref, S = R.linear_wgrad(x, dy) if ks == 1 else R.conv_wgrad(x, dy, ks, c["stride"])
    ref, S = ref.reshape(Cout, Cin, ks, ks), S.reshape(Cout, Cin, ks, ks)
    bref, bS = R.bias_grad(dy)

    xb = alloc(B * H * c["W"], g["ldx"], dt, DEV)
    xb[1][:, :Cin] = x.reshape(-1, Cin).to(DEV, dt)
    yb = alloc(M, g["lddy"], dt, DEV)
    yb[1][:, :Cout] = dy.reshape(-1, Cout).to(DEV, dt)

    with W.settings(lib, c):
        probe = W.make_desc(c, dn)
        rc, route = W.route_of(lib, probe)
        assert rc == 0, f"{name}: {lib.psg_last_error()}"
        L = dict(zip(W.ROUTE_FIELDS, route))
        kind = name.rsplit(".", 1)[1]
        want = {"direct": ("direct", "direct"), "sum": ("sum", "folded"), "reduce": ("reduce", "bias_sum"), "acc": ("sum", "folded")}[kind]
        geom = 0 if c["stride"] != 1 else (2 if ks == 1 else 1)
        assert (L["family"], L["dtype"], L["geom"], L["bias"], L["splits"]) == (c["family"], W.DTYPE_CODE[dn], geom, int(c["dbias"]), c["splits"]), f"{name}: {L}"
        assert (W.FINISH[L["finish"]], W.BIAS_FINISH[L["bias_finish"]]) == (want[0], want[1] if c["dbias"] else "none"), f"{name}: {L}"
        need = int(lib.psg_conv_wgrad_workspace_bytes(ctypes.byref(probe)))
        assert need == W.implied_ws_bytes(c, route) and need % 4 == 0

        outs = []
        for rep in range(2):
            dwb = _guarded(Cout * Q, dw0)
            dbb = _guarded(Cout, db0) if c["dbias"] else None
            wsb = torch.full((need // 4 + GUARD,), NAN, dtype=torch.float32, device=DEV)
            ptrs = dict(x=xb[1].data_ptr(), dy=yb[1].data_ptr(), dw=dwb[1].data_ptr(), dbias=dbb[1].data_ptr() if dbb else 0)
            d = W.make_desc(c, dn, ptrs, wsb.data_ptr() if need else 0, need)
            assert W.route_of(lib, d) == (0, route)
            _lib.check(lib.psg_conv_wgrad(ctypes.byref(d), _lib.stream_ptr()), "psg_conv_wgrad " + name)
            try:
                torch.cuda.synchronize()
            except RuntimeError as e:                           # a device error: nothing more runs on this GPU
                pytest.exit(f"{name}: {e}", returncode=3)
            assert not bool(torch.isnan(wsb[:need // 4]).any()), f"{name}: partials missing in the workspace"
            assert bool(torch.isnan(wsb[need // 4:]).all()), f"{name}: a store behind the workspace the plan reports"
            outs.append((dwb, dbb))

    tag = f"{name} [{dn} {W.FAMILIES[L['family']]} geom {L['geom']} tiles {L['rtiles']}x{L['qtiles']} splits {L['splits']} x {L['steps_per_split']}]"
    (dwb, dbb), (dwb2, dbb2) = outs
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
    R.check(got, ref, S, torch.float32, tag + " dw", M)
    if dbb:
        if c["acc"]:
            bref, bS = bref + db0.double(), bS + db0.double().abs()
        R.check(dbb[1].cpu(), bref, bS, torch.float32, tag + " dbias", M)
    assert torch.equal(dwb[0].view(torch.int32), dwb2[0].view(torch.int32)), f"{tag}: dw differs between two identical launches"
    if dbb:
        assert torch.equal(dbb[0].view(torch.int32), dbb2[0].view(torch.int32)), f"{tag}: dbias differs between two identical launches"
