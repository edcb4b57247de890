"""Host-side proofs of the weight-gradient plan (no GPU: psg_conv_wgrad_route plans on the host).  The routes of
tests/wgrad_cases.py are those of tests/golden/wgrad_routes.json - written down from the planner as it stood when the export
was added, never regenerated; the workspace is what the reported plan implies; the table reaches every row of the variant
table and every finishing kind; pins that cannot run are errors; the PSG_WGRAD_* environment still means what it meant."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

from tests import wgrad_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_routes_are_the_stored_ones_and_size_the_workspace(lib):
    n = 0
    for c in W.CASES:
        for dn in ("bf16", "f32"):
            for cus in W.CUS:
                rc, r = W.query_route(lib, c, dn, cus)
                assert rc == 0, f"{c['name']} {dn} {cus}: psg_conv_wgrad_route returned {rc}: {lib.psg_last_error()}"
                assert r == W.expected(W.key(c, dn, cus)), f"{c['name']} {dn} {cus} CUs: " + ", ".join(
                    f"{f} {a} (stored {b})" for f, a, b in zip(W.ROUTE_FIELDS, r, W.expected(W.key(c, dn, cus))) if a != b)
                with W.settings(lib, c, cus):
                    need = lib.psg_conv_wgrad_workspace_bytes(C.byref(W.make_desc(c, dn)))
                assert need == W.implied_ws_bytes(c, r), f"{c['name']} {dn} {cus}: workspace {need} vs the plan's {W.implied_ws_bytes(c, r)}"
                L = dict(zip(W.ROUTE_FIELDS, r))
                assert L["grid"] == L["rtiles"] * L["qtiles"] * L["splits"]
                assert L["launches"] == 1 + (L["finish"] != 0) + (L["bias_finish"] == 3)
                n += 1
    assert n == 4 * len(W.CASES)


def test_table_reaches_every_variant_and_finish():
    rows, fin, bfin = set(), set(), set()
    for c in W.CASES:
        for dn in ("bf16", "f32"):
            for cus in W.CUS:
                r = W.expected(W.key(c, dn, cus))
                rows.add(W.table_row(r))
                fin.add(r[W.ROUTE_FIELDS.index("finish")])
                bfin.add(r[W.ROUTE_FIELDS.index("bias_finish")])
    assert rows == set(W.ALL_ROWS), f"rows never reached: {set(W.ALL_ROWS) - rows}; unknown rows: {rows - set(W.ALL_ROWS)}"
    assert fin == {0, 1, 2} and bfin == {0, 1, 2, 3}


def test_small_cases_reach_the_row_they_are_listed_for(lib):
    """The launches of tests/test_wgrad_routes_gpu.py, under their pins: family, dtype, geometry, split count, finishing."""
    rows = set()
    for c in W.SMALL:
        for dn in c["dtypes"]:
            rc, r = W.query_route(lib, c, dn)
            assert rc == 0, f"{c['name']}: {rc} {lib.psg_last_error()}"
            L = dict(zip(W.ROUTE_FIELDS, r))
            g = W.geom(c)
            geom = 0 if c["stride"] != 1 else (2 if c["ks"] == 1 else 1)
            assert (L["family"], L["dtype"], L["geom"], L["bias"]) == (c["family"], W.DTYPE_CODE[dn], geom, int(c["dbias"])), f"{c['name']}: {L}"
            steps = -(-g["M"] // L["BKP"])
            assert L["splits"] == -(-steps // -(-steps // c["splits"])) and L["splits"] == c["splits"], f"{c['name']}: {L}"
            want = {"direct": ("direct", "direct"), "sum": ("sum", "folded"), "reduce": ("reduce", "bias_sum"), "acc": ("sum", "folded")}[c["name"].rsplit(".", 1)[1]]
            assert W.FINISH[L["finish"]] == want[0] and W.BIAS_FINISH[L["bias_finish"]] == (want[1] if c["dbias"] else "none"), f"{c['name']}: {L}"
            # a tail in every direction: a ragged last row tile, a ragged last q tile, a ragged last K step
            assert c["Cout"] % L["BR"] != 0 or L["family"] in (1, 3), c["name"]
            assert g["Q"] % L["BQ"] != 0 and g["M"] % L["BKP"] != 0 and g["ldx"] > c["Cin"], c["name"]
            rows.add(W.table_row(r))
    assert rows == set(W.ALL_ROWS), f"rows never reached: {set(W.ALL_ROWS) - rows}"


def test_pins(lib):
    """A family pin skips the thresholds and keeps what the kernels need; an impossible pin is PSG_ERR_ARG from the route (all
    zeros: no launches) and -1 from the workspace query."""
    base = dict(B=3, H=5, ks=3, Cin=64, Cout=320)
    ok = [(0, "bf16", {}), (0, "f32", {}), (0, "bf16", dict(stride=2, H=9)), (1, "bf16", {}), (1, "bf16", dict(Cout=640)), (2, "bf16", {}),
          (2, "bf16", dict(ks=1, Cout=136)), (3, "bf16", dict(dbias=False)), (3, "bf16", dict(Cin=1728))]
    bad = [(1, "f32", {}), (2, "f32", {}), (3, "f32", {}),                              # bf16 only
           (1, "bf16", dict(stride=2, H=9)), (2, "bf16", dict(stride=2, H=9)), (3, "bf16", dict(stride=2, H=9)),   # stride-1 same-size only
           (1, "bf16", dict(Cout=136)), (1, "bf16", dict(Cout=240)),                   # Cout % 160
           (3, "bf16", dict(Cout=160)), (3, "bf16", dict(Cout=480)),                   # Cout % 320
           (3, "bf16", dict(Cin=64)), (3, "bf16", dict(Cin=192)),                       # dbias with 3 / 9 q tiles
           (3, "bf16", dict(lddy=8_000_000, dbias=False))]                             # (M + 64) dY rows reach past 2 GiB
    for v, dn, kw in ok:
        c = W._mk(f"pin{v}", **dict(base, **kw), variant=v)
        rc, r = W.query_route(lib, c, dn)
        assert rc == 0 and r[0] == v and r[-1] >= 1, (v, dn, kw, rc, r)
        with W.settings(lib, c):
            assert lib.psg_conv_wgrad_workspace_bytes(C.byref(W.make_desc(c, dn))) == W.implied_ws_bytes(c, r)
    for v, dn, kw in bad:
        c = W._mk(f"pin{v}", **dict(base, **kw), variant=v)
        rc, r = W.query_route(lib, c, dn)
        assert rc == W.ERR_ARG and r == (0,) * W.NF, (v, dn, kw, rc, r)
        assert b"pinned" in lib.psg_last_error()
        with W.settings(lib, c):
            d = W.make_desc(c, dn)
            assert lib.psg_conv_wgrad_workspace_bytes(C.byref(d)) == -1
            assert lib.psg_conv_wgrad(C.byref(d), None) == W.ERR_ARG              # (before any device call)
    # any other value gives the choice back; a split pin of 0 returns it to the model
    c = W._mk("unpinned", **base)
    for v in (-1, 4, 99):
        assert W.query_route(lib, dict(c, variant=v), "bf16") == W.query_route(lib, c, "bf16")
    assert W.query_route(lib, dict(c, splits=2), "bf16")[1][W.ROUTE_FIELDS.index("splits")] == 2
    assert W.query_route(lib, dict(c, splits=-3), "bf16") == W.query_route(lib, c, "bf16")
    # argument errors: the codes of psg_conv_wgrad's own checks
    d = W.make_desc(c, "bf16")
    out = (C.c_int32 * W.NF)()
    assert lib.psg_conv_wgrad_route(C.byref(d), None) == W.ERR_ARG and lib.psg_conv_wgrad_route(None, out) == W.ERR_ARG
    d.Cin = 12
    assert lib.psg_conv_wgrad_route(C.byref(d), out) == -1                              # PSG_ERR_SHAPE
    d.dtype = 7
    assert lib.psg_conv_wgrad_route(C.byref(d), out) == -2                              # PSG_ERR_DTYPE


_CHILD = """
import json, sys
sys.path.insert(0, %r)
from pokemon_sprite_generator_amd import _lib
from tests import wgrad_cases as W
lib = _lib.load()
print(json.dumps({c["name"]: list(W.route_of(lib, W.make_desc(c, "bf16"))[1]) for c in W.ENV_CASES}))
"""


@pytest.mark.parametrize("var,val", W.ENV_SETTINGS)
def test_environment_switches_give_the_stored_routes(lib, var, val):
    """The settings block reads the environment once per process, so each switch gets a child process (host only)."""
    env = dict(os.environ)
    env[var] = val
    res = subprocess.run([sys.executable, "-c", _CHILD % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])
    changed = 0
    for c in W.ENV_CASES:
        want = W.expected(f"env:{var}={val}|{c['name']}")
        assert tuple(got[c["name"]]) == want, f"{var}={val} {c['name']}: {got[c['name']]} (stored {want})"
        changed += want != W.expected(W.key(c, "bf16", 256))
    assert changed > 0, f"{var}={val} changes no route of the table: the spot check checks nothing"
