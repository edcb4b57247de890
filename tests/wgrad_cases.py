"""The case table of the weight-gradient route tests (test infrastructure, not a conftest): psg_wgrad_desc shapes and, in
tests/golden/wgrad_routes.json, the route psg_conv_wgrad_route reported for each of them - at 256 and at 96 available CUs, in
bf16 and in fp32 - when the export was first added, on the planner as it stood.  The file is not regenerated: it is what a
refactor of csrc/wgrad.hip must keep reporting.

CASES  every weight-gradient shape of the batch-256 U-Net step (with and without dbias, OHWI and OIHW), the VAE and BERT
       shapes the trainers launch (the VGG16 of the perceptual loss is frozen: it launches none), the shapes of
       test_kernels_gpu's WIDE_CASES / PIPE_CASES / SPLITK_CASES, and the small shapes of SMALL without their pins.
SMALL  the launches of tests/test_wgrad_routes_gpu.py: the smallest shapes with a tail in every direction that reach each row
       of the variant table, each with its family / split pins and its finishing configuration.

tests/test_wgrad_routes_cpu.py holds the library to the stored routes on the host.
"""
import contextlib
import ctypes
import json
import os

from pokemon_sprite_generator_amd._lib import ERR_ARG

ROUTES_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_routes.json")
ROUTE_FIELDS = ("family", "dtype", "geom", "bias", "BR", "BQ", "BKP", "lds", "wg_per_cu", "rtiles", "qtiles", "splits",
                "steps_per_split", "grid", "finish", "bias_finish", "launches")
NF = len(ROUTE_FIELDS)
FAMILIES = ("narrow128", "narrow160", "wide", "pipe")                      # psg_conv_wgrad_set_variant 0..3
FINISH = ("direct", "sum", "reduce")
BIAS_FINISH = ("none", "direct", "folded", "bias_sum")
DTYPE_CODE = {"f32": 0, "bf16": 1}
LAYOUT_CODE = {"oihw": 0, "ohwi": 1}
CUS = (256, 96)
# the environment spot checks: (variable, value) -> routes of ENV_CASES at bf16 / 256 CUs
ENV_SETTINGS = (("PSG_WGRAD_WIDE", "0"), ("PSG_WGRAD_PIPE", "0"), ("PSG_WGRAD_BR160", "0"), ("PSG_WGRAD_SPLITS", "3"))

DEFAULTS = dict(B=1, H=1, W=None, Cin=64, Cout=64, ks=1, stride=1, dbias=True, layout="ohwi", acc=False, ldx=0, lddy=0,
                variant=-1, splits=0)

# (H, Cin, Cout, ks, stride) of the U-Net's convs at batch 256 (tools/wgrad_bench.py, tests/test_gemm_b256_gpu.py) ...
UNET_CONVS = [(27, 8, 320, 3, 1), (27, 320, 320, 3, 1), (27, 640, 320, 3, 1), (27, 320, 8, 3, 1), (27, 640, 320, 1, 1), (27, 320, 640, 3, 2),
              (14, 640, 640, 3, 1), (14, 1280, 640, 3, 1), (14, 1280, 640, 1, 1), (14, 640, 1280, 3, 2),
              (7, 1280, 1280, 3, 1), (7, 2560, 1280, 3, 1), (7, 2560, 1280, 1, 1), (7, 1280, 1280, 3, 2),
              (4, 1280, 1280, 3, 1), (4, 2560, 1280, 3, 1), (4, 2560, 1280, 1, 1)]
# ... and (rows, Cin, Cout) of its Linears: attention projections and FFNs per level, text projections, ProjGroup, time MLP
UNET_LINEARS = [(256 * 196, 640, 640), (256 * 196, 640, 1920), (256 * 196, 640, 1280), (256 * 196, 1280, 640),
                (256 * 49, 1280, 1280), (256 * 49, 1280, 3840), (256 * 49, 1280, 2560), (256 * 49, 2560, 1280),
                (256 * 16, 1280, 1280), (256 * 16, 1280, 3840), (256 * 16, 1280, 2560), (256 * 16, 2560, 1280),
                (256 * 32, 256, 640), (256 * 32, 256, 1280), (256 * 32, 640, 1280), (256 * 32, 1280, 2560),
                (256, 128, 15360), (256, 256, 15360), (256, 128, 512), (256, 512, 512), (256, 512, 128)]
# VAE (batch 32; its 4x4 stride-2 convs do not take this entry): 3x3 / 1x1 convs of the ResNet blocks, the latent projections
# and the final conv; its cross-attention Linears.  BERT (32 x 32 tokens): the encoder's Linears and the projection.
VAE_CONVS = [(108, 32, 32, 3, 1), (54, 64, 64, 3, 1), (28, 128, 128, 3, 1), (27, 128, 512, 3, 1), (27, 512, 512, 3, 1), (27, 128, 512, 1, 1),
             (27, 512, 8, 3, 1), (27, 8, 512, 3, 1), (27, 512, 512, 1, 1), (54, 512, 256, 3, 1), (54, 256, 256, 3, 1), (54, 512, 256, 1, 1),
             (108, 256, 128, 3, 1), (108, 128, 128, 3, 1), (216, 32, 8, 3, 1)]
OTHER_LINEARS = [(32 * 32, 256, 512), (32 * 32, 768, 768), (32 * 32, 768, 3072), (32 * 32, 3072, 768), (32 * 32, 768, 256)]
# test_kernels_gpu.py: WIDE_CASES / PIPE_CASES (B, H, Cin, Cout, ks) and SPLITK_CASES (..., stride)
WIDE_CASES = [(3, 14, 256, 128, 3), (5, 7, 248, 192, 3), (2, 27, 256, 128, 3), (37, 4, 512, 256, 3), (3, 9, 1280, 128, 1),
              (64, 14, 256, 256, 3), (1, 5, 256, 64, 3), (130, 7, 768, 128, 1), (5, 14, 1280, 3840, 1), (9, 27, 256, 320, 3)]
PIPE_CASES = [(2, 4, 1280, 640, 3), (4, 4, 1280, 640, 3), (6, 4, 1024, 320, 3), (2, 7, 1280, 640, 3), (3, 7, 1024, 320, 3), (1, 14, 1280, 640, 3),
              (5, 14, 1024, 320, 3), (2, 27, 1024, 320, 3), (3, 9, 1920, 1280, 1), (33, 7, 1280, 640, 3), (3, 9, 1888, 1280, 1)]
SPLITK_CASES = [(2, 7, 1280, 1280, 3, 1), (4, 4, 2560, 1280, 3, 1), (3, 7, 2560, 640, 1, 1), (1, 14, 640, 640, 3, 1), (6, 4, 1280, 2560, 1, 1),
                (2, 14, 320, 640, 3, 2)]


def _mk(name, **kw):
    c = dict(DEFAULTS)
    c.update(kw)
    c["name"] = name
    if c["W"] is None:
        c["W"] = c["H"]
    return c


def _small():
    """name -> case of the GPU route test: (shape) x (finishing configuration).  A shape's `dtypes` says where it runs."""
    shapes = []
    g0 = dict(B=3, H=9, ks=3, stride=2, Cin=24, Cout=136)                    # Ho = 5, M = 75
    g1 = dict(B=3, H=5, ks=3, Cin=24, Cout=136)
    g2 = dict(B=3, H=5, ks=1, Cin=264, Cout=136)
    for dn in ("bf16", "f32"):
        for g, kw in (("g0", g0), ("g1", g1), ("g2", g2)):
            shapes.append((f"narrow128.{dn}.{g}", dn, 0, kw))
    shapes.append(("narrow160.bf16.g1", "bf16", 1, dict(g1, Cout=160)))
    shapes.append(("narrow160.bf16.g2", "bf16", 1, dict(g2, Cout=160)))
    shapes.append(("wide.bf16.g1", "bf16", 2, dict(g1, Cin=32, variant=2)))      # Q = 288: one whole, one ragged 256-column tile
    shapes.append(("wide.bf16.g2", "bf16", 2, dict(g2, variant=2)))
    for bias in (False, True):
        for B in (3, 9):                                                      # M = 75: three K steps; 225: eight
            bn = "bias" if bias else "nobias"
            shapes.append((f"pipe.{bn}.g1.m{B * 25}", "bf16", 3, dict(B=B, H=5, ks=3, Cin=216, Cout=320, dbias=bias, variant=3)))
            shapes.append((f"pipe.{bn}.g2.m{B * 25}", "bf16", 3, dict(B=B, H=5, ks=1, Cin=1944, Cout=320, dbias=bias, variant=3)))
    out = []
    for name, dn, fam, kw in shapes:
        cfgs = [("direct", dict(splits=1, layout="ohwi")), ("sum", dict(splits=2, layout="ohwi"))]
        if kw["ks"] == 3:
            cfgs.append(("reduce", dict(splits=2, layout="oihw")))
        cfgs.append(("acc", dict(splits=1, layout="ohwi", acc=True)))
        for cn, ckw in cfgs:
            c = _mk(f"small.{name}.{cn}", **dict(kw, **ckw), ldx=16)
            c["dtypes"], c["family"] = (dn,), fam
            out.append(c)
    return out


SMALL = _small()


def _build():
    cs = []
    add = lambda *a, **k: cs.append(_mk(*a, **k))
    for H, Cin, Cout, ks, stride in UNET_CONVS:
        for db in (True, False):
            for lay in ("ohwi", "oihw"):
                add(f"unet.{H}x{H}.{Cin}-{Cout}.k{ks}s{stride}.{'db' if db else 'nodb'}.{lay}", B=256, H=H, Cin=Cin, Cout=Cout, ks=ks,
                    stride=stride, dbias=db, layout=lay)
    for M, Cin, Cout in UNET_LINEARS:
        for db in (True, False):
            add(f"unet.lin{M}.{Cin}-{Cout}.{'db' if db else 'nodb'}", B=M, Cin=Cin, Cout=Cout, dbias=db, layout="oihw")
    for H, Cin, Cout, ks, stride in VAE_CONVS:
        for lay in ("ohwi", "oihw"):
            add(f"vae.{H}x{H}.{Cin}-{Cout}.k{ks}.{lay}", B=32, H=H, Cin=Cin, Cout=Cout, ks=ks, stride=stride, layout=lay)
    for M, Cin, Cout in OTHER_LINEARS:
        add(f"lin{M}.{Cin}-{Cout}", B=M, Cin=Cin, Cout=Cout, layout="oihw")
        add(f"lin{M}.{Cin}-{Cout}.acc", B=M, Cin=Cin, Cout=Cout, layout="oihw", acc=True)
    for tag, rows in (("wide", WIDE_CASES), ("pipe", PIPE_CASES), ("splitk", SPLITK_CASES)):
        for r in rows:
            B, H, Cin, Cout, ks = r[:5]
            stride = r[5] if len(r) > 5 else 1
            for lay in ("ohwi", "oihw"):
                for db in (True, False) if tag == "pipe" else (True,):
                    add(f"{tag}.{B}.{H}.{Cin}.{Cout}.{ks}.{stride}.{'db' if db else 'nodb'}.{lay}", B=B, H=H, Cin=Cin, Cout=Cout, ks=ks,
                        stride=stride, dbias=db, layout=lay, ldx=64 if tag == "wide" else 0)
            if tag == "wide":
                add(f"wide.{B}.{H}.{Cin}.{Cout}.{ks}.acc", B=B, H=H, Cin=Cin, Cout=Cout, ks=ks, acc=True, ldx=64)
    # a 3x3 layer the plan itself sends to the wide kernel (288 narrow tiles, no column waste, Cout % 320 != 0): no U-Net layer is one
    for lay in ("ohwi", "oihw"):
        add(f"wide3x3.4.7.512.1024.{lay}", B=4, H=7, Cin=512, Cout=1024, ks=3, layout=lay)
    for c in SMALL:                                          # the small shapes, as the plan itself sends them
        cs.append(dict(c, name="plan." + c["name"], variant=-1, splits=0))
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names), "duplicate case names"
    return cs


CASES = _build()
ENV_CASES = [c for c in CASES if c["name"].startswith("unet.") and c["name"].endswith(".db.ohwi")]


def key(c, dn, cus):
    return f"{c['name']}|{dn}|{cus}"


def geom(c):
    pad = c["ks"] // 2
    Ho, Wo = (c["H"] + 2 * pad - c["ks"]) // c["stride"] + 1, (c["W"] + 2 * pad - c["ks"]) // c["stride"] + 1
    return dict(pad=pad, Ho=Ho, Wo=Wo, M=c["B"] * Ho * Wo, taps=c["ks"] ** 2, Q=c["ks"] ** 2 * c["Cin"],
                ldx=c["Cin"] + c["ldx"], lddy=c["Cout"] + c["lddy"])


FAKE_PTRS = dict(x=0x10000, dy=0x20000, dw=0x30000, dbias=0x40000)


def make_desc(c, dn, ptrs=FAKE_PTRS, ws=0, ws_bytes=0):
    """psg_wgrad_desc of a case; the host-only queries take any aligned non-null numbers for the pointers."""
    from pokemon_sprite_generator_amd._lib import WgradDesc
    g = geom(c)
    d = WgradDesc()
    d.dtype, d.B, d.Hi, d.Wi, d.Cin, d.Ho, d.Wo, d.Cout = DTYPE_CODE[dn], c["B"], c["H"], c["W"], c["Cin"], g["Ho"], g["Wo"], c["Cout"]
    d.ksize, d.stride, d.pad = c["ks"], c["stride"], g["pad"]
    d.accumulate, d.accumulate_bias, d.dw_layout, d.scale = int(c["acc"]), int(c["acc"] and c["dbias"]), LAYOUT_CODE[c["layout"]], 1.0
    d.ldx, d.lddy = g["ldx"], g["lddy"]
    d.x, d.dy, d.dw, d.dbias = ptrs["x"], ptrs["dy"], ptrs["dw"], ptrs["dbias"] if c["dbias"] else None
    d.ws, d.ws_bytes = (ws or None), ws_bytes
    return d


@contextlib.contextmanager
def settings(lib, c, cus=256):
    """The library settings of a case, restored to the defaults afterwards whatever happens."""
    try:
        assert lib.psg_conv_wgrad_set_variant(c["variant"]) == 0 and lib.psg_conv_wgrad_set_splits(c["splits"]) == 0
        assert lib.psg_set_available_cus(0 if cus == 256 else cus) == 0 and lib.psg_set_reserve_rounds(0) == 0
        yield
    finally:
        lib.psg_conv_wgrad_set_variant(-1)
        lib.psg_conv_wgrad_set_splits(0)
        lib.psg_set_available_cus(0)
        lib.psg_set_reserve_rounds(0)


def route_of(lib, d):
    """psg_conv_wgrad_route -> (return code, tuple of the NF fields; all zero on an error)."""
    out = (ctypes.c_int32 * NF)()
    rc = lib.psg_conv_wgrad_route(ctypes.byref(d), ctypes.cast(out, ctypes.c_void_p))
    return rc, tuple(out)


def query_route(lib, c, dn, cus=256):
    with settings(lib, c, cus):
        return route_of(lib, make_desc(c, dn))


def implied_ws_bytes(c, route):
    """Workspace bytes of a reported plan: fp32 slabs [splits][Cout][Q] unless the tiles go straight into dw, then the bias
    partials [splits][Cout] unless the kernel writes dbias itself."""
    L = dict(zip(ROUTE_FIELDS, route))
    slabs = 0 if FINISH[L["finish"]] == "direct" else L["splits"] * c["Cout"] * geom(c)["Q"]
    bias = L["splits"] * c["Cout"] if BIAS_FINISH[L["bias_finish"]] in ("folded", "bias_sum") else 0
    return 4 * (slabs + bias)


def table_row(route):
    """The row of csrc/wgrad.hip's variant table a route names: (family, dtype, geom, bias) - bias only where the family has a
    kernel of its own for it (pipe)."""
    L = dict(zip(ROUTE_FIELDS, route))
    return (FAMILIES[L["family"]], L["dtype"], L["geom"], L["bias"] if L["family"] == 3 else 0)


# every instantiation: wgrad_kernel<T, 0..2, 128>, <bf16, 1..2, 160>, wgrad_wide_kernel<1..2>, wgrad_pipe_kernel<1..2, BIAS>
ALL_ROWS = ([("narrow128", dt, g, 0) for dt in (0, 1) for g in (0, 1, 2)] + [("narrow160", 1, g, 0) for g in (1, 2)]
            + [("wide", 1, g, 0) for g in (1, 2)] + [("pipe", 1, g, b) for g in (1, 2) for b in (0, 1)])

_routes = None


def expected(k):
    global _routes
    if _routes is None:
        with open(ROUTES_JSON) as f:
            _routes = {n: tuple(v) for n, v in json.load(f).items()}
    return _routes[k]
