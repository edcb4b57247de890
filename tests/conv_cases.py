"""The case table of the conv forward / data-gradient route tests (test infrastructure, not a conftest): tiny psg_conv_fwd
launches that together reach every launch variant - dtype and tile, gather mode 0..3, split-K and its finishing kernel, the
border-class order, the persistent pointwise kernel and every epilogue form - each with the settings it needs (tile pin,
border-class mode, pointwise kernel on / off, available CUs, workspace offered / too small / none) and, in
tests/golden/conv_routes.json, the route psg_conv_route must report for it.

tests/test_conv_ref_cpu.py proves on the host that the stored routes are the library's, that the table reaches every
variant a sweep of shapes reaches, and that the comparator (verify) rejects a list of injected defects at these very shapes;
tests/test_conv_routes_gpu.py launches every case and checks each element of y / preact against the fp64 reference of the
operands the kernel read (tests/gemm_ref.py).

A case names the LAUNCH's quantities: Cin = channels gathered per tap (K = taps x Cin), Cout = N.  (H, W) is always the larger
grid - the conv's input: a forward launch reads it, a data-gradient launch (tr = 1) writes it and reads the gradient on the
grid (H + 2 pad - ks) // stride + 1.
"""
import contextlib
import ctypes
import json
import math
import os

import numpy as np
import torch

from tests import gemm_ref as R
from tests.util import h

ROUTES_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_routes.json")
ROUTE_FIELDS = ("BM", "BN", "mode", "splits", "kt_per_split", "tapcls", "pw", "epi_lds", "mtiles", "ntiles", "grid", "M", "KT",
                "sub_h0", "sub_w0", "sub_nH", "sub_nW", "ntap")
NF = len(ROUTE_FIELDS)
TILES = ((128, 128), (128, 64), (64, 64), (128, 160), (64, 160))           # psg_conv_set_tile candidates 0..4
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
DTYPE_CODE = {"f32": 0, "bf16": 1}
ACT_CODE = {"none": 0, "silu": 1, "gelu": 2, "relu": 3, "tanh": 4, "quick_gelu": 5}
SAVE_DACT, DACT_MUL, GENERIC = 1, 2, 4
NAN = float("nan")
GUARD = 64                                                                  # guard elements before and after every buffer

DEFAULTS = dict(dtype="bf16", B=1, H=1, W=1, Cin=64, Cout=64, ks=1, stride=1, pad=None, tr=0,
                act="none", bias=False, rowadd=False, residual=False, alias=False, preact=False, save_dact=False, dact=None,
                drop_p=0.0, alpha=1.0, generic=False,
                ldx=0, ldy=0, ldres=0, ldpre=0, lddact=0, ldw=0, woff=0,      # extra elements per row beyond the dense stride
                tile=-1, tapcls=1, pw=1, cus=256, ws="none")

# epilogue recipes: every operand of the descriptor, in the combinations conv_setup allows
RECIPES = {
    "plain": dict(bias=True),
    "res": dict(bias=True, residual=True, alpha=0.7),
    "rowadd": dict(bias=True, rowadd=True, act="silu"),
    "gelu_pre": dict(bias=True, act="gelu", preact=True),
    "gelu_drop_save": dict(bias=True, act="gelu", drop_p=0.05, preact=True, save_dact=True),
    "drop_res": dict(drop_p=0.5, residual=True),
    "drop": dict(bias=True, drop_p=0.05),
    "relu_save": dict(bias=True, act="relu", preact=True, save_dact=True),
    "tanh": dict(bias=True, act="tanh", alpha=1.3),
    "silu_save_res": dict(rowadd=True, act="silu", preact=True, save_dact=True, residual=True),
    "dactu_silu": dict(dact="u", act="silu", alpha=0.5),
    "dactu_gelu_drop": dict(dact="u", act="gelu", drop_p=0.05, bias=True, preact=True),
    "dactu_tanh": dict(dact="u", act="tanh"),
    "dmul": dict(dact="mul", alpha=1.3),
    "all": dict(bias=True, rowadd=True, residual=True, act="silu", alpha=0.7, drop_p=0.05, preact=True),
}
# quick-GELU (both CLIP towers' MLP) in each form an epilogue evaluates an activation in: the value (act_f), value and saved
# derivative (act_both), the value under dropout, the derivative of a saved pre-activation (act_grad).  Listed apart: the cases
# of _build() take the fifteen recipes above by position, which must not move.
QGELU_RECIPES = {
    "qgelu": dict(bias=True, act="quick_gelu"),
    "qgelu_save": dict(bias=True, act="quick_gelu", preact=True, save_dact=True),
    "qgelu_drop_pre": dict(act="quick_gelu", drop_p=0.05, preact=True),
    "dactu_qgelu": dict(dact="u", act="quick_gelu"),
}
# recipes whose bf16 staged epilogue has a per-kind copy (EK_*); the rest run EK_GENERIC
EK_OF = {"plain": "PLAIN", "res": "PLAIN", "drop": "DROP", "drop_res": "DROP", "gelu_pre": "GELU", "gelu_drop_save": "GELU_DROP",
         "dmul": "DMUL"}


def _mk(name, recipe=None, **kw):
    c = dict(DEFAULTS)
    c["name"] = name
    c["recipe"] = recipe
    if recipe:
        c.update(RECIPES[recipe] if recipe in RECIPES else QGELU_RECIPES[recipe])
    c.update(kw)
    if c["pad"] is None:
        c["pad"] = c["ks"] // 2
    return c


def _build():
    cs = []
    add = lambda *a, **k: cs.append(_mk(*a, **k))
    rec = list(RECIPES)

    # ---- (A) every (dtype, tile), pinned: ragged M and N around the tile, K steps 1, 2, 3, 5, 4 (double-buffer parity) --------
    # Linear geometry (B = M samples, so a row-add has one row per GEMM row).
    for dn in ("bf16", "f32"):
        kstep = 64 if dn == "bf16" else 32
        for ti, (BM, BN) in enumerate(TILES):
            if dn == "f32" and BN == 160:
                continue
            pairs = [(1, 4), (BM - 1, 8), (BM, 12), (BM + 1, BN - 4), (2 * BM + 3, BN), (BM, BN + 8), (2 * BM + 3, BN + 8)]
            for i, (M, N) in enumerate(pairs):
                add(f"tile.{dn}.{BM}x{BN}.m{M}.n{N}", rec[(i + 3 * ti) % len(rec)], dtype=dn, B=M, Cin=kstep * (1, 2, 3, 5, 4, 1, 2)[i],
                    Cout=N, tile=ti)
            # grids whose workgroup count and M-tile count are no multiples of 8, two N tiles: XCD remap + grouped raster
            for mt in (9, 17):
                add(f"tile.{dn}.{BM}x{BN}.mt{mt}", "res" if mt == 9 else "gelu_pre", dtype=dn, B=mt * BM - 5, Cin=kstep,
                    Cout=BN + 8, tile=ti)
    # every (dtype, tile) x gather mode x {direct / fp32 (N = 12), staged (N = 24)} x border-class order, pinned, on a 3x5 image
    # (mode 3: its data gradient grid 5x8 -> 3x4), the recipes taking turns
    k = 0
    for dn in ("bf16", "f32"):
        for ti, (BM, BN) in enumerate(TILES):
            if dn == "f32" and BN == 160:
                continue
            fast, slow = (64, 24) if dn == "bf16" else (32, 12)
            for mode in (0, 1, 2, 3):
                if mode == 3 and BN == 160:
                    continue
                for N in (12, 24) if dn == "bf16" else (12,):
                    for cls in (0, 2) if dn == "bf16" and mode in (0, 1) else (0,):
                        r = rec[k % len(rec)]
                        k += 1
                        kw = dict(H=3, W=5, tr=int(mode == 1)) if mode != 3 else dict(H=5, W=8, stride=2, tr=1)
                        add(f"mat.{dn}.{BM}x{BN}.mode{mode}.n{N}.cls{cls}", r, dtype=dn, B=3, Cin=slow if mode == 2 else fast, Cout=N,
                            ks=3, tapcls=cls, tile=ti, **kw)
    # the plan's own choice of each tile (8 resident-slot pairs: psg_set_available_cus(8))
    for dn, kstep in (("bf16", 64), ("f32", 32)):
        add(f"plan.{dn}.128x128", "plain", dtype=dn, B=700, Cin=kstep, Cout=200 if dn == "bf16" else 136, cus=8)
        add(f"plan.{dn}.128x64", "rowadd", dtype=dn, B=2048, Cin=kstep, Cout=8, cus=8)
        add(f"plan.{dn}.64x64", "res", dtype=dn, B=60, Cin=kstep, Cout=72)
    add("plan.bf16.128x160", "gelu_pre", B=700, Cin=64, Cout=320, cus=8)
    add("plan.bf16.64x160", "drop_res", B=700, Cin=64, Cout=136, cus=8)

    # ---- (B) K axis of the generic gather (mode 2): K tail with Kpad > K, a K step crossing a tap; 4x4 stride 2 --------------
    for dn, cins in (("bf16", (8, 24, 40)), ("f32", (4, 12, 20))):
        for i, ci in enumerate(cins):
            add(f"k.{dn}.3x3.cin{ci}", ("plain", "rowadd", "tanh")[i], dtype=dn, B=3, H=5, W=7, Cin=ci, Cout=16, ks=3)
            add(f"k.{dn}.3x3s2.cin{ci}", ("res", "gelu_pre", "drop")[i], dtype=dn, B=3, H=5, W=7, Cin=ci, Cout=12, ks=3, stride=2)
        for ci in (8, 16):
            for pad in (1, 2):
                add(f"k.{dn}.4x4s2.cin{ci}.p{pad}", "rowadd" if pad == 1 else "relu_save", dtype=dn, B=3, H=6, W=8, Cin=ci, Cout=16,
                    ks=4, stride=2, pad=pad)
    add("k.bf16.ldw", "plain", B=3, H=3, W=5, Cin=24, Cout=16, ks=3, ldw=64, woff=24)
    add("k.bf16.ldw.fast", "res", B=3, H=3, W=5, Cin=64, Cout=72, ks=3, ldw=128, woff=64)
    add("k.f32.ldw", "plain", dtype="f32", B=5, Cin=96, Cout=20, ldw=32, woff=12)

    # ---- (C) geometry: fast gathers (modes 0, 1), stride 2, 1x1 stride 2, every parity class (mode 3), generic data gradients --
    imgs = ((1, 1), (1, 6), (6, 1), (2, 2), (3, 3), (3, 5), (5, 7), (14, 14))
    for i, (H, W) in enumerate(imgs):
        for dn, ci in (("bf16", 64), ("f32", 32)):
            add(f"g.{dn}.3x3.{H}x{W}", rec[i % len(rec)], dtype=dn, B=3, H=H, W=W, Cin=ci, Cout=24, ks=3, tapcls=0)
            add(f"g.{dn}.3x3.dgrad.{H}x{W}", ("plain", "dactu_silu", "dmul", "drop")[i % 4], dtype=dn, B=3, H=H, W=W, Cin=ci, Cout=24,
                ks=3, tr=1, tapcls=0)
    for H, W in ((1, 1), (2, 2), (3, 3), (4, 4), (5, 8), (7, 7), (14, 14)):
        add(f"g.bf16.3x3s2.{H}x{W}", "rowadd", B=3, H=H, W=W, Cin=64, Cout=24, ks=3, stride=2)
    add("g.f32.3x3s2.5x8", "res", dtype="f32", B=3, H=5, W=8, Cin=32, Cout=24, ks=3, stride=2)
    for dn, ci in (("bf16", 64), ("f32", 32)):
        add(f"g.{dn}.1x1.5x7", "gelu_pre", dtype=dn, B=3, H=5, W=7, Cin=ci, Cout=24)
        add(f"g.{dn}.1x1s2.5x7", "rowadd", dtype=dn, B=3, H=5, W=7, Cin=ci, Cout=24, stride=2)
        add(f"g.{dn}.1x1s2.dgrad.5x7", "plain", dtype=dn, B=3, H=5, W=7, Cin=ci, Cout=24, stride=2, tr=1)
        add(f"g.{dn}.1x1s2.dgrad.4x6", "dmul", dtype=dn, B=3, H=4, W=6, Cin=ci, Cout=24, stride=2, tr=1)
    # parity-class data gradients of a stride-2 3x3: result grid -> gradient grid 27 -> 14, 14 -> 7, 7 -> 4, 4 -> 2, 3 -> 2, 2 -> 1,
    # 1 -> 1 (three empty classes) and a non-square one; fp32 too
    for i, (H, W) in enumerate(((27, 27), (14, 14), (7, 7), (4, 4), (3, 3), (2, 2), (1, 1), (5, 8), (1, 4), (2, 1))):
        add(f"g.bf16.3x3s2.dgrad.{H}x{W}", ("plain", "rowadd", "drop", "dactu_silu", "gelu_pre", "dmul", "res", "all", "drop_res",
                                            "tanh")[i], B=3 if H < 27 else 2, H=H, W=W, Cin=64, Cout=24 if i % 2 else 12, ks=3, stride=2, tr=1)
    add("g.f32.3x3s2.dgrad.7x7", "rowadd", dtype="f32", B=3, H=7, W=7, Cin=32, Cout=24, ks=3, stride=2, tr=1)
    add("g.f32.3x3s2.dgrad.2x2", "drop", dtype="f32", B=3, H=2, W=2, Cin=32, Cout=24, ks=3, stride=2, tr=1)
    # generic-mode data gradients: non-fast channel counts
    for dn, ci in (("bf16", 24), ("f32", 12)):
        add(f"g.{dn}.3x3.dgrad.gen", "drop", dtype=dn, B=3, H=5, W=7, Cin=ci, Cout=16, ks=3, tr=1)
        add(f"g.{dn}.3x3s2.dgrad.gen", "plain", dtype=dn, B=3, H=5, W=8, Cin=ci, Cout=16, ks=3, stride=2, tr=1)
        add(f"g.{dn}.3x3s2.dgrad.gen.7x7", "dactu_silu", dtype=dn, B=3, H=7, W=7, Cin=ci, Cout=16, ks=3, stride=2, tr=1)

    # ---- (D) split-K (modes 0, 1, 2) and its finishing kernel: B >= 3 samples, so that a wrong row-add sample shows -----------
    # three plans: 64x64 3 x 9 of 27 steps; 128x64 4 x 12 of 45 (KT % splits != 0, a shorter last split, and kt0 = 12, 24, 36 inside a
    # 9-tap group: the tap state restarts mid-group); 64x64 3 x 12 of 36 (kt0 inside a tap group, five N tiles)
    shapes = (dict(B=3, H=3, W=3, Cin=192, Cout=12), dict(B=5, H=5, W=7, Cin=320, Cout=72, cus=8), dict(B=3, H=3, W=3, Cin=256, Cout=320, cus=8))
    for i, r in enumerate(rec):
        add(f"split.bf16.{r}", r, ks=3, tr=(i // 3) % 2, tapcls=0, ws="ok", **shapes[i % 3])
    f32shapes = (dict(B=3, H=3, W=3, Cin=96, Cout=12), dict(B=5, H=5, W=7, Cin=160, Cout=72, cus=8), dict(B=5, H=5, W=7, Cin=320, Cout=72, cus=8))
    for i, r in enumerate(("all", "dactu_gelu_drop", "rowadd", "res", "dmul", "relu_save")):
        add(f"split.f32.{r}", r, dtype="f32", ks=3, tr=i % 2, ws="ok", **f32shapes[i % 3])
    # generic gather: a K step crosses taps, the last split is shorter (3 x 10 of 29) or not (4 x 11 of 44)
    add("split.bf16.mode2", "all", B=3, H=3, W=3, Cin=200, Cout=12, ks=3, ws="ok")
    add("split.bf16.mode2.even", "plain", B=3, H=3, W=3, Cin=312, Cout=12, ks=3, ws="ok")
    add("split.bf16.mode2.dgrad", "dactu_silu", B=3, H=3, W=3, Cin=200, Cout=12, ks=3, tr=1, ws="ok")
    add("split.bf16.mode2.dgrad.s2", "rowadd", B=3, H=3, W=3, Cin=200, Cout=12, ks=3, stride=2, tr=1, ws="ok")
    add("split.bf16.mode2.s2", "res", B=3, H=3, W=3, Cin=200, Cout=12, ks=3, stride=2, ws="ok")
    add("split.f32.mode2", "res", dtype="f32", B=3, H=3, W=3, Cin=100, Cout=12, ks=3, ws="ok")
    add("split.f32.mode2.dgrad", "drop", dtype="f32", B=3, H=3, W=3, Cin=156, Cout=12, ks=3, tr=1, ws="ok")
    # the other tiles a split plan picks at 8 CUs
    add("split.bf16.64x160", "all", B=1, H=1, W=1, Cin=320, Cout=640, ks=3, ws="ok", cus=8)
    add("split.bf16.64x160.dgrad", "dmul", B=1, H=1, W=1, Cin=320, Cout=640, ks=3, tr=1, ws="ok", cus=8)
    add("split.bf16.64x160.mode2", "rowadd", B=3, H=3, W=3, Cin=200, Cout=640, ks=4, stride=2, pad=1, ws="ok", cus=8)
    add("split.bf16.128x64.mode2", "res", B=83, H=5, W=5, Cin=200, Cout=4, ks=4, stride=2, pad=1, ws="ok", cus=8)
    add("split.bf16.128x128", "gelu_drop_save", B=37, H=3, W=3, Cin=320, Cout=72, ks=3, tapcls=0, ws="ok", cus=8)
    add("split.bf16.128x128.dgrad", "dactu_gelu_drop", B=37, H=3, W=3, Cin=320, Cout=72, ks=3, tr=1, tapcls=0, ws="ok", cus=8)
    add("split.bf16.128x128.mode2", "tanh", B=83, H=5, W=5, Cin=200, Cout=72, ks=4, stride=2, pad=1, ws="ok", cus=8)
    add("split.bf16.128x160", "silu_save_res", B=37, H=3, W=3, Cin=320, Cout=136, ks=3, tapcls=0, ws="ok", cus=8)
    add("split.bf16.128x160.dgrad", "drop", B=37, H=3, W=3, Cin=320, Cout=136, ks=3, tr=1, tapcls=0, ws="ok", cus=8)
    add("split.bf16.128x160.mode2", "res", B=83, H=5, W=5, Cin=200, Cout=136, ks=4, stride=2, pad=1, ws="ok", cus=8)
    add("split.f32.128x64.mode2", "all", dtype="f32", B=83, H=5, W=5, Cin=100, Cout=4, ks=4, stride=2, pad=1, ws="ok", cus=8)
    add("split.f32.128x128.mode2", "rowadd", dtype="f32", B=83, H=5, W=5, Cin=100, Cout=72, ks=4, stride=2, pad=1, ws="ok", cus=8)
    # workspace too small / none / tile pinned: the unsplit best tile, not the split plan's
    add("split.bf16.ws_small", "all", ks=3, tapcls=0, ws="small", **shapes[1])
    add("split.bf16.ws_none", "all", ks=3, tapcls=0, ws="none", **shapes[1])
    add("split.bf16.pinned", "all", ks=3, tapcls=0, ws="big", tile=2, **shapes[1])
    add("split.bf16.ws_small.mode1", "dmul", ks=3, tr=1, tapcls=0, ws="small", **shapes[2])
    add("split.f32.ws_small", "res", dtype="f32", ks=3, ws="small", **f32shapes[1])

    # ---- (E) border-class order: forward and data gradient, 3x3 (one interior position), 3x5, 7x7; several classes end in
    # padding rows and mtiles is no multiple of 8; each staging sub-path (residual, preact, both) and the 160-wide tiles --------
    sub = ("res", "gelu_pre", "all", "plain", "drop_res", "gelu_drop_save", "dmul", "rowadd")
    k = 0
    for (H, W, B) in ((3, 3, 37), (3, 5, 21), (7, 7, 5), (7, 7, 37)):
        for tr in (0, 1):
            for ti in (0, 2, 3, 4):
                if (H, W, B) != (3, 5, 21) and ti in (3, 4) and tr:
                    continue
                r = sub[k % len(sub)]
                if tr and r in ("gelu_pre", "gelu_drop_save"):
                    r = "dmul"
                k += 1
                add(f"cls.{H}x{W}.b{B}.{'dgrad' if tr else 'fwd'}.t{ti}", r, B=B, H=H, W=W, Cin=64, Cout=(24, 72, 176, 168)[k % 4],
                    ks=3, tr=tr, tapcls=2, tile=ti)
    add("cls.3x5.direct", "all", B=21, H=3, W=5, Cin=64, Cout=12, ks=3, tapcls=2, tile=2)
    add("cls.3x5.ldpre", "gelu_pre", B=21, H=3, W=5, Cin=64, Cout=24, ks=3, tapcls=2, tile=2, ldpre=4)
    # the plan's own decision (setting 1) at 8 CUs: more than one round of resident workgroups
    # (17 plain M-tiles of 128 rows, 18 in class order, two N tiles: 36 workgroups on 16 slots)
    add("cls.plan.fwd", "res", B=83, H=5, W=5, Cin=64, Cout=72, ks=3, tapcls=1, cus=8)
    add("cls.plan.dgrad", "plain", B=83, H=5, W=5, Cin=64, Cout=72, ks=3, tr=1, tapcls=1, cus=8)
    add("cls.plan.160", "gelu_pre", B=83, H=5, W=5, Cin=64, Cout=136, ks=3, tapcls=1, cus=8)
    add("cls.plan.off", "res", B=83, H=5, W=5, Cin=64, Cout=72, ks=3, tapcls=0, cus=8)
    add("cls.plan.one_round", "res", B=23, H=5, W=5, Cin=64, Cout=72, ks=3, tapcls=1, cus=8)

    # ---- (F) persistent pointwise kernel: 24 whole tiles on 16 slots; every (kind, aux, preact) it instantiates, with it off too
    pwk = (("plain", {}), ("res", {}), ("drop", {}), ("drop_res", {}), ("gelu", dict(act="gelu", bias=True)), ("gelu_pre", {}),
           ("gelu_drop", dict(act="gelu", bias=True, drop_p=0.05)), ("gelu_drop_save", {}), ("dmul", {}),
           ("res_alias", dict(bias=True, residual=True, alias=True, alpha=0.7)), ("res_ld", dict(bias=True, residual=True, ldres=8, ldy=16)),
           ("gelu_pre_ld", dict(bias=True, act="gelu", preact=True, ldpre=8, ldx=8)))
    for nm, kw in pwk:
        for on in (1, 0):
            # (the plan itself prefers 128x64 for this grid: the 128x128 tile is pinned, which the pointwise kernel needs)
            add(f"pw.{nm}.{'on' if on else 'off'}", nm if nm in RECIPES else None, B=768, Cin=192, Cout=512, cus=8, pw=on, tile=0, **kw)
    # the plan's own 128x128: 30 and 27 tiles on 16 slots
    add("pw.plan.on", "res", B=768, Cin=192, Cout=640, cus=8)
    add("pw.plan.off", "res", B=768, Cin=192, Cout=640, cus=8, pw=0)
    add("pw.plan.dgrad.on", "plain", B=1152, Cin=192, Cout=384, cus=8, tr=1)
    add("pw.not.rowadd", "rowadd", B=768, Cin=192, Cout=512, cus=8, tile=0)
    add("pw.not.generic", "plain", B=768, Cin=192, Cout=512, cus=8, tile=0, generic=True)
    add("pw.not.ragged", "plain", B=760, Cin=192, Cout=512, cus=8, tile=0)
    add("pw.not.few_tiles", "plain", B=768, Cin=192, Cout=512, tile=0)

    # ---- (G) every recipe on every epilogue path: staged (with its EK kind, and under the generic flag), direct bf16, fp32 ----
    for i, r in enumerate(rec):
        add(f"epi.staged.{r}", r, B=3, H=3, W=5, Cin=64, Cout=72, ks=3, tapcls=0)
        add(f"epi.direct.{r}", r, B=3, H=3, W=5, Cin=64, Cout=12, ks=3, tapcls=0)
        add(f"epi.f32.{r}", r, dtype="f32", B=3, H=3, W=5, Cin=32, Cout=12, ks=3)
        if r in EK_OF:
            add(f"epi.generic.{r}", r, B=3, H=3, W=5, Cin=64, Cout=72, ks=3, tapcls=0, generic=True)
    add("epi.staged.pre", None, B=3, H=3, W=5, Cin=64, Cout=72, ks=3, tapcls=0, bias=True, preact=True)
    add("epi.staged.drop_save", None, B=3, H=3, W=5, Cin=64, Cout=72, ks=3, tapcls=0, bias=True, drop_p=0.05, preact=True, save_dact=True)
    add("epi.staged.p50", "gelu_drop_save", B=3, H=3, W=5, Cin=64, Cout=72, ks=3, tapcls=0, drop_p=0.5)
    # strides: ldx > Cin, ldy > Cout (a concat-slot half), the aux / preact rows wider than Cout; a stride that is no multiple
    # of 8 turns the staged epilogue off for the whole launch; a residual aliasing y on a tiled launch
    add("ld.staged.all", "all", B=3, H=3, W=5, Cin=64, Cout=72, ks=3, tapcls=0, ldx=64, ldy=72, ldres=8, ldpre=16)
    add("ld.staged.dmul", "dmul", B=3, H=3, W=5, Cin=64, Cout=72, ks=3, tapcls=0, tr=1, ldx=8, ldy=8, lddact=24)
    add("ld.staged.dactu", "dactu_gelu_drop", B=3, H=3, W=5, Cin=64, Cout=72, ks=3, tapcls=0, ldy=8, lddact=8, ldpre=8)
    add("ld.off.ldpre", "gelu_pre", B=3, H=3, W=5, Cin=64, Cout=72, ks=3, tapcls=0, ldpre=4)
    add("ld.off.ldres", "res", B=3, H=3, W=5, Cin=64, Cout=72, ks=3, tapcls=0, ldres=12)
    add("ld.off.ldy", "all", B=3, H=3, W=5, Cin=64, Cout=72, ks=3, tapcls=0, ldy=4)
    add("ld.off.lddact", "dmul", B=3, H=3, W=5, Cin=64, Cout=72, ks=3, tapcls=0, lddact=4)
    add("ld.f32.all", "all", dtype="f32", B=3, H=3, W=5, Cin=32, Cout=12, ks=3, ldx=4, ldy=12, ldres=4, ldpre=8)
    add("ld.mode3.all", "all", B=3, H=5, W=8, Cin=64, Cout=24, ks=3, stride=2, tr=1, ldx=8, ldy=24, ldres=8, ldpre=16)
    add("alias.staged", None, B=3, H=3, W=5, Cin=64, Cout=72, ks=3, tapcls=0, bias=True, residual=True, alias=True, alpha=0.7, ldy=8)
    add("alias.direct", None, B=3, H=3, W=5, Cin=64, Cout=12, ks=3, tapcls=0, bias=True, residual=True, alias=True)
    add("alias.f32", None, dtype="f32", B=130, Cin=64, Cout=72, bias=True, residual=True, alias=True, act="silu")
    add("alias.cls", None, B=21, H=3, W=5, Cin=64, Cout=72, ks=3, tapcls=2, residual=True, alias=True, tile=2)
    add("alias.mode3", None, B=3, H=5, W=8, Cin=64, Cout=24, ks=3, stride=2, tr=1, residual=True, alias=True)

    # ---- (H) quick-GELU on every epilogue path (appended: the cases above keep their places) ---------------------------------
    for r in QGELU_RECIPES:
        add(f"epi.staged.{r}", r, B=3, H=3, W=5, Cin=64, Cout=72, ks=3, tapcls=0)
        add(f"epi.direct.{r}", r, B=3, H=3, W=5, Cin=64, Cout=12, ks=3, tapcls=0)
        add(f"epi.f32.{r}", r, dtype="f32", B=3, H=3, W=5, Cin=32, Cout=12, ks=3)
    add("split.bf16.qgelu_save", "qgelu_save", ks=3, tapcls=0, ws="ok", **shapes[0])               # the finishing kernel
    add("split.f32.dactu_qgelu", "dactu_qgelu", dtype="f32", ks=3, tr=1, ws="ok", **f32shapes[0])
    add("g.bf16.3x3s2.dgrad.7x7.dactu_qgelu", "dactu_qgelu", B=3, H=7, W=7, Cin=64, Cout=24, ks=3, stride=2, tr=1)   # parity classes
    # the CLIP MLP's shape class: whole 128x128 tiles of a pointwise launch, more of them than resident slots, nothing pinned -
    # the stored route says which kernel takes it (the persistent pointwise kernel has no quick-GELU copy)
    add("pw.qgelu.plan", "qgelu", B=768, Cin=192, Cout=640, cus=8)
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names), "duplicate case names"
    return cs


CASES = _build()
BY_NAME = {c["name"]: c for c in CASES}


def case_ids():
    return [c["name"] for c in CASES]


# ------------------------------------------------------------------------------------------------------------- geometry
def geom(c):
    """Descriptor geometry of a case: Hi, Wi, Ho, Wo (as psg_conv_desc names them), M = rows of y, taps, K, Kpad, CH."""
    ks, s, p = c["ks"], c["stride"], c["pad"]
    Hs, Ws = (c["H"] + 2 * p - ks) // s + 1, (c["W"] + 2 * p - ks) // s + 1          # the smaller grid
    Hi, Wi, Ho, Wo = (Hs, Ws, c["H"], c["W"]) if c["tr"] else (c["H"], c["W"], Hs, Ws)
    CH = 8 if c["dtype"] == "bf16" else 4
    K = ks * ks * c["Cin"]
    Kpad = -(-K // (8 * CH)) * (8 * CH)
    return dict(Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, M=c["B"] * Ho * Wo, Min=c["B"] * Hi * Wi, taps=ks * ks, K=K, Kpad=Kpad, CH=CH,
                ldx=c["Cin"] + c["ldx"], ldy=c["Cout"] + c["ldy"], ldres=c["Cout"] + (c["ldy"] if c["alias"] else c["ldres"]),
                ldpre=c["Cout"] + c["ldpre"], lddact=c["Cout"] + c["lddact"], ldw=Kpad + c["ldw"])


def flags(c):
    return (SAVE_DACT if c["save_dact"] else 0) | (DACT_MUL if c["dact"] == "mul" else 0) | (GENERIC if c["generic"] else 0)


SEED_BASE = 0x1234_5678_9ABC_DEF1


def drop_seed(c):
    """A 64-bit seed with both halves set (the high word enters the hash separately)."""
    import zlib
    return (SEED_BASE + 0x1_0000_0001 * (zlib.crc32(c["name"].encode()) & 0xFFFF)) & 0xFFFFFFFFFFFFFFFF


def make_desc(c, ptrs, ws=0, ws_bytes=0):
    """psg_conv_desc of a case.  ptrs: name -> address (x, w, y, bias, rowadd, residual, preact, dact_u); the host-only route
    query takes any aligned non-null numbers."""
    from pokemon_sprite_generator_amd._lib import ConvDesc
    g = geom(c)
    d = ConvDesc()
    d.dtype, d.B, d.Hi, d.Wi, d.Cin, d.Ho, d.Wo, d.Cout = DTYPE_CODE[c["dtype"]], c["B"], g["Hi"], g["Wi"], c["Cin"], g["Ho"], g["Wo"], c["Cout"]
    d.ksize, d.stride, d.pad, d.transposed, d.act = c["ks"], c["stride"], c["pad"], c["tr"], ACT_CODE[c["act"]]
    d.alpha, d.drop_p, d.flags, d.drop_seed = c["alpha"], c["drop_p"], flags(c), drop_seed(c)
    d.ldx, d.ldy, d.ld_rowadd, d.ld_residual, d.ld_preact, d.ld_dact, d.ldw = g["ldx"], g["ldy"], c["Cout"], g["ldres"], g["ldpre"], g["lddact"], g["ldw"]
    use = dict(x=True, w=True, y=True, bias=c["bias"], rowadd=c["rowadd"], residual=c["residual"], preact=c["preact"], dact_u=c["dact"] is not None)
    for n, on in use.items():
        setattr(d, n, ptrs[n] if on else None)
    d.ws, d.ws_bytes = (ws or None), ws_bytes
    return d


FAKE_PTRS = {n: 0x10000 * (i + 1) for i, n in enumerate(("x", "w", "y", "bias", "rowadd", "residual", "preact", "dact_u"))}


@contextlib.contextmanager
def settings(lib, c):
    """The library settings of a case, restored to the defaults afterwards whatever happens."""
    try:
        assert lib.psg_conv_set_tile(c["tile"]) == 0 and lib.psg_conv_set_tapclass(c["tapcls"]) == 0 and lib.psg_conv_set_pw(c["pw"]) == 0
        assert lib.psg_set_available_cus(0 if c["cus"] == 256 else c["cus"]) == 0 and lib.psg_set_reserve_rounds(0) == 0
        yield
    finally:
        lib.psg_conv_set_tile(-1)
        lib.psg_conv_set_tapclass(1)
        lib.psg_conv_set_pw(1)
        lib.psg_set_available_cus(0)
        lib.psg_set_reserve_rounds(0)


def route_of(lib, d):
    """psg_conv_route -> (return code, tuple of launches, each a tuple of the NF fields)."""
    out = (ctypes.c_int32 * (1 + 4 * NF))()
    rc = lib.psg_conv_route(ctypes.byref(d), ctypes.cast(out, ctypes.c_void_p))
    if rc:
        return rc, ()
    return 0, tuple(tuple(out[1 + i * NF: 1 + (i + 1) * NF]) for i in range(out[0]))


def ws_for(lib, c, ptrs=FAKE_PTRS, ws_ptr=0x900000):
    """(ws pointer, bytes) a case offers: "ok" what psg_conv_fwd_workspace_bytes asks for, "small" 16 bytes less, "none" nothing,
    "big" 1 MiB whatever the plan asks for.
    Call inside settings()."""
    if c["ws"] == "none":
        return 0, 0
    if c["ws"] == "big":                                   # (a pinned tile: the plan asks for nothing and must not split)
        return ws_ptr, 1 << 20
    lib.psg_conv_set_tile(-1)                              # what the unpinned plan would ask for
    need = int(lib.psg_conv_fwd_workspace_bytes(ctypes.byref(make_desc(c, ptrs))))
    lib.psg_conv_set_tile(c["tile"])
    assert need > 0, f"{c['name']}: the plan does not split this launch - the case offers a workspace for nothing"
    return ws_ptr, need if c["ws"] == "ok" else need - 16


def query_route(lib, c):
    """The library's route of a case, under its settings and workspace state (host only)."""
    with settings(lib, c):
        ws, nb = ws_for(lib, c)
        return route_of(lib, make_desc(c, FAKE_PTRS, ws, nb))


_routes = None


def expected_route(name):
    global _routes
    if _routes is None:
        with open(ROUTES_JSON) as f:
            _routes = {k: tuple(tuple(l) for l in v) for k, v in json.load(f).items()}
    return _routes[name]


def epi_form(c, launch):
    """The epilogue a launch runs - a restatement of the rule in csrc/conv_gemm_kernel.h (the `ek` choice and the staging
    sub-paths at the end of the staged epilogue) and of csrc/conv_pw.hip's pw_kind: "split" (the finishing kernel's conv_emit),
    "f32", "direct" (bf16 without LDS staging), "pw:<EK>" or "lds:<EK>:<stage_aux | stage_both | two_pass>"."""
    L = dict(zip(ROUTE_FIELDS, launch))
    if L["splits"] > 1:
        return "split"
    if c["dtype"] == "f32":
        return "f32"
    if not L["epi_lds"]:
        return "direct"
    ek = "GENERIC"
    if not c["generic"]:
        if c["dact"] is not None:
            if c["dact"] == "mul" and not c["drop_p"] > 0:
                ek = "DMUL"
        elif c["act"] == "none":
            ek = "DROP" if c["drop_p"] > 0 else "PLAIN"
        elif c["act"] == "gelu":
            ek = "GELU_DROP" if c["drop_p"] > 0 else "GELU"
    if L["pw"]:
        return "pw:" + ek
    if L["mode"] == 3:
        ek = "GENERIC"
    aux = c["residual"] or c["dact"] is not None
    WM, WN = L["BM"] // 2, L["BN"] // 2
    NB, CPRW = WM // 16, WN // 8
    NIT = -(-(WM * CPRW) // 64)
    if NB % 2 == 0 and ek != "GENERIC" and L["mode"] != 3 and NIT % 2 == 0 and ((WM // 2) * CPRW) % 64 == 0 and aux and not c["preact"]:
        return f"lds:{ek}:stage_aux"
    if NB % 2 == 0 and L["BN"] != 160 and L["mode"] != 3 and c["preact"] and not aux:
        return f"lds:{ek}:stage_both"
    return f"lds:{ek}:two_pass"


def route_key(dname, launch):
    """What the reachability sweep collects: (dtype, BM, BN, mode, split, tapcls, pw, epi_lds)."""
    L = dict(zip(ROUTE_FIELDS, launch))
    return (dname, L["BM"], L["BN"], L["mode"], int(L["splits"] > 1), L["tapcls"], L["pw"], L["epi_lds"])


# ------------------------------------------------------------------------------------------------------------- operands
def _q(t, dtype):
    return t.to(dtype).float()


def operands(c):
    """CPU fp32 tensors holding exactly the values the launch reads (representable in the case's dtype; bias fp32):
    x [B, Hi, Wi, Cin]; wl, the logical conv weight - [Cout, Cin, ks, ks] for a forward launch, [Cin, Cout, ks, ks] (O, I of the
    conv whose data gradient this is) for tr = 1; bias [Cout]; rowadd [B, Cout]; residual, dact [M, Cout].  Means well away
    from zero: a missing tap or slice moves a result by a whole term, not by a fluctuation.  Not so under ReLU and tanh: there
    the weights and the bias are zero-mean, so that the pre-activation u straddles zero at any K and on border pixels alike
    (standard deviation ~0.5: about half the elements on either side of ReLU's kink, |u| mostly below 1.5 for tanh) - a ReLU
    that clamps nothing, a saved derivative of constant 1 or a saturated tanh would otherwise pass
    (tests/test_conv_ref_cpu.py asserts the fractions).  Nor under quick-GELU: for |u| of a few tenths to 2 it lies visibly
    off GELU-erf and off SiLU, further out all three are u or 0 (tests/test_conv_ref_cpu.py swaps them and must see it)."""
    g = geom(c)
    dt = DTYPES[c["dtype"]]
    t = "cv." + c["name"]
    N, M = c["Cout"], g["M"]
    o = dict(x=_q(0.3 + 0.8 * h((c["B"], g["Hi"], g["Wi"], c["Cin"]), t + ".x"), dt))
    wshape = (c["Cin"], N, c["ks"], c["ks"]) if c["tr"] else (N, c["Cin"], c["ks"], c["ks"])
    centred = c["dact"] is None and c["act"] in ("relu", "tanh", "quick_gelu")
    o["wl"] = _q(((0.0 if centred else 0.25) + h(wshape, t + ".w")) * (1.5 / math.sqrt(g["K"])), dt)
    o["bias"] = (0.0 if centred else 0.2) + 0.3 * h((N,), t + ".b") if c["bias"] else None
    o["rowadd"] = _q(0.6 * h((c["B"], N), t + ".ra") - 0.1, dt) if c["rowadd"] else None
    o["residual"] = _q(0.4 + h((M, N), t + ".res"), dt) if c["residual"] else None
    if c["dact"] == "u" and c["act"] == "tanh":
        o["dact"] = _q(1.2 * h((M, N), t + ".u") + 0.1, dt)              # a saved pre-activation, tanh' >= 0.26
    elif c["dact"] == "u":
        o["dact"] = _q(1.7 * h((M, N), t + ".u") + 0.2, dt)              # a saved pre-activation
    elif c["dact"] == "mul":
        o["dact"] = _q(0.55 + 0.6 * h((M, N), t + ".d"), dt)             # a saved derivative
    else:
        o["dact"] = None
    return o


def gemm_K(c):
    return geom(c)["K"]


def reference(c, o):
    """fp64 reference of a launch on the operands `o`: name -> (ref [M, N], S, extra, r_extra) for "y" and, with preact,
    "preact", plus "keep" ([M, N] bool or None, from the integer restatement: index m * Cout + n, m the row of y) and "u"."""
    g = geom(c)
    M, N = g["M"], c["Cout"]
    if c["tr"]:
        acc, S = R.conv_dgrad(o["x"], o["wl"], (c["H"], c["W"]), c["stride"], c["pad"])
    else:
        acc, S = R.conv_fwd(o["x"], o["wl"], c["stride"], c["pad"])
    p = float(np.float32(c["drop_p"]))
    keep = R.conv_keep_mask(drop_seed(c), M, N, c["drop_p"]) if c["drop_p"] > 0 else None
    out = {"keep": keep}
    B = c["B"]
    sh = lambda t: None if t is None else t.reshape(acc.shape)
    if c["dact"] is None:
        u, Su, _ = R.epilogue(acc, S, bias=o["bias"], rowadd=o["rowadd"])
        y, Sy, A = R.epilogue(acc, S, bias=o["bias"], rowadd=o["rowadd"], residual=sh(o["residual"]), kind=c["act"], alpha=c["alpha"],
                              keep=sh(keep), p=p)
        out["y"] = (y.reshape(M, N), Sy.reshape(M, N), A.reshape(M, N), 0.0)
        if c["preact"]:
            if c["save_dact"]:
                d, Sd, Ad = R.saved_dact(u, Su, c["act"], keep=sh(keep), p=p)
                out["preact"] = (d.reshape(M, N), Sd.reshape(M, N), Ad.reshape(M, N), 0.0)
            else:
                out["preact"] = (u.reshape(M, N), Su.reshape(M, N), None, 0.0)
    else:
        u, Su, _ = R.epilogue(acc, S, bias=o["bias"], rowadd=o["rowadd"])
        if c["dact"] == "mul":
            v, Sv = R.dact_mul(u, Su, sh(o["dact"]))
            rx, A = 0.0, torch.zeros_like(v)
        else:
            v, Sv, rx = R.dact_u(u, Su, sh(o["dact"]), c["act"])
            A = u.abs() * R.ACT_APPROX[c["act"]]
        if keep is not None:
            m = sh(keep).to(torch.float64) / (1.0 - p)
            v, Sv, A = v * m, Sv * m, A * m
        a = c["alpha"]
        out["y"] = ((v * a).reshape(M, N), (Sv * abs(a)).reshape(M, N), (A * abs(a)).reshape(M, N), rx)
        if c["preact"]:
            out["preact"] = (u.reshape(M, N), Su.reshape(M, N), None, 0.0)
    out["u"] = u.reshape(M, N)
    return out


# -------------------------------------------------------------------------------------------------------------- buffers
def alloc(rows, ld, dtype, device="cpu", fill=NAN):
    """A guarded row buffer: GUARD elements, rows x ld, GUARD elements, all `fill`.  Returns (flat buffer, [rows, ld] view)."""
    buf = torch.full((2 * GUARD + rows * ld,), fill, dtype=dtype, device=device)
    return buf, buf[GUARD:GUARD + rows * ld].view(rows, ld)


def verify(c, launches, ref, ybuf, prebuf, what=""):
    """The comparator of both tests.  ybuf / prebuf: (flat, view) of alloc() after the launch (prebuf None without preact).
    Guards and the unwritten columns of strided rows must still be NaN, everything inside must be a number; the dropout zero
    pattern must be the restatement's exactly; every element must lie within gemm_ref.check's bound of its fp64 reference.
    Returns name -> worst err / bound."""
    g = geom(c)
    N, M = c["Cout"], g["M"]
    dt = DTYPES[c["dtype"]]
    tag = f"{what}{c['name']} [{c['dtype']} " + "; ".join(
        "tile %dx%d mode %d splits %d class %d pw %d" % (l[0], l[1], l[2], l[3], l[5], l[6]) for l in launches) + "]"
    worst = {}
    for name, pair in (("y", ybuf), ("preact", prebuf)):
        if pair is None:
            continue
        flat, view = pair
        flat, view = flat.detach().cpu(), view.detach().cpu()
        assert bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[flat.numel() - GUARD:]).all()), f"{tag} {name}: a store outside the buffer (guard)"
        if view.shape[1] > N:
            bad = (~torch.isnan(view[:, N:])).nonzero()
            assert bad.numel() == 0, f"{tag} {name}: a store in the unwritten columns of a strided row, first at (row, col) {tuple(int(v) for v in bad[0] + torch.tensor([0, N]))}"
        inner = view[:, :N]
        bad = torch.isnan(inner).nonzero()
        assert bad.numel() == 0, f"{tag} {name}: {bad.shape[0]} elements never stored (or NaN), first at (m, n) {tuple(int(v) for v in bad[0])}"
        r, S, extra, rx = ref[name]
        if ref["keep"] is not None and (name == "y" and not c["residual"] or name == "preact" and c["save_dact"]):
            # kept elements are nowhere exactly zero in the reference, so the zero pattern IS the mask
            assert bool((r[ref["keep"]] != 0).all()), f"{tag} {name}: the reference has a kept element that is exactly zero - change the inputs"
            gotz = inner == 0
            diff = (gotz != ~ref["keep"]).nonzero()
            assert diff.numel() == 0, (f"{tag} {name}: dropout zero pattern differs from the restatement at {diff.shape[0]} elements, "
                                       f"first (m, n) {tuple(int(v) for v in diff[0])}")
        worst[name] = R.check(inner, r, S, dt, f"{tag} {name}", g["K"], extra=extra, r_extra=rx)
    return worst
