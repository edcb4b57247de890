"""The case tables of the row-kernel tests (upsample, colsum, sum_rows, prep_weight, epilogue_bwd, dropout_apply): shapes,
layouts, inputs, and the route or plan each launch is expected to take (test infrastructure, not a conftest).
tests/test_row_ref_cpu.py checks the stored routes and plans against the library's host-only answers and a restatement;
tests/test_row_kernels_gpu.py asserts them again before it launches."""
import ctypes

import numpy as np
import torch

from tests.util import h

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
DTYPE_CODE = {"f32": 0, "bf16": 1}
CHUNK = {"f32": 4, "bf16": 8}          # elements per 16-byte chunk
GUARD = 64                             # guard elements before and after every buffer (128 / 256 bytes: pointers stay 16-byte aligned)


def q(t, dname):
    """fp32 values representable in the dtype."""
    return t.to(DTYPES[dname]).float()


# ------------------------------------------------------------------------------------------------------------- upsample
UP_B = 2
# ((Hi, Wi), (Ho, Wo), Wo <= 3 Wi: the 8-channel backward may take it): why
UP_GEOMS = [
    ((3, 5), (6, 9), True),        # non-square, a different ratio per axis
    ((4, 4), (7, 7), True),        # non-integer ratio
    ((5, 5), (9, 9), True),        # 2n - 1, the form of 108 -> 215
    ((2, 3), (6, 9), True),        # exactly 3x: the 8-channel backward's limit, 6 contributing columns
    ((2, 2), (7, 8), False),       # more than 3x in W only: forward 8-channel, backward generic
    ((1, 1), (4, 4), False),       # a single input pixel: i1 clamps onto i0
    ((3, 3), (3, 3), True),        # identity
    ((7, 7), (28, 28), False),     # 8 contributors per input column
    ((2, 12), (6, 12), True),      # ratios 3 and 1: a backward window taken from the other axis loses contributors (its slack
                                   # of one index hides that at (3,5) -> (6,9)); the 8-channel backward still takes it
]
# name: (dtype, C, (ld, column offset) of the operand read, (ld, offset) of the operand written, 8-channel layout)
UP_LAYOUTS = {
    "bf16-c8": ("bf16", 8, (8, 0), (8, 0), True),
    "bf16-c16": ("bf16", 16, (16, 0), (16, 0), True),
    "bf16-c24-slot": ("bf16", 24, (40, 8), (32, 0), True),        # a view of a concat buffer; the padding must stay intact
    "bf16-c12": ("bf16", 12, (12, 0), (12, 0), False),            # C % 8
    "bf16-c8-ld12": ("bf16", 8, (12, 0), (12, 0), False),         # ld % 8
    "bf16-c8-off4": ("bf16", 8, (16, 4), (16, 4), False),         # pointers 8-byte but not 16-byte aligned
    "f32-c4": ("f32", 4, (4, 0), (4, 0), False),
    "f32-c12": ("f32", 12, (12, 0), (12, 0), False),
    "f32-c4-strided": ("f32", 4, (12, 4), (8, 0), False),
    "f32-c12-strided": ("f32", 12, (20, 4), (16, 4), False),
}
# the generic kernels' grid is capped at 8192 blocks of 256 lanes: 2.98 M four-channel items make every lane loop
UP_GRID_STRIDE = dict(dtype="f32", B=4, Hi=54, Wi=54, Ho=108, Wo=108, C=256)


def up_expected_route(layout, geom, backward):
    return int(UP_LAYOUTS[layout][4] and (not backward or geom[2]))


def up_ids():
    return [f"{hi}x{wi}-{ho}x{wo}" for (hi, wi), (ho, wo), _ in UP_GEOMS]


def up_operands(layout, geom, B=UP_B):
    """x [B, Hi, Wi, C] and dy [B, Ho, Wo, C], fp32 values representable in the layout's dtype, in about [-1.5, 1.5]."""
    dname, C = UP_LAYOUTS[layout][:2]
    (Hi, Wi), (Ho, Wo), _ = geom
    tag = f"row.up.{Hi}.{Wi}.{Ho}.{Wo}.{C}"
    return q(h((B, Hi, Wi, C), tag + ".x", 1.5), dname), q(h((B, Ho, Wo, C), tag + ".dy", 1.5), dname)


def query_upsample_route(lib, backward, dname, rd, ldrd, wr, ldwr, B, Hi, Wi, Ho, Wo, C):
    """psg_upsample_route -> (return code, out[0]); rd / wr: addresses."""
    out = (ctypes.c_int32 * 1)(-1)
    rc = lib.psg_upsample_route(int(backward), DTYPE_CODE[dname], ctypes.c_void_p(rd), ldrd, ctypes.c_void_p(wr), ldwr, B, Hi, Wi, Ho, Wo, C,
                                ctypes.cast(out, ctypes.c_void_p))
    return rc, out[0]


# --------------------------------------------------------------------------------------------------------------- colsum
# (R, groups, cols, lda, (splits, rows per split, rows of the last split)): what the row is meant to hit.  The plans were
# computed from colsum_plan; they are asserted against psg_colsum_workspace_bytes and a restatement, so a plan change is a diff.
COLSUM = [
    (1, 1, 8, 8, (1, 1, 1)),               # a single row, three idle row lanes
    (3, 2, 65, 72, (1, 3, 3)),             # groups > 1, a second column block of one column
    (17, 1, 4, 4, (1, 17, 17)),            # the first row past the 16-row unroll
    (64, 1, 72, 80, (1, 64, 64)),          # the last single-pass R
    (65, 1, 72, 80, (2, 33, 32)),          # the first two-stage R
    (130, 3, 100, 104, (3, 44, 42)),
    (729, 40, 128, 128, (12, 61, 58)),     # the rowadd gradient
    (70, 300, 449, 456, (1, 70, 70)),      # groups * column blocks > 2048: one pass although R > 64
    (4097, 1, 1, 8, (65, 64, 1)),          # a last split of one row
    (16500, 1, 8, 8, (254, 65, 55)),       # the 256 cap
]
COLSUM_BF16_OUT_MAX_R = 729                # the package uses a bf16 output only with R = Ho * Wo <= 729
COLSUM_ACCUMULATE = {3, 130, 70}           # rows (by R) that also run accumulate = 1 onto a non-zero fp32 out
COLSUM_LD_OUT = {3: 72, 65: 80}            # rows (by R) that also run with ld_out > cols


def colsum_variants():
    """(R, groups, cols, lda, plan, in dtype, out dtype, accumulate, ld_out) of every launch."""
    out = []
    for R, groups, cols, lda, plan in COLSUM:
        combos = [("bf16", "f32"), ("f32", "f32")] + ([("bf16", "bf16")] if R <= COLSUM_BF16_OUT_MAX_R else [])
        for di, do in combos:
            out.append((R, groups, cols, lda, plan, di, do, 0, cols))
            if R in COLSUM_ACCUMULATE and do == "f32":
                out.append((R, groups, cols, lda, plan, di, do, 1, cols))
            if R in COLSUM_LD_OUT:
                out.append((R, groups, cols, lda, plan, di, do, 0, COLSUM_LD_OUT[R]))
    return out


def colsum_id(v):
    R, groups, cols, lda, plan, di, do, acc, ldo = v
    return f"R{R}-g{groups}-c{cols}-{di}-{do}" + ("-acc" if acc else "") + (f"-ldo{ldo}" if ldo != cols else "")


def colsum_operands(R, groups, cols, dname, extra_groups=0):
    """a [groups (+ extra), R, cols]: magnitudes in [0.5, 1) with a hashed sign, so that every single row matters; prev
    [groups, cols]: the non-zero fp32 output an accumulating launch adds to."""
    u = h((groups + extra_groups, R, cols), f"row.colsum.{R}.{groups}.{cols}")
    a = torch.where(u >= 0, 0.5 + 0.5 * u, -0.5 + 0.5 * u)
    return q(a, dname), h((groups, cols), f"row.colsum.prev.{R}.{groups}.{cols}", 3.0)


# ------------------------------------------------------------------------------------------------------------- sum_rows
SUM_ROWS = [("bf16", 1, 8), ("bf16", 5, 24), ("bf16", 333, 40), ("bf16", 50, 1280),
            ("f32", 1, 8), ("f32", 5, 24), ("f32", 333, 40), ("f32", 50, 1280), ("f32", 5, 4), ("f32", 5, 12)]
SUM_ROWS_BIG = dict(dtype="bf16", rows=131073, cols=1024)      # 16.78 M chunks: beyond the 65 536-block cap, every lane loops


def sum_rows_layout(dname, cols):
    """(ld, column offset) of a, b, c, and of y: y is the right half of a [rows, C1 + cols] concat buffer."""
    N = CHUNK[dname]
    C1 = 3 * N
    return dict(a=(cols + N, N), b=(cols + 2 * N, 0), c=(cols + 5 * N, 2 * N), y=(C1 + cols, C1))


# -0.0, +inf, -inf, a NaN with a payload, the largest and the smallest subnormal (both signs)
SPECIAL_BITS = {"f32": [0x80000000, 0x7F800000, 0xFF800000, 0x7FC12345, 0x007FFFFF, 0x80000001],
                "bf16": [0x8000, 0x7F80, 0xFF80, 0x7FC5, 0x007F, 0x8001]}


def special_values(dname):
    bits = np.array(SPECIAL_BITS[dname], dtype=np.uint32 if dname == "f32" else np.uint16)
    t = torch.from_numpy(bits.view(np.int32 if dname == "f32" else np.int16).copy())
    return t.view(DTYPES[dname])


def sum_rows_operands(dname, rows, cols):
    tag = f"row.sum.{dname}.{rows}.{cols}"
    dt = DTYPES[dname]
    a, b, c = (h((rows, cols), f"{tag}.{n}", 1.5).to(dt) for n in "abc")
    left = h((rows, sum_rows_layout(dname, cols)["y"][1]), tag + ".left").to(dt)
    return a, b, c, left


# ---------------------------------------------------------------------------------------------------------- prep_weight
PREP_KERNELS = {"generic": 0, "ohwi_f32": 1, "ohwi_bf16": 2, "wd_bf16": 3}      # enum psg_prep_kernel
# (source dtype, source layout, O, I, ksize, target dtypes, kernel of the request "f" (wf only), "d" (wd only), "fd" (both))
_G, _F, _B, _W = "generic", "ohwi_f32", "ohwi_bf16", "wd_bf16"
PREP = (
    [("f32", "oihw", O, I, 3, ("f32", "bf16"), (_G, _G, _G)) for O, I in ((5, 7), (33, 3), (36, 68), (64, 6))]
    + [("f32", "oihw", 33, 3, 1, ("f32", "bf16"), (_G, _G, _G))]
    + [("f32", "ohwi", O, I, ks, ("f32", "bf16"), (_F, _F, _F)) for O, I in ((4, 4), (36, 68), (72, 40)) for ks in (1, 3, 4)]
    + [("f32", "oihw", 36, 68, 1, ("f32", "bf16"), (_F, _F, _F))]
    + [("bf16", "ohwi", 36, 68, ks, ("bf16",), (_B, _B, _B)) for ks in (1, 3)]
    + [("bf16", "ohwi", 72, 40, ks, ("bf16",), (_B, _W, _B)) for ks in (1, 3, 4)]
    + [("bf16", "ohwi", O, I, ks, ("bf16",), (_B, _W, _B)) for O, I in ((8, 8), (136, 64)) for ks in (1, 3, 4)]
)
PREP_REQUESTS = ("f", "d", "fd")


def prep_variants():
    return [(sd, lay, O, I, ks, td, kern) for sd, lay, O, I, ks, tds, kern in PREP for td in tds]


def prep_id(v):
    sd, lay, O, I, ks, td, _ = v
    return f"{sd}-{lay}-{O}x{I}-k{ks}-{td}"


def prep_source(sd, lay, O, I, ks):
    """(logical [O, I, k, k] fp32 values representable in the source dtype, the source tensor in its memory order and dtype)."""
    w = q(h((O, I, ks, ks), f"row.prep.{O}.{I}.{ks}"), sd)
    mem = w.permute(0, 2, 3, 1).contiguous() if lay == "ohwi" else w.contiguous()
    return w, mem.to(DTYPES[sd])


def query_prep_route(lib, w, sd, lay, wf, wd, O, I, ks, td):
    """psg_prep_weight_route -> (return code, out[0]); w, wf, wd: addresses (0: not asked for)."""
    out = (ctypes.c_int32 * 1)(-1)
    rc = lib.psg_prep_weight_route(ctypes.c_void_p(w), DTYPE_CODE[sd], 1 if lay == "ohwi" else 0, ctypes.c_void_p(wf), ctypes.c_void_p(wd),
                                   O, I, ks, DTYPE_CODE[td], ctypes.cast(out, ctypes.c_void_p))
    return rc, out[0]


# -------------------------------------------------------------------------------------------- epilogue_bwd, dropout_apply
EPI_SHAPES = [(3, 4), (77, 36), (300, 256)]
EPI_ACTS = ["none", "silu", "gelu", "relu", "tanh", "quick_gelu"]
EPI_P = (0.0, 0.1)
EPI_ALPHA = (1.0, 0.5)
DROP_P = (0.1, 0.5)
EPI_GRID_STRIDE = (8200, 1024)            # fp32: 2.1 M four-element items > 8192 * 256
GRID_STRIDE_ROWS = 64                     # rows of a grid-stride case that are compared with the reference


def epi_layout(cols):
    """(ld, column offset) of dy, u, g (and x, y of dropout_apply): each its own."""
    return dict(dy=(cols + 4, 4), u=(cols + 8, 0), g=(cols + 12, 8))


def epi_operands(rows, cols, dname):
    """dy with |dy| in [0.25, 1.25) and u with |u| in [0.02, 3): no kept reference element is exactly zero but ReLU's."""
    tag = f"row.epi.{rows}.{cols}"
    d, u = h((rows, cols), tag + ".dy"), h((rows, cols), tag + ".u")
    dy = torch.where(d >= 0, 0.25 + d, -0.25 + d)
    uu = torch.where(u >= 0, 0.02 + 2.98 * u, -0.02 + 2.98 * u)
    return q(dy, dname), q(uu, dname)


def fixed_rows(rows, n=GRID_STRIDE_ROWS):
    """n row indices of a grid-stride case: the first, the last, and an even spread in between."""
    return torch.unique(torch.linspace(0, rows - 1, n).round().long())
