"""The case table of the GroupNorm route tests: shapes, launch variations, inputs and the route each launch is expected to
take (test infrastructure, not a conftest).  tests/test_gn_ref_cpu.py checks the stored routes against the library's own
answer (psg_groupnorm_route) and that the table reaches every reachable kernel variant; tests/test_groupnorm_routes_gpu.py
asserts them again before it launches."""
import ctypes

import torch

from tests.util import h

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
DTYPE_CODE = {"f32": 0, "bf16": 1}
CHUNK = {"f32": 4, "bf16": 8}          # elements per 16-byte chunk: row strides and column offsets are multiples of it
ROUTE_FIELDS = ("fused", "N", "R", "grid", "threads", "lds", "lds2", "slabC", "nslab", "PP", "NS", "pps")

# (B, HW, C, G): what the shape is in the table for
SHAPES = [
    (3, 25, 128, 32),      # fp32 forward R4, bf16 forward split (Cg = 4 < 8), bf16 backward N4/R4
    (2, 81, 96, 8),        # R16 / R4 forward; fp32 backward R4 in four slabs; bf16 backward N8/R4 with dres
    (3, 49, 160, 16),      # Cg = 10 straddles chunks; backward grid 12, not a multiple of the 8 XCDs
    (3, 196, 80, 8),       # HW / PP exact at r = 8; bf16 backward N8/R8 with dres
    (2, 9, 384, 32),       # PP = 2
    (3, 9, 640, 32),       # PP = 1 (fp32 forward), 640-wide slab
    (2, 729, 40, 4),       # ragged tail (r = 15 of 16); 460 threads backward; N8/R8 with 33 KB LDS
    (2, 400, 640, 32),     # r = 16 exactly; 500 threads backward
    (3, 100, 1280, 64),    # G = 64, 64 slabs
    (3, 49, 24, 1),        # G = 1, C below 32
    (2, 1, 64, 8),         # HW = 1: workgroups of 8-32 lanes; the variance is across channels only
    (2, 1089, 32, 32),     # Cg = 1: split in both directions and dtypes; ragged last split
    (3, 1089, 32, 8),      # bf16 forward split NS = 5, all else fused with slabC 4
    (5, 2000, 64, 32),     # Cg = 2: split NS 16 forward, bf16 backward split, fp32 backward fused slabC 2
    (3, 729, 640, 32),     # fp32 backward split, PP = 1, 160 threads
    (2, 729, 1280, 32),    # backward split, PP = 1, 320 threads, one channel-loop trip
    (2, 2916, 256, 32),    # backward split NS 16 in both dtypes
    (40, 9, 64, 8),        # B > 32: the second trip of the parameter reduction's row loop
]

# Launch variations.  Every case runs twice per dtype: variant 0 with the flags below, variant 1 with every flag inverted,
# so each route of the table meets both values of each flag; `silu` and `dres` agree in some cases and differ in others so
# that every (SiLU, dres) combination of a backward kernel family is reached (checked by test_gn_ref_cpu.py).
#   silu | dres present | accumulate (non-trivial prefill) | strided (five distinct row strides, offset base) | eps 1e-5 (else 1e-6)
FLAGS = {
    (3, 25, 128, 32): (1, 1, 0, 1, 1), (2, 81, 96, 8): (1, 1, 1, 0, 0), (3, 49, 160, 16): (0, 0, 1, 1, 0),
    (3, 196, 80, 8): (1, 0, 0, 1, 1), (2, 9, 384, 32): (0, 1, 1, 0, 1), (3, 9, 640, 32): (1, 0, 1, 1, 0),
    (2, 729, 40, 4): (1, 1, 0, 0, 1), (2, 400, 640, 32): (0, 1, 1, 1, 1), (3, 100, 1280, 64): (0, 1, 0, 1, 0),
    (3, 49, 24, 1): (0, 1, 0, 0, 1), (2, 1, 64, 8): (1, 1, 1, 1, 0), (2, 1089, 32, 32): (1, 0, 0, 1, 1),
    (3, 1089, 32, 8): (0, 0, 1, 0, 0), (5, 2000, 64, 32): (0, 1, 1, 1, 1), (3, 729, 640, 32): (1, 1, 0, 1, 0),
    (2, 729, 1280, 32): (0, 1, 1, 0, 1), (2, 2916, 256, 32): (1, 1, 1, 1, 0), (40, 9, 64, 8): (1, 0, 0, 0, 1),
}
# x = 4 + 0.75 u instead of 0.4 + 1.3 u (|mu| / sigma ~ 9): one case that is fused in every launch, and one whose forward is
# split in both dtypes (NS 16, as the VAE decoder runs it) and whose bf16 backward is split too.  On the split forward y
# inherits the cancellation of rstd = 1 / sqrt(E[x^2] - mu^2 + eps), which its bound has no term for: the sums must be
# good enough for y as well.
SHIFTED = {(3, 196, 80, 8), (5, 2000, 64, 32)}
# an extra forward launch with sample 1 constant (var = 0): one fused forward, one split
CONST_SAMPLE = {(3, 49, 160, 16), (2, 1089, 32, 32)}

# Expected routes per dtype: (forward, backward without dres, backward with dres), fields in ROUTE_FIELDS order
ROUTES = {
    (3, 25, 128, 32): {
        "f32": ((1, 4, 4, 3, 256, 5888, 0, 128, 1, 8, 0, 0),
                 (1, 2, 8, 3, 256, 8704, 0, 128, 1, 4, 0, 0),
                 (1, 2, 8, 3, 256, 8704, 0, 128, 1, 4, 0, 0)),
        "bf16": ((0, 8, 0, 3, 256, 16384, 256, 0, 0, 16, 1, 25),
                  (1, 4, 4, 3, 256, 12800, 0, 128, 1, 8, 0, 0),
                  (1, 4, 4, 3, 256, 12800, 0, 128, 1, 8, 0, 0)),
    },
    (2, 81, 96, 8): {
        "f32": ((1, 4, 16, 2, 240, 5248, 0, 96, 1, 10, 0, 0),
                 (1, 2, 4, 8, 252, 6464, 0, 24, 4, 21, 0, 0),
                 (1, 2, 4, 8, 252, 6464, 0, 24, 4, 21, 0, 0)),
        "bf16": ((1, 8, 4, 2, 252, 9520, 0, 96, 1, 21, 0, 0),
                  (1, 4, 4, 4, 252, 10912, 0, 48, 2, 21, 0, 0),
                  (1, 8, 4, 2, 252, 19808, 0, 96, 1, 21, 0, 0)),
    },
    (3, 49, 160, 16): {
        "f32": ((1, 4, 16, 3, 240, 5568, 0, 160, 1, 6, 0, 0),
                 (1, 2, 8, 12, 240, 6464, 0, 40, 4, 12, 0, 0),
                 (1, 2, 8, 12, 240, 6464, 0, 40, 4, 12, 0, 0)),
        "bf16": ((1, 8, 8, 3, 240, 9408, 0, 160, 1, 12, 0, 0),
                  (1, 4, 8, 6, 240, 11008, 0, 80, 2, 12, 0, 0),
                  (1, 4, 8, 6, 240, 11008, 0, 80, 2, 12, 0, 0)),
    },
    (3, 196, 80, 8): {
        "f32": ((1, 4, 8, 6, 250, 5192, 0, 40, 2, 25, 0, 0),
                 (1, 2, 8, 12, 250, 6352, 0, 20, 4, 25, 0, 0),
                 (1, 2, 8, 12, 250, 6352, 0, 20, 4, 25, 0, 0)),
        "bf16": ((1, 8, 8, 3, 250, 9384, 0, 80, 1, 25, 0, 0),
                  (1, 4, 8, 6, 250, 10704, 0, 40, 2, 25, 0, 0),
                  (1, 8, 8, 3, 250, 19408, 0, 80, 1, 25, 0, 0)),
    },
    (2, 9, 384, 32): {
        "f32": ((1, 4, 8, 2, 192, 6400, 0, 384, 1, 2, 0, 0),
                 (1, 2, 8, 4, 192, 7936, 0, 192, 2, 2, 0, 0),
                 (1, 2, 8, 4, 192, 7936, 0, 192, 2, 2, 0, 0)),
        "bf16": ((1, 8, 4, 2, 240, 11008, 0, 384, 1, 5, 0, 0),
                  (1, 4, 8, 2, 192, 15872, 0, 384, 1, 2, 0, 0),
                  (1, 4, 8, 2, 192, 15872, 0, 384, 1, 2, 0, 0)),
    },
    (3, 9, 640, 32): {
        "f32": ((1, 4, 16, 3, 160, 7936, 0, 640, 1, 1, 0, 0),
                 (1, 2, 4, 12, 240, 8448, 0, 160, 4, 3, 0, 0),
                 (1, 2, 4, 12, 240, 8448, 0, 160, 4, 3, 0, 0)),
        "bf16": ((1, 8, 4, 3, 240, 13056, 0, 640, 1, 3, 0, 0),
                  (1, 4, 4, 6, 240, 15616, 0, 320, 2, 3, 0, 0),
                  (1, 4, 4, 6, 240, 15616, 0, 320, 2, 3, 0, 0)),
    },
    (2, 729, 40, 4): {
        "f32": ((1, 4, 16, 4, 255, 5196, 0, 20, 2, 51, 0, 0),
                 (1, 2, 8, 8, 460, 11216, 0, 10, 4, 92, 0, 0),
                 (1, 2, 8, 8, 460, 11216, 0, 10, 4, 92, 0, 0)),
        "bf16": ((1, 8, 16, 2, 255, 9372, 0, 40, 1, 51, 0, 0),
                  (1, 4, 8, 4, 460, 18752, 0, 20, 2, 92, 0, 0),
                  (1, 8, 8, 2, 460, 33824, 0, 40, 1, 92, 0, 0)),
    },
    (2, 400, 640, 32): {
        "f32": ((1, 4, 16, 32, 250, 5176, 0, 40, 16, 25, 0, 0),
                 (1, 2, 8, 64, 500, 12336, 0, 20, 32, 50, 0, 0),
                 (1, 2, 8, 64, 500, 12336, 0, 20, 32, 50, 0, 0)),
        "bf16": ((1, 8, 16, 16, 250, 9352, 0, 80, 8, 25, 0, 0),
                  (1, 4, 8, 64, 255, 10536, 0, 20, 32, 51, 0, 0),
                  (1, 8, 8, 32, 255, 19032, 0, 40, 16, 51, 0, 0)),
    },
    (3, 100, 1280, 64): {
        "f32": ((1, 4, 16, 48, 240, 5152, 0, 80, 16, 12, 0, 0),
                 (1, 2, 4, 192, 250, 6336, 0, 20, 64, 25, 0, 0),
                 (1, 2, 4, 192, 250, 6336, 0, 20, 64, 25, 0, 0)),
        "bf16": ((1, 8, 16, 24, 240, 9344, 0, 160, 8, 12, 0, 0),
                  (1, 4, 4, 96, 250, 10672, 0, 40, 32, 25, 0, 0),
                  (1, 8, 4, 48, 250, 19344, 0, 80, 16, 25, 0, 0)),
    },
    (3, 49, 24, 1): {
        "f32": ((1, 4, 4, 3, 252, 5144, 0, 24, 1, 42, 0, 0),
                 (1, 2, 4, 3, 252, 6448, 0, 24, 1, 21, 0, 0),
                 (1, 2, 4, 3, 252, 6448, 0, 24, 1, 21, 0, 0)),
        "bf16": ((1, 8, 4, 3, 147, 5396, 0, 24, 1, 49, 0, 0),
                  (1, 4, 4, 3, 252, 10480, 0, 24, 1, 42, 0, 0),
                  (1, 4, 4, 3, 252, 10480, 0, 24, 1, 42, 0, 0)),
    },
    (2, 1, 64, 8): {
        "f32": ((1, 4, 4, 2, 16, 832, 0, 64, 1, 1, 0, 0),
                 (1, 2, 4, 2, 32, 2176, 0, 64, 1, 1, 0, 0),
                 (1, 2, 4, 2, 32, 2176, 0, 64, 1, 1, 0, 0)),
        "bf16": ((1, 8, 4, 2, 8, 832, 0, 64, 1, 1, 0, 0),
                  (1, 4, 4, 2, 16, 2176, 0, 64, 1, 1, 0, 0),
                  (1, 4, 4, 2, 16, 2176, 0, 64, 1, 1, 0, 0)),
    },
    (2, 1089, 32, 32): {
        "f32": ((0, 4, 0, 18, 256, 8192, 256, 0, 0, 32, 9, 121),
                 (0, 4, 0, 18, 256, 8192, 512, 0, 0, 32, 9, 121),
                 (0, 4, 0, 18, 256, 8192, 512, 0, 0, 32, 9, 121)),
        "bf16": ((0, 8, 0, 10, 256, 16384, 256, 0, 0, 64, 5, 218),
                  (0, 8, 0, 10, 256, 16384, 512, 0, 0, 64, 5, 218),
                  (0, 8, 0, 10, 256, 16384, 512, 0, 0, 64, 5, 218)),
    },
    (3, 1089, 32, 8): {
        "f32": ((1, 4, 16, 12, 256, 5168, 0, 8, 4, 128, 0, 0),
                 (1, 2, 8, 24, 274, 6656, 0, 4, 8, 137, 0, 0),
                 (1, 2, 8, 24, 274, 6656, 0, 4, 8, 137, 0, 0)),
        "bf16": ((0, 8, 0, 15, 256, 16384, 64, 0, 0, 64, 5, 218),
                  (1, 4, 8, 24, 256, 10320, 0, 4, 8, 256, 0, 0),
                  (1, 4, 8, 24, 256, 10320, 0, 4, 8, 256, 0, 0)),
    },
    (5, 2000, 64, 32): {
        "f32": ((0, 4, 0, 80, 256, 8192, 256, 0, 0, 16, 16, 125),
                 (1, 2, 8, 160, 256, 6192, 0, 2, 32, 256, 0, 0),
                 (1, 2, 8, 160, 256, 6192, 0, 2, 32, 256, 0, 0)),
        "bf16": ((0, 8, 0, 80, 256, 16384, 256, 0, 0, 32, 16, 125),
                  (0, 8, 0, 80, 256, 16384, 768, 0, 0, 32, 16, 125),
                  (0, 8, 0, 80, 256, 16384, 768, 0, 0, 32, 16, 125)),
    },
    (3, 729, 640, 32): {
        "f32": ((1, 4, 16, 96, 255, 5188, 0, 20, 32, 51, 0, 0),
                 (0, 4, 0, 48, 160, 5120, 5376, 0, 0, 1, 16, 46),
                 (0, 4, 0, 48, 160, 5120, 5376, 0, 0, 1, 16, 46)),
        "bf16": ((1, 8, 16, 48, 255, 9356, 0, 40, 16, 51, 0, 0),
                  (1, 4, 8, 96, 460, 18736, 0, 20, 32, 92, 0, 0),
                  (1, 8, 8, 48, 460, 33792, 0, 40, 16, 92, 0, 0)),
    },
    (2, 729, 1280, 32): {
        "f32": ((1, 4, 16, 64, 460, 9368, 0, 40, 32, 46, 0, 0),
                 (0, 4, 0, 32, 320, 10240, 10496, 0, 0, 1, 16, 46),
                 (0, 4, 0, 32, 320, 10240, 10496, 0, 0, 1, 16, 46)),
        "bf16": ((1, 8, 16, 64, 255, 9348, 0, 40, 32, 51, 0, 0),
                  (0, 8, 0, 32, 160, 10240, 10496, 0, 0, 1, 16, 46),
                  (0, 8, 0, 32, 160, 10240, 10496, 0, 0, 1, 16, 46)),
    },
    (2, 2916, 256, 32): {
        "f32": ((1, 4, 16, 64, 366, 7360, 0, 8, 32, 183, 0, 0),
                 (0, 4, 0, 32, 256, 8192, 2304, 0, 0, 4, 16, 183),
                 (0, 4, 0, 32, 256, 8192, 2304, 0, 0, 4, 16, 183)),
        "bf16": ((1, 8, 16, 64, 256, 9256, 0, 8, 32, 256, 0, 0),
                  (0, 8, 0, 32, 256, 16384, 2304, 0, 0, 8, 16, 183),
                  (0, 8, 0, 32, 256, 16384, 2304, 0, 0, 8, 16, 183)),
    },
    (40, 9, 64, 8): {
        "f32": ((1, 4, 4, 40, 144, 3200, 0, 64, 1, 9, 0, 0),
                 (1, 2, 4, 40, 256, 7296, 0, 64, 1, 8, 0, 0),
                 (1, 2, 4, 40, 256, 7296, 0, 64, 1, 8, 0, 0)),
        "bf16": ((1, 8, 4, 40, 72, 2912, 0, 64, 1, 9, 0, 0),
                  (1, 4, 4, 40, 144, 6912, 0, 64, 1, 9, 0, 0),
                  (1, 4, 4, 40, 144, 6912, 0, 64, 1, 9, 0, 0)),
    },
}


def variants(shape):
    """The two launch variations of a case: dicts silu, dres, accumulate, strided, eps."""
    s, r, a, t, e = FLAGS[shape]
    out = []
    for inv in (0, 1):
        f = [bool(v ^ inv) for v in (s, r, a, t, e)]
        out.append(dict(silu=f[0], dres=f[1], accumulate=f[2], strided=f[3], eps=1e-5 if f[4] else 1e-6))
    return out


def extra_forwards(shape):
    """The extra forward-only launches of a case: "const" (see CONST_SAMPLE)."""
    return ["const"] if shape in CONST_SAMPLE else []


def case_ids():
    return [("x".join(str(v) for v in s), s) for s in SHAPES]


def expected_route(shape, dname, backward, dres):
    return ROUTES[shape][dname][(1 + int(bool(dres))) if backward else 0]


def query_route(lib, backward, dname, B, HW, C, G, dres):
    """psg_groupnorm_route -> (return code, tuple of the 12 fields)."""
    out = (ctypes.c_int32 * 12)()
    rc = lib.psg_groupnorm_route(int(backward), DTYPE_CODE[dname], B, HW, C, G, int(bool(dres)), ctypes.cast(out, ctypes.c_void_p))
    return rc, tuple(out)


def _q(t, dtype):
    return t.to(dtype).float()


def operands(shape, dname, extra=None):
    """CPU fp32 tensors holding the values the launch of this dtype reads: x, dy, dres [B, HW, C] (representable in the dtype),
    gamma, beta, and the accumulate prefill (dgamma0, dbeta0), all fp32.  extra: None, or the input of an extra forward
    launch: "const" (sample 1 constant)."""
    B, HW, C, G = shape
    dtype = DTYPES[dname]
    tag = "gnr." + "x".join(str(v) for v in shape)
    u = h((B, HW, C), tag + ".x")
    x = 4.0 + 0.75 * u if shape in SHIFTED else 0.4 + 1.3 * u
    if extra == "const":
        x[1] = 0.75
    return dict(x=_q(x, dtype), dy=_q(h((B, HW, C), tag + ".dy"), dtype), dres=_q(h((B, HW, C), tag + ".dres", 0.7), dtype),
                gamma=1.0 + h((C,), tag + ".g", 0.3), beta=h((C,), tag + ".b", 0.2),
                prefill=(h((C,), tag + ".pg", 3.0), h((C,), tag + ".pb", 3.0)))


def strides(shape, dname, strided):
    """name -> (row stride, column offset) of x, y, dy, dres, dx: C + k N and an offset of whole chunks, k = 1..5, or (C, 0)."""
    C, N = shape[2], CHUNK[dname]
    names = ("x", "y", "dy", "dres", "dx")
    if not strided:
        return {n: (C, 0) for n in names}
    return {n: (C + k * N, N * ((k + 1) // 2)) for k, n in enumerate(names, start=1)}
