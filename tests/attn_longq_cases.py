"""The case table of the long-query attention backward (psg_attn_bwd_longq, csrc/attention_longq.hip): shapes, layouts and
inputs (test infrastructure, not a conftest; the style of tests/attn_cases.py).  tests/test_attn_longq_ref_cpu.py checks the
restated slab arithmetic against the library and that the table reaches what this docstring claims;
tests/test_attn_longq_gpu.py launches every case.

The kernel walks 64-query tiles in slabs of `tps` tiles and the keys in `nkt` tiles of 32.  Four paths follow:

    nkt == 1, tps == 1   one flush of the registers per workgroup                                  path "k1t1"
    nkt  > 1, tps == 1   one flush per key tile, every one a store                                 path "kNt1"
    nkt == 1, tps  > 1   the registers accumulate over the slab's tiles, one flush                 path "k1tN"
    nkt  > 1, tps  > 1   the slab's later tiles ADD into the workspace partial (flush's !first)    path "kNtN"

tps = ntiles B heads / 1024 (clamped to 1 ... 16), so tps > 1 is reached with many (sample, head) pairs rather than a long
L: B = 4, heads = 171, L >= 129 (3 tiles, tps 2) and B = 3, heads = 171, L >= 257 (5 tiles, tps 2: three slabs, the last of one
tile); "tps3" (B = 3, heads = 205, L = 259) has tps = 3, so a partial is added into twice.  Everywhere else heads = 3 and
B = 2 ... 3, so that a wrong head or sample offset lands in another slice.

Every head_dim 4, 8, 16, 32, 64 (the NG = 8, 4, 2, 1, 1 variants) meets every path in both dtypes: PATH_SHAPES lists ten
(L, S) per path, and head_dim x dtype number j takes entry j, so the edges are spread over the variants:

    L = 1, 63, 64, 65 and 129 / 130 (three slabs at tps = 1; 129: the last tile holds one row) on k1t1 and kNt1;
    L = 129, 191, 192, 193 on k1tN (193: four tiles, the last of one row); L = 257, 259, 319, 320 on kNtN;
    S = 1, 7, 17, 31, 32 on the nkt == 1 paths; S = 33, 45, 64, 65, 97 (last key tile of one key), 256 (8 key tiles) on the
    others; S d < 256 (one partial block of the reduce kernel) and S d > 256 (several) both occur on every path.

The layout of a case follows from its position in the table (layout()), as attn_cases.variations does:

    packed   every operand has row stride heads d and column offset 0
    kv       the product's (ops._AttnLongQFn): k and v are columns 0 and E of one [B, S, 2E] buffer, dk / dv of another
    padded   every operand has a row stride (a multiple of 4) and a column offset of its own
    ptr4     bf16 only: q, k, v, o, dout, dq start 4 elements (8 bytes) into a 16-byte aligned buffer
    odd      dk and dv start at an odd element offset (the contract puts no alignment on them)
"""
import collections

import torch

from tests.attn_ref import C_TORCH
from tests.util import h

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
DTYPE_CODE = {"f32": 0, "bf16": 1}
HEAD_DIMS = (4, 8, 16, 32, 64)
PATHS = ("k1t1", "kNt1", "k1tN", "kNtN")
MODES = {"f32": ("packed", "kv", "padded", "odd"), "bf16": ("packed", "kv", "padded", "ptr4", "odd")}
OPERANDS = ("q", "k", "v", "o", "dout", "dq", "dk", "dv")

# Largest smallest-passing c of torch's fp32 restatement against attn_ref's bounds on THIS table (measured by
# tests/test_attn_longq_ref_cpu.py, never against the kernel; tests/golden/REPORT_attn_longq.txt lists it per output).
C_TORCH_LONGQ = 0.05
# The constant the long-query tests hold the kernel to: the project's factor 4 (a different but fixed summation order) over
# what torch's restatement needs on either table.
C_LONGQ = 4.0 * max(C_TORCH, C_TORCH_LONGQ)

LQ_TQ, LQ_KT, LQ_MAX_TPS, LQ_MAX_S = 64, 32, 16, 256


def lq_tps(B, heads, L):
    """Query tiles per slab (attention_longq.hip, lq_tps)."""
    ntiles = (L + LQ_TQ - 1) // LQ_TQ
    return min(max(ntiles * B * heads // 1024, 1), LQ_MAX_TPS)


def lq_nslab(B, heads, L):
    ntiles, tps = (L + LQ_TQ - 1) // LQ_TQ, lq_tps(B, heads, L)
    return (ntiles + tps - 1) // tps


def lq_nkt(S):
    return (S + LQ_KT - 1) // LQ_KT


# path -> (B, heads) and ten (L, S), one per head_dim x dtype
PATH_BH = {"k1t1": None, "kNt1": None, "k1tN": (4, 171), "kNtN": (3, 171)}        # None: heads = 3, B = 2 + j % 2
PATH_SHAPES = {
    "k1t1": [(1, 1), (63, 31), (64, 32), (65, 7), (129, 32), (1, 32), (63, 1), (64, 31), (65, 32), (130, 17)],
    "kNt1": [(1, 33), (63, 65), (64, 256), (65, 33), (129, 97), (1, 256), (63, 33), (64, 45), (65, 97), (130, 64)],
    "k1tN": [(129, 1), (191, 31), (192, 32), (193, 7), (129, 32), (193, 17), (191, 1), (192, 31), (129, 7), (193, 32)],
    "kNtN": [(257, 33), (259, 65), (320, 33), (319, 45), (259, 64), (257, 65), (320, 45), (259, 33), (319, 65), (257, 64)],
}

Case = collections.namedtuple("Case", "name dname d B heads L S path i")


def _all():
    out = []
    for path in PATHS:
        j = 0
        for d in HEAD_DIMS:
            for dname in ("f32", "bf16"):
                L, S = PATH_SHAPES[path][j]
                B, heads = PATH_BH[path] or (2 + j % 2, 3)
                out.append(Case(f"{path}-{dname}-d{d}-L{L}-S{S}", dname, d, B, heads, L, S, path, len(out)))
                j += 1
    for dname in ("f32", "bf16"):                                    # tps = 3: two adds into one partial
        out.append(Case(f"tps3-{dname}-d8-L259-S33", dname, 8, 3, 205, 259, 33, "kNtN", len(out)))
    return out


CASES = _all()
IDS = [c.name for c in CASES]


def path_of(case):
    """The path the restated slab arithmetic gives a case."""
    return ("k1" if lq_nkt(case.S) == 1 else "kN") + ("t1" if lq_tps(case.B, case.heads, case.L) == 1 else "tN")


def mode_of(case):
    """The layout of a case: cycled over the cases of its dtype, in table order, and shifted by one from path to path (five
    cases of a dtype each), so that a head_dim does not meet the same layout on every path."""
    n = sum(1 for c in CASES[:case.i] if c.dname == case.dname)
    modes = MODES[case.dname]
    return modes[(n + n // len(HEAD_DIMS)) % len(modes)]


def layout(case):
    """(mode, name -> (row stride, column offset) in elements) for q, k, v, o, dout, dq, dk, dv.  In mode "kv" k / v (and
    dk / dv) are the two halves of one buffer of row stride 2 heads d."""
    HD = case.heads * case.d
    mode = mode_of(case)
    if mode == "packed":
        lay = {n: (HD, 0) for n in OPERANDS}
    elif mode == "kv":
        lay = {n: (HD, 0) for n in OPERANDS}
        lay.update(k=(2 * HD, 0), v=(2 * HD, HD), dk=(2 * HD, 0), dv=(2 * HD, HD))
    elif mode == "padded":
        lay = {n: (HD + 4 * k, 4 * ((k + 1) // 2)) for k, n in enumerate(OPERANDS, start=1)}
    elif mode == "ptr4":
        lay = {n: (HD + 8, 4) for n in OPERANDS}
    elif mode == "odd":
        lay = {n: (HD, 0) for n in OPERANDS}
        lay.update(dk=(HD + 4, 1), dv=(HD + 8, 3))
    else:
        raise ValueError(mode)
    return mode, lay


def _q(t, dtype):
    return t.to(dtype).float()


def operands(case):
    """CPU fp32 tensors holding the values the launch of the case reads (representable in its dtype): q, dout [B, L, heads d],
    k, v [B, S, heads d]; scale.  q / k amplitude 2: the scaled scores have a std of about 1.3."""
    dtype = DTYPES[case.dname]
    tag = "attnlq." + case.name
    HD = case.heads * case.d
    B, L, S = case.B, case.L, case.S
    return dict(q=_q(h((B, L, HD), tag + ".q", 2.0), dtype), k=_q(h((B, S, HD), tag + ".k", 2.0), dtype), v=_q(h((B, S, HD), tag + ".v"), dtype),
                dout=_q(h((B, L, HD), tag + ".do"), dtype), scale=float(case.d) ** -0.5)
