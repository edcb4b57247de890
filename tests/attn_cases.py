"""The case table of the attention route tests: shapes, strides, key lengths, dropout, inputs and the route each launch is
expected to take (test infrastructure, not a conftest).  tests/test_attn_ref_cpu.py checks the stored routes against the
library's own answer (psg_attn_route) and that the table reaches every launch variant any shape of its sweep reaches;
tests/test_attention_routes_gpu.py asserts them again before it launches.

A case is (dtype, head_dim, L, S) plus launch variations that follow from its position in the table (variations()), and runs
all five passes: psg_attn_fwd, psg_attn_bwd, psg_attn_fwd_varlen_train, psg_attn_bwd_varlen and the forward-only
psg_attn_fwd_varlen.  heads = 3 and B = 2 ... 4 (8 where every key length is wanted at once), so that a wrong head or sample
offset lands in another slice.  The expected routes are data: tests/golden/attn_routes.json, one row of
PSG_ATTN_ROUTE_FIELDS numbers per case and pass (tools/attn_routes_report.py --routes rewrites it from the library after a
deliberate routing change)."""
import ctypes
import json
import os

import torch

from tests.util import h

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
DTYPE_CODE = {"f32": 0, "bf16": 1}
HEADS = 3
PASSES = ("fwd", "fwd_varlen", "bwd", "fwd_varlen_train", "bwd_varlen")             # enum AttnPass, in order
FWD, FWD_VARLEN, BWD, FWD_VARLEN_TRAIN, BWD_VARLEN = range(5)
ROUTE_FIELDS = ("family", "ND", "waves", "KW", "QW", "dkv_waves", "qw_cut", "w_cut", "NH", "KV_REG", "lds_fwd", "lds_dq", "lds_dkv",
                "gfx", "gfy", "gqx", "gqy", "gkx", "gky", "varlen")
DROP_P = 0.3

# ---------------------------------------------------------------------------------------------------------------- the table
# (dtype, head_dim, L, S): chosen, smallest first, so that the table reaches every (family, ND, waves, KW, QW, reductions, NH,
# VARLEN) a sweep of L, S = 1 ... 260 reaches; L and S are no multiples of 16 (nor of 32), most S are odd.
GRID = [
    ("bf16", 16, 23, 21), ("bf16", 16, 45, 21), ("bf16", 16, 23, 49), ("bf16", 16, 23, 81), ("bf16", 16, 101, 21), ("bf16", 16, 45, 49),
    ("bf16", 16, 23, 111), ("bf16", 16, 163, 21), ("bf16", 16, 45, 81), ("bf16", 16, 75, 49), ("bf16", 16, 230, 21), ("bf16", 16, 101, 49),
    ("bf16", 16, 45, 111), ("bf16", 16, 75, 81), ("bf16", 16, 163, 49), ("bf16", 16, 101, 81), ("bf16", 16, 75, 111), ("bf16", 16, 101, 111),
    ("bf16", 32, 23, 21), ("bf16", 32, 45, 21), ("bf16", 32, 23, 49), ("bf16", 32, 75, 21), ("bf16", 32, 23, 81), ("bf16", 32, 101, 21),
    ("bf16", 32, 45, 49), ("bf16", 32, 23, 111), ("bf16", 32, 131, 21), ("bf16", 32, 45, 81), ("bf16", 32, 75, 49), ("bf16", 32, 45, 111),
    ("bf16", 32, 75, 81), ("bf16", 32, 101, 81), ("bf16", 32, 75, 111), ("bf16", 32, 101, 111), ("bf16", 64, 23, 21), ("bf16", 64, 45, 21),
    ("bf16", 64, 23, 49), ("bf16", 64, 75, 21), ("bf16", 64, 23, 81), ("bf16", 64, 101, 21), ("bf16", 64, 23, 111), ("bf16", 64, 163, 21),
    ("bf16", 64, 45, 81), ("bf16", 64, 75, 49), ("bf16", 64, 101, 49), ("bf16", 64, 45, 111), ("bf16", 64, 75, 81), ("bf16", 64, 101, 81),
    ("bf16", 64, 75, 111), ("bf16", 64, 101, 111), ("bf16", 80, 23, 21), ("bf16", 80, 45, 21), ("bf16", 80, 23, 49), ("bf16", 80, 75, 21),
    ("bf16", 80, 23, 81), ("bf16", 80, 101, 21), ("bf16", 80, 45, 49), ("bf16", 80, 23, 111), ("bf16", 80, 131, 21), ("bf16", 80, 45, 81),
    ("bf16", 80, 75, 49), ("bf16", 80, 196, 21), ("bf16", 80, 101, 49), ("bf16", 80, 45, 111), ("bf16", 80, 75, 81), ("bf16", 80, 131, 49),
    ("bf16", 80, 101, 81), ("bf16", 80, 75, 111), ("bf16", 80, 101, 111), ("bf16", 160, 23, 21), ("bf16", 160, 45, 21), ("bf16", 160, 23, 49),
    ("bf16", 160, 75, 21), ("bf16", 160, 23, 81), ("bf16", 160, 101, 21), ("bf16", 160, 45, 49), ("bf16", 160, 23, 111), ("bf16", 160, 45, 81),
    ("bf16", 160, 75, 49), ("bf16", 160, 101, 49), ("bf16", 160, 45, 111), ("bf16", 160, 75, 81), ("bf16", 160, 163, 49), ("bf16", 160, 101, 81),
    ("bf16", 160, 75, 111), ("bf16", 160, 101, 111), ("bf16", 320, 23, 21), ("bf16", 320, 45, 21), ("bf16", 320, 23, 49), ("bf16", 320, 23, 81),
    ("bf16", 320, 101, 21), ("bf16", 76, 17, 21), ("bf16", 92, 17, 21), ("bf16", 108, 17, 21), ("bf16", 124, 17, 21), ("bf16", 140, 17, 21),
    ("bf16", 172, 17, 21), ("bf16", 188, 17, 21), ("bf16", 204, 17, 21), ("bf16", 220, 17, 21), ("bf16", 236, 17, 21), ("bf16", 252, 17, 21),
    ("bf16", 268, 17, 21), ("bf16", 284, 17, 21), ("bf16", 300, 17, 21), ("f32", 16, 23, 21), ("f32", 16, 45, 21), ("f32", 16, 23, 49),
    ("f32", 16, 75, 21), ("f32", 16, 23, 81), ("f32", 16, 101, 21), ("f32", 16, 45, 49), ("f32", 16, 23, 111), ("f32", 16, 45, 81),
    ("f32", 16, 75, 49), ("f32", 16, 101, 49), ("f32", 16, 45, 111), ("f32", 16, 75, 81), ("f32", 16, 101, 81), ("f32", 16, 75, 111),
    ("f32", 16, 101, 111), ("f32", 32, 23, 21), ("f32", 32, 45, 21), ("f32", 32, 23, 49), ("f32", 32, 75, 21), ("f32", 32, 23, 81),
    ("f32", 32, 101, 21), ("f32", 32, 45, 49), ("f32", 32, 23, 111), ("f32", 32, 45, 81), ("f32", 32, 75, 49), ("f32", 32, 45, 111),
    ("f32", 32, 75, 81), ("f32", 32, 101, 81), ("f32", 32, 75, 111), ("f32", 32, 101, 111), ("f32", 64, 23, 21), ("f32", 64, 45, 21),
    ("f32", 64, 23, 49), ("f32", 64, 75, 21), ("f32", 64, 23, 81), ("f32", 64, 101, 21), ("f32", 64, 23, 111), ("f32", 64, 45, 81),
    ("f32", 64, 75, 49), ("f32", 64, 101, 49), ("f32", 64, 45, 111), ("f32", 64, 75, 81), ("f32", 64, 101, 81), ("f32", 64, 75, 111),
    ("f32", 64, 101, 111), ("f32", 80, 23, 21), ("f32", 80, 45, 21), ("f32", 80, 23, 49), ("f32", 80, 75, 21), ("f32", 80, 23, 81),
    ("f32", 80, 101, 21), ("f32", 80, 45, 49), ("f32", 80, 23, 111), ("f32", 80, 45, 81), ("f32", 80, 75, 49), ("f32", 80, 230, 21),
    ("f32", 80, 101, 49), ("f32", 80, 45, 111), ("f32", 80, 75, 81), ("f32", 80, 101, 81), ("f32", 80, 75, 111), ("f32", 80, 101, 111),
    ("f32", 160, 23, 21), ("f32", 160, 45, 21), ("f32", 160, 23, 49), ("f32", 160, 75, 21), ("f32", 160, 23, 81), ("f32", 160, 45, 49),
    ("f32", 160, 45, 81), ("f32", 160, 75, 49), ("f32", 60, 17, 21), ("f32", 92, 17, 21), ("f32", 108, 17, 21), ("f32", 124, 17, 21),
    ("f32", 140, 17, 21), ("f32", 172, 17, 21), ("f32", 188, 17, 21), ("f32", 204, 17, 21), ("f32", 220, 17, 21), ("f32", 236, 17, 21),
    ("f32", 252, 17, 21), ("f32", 268, 17, 21), ("f32", 284, 17, 21), ("f32", 300, 17, 21),
]

# Named cases: (name, dtype, head_dim, L, S, overrides of variations()).  Family boundaries come as pairs one step apart.
NAMED = [
    ("b320-S96", "bf16", 320, 40, 96, {}), ("b320-S97", "bf16", 320, 40, 97, {}),                  # forward LDS fit
    ("b320-L64", "bf16", 320, 64, 49, {}), ("b320-L65", "bf16", 320, 65, 49, {}),                  # backward: Q / dO images
    ("b320-S81", "bf16", 320, 33, 81, {"drop": True}),                                             # NH = 2, three key tiles on one wave
    ("b160-L196", "bf16", 160, 196, 49, {}),                                                       # forward-only MFMA, training pair VALU
    ("f160-96", "f32", 160, 96, 96, {}), ("f160-S97", "f32", 160, 96, 97, {}), ("f160-L97", "f32", 160, 97, 96, {}),
    ("b64-ld4", "bf16", 64, 45, 33, {"mode": "ld4"}), ("b64-ld8", "bf16", 64, 45, 33, {"mode": "padded"}),      # row stride 4 mod 8
    ("b64-ptr4", "bf16", 64, 45, 33, {"mode": "ptr4"}),                                            # pointer 8 bytes off
    ("b16-qwcut", "bf16", 16, 80, 32, {"drop": True}),                                             # QW 3 -> 2 by the partial-sum fit
    ("b160-wcut", "bf16", 160, 130, 70, {}),                                                       # waves cut by the private-tile fit
    ("b64-kv8", "bf16", 64, 40, 49, {"B": 8, "kv": 0, "drop": True}), ("f64-kv8", "f32", 64, 40, 49, {"B": 8, "kv": 0, "drop": True}),
    ("b40-kv8", "bf16", 40, 23, 70, {"B": 8, "kv": 0, "drop": True}), ("f40-kv8", "f32", 40, 23, 70, {"B": 8, "kv": 0, "drop": True}),
    ("b32-loop", "bf16", 32, 203, 49, {"drop": True}), ("f32-loop", "f32", 32, 203, 49, {"drop": True}),       # query-tile loop
    ("b20-loop", "bf16", 20, 203, 21, {}), ("f20-loop", "f32", 20, 203, 21, {}),
    ("b4", "bf16", 4, 23, 21, {"drop": True}), ("f4", "f32", 4, 23, 21, {"drop": True}),            # the VAE decoder's head dims
    ("b8", "bf16", 8, 23, 70, {}), ("f8", "f32", 8, 23, 70, {}),
    ("b20", "bf16", 20, 17, 21, {}), ("f20", "f32", 20, 17, 21, {}),
    ("b40", "bf16", 40, 17, 70, {"drop": True}), ("f40", "f32", 40, 17, 70, {"drop": True}),
    ("f320", "f32", 320, 17, 21, {}),
]

MODES = ("packed", "qkv", "padded")
KV_VALUES = ("zero", "one", "mid", "t32", "t33", "Sm1", "S", "over")      # kv_len: 0 (clamped), 1, inside the first tile, 32, 33, S-1, S, S+5


def _kv(tag, S):
    return {"zero": 0, "one": 1, "mid": min(7, S), "t32": 32, "t33": 33, "Sm1": S - 1, "S": S, "over": S + 5}[tag]


def _all():
    out = []
    for i, (dname, d, L, S) in enumerate(GRID):
        out.append((f"{dname}-d{d}-L{L}-S{S}", dname, d, L, S, {}, i))
    for j, (name, dname, d, L, S, over) in enumerate(NAMED):
        out.append((name, dname, d, L, S, over, len(GRID) + j))
    return out


def variations(case):
    """The launch variations of a case, from its position i in the table unless the case overrides them: B, the stride mode
    (packed rows; packed qkv rows ld = 3 heads d; padded rows with column offsets and gradient strides of their own; ld4 / ptr4:
    the two alignment fall-backs), dropout, the seed, the key lengths of the varlen passes and whether the forward-only launch
    passes lse = NULL."""
    name, dname, d, L, S, over, i = case
    B = over.get("B", 2 + i % 3)
    kv0 = over.get("kv", (3 * i) % len(KV_VALUES))
    return dict(B=B, mode=over.get("mode", MODES[i % 3]), drop=over.get("drop", i % 4 == 1), seed=0x1234ABCD5678 + 7919 * i + (i << 40),
                kv_len=[_kv(KV_VALUES[(kv0 + b) % len(KV_VALUES)], S) for b in range(B)], lse_null=(i % 5 == 2))


CASES = _all()
IDS = [c[0] for c in CASES]
_ROUTES_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_routes.json")
ROUTES = {k: [tuple(r) for r in v] for k, v in json.load(open(_ROUTES_PATH)).items()} if os.path.exists(_ROUTES_PATH) else {}


def layout(case):
    """name -> (row stride, column offset) of q, k, v, o, dout, dq, dk, dv in elements, and whether every pointer is 16-byte
    aligned.  The chunk N is 16 bytes of the dtype where heads d allows it, else 4 elements (the VALU kernels' unit)."""
    name, dname, d, L, S, over, i = case
    var = variations(case)
    HD = HEADS * d
    N = 4 if dname == "f32" or HD % 8 else 8
    names = ("q", "k", "v", "o", "dout", "dq", "dk", "dv")
    mode = var["mode"]
    if mode == "packed":
        lay = {n: (HD, 0) for n in names}
    elif mode == "qkv":
        lay = {"q": (3 * HD, 0), "k": (3 * HD, HD), "v": (3 * HD, 2 * HD), "o": (HD, 0), "dout": (HD, 0),
               "dq": (3 * HD, 0), "dk": (3 * HD, HD), "dv": (3 * HD, 2 * HD)}
    elif mode == "padded":
        lay = {n: (HD + k * N, N * ((k + 1) // 2)) for k, n in enumerate(names, start=1)}
    elif mode == "ld4":
        lay = {n: (HD + 4 + 8 * k, 8 * (k // 2)) for k, n in enumerate(names)}              # 4 mod 8: 8-byte aligned rows only
    elif mode == "ptr4":
        lay = {n: (HD + 8, 4) for n in names}                                                # every pointer 4 elements in
    else:
        raise ValueError(mode)
    return lay, mode != "ptr4"


def route_args(case, p):
    """The arguments of psg_attn_route for pass p of a case (after pass and dtype)."""
    name, dname, d, L, S, over, i = case
    lay, aligned = layout(case)
    ldg = lay["dout"][0] | lay["dq"][0] | lay["dk"][0] | lay["dv"][0]
    return (variations(case)["B"], HEADS, L, S, d, lay["q"][0], lay["k"][0], lay["v"][0], lay["o"][0], ldg, int(aligned))


def query_route(lib, p, dname, *args):
    """psg_attn_route -> (return code, tuple of the fields)."""
    out = (ctypes.c_int32 * len(ROUTE_FIELDS))()
    rc = lib.psg_attn_route(p, DTYPE_CODE[dname], *args, ctypes.cast(out, ctypes.c_void_p))
    return rc, tuple(out)


def expected_route(case, p):
    return ROUTES[case[0]][p]


def route_key(dname, p, route):
    """What identifies a launch variant: dtype, direction, family, ND, forward / dQ waves, KW, QW, the two reductions, NH, VARLEN."""
    rt = dict(zip(ROUTE_FIELDS, route))
    return (dname, "bwd" if p in (BWD, BWD_VARLEN) else "fwd", rt["family"], rt["ND"], rt["waves"], rt["KW"], rt["QW"], rt["qw_cut"],
            rt["w_cut"], rt["NH"], rt["varlen"])


def _q(t, dtype):
    return t.to(dtype).float()


def operands(case):
    """CPU fp32 tensors holding the values the launches of the case read (representable in its dtype): q, dout [B, L, heads d],
    k, v [B, S, heads d]; scale."""
    name, dname, d, L, S, over, i = case
    B = variations(case)["B"]
    dtype = DTYPES[dname]
    tag = "attnr." + name
    HD = HEADS * d
    return dict(q=_q(h((B, L, HD), tag + ".q", 2.0), dtype), k=_q(h((B, S, HD), tag + ".k", 2.0), dtype), v=_q(h((B, S, HD), tag + ".v"), dtype),
                dout=_q(h((B, L, HD), tag + ".do"), dtype), scale=float(d) ** -0.5)
