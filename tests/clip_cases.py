"""The case table of the element-wise CLIP kernel tests (test infrastructure, not a conftest): psg_attn_fwd_causal,
psg_clip_prep_fwd / _bwd and psg_cosine_loss of csrc/clip.hip at the smallest shapes that still have a tail in every direction,
through the C ABI on guarded, NaN-filled buffers whose bases and row strides are the least the header allows.

tests/clip_ref.py and tests/attn_ref.py hold the fp64 references and the per-element bounds; tests/test_clip_ref_cpu.py proves
on the host that the references are torch's, that the constants are what they are said to be and that the comparators reject
planted defects at these very shapes; tests/test_clip_kernels_gpu.py launches every case.

Inputs come from clip_ref.u (the hash generator) and are bf16-representable where a launch reads bf16.
"""
import functools

import torch

from tests import attn_ref
from tests import clip_ref as R
from tests.conv_cases import GUARD, NAN

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
DTYPE_CODE = {"f32": 0, "bf16": 1}
# Every operand starts OFF elements behind its front guard: a 4-element boundary that is not the next larger one - 8 bytes
# but not 16 for bf16; 16 bytes, the least the header allows, but not 32 for fp32 (the allocator's own alignment is >= 256).
OFF = 4


def alloc(rows, ld, dtype, device="cpu", fill=NAN):
    """A guarded row buffer: GUARD + OFF elements, rows x ld, GUARD elements, all `fill`.  Returns (flat buffer, [rows, ld] view)."""
    flat = torch.full((2 * GUARD + OFF + rows * ld,), fill, dtype=dtype, device=device)
    return flat, flat[GUARD + OFF:GUARD + OFF + rows * ld].view(rows, ld)


def filled(values, ld, dtype, device="cpu"):
    """`values` [rows, C] in the first C columns of a guarded [rows, ld] buffer; NaN everywhere else: a read outside shows."""
    flat, view = alloc(values.shape[0], ld, dtype, device)
    view[:, :values.shape[1]] = values.to(device=device, dtype=dtype)
    return flat, view


def guards_ok(pair, ncols, what):
    """After a launch: guards and the columns behind `ncols` still NaN, every element inside a number."""
    flat, view = (t.detach().cpu().float() for t in pair)
    rows, ld = view.shape
    assert bool(torch.isnan(flat[:GUARD + OFF]).all()) and bool(torch.isnan(flat[GUARD + OFF + rows * ld:]).all()), f"{what}: a store outside the buffer (guard)"
    bad = (~torch.isnan(view[:, ncols:])).nonzero()
    assert bad.numel() == 0, f"{what}: a store in the unwritten columns of a strided row, first at (row, col) {(int(bad[0][0]), int(bad[0][1]) + ncols) if bad.numel() else ()}"
    bad = torch.isnan(view[:, :ncols]).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} elements never stored (or NaN), first at {tuple(int(i) for i in bad[0]) if bad.numel() else ()}"


def q(t, dname):
    """fp32 values as a launch of the dtype reads them."""
    return R.bf16_exact(t) if dname == "bf16" else t


# ------------------------------------------------------------------------------------------------------------- causal
CAUSAL_L = (1, 2, 3, 63, 64, 65, 77, 127, 128)      # 64 / 65: a second wave starts; 128: the 64 KiB of LDS psg_init allows
CAUSAL_D = (16, 32, 64)
HOT_SCALE = 12.0                                     # scores beyond +-100: exp() without the running maximum overflows


def _causal():
    cs = []
    for dn in DTYPES:
        for d in CAUSAL_D:
            for L in CAUSAL_L:
                cs.append(dict(name=f"{dn}.d{d}.L{L}", dtype=dn, d=d, L=L, B=3, heads=3, scale=d ** -0.5, hot=False))
            cs.append(dict(name=f"{dn}.d{d}.L65.b1h1", dtype=dn, d=d, L=65, B=1, heads=1, scale=d ** -0.5, hot=False))
            cs.append(dict(name=f"{dn}.d{d}.L77.hot", dtype=dn, d=d, L=77, B=3, heads=3, scale=HOT_SCALE, hot=True))
    return cs


CAUSAL = _causal()
CAUSAL_BY_NAME = {c["name"]: c for c in CAUSAL}


def causal_ld(c):
    """Row strides of q, k, v, o (four separate buffers; q and o share a stride, not an address)."""
    E = c["heads"] * c["d"]
    return dict(q=E + 4, k=E + 8, v=E + 12, o=E + 4)


@functools.lru_cache(maxsize=None)
def causal_operands(name):
    """q, k, v [B, L, heads d] fp32 (bf16-representable for a bf16 launch), three separate tensors."""
    c = CAUSAL_BY_NAME[name]
    shape = (c["B"], c["L"], c["heads"] * c["d"])
    tag = f"cc.{c['d']}.{c['L']}.{c['B']}.{c['heads']}.{int(c['hot'])}"
    return tuple(q(R.u(shape, f"{tag}.{n}") * 1.5, c["dtype"]) for n in "qkv")


@functools.lru_cache(maxsize=None)
def causal_reference(name):
    c = CAUSAL_BY_NAME[name]
    qq, kk, vv = causal_operands(name)
    return attn_ref.reference(qq, kk, vv, c["heads"], c["scale"], attn_ref.VALU, c["dtype"] == "bf16", causal=True)


def causal_check(got_o, got_lse, name, what, c=None):
    """attn_ref.check of o and lse at C_CAUSAL: name -> worst err / bound."""
    case, r = CAUSAL_BY_NAME[name], causal_reference(name)
    cc = R.C_CAUSAL if c is None else c
    out = {"o": attn_ref.check(got_o, r.o, r.o_mag, DTYPES[case["dtype"]], f"{what} o", extra=r.o_extra, c=cc)}
    if got_lse is not None:
        out["lse"] = attn_ref.check(got_lse, r.lse, r.lse_mag, torch.float32, f"{what} lse", extra=r.lse_extra, c=cc)
    return out


def causal_store(o, lse, name):
    """fp32 results as the launch stores them: o in the case's dtype, lse in fp32."""
    return o.to(DTYPES[CAUSAL_BY_NAME[name]["dtype"]]), lse.float()


def measure_c_causal(threads=4):
    """(C_CAUSAL_TORCH, its case, C_CAUSAL_SEQ, its case): the smallest c at which torch's fp32 masked softmax + matmul, and the
    numpy-fp32 evaluation of the header's description (clip_ref.causal_seq_f32), pass the bounds of o and lse on every case."""
    before = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        best = {"torch": (0.0, ""), "seq": (0.0, "")}
        for c in CAUSAL:
            r, ops = causal_reference(c["name"]), causal_operands(c["name"])
            for how, fn in (("torch", R.causal_torch_f32), ("seq", R.causal_seq_f32)):
                o, lse = causal_store(*fn(*ops, c["heads"], c["scale"]), c["name"])
                v = max(attn_ref.smallest_c(o, r.o, r.o_mag, o.dtype, extra=r.o_extra),
                        attn_ref.smallest_c(lse, r.lse, r.lse_mag, torch.float32, extra=r.lse_extra))
                if v > best[how][0]:
                    best[how] = (v, c["name"])
        return best["torch"] + best["seq"]
    finally:
        torch.set_num_threads(before)


# --------------------------------------------------------------------------------------------------------------- prep
# (Hi, S, P).  Hi = 1, 2, 3: the window is clipped on both sides at once (n < 4 everywhere); 8: the exact half scale; 15:
# S - 1; P = 4 and P = S (one patch); 16 -> 16: no resampling; 30 -> 32: four patches of 16.  (215 -> 224 stays in clip_ref.PREP_CASES.)
PREP_SHAPES = ((1, 16, 8), (2, 16, 8), (3, 16, 8), (5, 16, 8), (8, 16, 8), (15, 16, 8), (7, 16, 4), (7, 16, 16), (16, 16, 4), (30, 32, 16))
PREP_BATCHES = (1, 3)
PREP_AB = ((0.5, 0.5), (1.0, 0.0), (-0.75, 0.3))
PREP_LD_EXTRA = (0, 8)                               # row stride 3 P P and 3 P P + 8


@functools.lru_cache(maxsize=None)
def prep_operands(Hi, S, P, B):
    """(img fp32 [B,3,Hi,Hi] in about +-1.2, dy [B (S/P)^2, 3 P P] bf16-representable: read exactly by both dtypes)."""
    G = S // P
    return R.image(f"pc.{Hi}.{S}.{P}", B, Hi), R.bf16_exact(R.u((B * G * G, 3 * P * P), f"pc.dy.{Hi}.{S}.{P}.{B}"))


# ------------------------------------------------------------------------------------------------------------- cosine
COS_B = (1, 2, 4, 5, 9)          # 5, 9: a wave takes a second (and wave 0 a third) row
COS_D = (4, 8, 252, 256, 260, 512, 516)      # the lane-strided loop ends mid-wave at 4, 252, 260, 516
# the kind of row planted at row 1 and, where B >= 5, at row 4 (wave 1's first row and wave 0's second): nothing, a zero u row,
# a zero v row, a u row of norm 1e-13 (below eps, not zero), u = -v
COS_KINDS = ("none", "zero_u", "zero_v", "tiny_u", "neg")


def cosine_ld(D):
    return dict(u=D, v=D + 4, du=D + 12)


def planted_rows(B):
    return [r for r in (1, 4) if r < B]


@functools.lru_cache(maxsize=None)
def cosine_operands(B, D, kind, dname):
    """u, v [B, D] fp32 as the launch reads them."""
    v = R.u((B, D), f"cs.v.{B}.{D}")
    u = 0.6 * v + 0.8 * R.u((B, D), f"cs.u.{B}.{D}")
    for r in planted_rows(B):
        if kind == "zero_u":
            u[r] = 0.0
        elif kind == "zero_v":
            v[r] = 0.0
        elif kind == "tiny_u":
            u[r] = (u[r].double() * (1e-13 / float(u[r].double().norm()))).float()
    u, v = q(u, dname), q(v, dname)
    if kind == "neg":
        for r in planted_rows(B):
            u[r] = -v[r]
    return u, v


def cosine_torch_f32(u, v, dname):
    """torch's fp32 evaluation of clip_loss.py:60-67 and its autograd gradient, stored like the launch's: (loss fp32, du)."""
    out, du = R.cosine_torch(u, v, torch.float32)
    return out, du.to(DTYPES[dname])


def measure_c_cos(threads=4):
    """(C_COS_TORCH, its case): the smallest c at which torch's fp32 evaluation passes cosine_ref's bounds on every case."""
    from tests.gemm_ref import BF16_ROUND, F32_ROUND
    before = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        best = (0.0, "")
        for dn in DTYPES:
            for B in COS_B:
                for D in COS_D:
                    for kind in COS_KINDS if B > 1 else ("none",):
                        u, v = cosine_operands(B, D, kind, dn)
                        r = R.cosine_ref(u, v)
                        out, du = cosine_torch_f32(u, v, dn)
                        c = max(R.smallest_c(out, r.loss, r.loss_mag, F32_ROUND),
                                R.smallest_c(du, r.du, r.du_mag, BF16_ROUND if dn == "bf16" else F32_ROUND))
                        if c > best[0]:
                            best = (c, f"{dn}.B{B}.D{D}.{kind}")
        return best
    finally:
        torch.set_num_threads(before)


def cosine_check(out, du, B, D, kind, dname, what, c=None):
    """The loss and its gradient against cosine_ref's bounds, plus what must hold exactly: a zero v row gives a du row of exact
    zeros (the reference's is one too, so the bound alone would allow A_FLOOR).  Returns name -> worst err / bound."""
    u, v = cosine_operands(B, D, kind, dname)
    r = R.cosine_ref(u, v)
    dt = DTYPES[dname]
    res = {"loss": R.check_bound(out.reshape(()), r.loss, R.cosine_bound(r.loss, r.loss_mag, torch.float32, c), f"{what} loss")}
    if du is not None:
        res["du"] = R.check_bound(du, r.du, R.cosine_bound(r.du, r.du_mag, dt, c), f"{what} du")
        if kind == "zero_v":
            for row in planted_rows(B):
                assert bool((du[row].float() == 0).all()), f"{what}: du row {row} of a zero v row is not exactly zero"
    return res
