"""-m gpu: every attention route and kernel variant, through the C ABI (psg_attn_fwd, psg_attn_bwd, psg_attn_fwd_varlen,
psg_attn_fwd_varlen_train, psg_attn_bwd_varlen), element by element against the fp64 reference and bounds of
tests/attn_ref.py on the cases of tests/attn_cases.py.

Per launch: the route is the one the table stores (psg_attn_route, asserted before the launch) and psg_attn_path_counts moves
by exactly one launch of that family; o, lse, delta, dq, dk and dv are within their bounds at every element; outputs pre-filled
with NaN hold none afterwards; the padding columns between heads d and the row stride, the inputs, and the guard regions
behind lse and delta keep their bits; and a second identical launch gives identical bits (the kernels use no atomics).  The
backward launch reads the reference's o and lse rounded to their storage types, so each direction is judged on its own.  The
reference draws its dropout mask from the integer restatement in attn_ref.py, never from the kernels; one test per family
compares the kernels' mask with it directly (q = k = 0, one-hot v)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import attn_cases as K
from tests import attn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256                                      # elements of guard behind lse and delta
REPORT = os.environ.get("PSG_ATTN_REPORT")      # optional: append the fraction of its bound each output used to this file


def _report(line):
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    lib = _lib.init(0)
    yield lib
    lib.psg_attn_set_paths(3)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _seed_word():
    """The device word the launches add to their seed (ops.SeedSource), 0 when none is set."""
    from pokemon_sprite_generator_amd import ops
    return int(ops.SeedSource._t.item()) if ops.SeedSource.enabled() else 0


class Rows:
    """A [B, N, heads d] operand inside a wider buffer [B, N, ld] at column `off`: the padding holds a sentinel."""

    def __init__(self, B, N, HD, ld_off, dtype, values=None):
        ld, off = ld_off
        self.ld, self.HD, self.off = ld, HD, off
        self.buf = torch.full((B, N, ld), -1234.5, dtype=dtype, device=DEV)
        self.view = self.buf[:, :, off:off + HD]
        self.values = values
        self.reset()
        self.before = _bits(self.buf).clone()

    def reset(self):
        if self.values is None:
            self.view.fill_(float("nan"))
        else:
            self.view.copy_(self.values)

    def ptr(self):
        from pokemon_sprite_generator_amd._lib import ptr
        return ptr(self.view)

    def padding_intact(self):
        now, was = _bits(self.buf), self.before
        return torch.equal(now[:, :, :self.off], was[:, :, :self.off]) and torch.equal(now[:, :, self.off + self.HD:], was[:, :, self.off + self.HD:])

    def unchanged(self):
        return torch.equal(_bits(self.buf), self.before)


class Flat:
    """n fp32 values followed by a guard region in the same allocation."""

    def __init__(self, shape, values=None):
        self.n = int(np.prod(shape))
        self.shape, self.values = shape, values
        self.buf = torch.full((self.n + GUARD,), -4321.0, dtype=torch.float32, device=DEV)
        self.out = self.buf[:self.n]
        self.reset()

    def reset(self):
        if self.values is None:
            self.out.fill_(float("nan"))
        else:
            self.out.copy_(self.values.reshape(-1))

    def guard_intact(self):
        return bool((self.buf[self.n:] == -4321.0).all())


def _counts(lib):
    c = [C.c_int64() for _ in range(3)]
    lib.psg_attn_path_counts(*[C.byref(v) for v in c])
    return [v.value for v in c]


def _assert_route(lib, case, p):
    rc, got = K.query_route(lib, p, case[1], *K.route_args(case, p))
    want = K.expected_route(case, p)
    assert rc == 0 and got == want, f"route of {case[0]} {K.PASSES[p]}: {dict(zip(K.ROUTE_FIELDS, got))}, table {dict(zip(K.ROUTE_FIELDS, want))}"
    return got[0]


def _twice(lib, family, outs, launch, what):
    """Launch twice into NaN-filled outputs; the path counters move by one launch of `family` each time.  Returns the first
    launch's outputs (name -> clone) after NaN and bit-identity checks."""
    from pokemon_sprite_generator_amd import _lib
    runs = []
    for _ in range(2):
        for o in outs.values():
            o.reset()
        before = _counts(lib)
        try:
            _lib.check(launch(), what)
            torch.cuda.synchronize()
        except Exception as e:                       # a device fault: launch nothing more in this session
            if "illegal" in str(e) or "hipError" in str(e) or "HIP error" in str(e):
                pytest.exit(f"{what}: {e}", returncode=3)
            raise
        moved = [a - b for a, b in zip(_counts(lib), before)]
        assert moved == [int(f == family) for f in range(3)], f"{what}: path counters moved by {moved}, expected family {family}"
        runs.append({n: (o.view if isinstance(o, Rows) else o.out.reshape(o.shape)).clone() for n, o in outs.items()})
    for n, t in runs[0].items():
        assert not bool(torch.isnan(t).any()), f"{what}: {n} still holds NaN"
        assert torch.equal(_bits(t), _bits(runs[1][n])), f"{what}: {n}: a second identical launch gives other bits"
    return runs[0]


def _forward(lib, case, p, ops, lay, drop_p, seed, kv_len, lse_null=False):
    from pokemon_sprite_generator_amd import _lib
    name, dname, d, L, S, over, i = case
    B = ops["q"].shape[0]
    dtype, HD = K.DTYPES[dname], K.HEADS * d
    family = _assert_route(lib, case, p)
    q = Rows(B, L, HD, lay["q"], dtype, ops["q"])
    k = Rows(B, S, HD, lay["k"], dtype, ops["k"])
    v = Rows(B, S, HD, lay["v"], dtype, ops["v"])
    o = Rows(B, L, HD, lay["o"], dtype)
    lse = Flat((B, K.HEADS, L))
    kv = torch.tensor(kv_len, dtype=torch.int32, device=DEV) if kv_len is not None else None
    outs = {"o": o} if lse_null else {"o": o, "lse": lse}
    head = lambda: (q.ptr(), q.ld, k.ptr(), k.ld, v.ptr(), v.ld, o.ptr(), o.ld, None if lse_null else _lib.ptr(lse.out), B, K.HEADS, L, S, d,
                    float(ops["scale"]), float(drop_p), int(seed), K.DTYPE_CODE[dname])
    fn = {K.FWD: lib.psg_attn_fwd, K.FWD_VARLEN: lib.psg_attn_fwd_varlen, K.FWD_VARLEN_TRAIN: lib.psg_attn_fwd_varlen_train}[p]
    launch = (lambda: fn(*head(), _lib.stream_ptr())) if p == K.FWD else (lambda: fn(*head(), _lib.ptr(kv), _lib.stream_ptr()))
    got = _twice(lib, family, outs, launch, f"{name} psg_attn_{K.PASSES[p]}")
    assert q.unchanged() and k.unchanged() and v.unchanged(), "the forward wrote into an input"
    assert o.padding_intact(), "the forward wrote into o's padding columns"
    assert lse.guard_intact(), "the forward wrote behind lse"
    if lse_null:
        assert bool(torch.isnan(lse.out).all()), "lse = NULL, yet the lse buffer of an earlier launch was written"
    return got, family


def _backward(lib, case, p, ops, lay, drop_p, seed, kv_len, ref):
    from pokemon_sprite_generator_amd import _lib
    name, dname, d, L, S, over, i = case
    B = ops["q"].shape[0]
    dtype, HD = K.DTYPES[dname], K.HEADS * d
    family = _assert_route(lib, case, p)
    q = Rows(B, L, HD, lay["q"], dtype, ops["q"])
    k = Rows(B, S, HD, lay["k"], dtype, ops["k"])
    v = Rows(B, S, HD, lay["v"], dtype, ops["v"])
    o = Rows(B, L, HD, lay["o"], dtype, ref.o_st)
    do = Rows(B, L, HD, lay["dout"], dtype, ops["dout"])
    dq = Rows(B, L, HD, lay["dq"], dtype)
    dk = Rows(B, S, HD, lay["dk"], dtype)
    dv = Rows(B, S, HD, lay["dv"], dtype)
    lse = Flat((B, K.HEADS, L), ref.lse_st.float())
    delta = Flat((B, K.HEADS, L))
    kv = torch.tensor(kv_len, dtype=torch.int32, device=DEV) if kv_len is not None else None
    head = lambda: (q.ptr(), q.ld, k.ptr(), k.ld, v.ptr(), v.ld, o.ptr(), o.ld, do.ptr(), do.ld, _lib.ptr(lse.out), _lib.ptr(delta.out),
                    dq.ptr(), dq.ld, dk.ptr(), dk.ld, dv.ptr(), dv.ld, B, K.HEADS, L, S, d, float(ops["scale"]), float(drop_p), int(seed),
                    K.DTYPE_CODE[dname])
    launch = (lambda: lib.psg_attn_bwd(*head(), _lib.stream_ptr())) if p == K.BWD else \
        (lambda: lib.psg_attn_bwd_varlen(*head(), _lib.ptr(kv), _lib.stream_ptr()))
    got = _twice(lib, family, dict(delta=delta, dq=dq, dk=dk, dv=dv), launch, f"{name} psg_attn_{K.PASSES[p]}")
    assert all(t.unchanged() for t in (q, k, v, o, do)), "the backward wrote into an input"
    assert torch.equal(_bits(lse.buf), _bits(torch.cat([ref.lse_st.float().reshape(-1), lse.buf[lse.n:]]))), "the backward wrote into lse or behind it"
    assert dq.padding_intact() and dk.padding_intact() and dv.padding_intact(), "the backward wrote into a gradient's padding columns"
    assert delta.guard_intact(), "the backward wrote behind delta"
    return got, family


def _dev(ops):
    return {n: (t.to(DEV) if torch.is_tensor(t) else t) for n, t in ops.items()}


@pytest.mark.parametrize("case", K.CASES, ids=K.IDS)
def test_attention_routes(lib, case):
    name, dname, d, L, S, over, i = case
    var = K.variations(case)
    dtype = K.DTYPES[dname]
    ops = _dev(K.operands(case))
    lay, _ = K.layout(case)
    p = K.DROP_P if var["drop"] else 0.0
    seed = var["seed"]
    mask_seed = (seed + _seed_word()) & 0xFFFFFFFFFFFFFFFF
    bf = dname == "bf16"
    lib.psg_attn_set_paths(3)
    for varlen, pf, pb in ((False, K.FWD, K.BWD), (True, K.FWD_VARLEN_TRAIN, K.BWD_VARLEN)):
        kv = var["kv_len"] if varlen else None
        fam = K.expected_route(case, pb)[0]
        assert K.expected_route(case, pf)[0] == fam                               # a training pair stays on one family
        ref = R.reference(ops["q"], ops["k"], ops["v"], K.HEADS, ops["scale"], fam, bf, kv_len=kv, drop_p=p, seed=mask_seed, dout=ops["dout"])
        got, _ = _forward(lib, case, pf, ops, lay, p, seed, kv)
        ratios = R.check_all(got, ref, dtype, f"{name} {K.PASSES[pf]} family {fam}")
        _report(f"gpu {name} {dname} {K.PASSES[pf]} family{fam} " + " ".join(f"{n}={v:.3g}" for n, v in ratios.items()))
        got, _ = _backward(lib, case, pb, ops, lay, p, seed, kv, ref)
        ratios = R.check_all(got, ref, dtype, f"{name} {K.PASSES[pb]} family {fam}")
        _report(f"gpu {name} {dname} {K.PASSES[pb]} family{fam} " + " ".join(f"{n}={v:.3g}" for n, v in ratios.items()))
    # the forward-only entry: no dropout, its own family rule, lse optional
    fam = K.expected_route(case, K.FWD_VARLEN)[0]
    ref = R.reference(ops["q"], ops["k"], ops["v"], K.HEADS, ops["scale"], fam, bf, kv_len=var["kv_len"])
    got, _ = _forward(lib, case, K.FWD_VARLEN, ops, lay, 0.0, seed, var["kv_len"], lse_null=var["lse_null"])
    ratios = R.check_all(got, ref, dtype, f"{name} fwd_varlen family {fam}")
    _report(f"gpu {name} {dname} fwd_varlen family{fam} " + " ".join(f"{n}={v:.3g}" for n, v in ratios.items()))


@pytest.mark.parametrize("dname,d,allow,family", [("bf16", 64, 3, 0), ("bf16", 64, 0, 1), ("f32", 64, 3, 2), ("f32", 64, 0, 1), ("bf16", 20, 3, 1)],
                         ids=["bf16-mfma", "bf16-valu", "f32-mfma", "f32-valu", "bf16-valu-d20"])
def test_dropout_mask_is_the_restatement(lib, dname, d, allow, family):
    """q = k = 0 makes P uniform (1 / S) and a one-hot v[s, c] = (s == c) copies P's row into o: o[l, c] = keep / ((1 - p) S)
    for c < S - so the forward kernel's mask is read off o (S = 19 <= d keys; the larger d = 64 cases use S = 49, odd, two
    key tiles, read in slices of the head dimension over the three heads).  psg_attn_set_paths pins the family."""
    from pokemon_sprite_generator_amd import _lib
    B, H, L = 2, K.HEADS, 45
    S = 49 if d == 64 else 19
    dtype = K.DTYPES[dname]
    seed, p = 0xABCDEF0123, K.DROP_P
    assert S <= d
    q = torch.zeros(B, L, H * d, dtype=dtype, device=DEV)
    k = torch.zeros(B, S, H * d, dtype=dtype, device=DEV)
    v = torch.zeros(B, S, H, d, dtype=dtype, device=DEV)
    for s in range(S):
        v[:, s, :, s] = 1.0
    v = v.reshape(B, S, H * d)
    o = torch.full((B, L, H * d), float("nan"), dtype=dtype, device=DEV)
    lse = torch.empty(B, H, L, dtype=torch.float32, device=DEV)
    try:
        lib.psg_attn_set_paths(allow)
        before = _counts(lib)
        _lib.check(lib.psg_attn_fwd(_lib.ptr(q), H * d, _lib.ptr(k), H * d, _lib.ptr(v), H * d, _lib.ptr(o), H * d, _lib.ptr(lse), B, H, L, S, d, 1.0,
                                    p, seed, K.DTYPE_CODE[dname], _lib.stream_ptr()), "psg_attn_fwd")
        torch.cuda.synchronize()
        assert [a - b for a, b in zip(_counts(lib), before)] == [int(f == family) for f in range(3)]
    finally:
        lib.psg_attn_set_paths(3)
    got = o.float().reshape(B, L, H, d)[..., :S].permute(0, 2, 1, 3).reshape(B * H, L, S).cpu()
    want = torch.from_numpy(R.keep_mask((seed + _seed_word()) & 0xFFFFFFFFFFFFFFFF, B * H, L, S, p))
    kept = got > 0.5 / S
    assert bool(((got - kept.float() / ((1.0 - p) * S)).abs() < 0.02 / S).all()), "o is not keep / ((1 - p) S)"
    bad = (kept != want).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} mask elements differ from the restatement, first at (bh, l, s) = {tuple(int(x) for x in bad[0])}"
    assert 0.6 < float(want.float().mean()) < 0.8
