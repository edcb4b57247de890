"""-m gpu: psg_attn_bwd_longq - the attention backward for few keys and very many queries (the VAE decoder's text
cross-attention under stage 3).

Element by element (test_longq_elementwise and below): every case of tests/attn_longq_cases.py - each head_dim and dtype on
each (key tiles, query tiles per slab) path, the edges of L and S, strided rows, the product's kv layout, 8-byte aligned bf16
pointers, odd dk / dv offsets - through the C ABI against the fp64 reference and per-element bounds of tests/attn_ref.py at
C_LONGQ.  The launch reads the reference's o and lse rounded to their storage types; delta, dq, dk and dv are within their
bounds at every element; outputs and workspace pre-filled with NaN hold none afterwards; padding columns, inputs and the
guards round delta and the workspace keep their bits; a second identical launch gives identical bits.  One test takes o and
lse from psg_attn_fwd, one goes through ops.attention_cross_longq and autograd, one walks the contract's refusals.
tests/golden/REPORT_attn_longq.txt holds the worst err / bound of every case and output (tools/attn_longq_report.py).

At the decoder's shapes (the older tests, bars of tests.util.TOL: o within TOL[dtype], dq / dk / dv within 2 x TOL[dtype],
max-abs over max-abs): against an fp64 torch softmax-attention on the same inputs, against psg_attn_bwd, deterministic bits at
L = 46 225, two argument errors, and no trace in psg_attn_path_counts."""
import math

import os

import pytest
import torch

from tests import attn_longq_cases as K
from tests import attn_ref as R
from tests.test_attention_routes_gpu import GUARD, Rows, _bits
from tests.test_kernels_gpu import _attn_paths
from tests.util import TOL, maxrel

pytestmark = pytest.mark.gpu
DEV = "cuda"
HEADS = 8
# (head_dim, L, S, B): the five decoder shapes; ragged S; S over several key tiles; L not a multiple of any tile; L = 1
DECODER = [(64, 729, 32, 2), (32, 729, 32, 2), (16, 2916, 32, 2), (8, 11664, 32, 2), (4, 46225, 32, 2)]
EXTRA = [(32, 729, 20, 2), (16, 729, 256, 2), (64, 731, 32, 2), (8, 1, 32, 2), (4, 200, 45, 1), (64, 100, 70, 1)]
SCORE_STD_WINDOW = (1.0, 8.0)


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    return _lib.init(0)


def _inputs(d, L, S, B, dt, seed=0):
    """q, k with scaled-score std 2 (uniform in [-a, a), a^2 / 3 = 2): a near-uniform softmax would hide a wrong dS."""
    g = torch.Generator(device=DEV).manual_seed(1000 * d + L + S + seed)
    E = HEADS * d
    u = lambda shape, a: ((torch.rand(shape, device=DEV, generator=g) * 2 - 1) * a).to(dt)
    a = math.sqrt(6.0)
    return u((B, L, E), a), u((B, S, E), a), u((B, S, E), 1.0), u((B, L, E), 1.0)


def _fwd(lib, q, k, v):
    from pokemon_sprite_generator_amd import _lib
    B, L, E = q.shape
    S, d = k.shape[1], E // HEADS
    o = torch.empty_like(q)
    lse = torch.empty((B, HEADS, L), dtype=torch.float32, device=DEV)
    _lib.check(lib.psg_attn_fwd(_lib.ptr(q), E, _lib.ptr(k), E, _lib.ptr(v), E, _lib.ptr(o), E, _lib.ptr(lse), B, HEADS, L, S, d, d ** -0.5, 0.0, 0,
                                _lib.dtype_code(q.dtype), _lib.stream_ptr()), "psg_attn_fwd")
    return o, lse


def _bwd(lib, q, k, v, o, lse, do, longq=True, ws_bytes=None, drop=0.0, raw=False):
    from pokemon_sprite_generator_amd import _lib
    B, L, E = q.shape
    S, d = k.shape[1], E // HEADS
    dq, dk, dv = torch.full_like(q, float("nan")), torch.full_like(k, float("nan")), torch.full_like(v, float("nan"))
    delta = torch.empty((B, HEADS, L), dtype=torch.float32, device=DEV)
    args = [_lib.ptr(q), E, _lib.ptr(k), E, _lib.ptr(v), E, _lib.ptr(o), E, _lib.ptr(do), E, _lib.ptr(lse), _lib.ptr(delta), _lib.ptr(dq), E,
            _lib.ptr(dk), E, _lib.ptr(dv), E, B, HEADS, L, S, d, d ** -0.5, drop, 0, _lib.dtype_code(q.dtype)]
    if longq:
        need = lib.psg_attn_bwd_longq_workspace_bytes(B, HEADS, L, S, d)
        assert need > 0
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        rc = lib.psg_attn_bwd_longq(*args, _lib.ptr(ws), need if ws_bytes is None else ws_bytes, _lib.stream_ptr())
    else:
        rc = lib.psg_attn_bwd(*args, _lib.stream_ptr())
    if raw:
        return rc
    _lib.check(rc, "psg_attn_bwd_longq" if longq else "psg_attn_bwd")
    torch.cuda.synchronize()
    return dq, dk, dv


def _ref(q, k, v, do):
    """fp64 softmax attention and its gradients on the same (already rounded) inputs; also the scaled scores' std."""
    B, L, E = q.shape
    d = E // HEADS
    split = lambda t: t.double().view(B, -1, HEADS, d).transpose(1, 2).detach().requires_grad_(True)
    qh, kh, vh = split(q), split(k), split(v)
    sc = qh @ kh.transpose(-1, -2) / math.sqrt(d)
    o = (torch.softmax(sc, dim=-1) @ vh).transpose(1, 2).reshape(B, L, E)
    o.backward(do.double())
    join = lambda t: t.transpose(1, 2).reshape(B, -1, E)
    return o.detach(), join(qh.grad), join(kh.grad), join(vh.grad), float(sc.detach().std())


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("d,L,S,B", DECODER + EXTRA)
def test_longq_matches_fp64_attention(lib, d, L, S, B, dt):
    q, k, v, do = _inputs(d, L, S, B, dt)
    ro, rdq, rdk, rdv, std = _ref(q, k, v, do)
    lo, hi = SCORE_STD_WINDOW
    assert lo <= std <= hi, f"score std {std:.2f} outside [{lo}, {hi}]"
    o, lse = _fwd(lib, q, k, v)
    dq, dk, dv = _bwd(lib, q, k, v, o, lse, do)
    e = [maxrel(o, ro), maxrel(dq, rdq), maxrel(dk, rdk), maxrel(dv, rdv)]
    print(f"d={d} L={L} S={S} B={B} {dt}: score std {std:.2f}; o {e[0]:.2e} dq {e[1]:.2e} dk {e[2]:.2e} dv {e[3]:.2e}")
    assert all(torch.isfinite(t.float()).all() for t in (dq, dk, dv))
    assert e[0] < TOL[dt], e
    assert max(e[1:]) < 2 * TOL[dt], e


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_longq_agrees_with_attn_bwd(lib, dt):
    """A shape the VALU backward handles cheaply (L = 729, head_dim 8): the two entries agree within 2 x TOL."""
    q, k, v, do = _inputs(8, 729, 32, 2, dt, seed=5)
    o, lse = _fwd(lib, q, k, v)
    a = _bwd(lib, q, k, v, o, lse, do, longq=True)
    b = _bwd(lib, q, k, v, o, lse, do, longq=False)
    for x, y, n in zip(a, b, ("dq", "dk", "dv")):
        assert maxrel(x, y) < 2 * TOL[dt], (n, maxrel(x, y))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_longq_is_deterministic(lib, dt):
    """Two calls on the largest decoder map (L = 46 225) give the same bits: the slab partials are summed in slab order."""
    q, k, v, do = _inputs(4, 46225, 32, 2, dt, seed=9)
    o, lse = _fwd(lib, q, k, v)
    a = _bwd(lib, q, k, v, o, lse, do)
    b = _bwd(lib, q, k, v, o, lse, do)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_longq_argument_errors(lib):
    q, k, v, do = _inputs(8, 729, 32, 2, torch.float32)
    o, lse = _fwd(lib, q, k, v)
    need = lib.psg_attn_bwd_longq_workspace_bytes(2, HEADS, 729, 32, 8)
    assert _bwd(lib, q, k, v, o, lse, do, ws_bytes=need - 4, raw=True) == -4       # PSG_ERR_WORKSPACE
    assert b"workspace" in lib.psg_last_error()
    assert _bwd(lib, q, k, v, o, lse, do, drop=0.1, raw=True) == -6                # PSG_ERR_ARG
    assert _bwd(lib, q, k, v, o, lse, do, raw=True) == 0
    torch.cuda.synchronize()


def test_longq_is_not_a_counted_family(lib):
    """psg_attn_path_counts counts the three families psg_attn_fwd / psg_attn_bwd route to; longq calls leave it alone."""
    q, k, v, do = _inputs(16, 729, 32, 2, torch.bfloat16)
    o, lse = _fwd(lib, q, k, v)
    before = _attn_paths()
    for _ in range(3):
        _bwd(lib, q, k, v, o, lse, do)
    assert _attn_paths() == before


# =============================================================================================== element by element vs fp64
REPORT = os.environ.get("PSG_ATTN_LONGQ_REPORT")      # optional: append the fraction of its bound each output used to this file
NAMES = ("delta", "dq", "dk", "dv")


def _report(line):
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(line + "\n")


def _sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                   # a device error: nothing more runs on this GPU
        pytest.exit(f"{what}: {e}", returncode=3)


class Guarded:
    """n fp32 values between two guard regions of one allocation; the values start NaN (or as `values`)."""
    SENTINEL = -4321.0

    def __init__(self, n, values=None):
        self.n, self.values = n, values
        self.buf = torch.full((n + 2 * GUARD,), self.SENTINEL, dtype=torch.float32, device=DEV)
        self.out = self.buf[GUARD:GUARD + n]
        self.reset()

    def reset(self):
        if self.values is None:
            self.out.fill_(float("nan"))
        else:
            self.out.copy_(self.values.reshape(-1))

    def guards_intact(self):
        return bool((self.buf[:GUARD] == self.SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == self.SENTINEL).all())

    def all_nan(self):
        return bool(torch.isnan(self.out).all())


class Launch:
    """The operands of one psg_attn_bwd_longq call in the layout of a case: every [B, N, heads d] operand inside a wider buffer
    whose padding holds a sentinel (Rows), k | v and dk | dv as the halves of one buffer each in mode "kv", lse, delta and the
    workspace between guards; outputs and workspace NaN."""

    def __init__(self, lib, cs, ops, o, lse):
        from pokemon_sprite_generator_amd import _lib
        self.lib, self.cs = lib, cs
        self.mode, lay = K.layout(cs)
        B, H, L, S, d = cs.B, cs.heads, cs.L, cs.S, cs.d
        dtype, HD = K.DTYPES[cs.dname], cs.heads * cs.d
        esz = 2 if cs.dname == "bf16" else 4
        self.q = Rows(B, L, HD, lay["q"], dtype, ops["q"])
        self.o = Rows(B, L, HD, lay["o"], dtype, o)
        self.do = Rows(B, L, HD, lay["dout"], dtype, ops["dout"])
        self.dq = Rows(B, L, HD, lay["dq"], dtype)
        if self.mode == "kv":
            self.kv = Rows(B, S, 2 * HD, (2 * HD, 0), dtype, torch.cat([ops["k"], ops["v"]], -1))
            self.dkv = Rows(B, S, 2 * HD, (2 * HD, 0), dtype)
            self.inputs, self.grads = [self.q, self.kv, self.o, self.do], [self.dq, self.dkv]
            kp, dkp = self.kv.view.data_ptr(), self.dkv.view.data_ptr()
            self.ptr = dict(k=kp, v=kp + HD * esz, dk=dkp, dv=dkp + HD * esz)
            self.views = dict(dq=self.dq.view, dk=self.dkv.view[:, :, :HD], dv=self.dkv.view[:, :, HD:])
        else:
            self.k = Rows(B, S, HD, lay["k"], dtype, ops["k"])
            self.v = Rows(B, S, HD, lay["v"], dtype, ops["v"])
            self.dk = Rows(B, S, HD, lay["dk"], dtype)
            self.dv = Rows(B, S, HD, lay["dv"], dtype)
            self.inputs, self.grads = [self.q, self.k, self.v, self.o, self.do], [self.dq, self.dk, self.dv]
            self.ptr = dict(k=self.k.view.data_ptr(), v=self.v.view.data_ptr(), dk=self.dk.view.data_ptr(), dv=self.dv.view.data_ptr())
            self.views = dict(dq=self.dq.view, dk=self.dk.view, dv=self.dv.view)
        self.ptr.update(q=self.q.view.data_ptr(), o=self.o.view.data_ptr(), dout=self.do.view.data_ptr(), dq=self.dq.view.data_ptr())
        self.ld = {n: lay[n][0] for n in K.OPERANDS}
        self.lse = Guarded(B * H * L, lse.float())
        self.lse_before = _bits(self.lse.buf).clone()
        self.delta = Guarded(B * H * L)
        self.need = lib.psg_attn_bwd_longq_workspace_bytes(B, H, L, S, d)
        assert self.need > 0 and self.need % 16 == 0
        self.ws = Guarded(self.need // 4)
        self.ptr.update(lse=self.lse.out.data_ptr(), delta=self.delta.out.data_ptr(), ws=self.ws.out.data_ptr())
        self.dims = dict(B=B, heads=H, L=L, S=S, d=d, scale=float(ops["scale"]), drop_p=0.0, seed=0, dtype=K.DTYPE_CODE[cs.dname], ws_bytes=self.need)
        self.stream = _lib.stream_ptr

    def reset(self):
        for g in self.grads:
            g.reset()
        self.delta.reset()
        self.ws.reset()

    def call(self, ptr=None, ld=None, **dims):
        """psg_attn_bwd_longq with the case's arguments, `ptr` / `ld` / dims overriding single ones; returns the code."""
        p, s, a = dict(self.ptr, **(ptr or {})), dict(self.ld, **(ld or {})), dict(self.dims, **dims)
        return self.lib.psg_attn_bwd_longq(p["q"], s["q"], p["k"], s["k"], p["v"], s["v"], p["o"], s["o"], p["dout"], s["dout"], p["lse"], p["delta"],
                                           p["dq"], s["dq"], p["dk"], s["dk"], p["dv"], s["dv"], a["B"], a["heads"], a["L"], a["S"], a["d"], a["scale"],
                                           a["drop_p"], a["seed"], a["dtype"], p["ws"], a["ws_bytes"], self.stream())

    def outputs(self):
        B, H, L = self.cs.B, self.cs.heads, self.cs.L
        return dict(delta=self.delta.out.reshape(B, H, L).clone(), **{n: v.clone() for n, v in self.views.items()})

    def untouched(self):
        """Nothing was launched: outputs and workspace are still all NaN, guards and inputs as they were."""
        return all(bool(torch.isnan(v).all()) for v in self.views.values()) and self.delta.all_nan() and self.ws.all_nan() and self.intact() is None

    def intact(self):
        """None, or what a launch damaged outside its results."""
        if not all(t.unchanged() for t in self.inputs):
            return "the launch wrote into an input"
        if not torch.equal(_bits(self.lse.buf), self.lse_before):
            return "the launch wrote into lse or its guards"
        if not all(g.padding_intact() for g in self.grads):
            return "the launch wrote into a gradient's padding columns"
        if not self.delta.guards_intact():
            return "the launch wrote outside delta"
        if not self.ws.guards_intact():
            return "the launch wrote outside the workspace bytes its query reports"
        return None

    def twice(self, what):
        """Two launches into NaN-filled outputs and workspace; the first one's outputs after the NaN, guard and bit-identity
        checks."""
        from pokemon_sprite_generator_amd import _lib
        runs = []
        for _ in range(2):
            self.reset()
            _lib.check(self.call(), what)
            _sync(what)
            assert not bool(torch.isnan(self.ws.out).any()), f"{what}: the workspace's {self.need} bytes still hold NaN"
            assert self.intact() is None, f"{what}: {self.intact()}"
            runs.append(self.outputs())
        for n, t in runs[0].items():
            assert not bool(torch.isnan(t).any()), f"{what}: {n} still holds NaN"
            assert torch.equal(_bits(t), _bits(runs[1][n])), f"{what}: {n}: a second identical launch gives other bits"
        return runs[0]


def _dev(ops):
    return {n: (t.to(DEV) if torch.is_tensor(t) else t) for n, t in ops.items()}


def _reference(cs, ops):
    return R.reference(ops["q"], ops["k"], ops["v"], cs.heads, ops["scale"], R.VALU, cs.dname == "bf16", dout=ops["dout"])


@pytest.mark.parametrize("cs", K.CASES, ids=K.IDS)
def test_longq_elementwise(lib, cs):
    ops = _dev(K.operands(cs))
    ref = _reference(cs, ops)
    run = Launch(lib, cs, ops, ref.o_st, ref.lse_st)
    if run.mode == "ptr4":
        assert all(run.ptr[n] % 16 == 8 for n in ("q", "k", "v", "o", "dout", "dq"))
    if run.mode == "odd":
        assert all((run.ptr[n] // (2 if cs.dname == "bf16" else 4)) % 2 == 1 for n in ("dk", "dv"))
    got = run.twice(f"{cs.name} psg_attn_bwd_longq")
    ratios, failed = {}, []
    for n in NAMES:                                   # (every output is measured and printed before any verdict)
        try:
            ratios[n] = f"{R.check_all(got, ref, K.DTYPES[cs.dname], cs.name, names=[n], c=K.C_LONGQ)[n]:.3g}"
        except AssertionError as e:
            ratios[n] = "FAIL"
            failed.append(str(e))
    line = (f"gpu {cs.name} {run.mode} tps={K.lq_tps(cs.B, cs.heads, cs.L)} nslab={K.lq_nslab(cs.B, cs.heads, cs.L)} nkt={K.lq_nkt(cs.S)} "
            + " ".join(f"{n}={ratios[n]}" for n in NAMES))
    print(line)
    _report(line)
    assert not failed, "\n".join(failed)


FWD_PAIR = [cs for cs in K.CASES if cs.name in ("kNt1-f32-d64-L65-S97", "kNt1-bf16-d16-L1-S256", "k1t1-bf16-d8-L65-S7", "k1t1-f32-d16-L129-S32")]


@pytest.mark.parametrize("cs", FWD_PAIR, ids=[c.name for c in FWD_PAIR])
def test_longq_on_the_forwards_o_and_lse(lib, cs):
    """The real pairing: o and lse from psg_attn_fwd.  dq, dk and dv are judged by the same bounds; delta against
    rowsum(dO o) of the o the launch was given, within the bound of that sum."""
    from pokemon_sprite_generator_amd import _lib
    assert len(FWD_PAIR) == 4
    ops = _dev(K.operands(cs))
    ref = _reference(cs, ops)
    dtype, HD, H = K.DTYPES[cs.dname], cs.heads * cs.d, cs.heads
    q, k, v = (ops[n].to(dtype).contiguous() for n in ("q", "k", "v"))
    o = torch.full_like(q, float("nan"))
    lse = torch.full((cs.B, H, cs.L), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(lib.psg_attn_fwd(_lib.ptr(q), HD, _lib.ptr(k), HD, _lib.ptr(v), HD, _lib.ptr(o), HD, _lib.ptr(lse), cs.B, H, cs.L, cs.S, cs.d,
                                float(ops["scale"]), 0.0, 0, K.DTYPE_CODE[cs.dname], _lib.stream_ptr()), "psg_attn_fwd")
    _sync("psg_attn_fwd")
    got = Launch(lib, cs, ops, o, lse).twice(f"{cs.name} psg_attn_fwd + psg_attn_bwd_longq")
    ratios = R.check_all(got, ref, dtype, cs.name, names=["dq", "dk", "dv"], c=K.C_LONGQ)
    G, O = R._heads(ops["dout"], H), R._heads(o, H)
    ratios["delta"] = R.check(got["delta"], (G * O).sum(-1), R._sq(cs.d) * (G.abs() * O.abs()).sum(-1), torch.float32, f"{cs.name} delta", c=K.C_LONGQ)
    line = f"gpu-fwd-pair {cs.name} " + " ".join(f"{n}={ratios[n]:.3g}" for n in NAMES)
    print(line)
    _report(line)


OPS_CASES = [K.Case("ops-f32-d16-L130-S32", "f32", 16, 2, 3, 130, 32, "k1t1", 0), K.Case("ops-bf16-d8-L65-S33", "bf16", 8, 3, 3, 65, 33, "kNt1", 0)]


@pytest.mark.parametrize("cs", OPS_CASES, ids=[c.name for c in OPS_CASES])
def test_ops_attention_cross_longq_elementwise(cs):
    """ops.attention_cross_longq(q, kv, heads) through autograd: the pointers and strides the product passes (k | v and dk | dv
    as the halves of [B, S, 2E] buffers).  dq and the two halves of dkv are within the element-wise bounds."""
    from pokemon_sprite_generator_amd import ops as P
    ops = _dev(K.operands(cs))
    ref = _reference(cs, ops)
    dtype, HD = K.DTYPES[cs.dname], cs.heads * cs.d
    q = ops["q"].to(dtype).requires_grad_(True)
    kv = torch.cat([ops["k"], ops["v"]], -1).to(dtype).requires_grad_(True)
    out = P.attention_cross_longq(q, kv, cs.heads)
    out.backward(ops["dout"].to(dtype))
    _sync("ops.attention_cross_longq")
    assert kv.grad.shape == (cs.B, cs.S, 2 * HD)
    got = dict(o=out.detach(), dq=q.grad, dk=kv.grad[:, :, :HD], dv=kv.grad[:, :, HD:])
    ratios = R.check_all(got, ref, dtype, cs.name, names=["o", "dq", "dk", "dv"], c=K.C_LONGQ)
    line = f"gpu-ops {cs.name} " + " ".join(f"{n}={v:.3g}" for n, v in ratios.items())
    print(line)
    _report(line)


@pytest.mark.parametrize("dname", ["f32", "bf16"])
def test_longq_contract(lib, dname):
    """Every host-side refusal returns its code and launches nothing - outputs and workspace are still all NaN after a
    synchronise - and the call inside the contract then returns 0."""
    from pokemon_sprite_generator_amd import _lib
    cs = [c for c in K.CASES if c.dname == dname and K.mode_of(c) == "padded" and c.path == "kNt1"][0]       # (padded: room to move pointers)
    ops = _dev(K.operands(cs))
    ref = _reference(cs, ops)
    run = Launch(lib, cs, ops, ref.o_st, ref.lse_st)
    esz = 2 if dname == "bf16" else 4
    HD = cs.heads * cs.d
    tiny = torch.zeros(64, dtype=torch.float32, device=DEV)
    tp = tiny.data_ptr()
    refusals = [
        ("head_dim 12", _lib.ERR_SHAPE, dict(d=12)),
        ("head_dim 128", _lib.ERR_SHAPE, dict(d=128)),
        ("S = 257", _lib.ERR_SHAPE, dict(S=257)),
        ("row stride below heads d", _lib.ERR_SHAPE, dict(ld=dict(dout=HD - 4))),
        ("row stride no multiple of 4", _lib.ERR_ALIGN, dict(ld=dict(k=run.ld["k"] + 2))),
        ("q one element off", _lib.ERR_ALIGN, dict(ptr=dict(q=run.ptr["q"] + esz))),
        ("dq one element off", _lib.ERR_ALIGN, dict(ptr=dict(dq=run.ptr["dq"] + esz))),
        ("workspace 4 bytes off", _lib.ERR_WORKSPACE, dict(ptr=dict(ws=run.ptr["ws"] + 4))),
        ("workspace 4 bytes short", _lib.ERR_WORKSPACE, dict(ws_bytes=run.need - 4)),
        ("dropout", _lib.ERR_ARG, dict(drop_p=0.1)),
        ("null lse", _lib.ERR_ARG, dict(ptr=dict(lse=None))),
        ("null dv", _lib.ERR_ARG, dict(ptr=dict(dv=None))),
        ("B heads = 65536", _lib.ERR_SHAPE, dict(B=256, heads=256, L=1, S=1, d=4, ld={n: 1024 for n in K.OPERANDS}, ptr={n: tp for n in run.ptr})),
    ]
    for what, code, over in refusals:
        run.reset()
        assert run.call(**over) == code, what
        assert lib.psg_last_error(), what
        _sync(what)
        assert run.untouched(), f"{what}: refused, yet something was written"
        assert not bool(tiny.any()), what
        assert run.call() == 0, f"after {what}"
        _sync(what)
        assert not bool(torch.isnan(run.ws.out).any()) and run.intact() is None
    got = run.outputs()
    R.check_all(got, ref, K.DTYPES[dname], cs.name, names=list(NAMES), c=K.C_LONGQ)
