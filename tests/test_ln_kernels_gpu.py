"""-m gpu: the row kernels of csrc/text_encoder.hip on every instantiation, through the C ABI (psg_layernorm, psg_layernorm_bwd,
psg_bert_embed_ln, psg_bert_embed_ln_bwd, psg_embed_scatter) and through ops.layer_norm, element by element against the fp64
references and bounds of tests/ln_ref.py on the cases of tests/ln_cases.py.

Per launch: operands sit in row buffers of their own stride whose padding columns hold NaN (inputs) or a sentinel (outputs);
outputs lie between guard rows, dgamma / dbeta / the workspace (allocated at exactly *_workspace_bytes) before guard
elements; outputs pre-filled with NaN hold none afterwards; guards and padding keep their bits; a second identical launch
gives identical bits; and every element lies within its bound.  Besides the bounds, the bit identities the kernel file's
header states: a row's bits do not depend on the launch geometry, the residual as an operand equals the pre-added input,
accumulate = 1 is the prefill plus the accumulate = 0 result, NULL outputs change no other output, and the embedding kernels
are the LayerNorm kernels on the fp32 rows (word[id] + type[tt]) + pos[s].  A device error ends the run."""
import os
import time
import types

import pytest
import torch

from tests import ln_cases as K
from tests import ln_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
SENTINEL = 77.0                                # guard rows, padding columns of outputs, guard elements (exact in bf16)
GUARD = 64                                     # guard elements behind a flat output; guard bytes behind a workspace: 4 x
REPORT = os.environ.get("PSG_LN_REPORT")      # optional: append the worst err / bound per kernel, output and dtypes to this file
_WORST, _T = {}, {"t0": None, "n": 0}


def _note(key, ratio):
    _T["n"] += 1
    R.worst(_WORST, key, ratio)


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    lib = _lib.init(0)
    _T["t0"] = time.perf_counter()
    yield lib
    lines = [f"gpu {k:<44s} {_WORST[k]:.3g}" for k in sorted(_WORST)]
    lines.append(f"gpu comparisons {_T['n']}, wall time of the file {time.perf_counter() - _T['t0']:.1f} s")
    print("\n" + "\n".join(lines))
    if REPORT:
        with open(REPORT, "a") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture(scope="module")
def chunk(lib):
    return lib.psg_embed_scatter_chunk_rows()


def _sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                   # a device error: nothing more runs on this GPU
        pytest.exit(f"{what}: {e}", returncode=3)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _ptr(t):
    from pokemon_sprite_generator_amd._lib import ptr
    return ptr(t)


def _code(dt):
    from pokemon_sprite_generator_amd._lib import dtype_code
    return dtype_code(dt)


class In:
    """An input [rows, N] at row stride ld (class: the row-0 view of a [rows, 50, N] tensor); everything around it is NaN."""

    def __init__(self, values, ld, dtype, cls=False):
        rows, N = values.shape
        if cls:
            assert ld == K.CLASS_TOKENS * N
            self.buf = torch.full((rows, K.CLASS_TOKENS, N), NAN, dtype=dtype, device=DEV)
            self.view = self.buf[:, 0, :]
        else:
            self.buf = torch.full((rows, ld), NAN, dtype=dtype, device=DEV)
            self.view = self.buf[:, :N]
        self.view.copy_(values)
        self.ld = ld
        assert self.view.stride(0) == ld
        self.before = _bits(self.buf).clone()

    def unchanged(self):
        return torch.equal(_bits(self.buf), self.before)


class Out:
    """An output [rows, N] at row stride ld between two guard rows; the padding columns and the guard rows hold SENTINEL."""

    def __init__(self, rows, N, ld, dtype):
        self.buf = torch.full((rows + 2, ld), SENTINEL, dtype=dtype, device=DEV)
        self.view = self.buf[1:-1, :N]
        self.ld, self.N = ld, N

    def reset(self, values=None):
        self.view.fill_(NAN) if values is None else self.view.copy_(values)

    def guards_intact(self):
        return bool((self.buf[0] == SENTINEL).all()) and bool((self.buf[-1] == SENTINEL).all()) and bool((self.buf[1:-1, self.N:] == SENTINEL).all())


class Flat:
    """n fp32 outputs followed by guard elements in the same allocation."""

    def __init__(self, n):
        self.buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        self.out, self.n = self.buf[:n], n

    def reset(self, values=None):
        self.out.fill_(NAN) if values is None else self.out.copy_(values)

    def guards_intact(self):
        return bool((self.buf[self.n:] == SENTINEL).all())


class Workspace:
    """Exactly nbytes of NaN-filled workspace and guard elements behind it (nbytes = 0: no workspace, a NULL pointer)."""

    def __init__(self, nbytes):
        assert nbytes % 16 == 0
        self.nbytes, self.n = nbytes, nbytes // 4
        self.buf = torch.full((self.n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        self.buf[:self.n].fill_(NAN)

    def ptr(self):
        return _ptr(self.buf if self.nbytes else None)

    def guards_intact(self):
        return bool((self.buf[self.n:] == SENTINEL).all())


def _dev(ops):
    def dev(v):
        return tuple(dev(t) for t in v) if isinstance(v, tuple) else (v.to(DEV) if torch.is_tensor(v) else v)
    return {k: dev(v) for k, v in ops.items()}


# ---------------------------------------------------------------------------------------------------------------- launches
def ln_forward(lib, x, r, y, gamma, beta, eps, runs=2):
    """psg_layernorm of In x (+ In r) into Out y, `runs` times; the invariants; returns the first run's y (a copy)."""
    from pokemon_sprite_generator_amd import _lib
    rows, N = x.view.shape
    got = []
    for _ in range(runs):
        y.reset()
        _lib.check(lib.psg_layernorm(_ptr(x.view), x.ld, _ptr(r.view if r else None), r.ld if r else 0, _ptr(y.view), y.ld, _ptr(gamma), _ptr(beta),
                                     rows, N, float(eps), _code(x.view.dtype), _code(y.view.dtype), _lib.stream_ptr()), "psg_layernorm")
        _sync("psg_layernorm")
        got.append(y.view.clone())
    assert x.unchanged() and (r is None or r.unchanged()), "the forward wrote into an input"
    assert y.guards_intact(), "the forward wrote into y's guard rows or padding columns"
    assert all(_same(got[0], g) for g in got[1:]), "y: a second identical launch gives other bits"
    return got[0]


def ln_backward(lib, x, r, dy, gamma, dz, dg, db, ws, eps, accumulate=0, prefill=None, runs=2):
    """psg_layernorm_bwd into Out dz and the Flat dg / db (None: a NULL output); returns the first run's dict of copies."""
    from pokemon_sprite_generator_amd import _lib
    rows, N = x.view.shape
    got = []
    for _ in range(runs):
        dz.reset()
        for f, p in ((dg, 0), (db, 1)):
            if f is not None:
                f.reset(prefill[p] if accumulate else None)
        _lib.check(lib.psg_layernorm_bwd(_ptr(x.view), x.ld, _ptr(r.view if r else None), r.ld if r else 0, _ptr(dy.view), dy.ld, _ptr(gamma),
                                         _ptr(dz.view), dz.ld, _ptr(dg.out if dg else None), _ptr(db.out if db else None), int(accumulate), rows, N,
                                         float(eps), _code(x.view.dtype), _code(dy.view.dtype), ws.ptr(), ws.nbytes, _lib.stream_ptr()),
                   "psg_layernorm_bwd")
        _sync("psg_layernorm_bwd")
        got.append(dict(dz=dz.view.clone(), **({"dgamma": dg.out.clone()} if dg else {}), **({"dbeta": db.out.clone()} if db else {})))
    assert x.unchanged() and dy.unchanged() and (r is None or r.unchanged()), "the backward wrote into an input"
    assert dz.guards_intact(), "the backward wrote into dz's guard rows or padding columns"
    assert all(f is None or f.guards_intact() for f in (dg, db)) and ws.guards_intact(), "the backward wrote behind dgamma / dbeta / the workspace"
    for n, t in got[0].items():
        assert all(_same(t, g[n]) for g in got[1:]), f"{n}: a second identical launch gives other bits"
    return got[0]


def _ln_operands(v, ops):
    ld = K.strides(v)
    xd, od = K.DTYPES[v["xd"]], K.DTYPES[v["od"]]
    x = In(ops["x"], ld["x"], xd, cls=v["stride"] == "class")
    r = In(ops["r"], ld["r"], xd) if v["res"] else None
    dy = In(ops["dy"], ld["dy"], od)
    return x, r, dy, Out(v["rows"], v["N"], ld["y"], od), Out(v["rows"], v["N"], ld["dz"], xd)


def _no_nan(got, what):
    for n, t in got.items():
        assert not bool(torch.isnan(t.float()).any()), f"{what}: {n} still holds NaN"


# -------------------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("shape", K.shapes(), ids=[f"N{n}-r{r}" for n, r in K.shapes()])
def test_layernorm_cases(lib, shape):
    """The eight launches of a shape (every dtype pair, with and without a residual), forward and backward."""
    for v in K.variants(*shape):
        N, rows = v["N"], v["rows"]
        xd, od = K.DTYPES[v["xd"]], K.DTYPES[v["od"]]
        ops = _dev(K.operands(v))
        what = K.vid(v)
        x, r, dy, y, dz = _ln_operands(v, ops)
        dg, db = Flat(N), Flat(N)
        need = lib.psg_layernorm_bwd_workspace_bytes(rows, N)
        assert need == 2 * R.nwg_bwd(rows) * N * 4
        ws = Workspace(need)
        got = dict(y=ln_forward(lib, x, r, y, ops["gamma"], ops["beta"], v["eps"]))
        got.update(ln_backward(lib, x, r, dy, ops["gamma"], dz, dg, db, ws, v["eps"]))
        _no_nan(got, what)
        o = R.reference(ops["x"], ops["r"], ops["gamma"], ops["beta"], v["eps"], dy=ops["dy"])
        ratios = R.check_all(got, o, xd, od, what)
        if v["accumulate"]:                                # the prefill plus the accumulate = 0 result, to the bit; and within the bound
            acc = ln_backward(lib, x, r, dy, ops["gamma"], dz, dg, db, ws, v["eps"], accumulate=1, prefill=ops["prefill"])
            assert _same(acc["dz"], got["dz"]), f"{what}: dz depends on accumulate"
            for n, p in (("dgamma", 0), ("dbeta", 1)):
                assert _same(acc[n], ops["prefill"][p] + got[n]), f"{what}: accumulate = 1 is not the prefill + the accumulate = 0 {n}"
            oa = R.reference(ops["x"], ops["r"], ops["gamma"], ops["beta"], v["eps"], dy=ops["dy"], prefill=ops["prefill"])
            for n, val in R.check_all(acc, oa, xd, od, what + " accumulate", names=("dgamma", "dbeta")).items():
                ratios[n] = max(ratios[n], val)
        for n, val in ratios.items():
            _note(f"layernorm{'_bwd' if n != 'y' else ''} {v['xd']}>{v['od']} {n}", val)
        if v["kind"] == "const":
            assert bool(torch.isfinite(got["y"][K.const_row(rows)].float()).all()) and bool(torch.isfinite(got["dz"][K.const_row(rows)].float()).all())
        if rows > K.GEOMETRY_ROWS[1]:                      # a row's bits do not depend on the launch geometry
            a, b = K.GEOMETRY_ROWS
            sub = dict(v, rows=b - a, stride="contiguous")
            xs, rs, dys, ys, dzs = _ln_operands(sub, {k: (t[a:b] if k in ("x", "r", "dy") and t is not None else t) for k, t in ops.items()})
            assert _same(ln_forward(lib, xs, rs, ys, ops["gamma"], ops["beta"], v["eps"], runs=1), got["y"][a:b]), f"{what}: y bits of rows {a}:{b}"
            small = ln_backward(lib, xs, rs, dys, ops["gamma"], dzs, None, None, Workspace(0), v["eps"], runs=1)
            assert _same(small["dz"], got["dz"][a:b]), f"{what}: dz bits of rows {a}:{b} depend on the launch geometry"


@pytest.mark.parametrize("N", K.NULL_WIDTHS)
def test_layernorm_bwd_null_outputs(lib, N):
    """dgamma only, dbeta only, neither (the PG = false instantiation): dz has the same bits in all three, the output that is
    asked for too, and what is not asked for is not written."""
    for v in K.variants(N, K.ROWS_ALL_N):
        ops = _dev(K.operands(v))
        x, r, dy, y, dz = _ln_operands(v, ops)
        need = lib.psg_layernorm_bwd_workspace_bytes(v["rows"], N)
        full = ln_backward(lib, x, r, dy, ops["gamma"], dz, Flat(N), Flat(N), Workspace(need), v["eps"], runs=1)
        dg, db = Flat(N), Flat(N)
        only_g = ln_backward(lib, x, r, dy, ops["gamma"], dz, dg, None, Workspace(need), v["eps"], runs=1)
        assert _same(only_g["dz"], full["dz"]) and _same(only_g["dgamma"], full["dgamma"]), K.vid(v)
        only_b = ln_backward(lib, x, r, dy, ops["gamma"], dz, None, db, Workspace(need), v["eps"], runs=1)
        assert _same(only_b["dz"], full["dz"]) and _same(only_b["dbeta"], full["dbeta"]), K.vid(v)
        assert _same(dg.out, full["dgamma"]) and dg.guards_intact() and db.guards_intact()       # the later launch left dgamma alone
        none = ln_backward(lib, x, r, dy, ops["gamma"], dz, None, None, Workspace(0), v["eps"])
        assert _same(none["dz"], full["dz"]), f"{K.vid(v)}: dz of the PG = false instantiation has other bits"
        o = R.reference(ops["x"], ops["r"], ops["gamma"], ops["beta"], v["eps"], dy=ops["dy"])
        _note(f"layernorm_bwd {v['xd']}>{v['od']} dz (no dgamma / dbeta)", R.check(none["dz"], o, "dz", K.DTYPES[v["xd"]], K.vid(v) + " PG=false"))


@pytest.mark.parametrize("N", K.NULL_WIDTHS + [768])
def test_residual_operand_equals_the_pre_added_input(lib, N):
    """fp32: the residual is an operand of the kernels, not an extra pass - y, dz, dgamma and dbeta have the bits of the launch
    on x + r (one width per CPL)."""
    v = dict(N=N, rows=K.ROWS_ALL_N, xd="f32", od="f32", res=True, kind="plain", stride="padded", eps=1e-12, accumulate=False)
    ops = _dev(K.operands(v))
    x, r, dy, y, dz = _ln_operands(v, ops)
    ws = Workspace(lib.psg_layernorm_bwd_workspace_bytes(v["rows"], N))
    a = dict(y=ln_forward(lib, x, r, y, ops["gamma"], ops["beta"], v["eps"], runs=1))
    a.update(ln_backward(lib, x, r, dy, ops["gamma"], dz, Flat(N), Flat(N), ws, v["eps"], runs=1))
    xr = In(ops["x"] + ops["r"], K.strides(v)["x"], torch.float32)
    b = dict(y=ln_forward(lib, xr, None, y, ops["gamma"], ops["beta"], v["eps"], runs=1))
    b.update(ln_backward(lib, xr, None, dy, ops["gamma"], dz, Flat(N), Flat(N), ws, v["eps"], runs=1))
    for n in R.OUTPUTS:
        assert _same(a[n], b[n]), f"N={N}: {n} with the residual as an operand differs from the pre-added input"


def test_nan_row_leaves_the_other_rows_alone(lib):
    v = dict(N=768, rows=K.ROWS_ALL_N, xd="bf16", od="f32", res=False, kind="plain", stride="contiguous", eps=1e-12, accumulate=False)
    ops = _dev(K.operands(v))
    x, r, dy, y, dz = _ln_operands(v, ops)
    clean = ln_forward(lib, x, r, y, ops["gamma"], ops["beta"], v["eps"], runs=1)
    bad = ops["x"].clone()
    bad[9, 300] = NAN
    got = ln_forward(lib, In(bad, v["N"], torch.bfloat16), None, y, ops["gamma"], ops["beta"], v["eps"], runs=1)
    keep = torch.arange(v["rows"], device=DEV) != 9
    assert bool(torch.isnan(got[9]).all()) and _same(got[keep], clean[keep])


# ------------------------------------------------------------------------------------------------------------ embeddings
def _embed_launch(lib, v, ops, y, dz, dg, db, ws, accumulate=0):
    from pokemon_sprite_generator_amd import _lib
    N, B, S = v["N"], v["B"], v["S"]
    V, P, T = ops["word"].shape[0], ops["pos"].shape[0], ops["typ"].shape[0]
    dt = K.DTYPES[v["dname"]]
    tabs = (_ptr(ops["ids"]), _ptr(ops["tt"]), _ptr(ops["word"]), _ptr(ops["pos"]), _ptr(ops["typ"]), _ptr(ops["gamma"]))
    out = {}
    if y is not None:
        y.reset()
        _lib.check(lib.psg_bert_embed_ln(*tabs, _ptr(ops["beta"]), _ptr(y.view), y.ld, B, S, N, V, P, T, float(v["eps"]), _code(dt),
                                         _lib.stream_ptr()), "psg_bert_embed_ln")
        _sync("psg_bert_embed_ln")
        out["y"] = y.view.clone()
        assert y.guards_intact(), "psg_bert_embed_ln wrote into y's guard rows or padding columns"
    if dz is not None:
        dz.reset()
        for f, p in ((dg, 0), (db, 1)):
            if f is not None:
                f.reset(ops["prefill"][p] if accumulate else None)
        _lib.check(lib.psg_bert_embed_ln_bwd(*tabs, _ptr(ops["dyb"].view), ops["dyb"].ld, _ptr(dz.view), _ptr(dg.out if dg else None),
                                             _ptr(db.out if db else None), int(accumulate), B, S, N, V, P, T, float(v["eps"]), _code(dt), ws.ptr(),
                                             ws.nbytes, _lib.stream_ptr()), "psg_bert_embed_ln_bwd")
        _sync("psg_bert_embed_ln_bwd")
        out["dz"] = dz.view.clone()
        for n, f in (("dgamma", dg), ("dbeta", db)):
            if f is not None:
                out[n] = f.out.clone()
        assert dz.guards_intact() and all(f is None or f.guards_intact() for f in (dg, db)) and ws.guards_intact(), \
            "psg_bert_embed_ln_bwd wrote behind dz / dgamma / dbeta / the workspace"
        assert ops["dyb"].unchanged()
    return out


@pytest.mark.parametrize("v", K.embed_variants(), ids=[K.embed_vid(v) for v in K.embed_variants()])
def test_embedding_cases(lib, v):
    N, B, S = v["N"], v["B"], v["S"]
    rows = B * S
    dt = K.DTYPES[v["dname"]]
    ops = _dev(K.embed_operands(v))
    ops["dyb"] = In(ops["dy"], v["lddy"], dt)
    what = K.embed_vid(v)
    y, dz, dg, db = Out(rows, N, v["ldy"], dt), Out(rows, N, N, torch.float32), Flat(N), Flat(N)
    need = lib.psg_bert_embed_ln_bwd_workspace_bytes(rows, N)
    assert need == lib.psg_layernorm_bwd_workspace_bytes(rows, N)
    got = _embed_launch(lib, v, ops, y, dz, dg, db, Workspace(need))
    again = _embed_launch(lib, v, ops, y, dz, dg, db, Workspace(need))
    o = R.embed_reference_bounds(ops["ids"], ops["tt"], ops["word"], ops["pos"], ops["typ"], ops["gamma"], ops["beta"], v["eps"], ops["dy"])
    valid = o.valid
    bad_rows = [r for r, _ in K.embed_bad_rows(v)] if v["bad"] else []
    assert (~valid).nonzero().view(-1).tolist() == sorted(bad_rows)
    # rows outside the tables: NaN forward, an exactly zero dz row; everything else finite and the same bits again
    assert bool(torch.isnan(got["y"][~valid].float()).all()) and not bool(got["dz"][~valid].any())
    assert _same(got["y"][valid], again["y"][valid]) and all(_same(got[n], again[n]) for n in ("dz", "dgamma", "dbeta")), what
    _no_nan(dict(got, y=got["y"][valid]), what)
    # element-wise against embed_reference (the rows outside the tables have no share in dgamma / dbeta; their neighbours are whole)
    oy = types.SimpleNamespace(y=o.y[valid], y_mag=o.y_mag[valid], y_extra=o.y_extra[valid])
    _note(f"embed_ln {v['dname']} y", R.check(got["y"][valid], oy, "y", dt, what))
    for n, val in R.check_all(got, o, torch.float32, dt, what, names=("dz", "dgamma", "dbeta")).items():
        _note(f"embed_ln_bwd {v['dname']} {n}", val)
    if v["accumulate"]:
        acc = _embed_launch(lib, v, ops, None, dz, dg, db, Workspace(need), accumulate=1)
        assert _same(acc["dz"], got["dz"])
        for n, p in (("dgamma", 0), ("dbeta", 1)):
            assert _same(acc[n], ops["prefill"][p] + got[n]), f"{what}: accumulate = 1 is not the prefill + the accumulate = 0 {n}"
    # the embedding kernels are the LayerNorm kernels on the fp32 rows torch forms in the kernels' association
    z, _ = R.embed_rows(ops["ids"], ops["tt"], ops["word"], ops["pos"], ops["typ"])
    zin = In(z, N, torch.float32)
    yl = ln_forward(lib, zin, None, Out(rows, N, N, dt), ops["gamma"], ops["beta"], v["eps"], runs=1)
    assert _same(got["y"][valid], yl[valid]), f"{what}: psg_bert_embed_ln differs from psg_layernorm on the same fp32 rows"
    if not v["bad"]:
        lb = ln_backward(lib, zin, None, ops["dyb"], ops["gamma"], Out(rows, N, N, torch.float32), Flat(N), Flat(N), Workspace(need), v["eps"], runs=1)
        for n in ("dz", "dgamma", "dbeta"):
            assert _same(got[n], lb[n]), f"{what}: psg_bert_embed_ln_bwd's {n} differs from psg_layernorm_bwd's on the same fp32 rows"


@pytest.mark.parametrize("v", K.embed_null_output_variants(), ids=[K.embed_vid(v) for v in K.embed_null_output_variants()])
def test_embedding_bwd_null_outputs(lib, v):
    N, rows = v["N"], v["B"] * v["S"]
    dt = K.DTYPES[v["dname"]]
    ops = _dev(K.embed_operands(v))
    ops["dyb"] = In(ops["dy"], v["lddy"], dt)
    need = lib.psg_bert_embed_ln_bwd_workspace_bytes(rows, N)
    dz = Out(rows, N, N, torch.float32)
    full = _embed_launch(lib, v, ops, None, dz, Flat(N), Flat(N), Workspace(need))
    only_g = _embed_launch(lib, v, ops, None, dz, Flat(N), None, Workspace(need))
    only_b = _embed_launch(lib, v, ops, None, dz, None, Flat(N), Workspace(need))
    none = _embed_launch(lib, v, ops, None, dz, None, None, Workspace(0))
    assert _same(only_g["dz"], full["dz"]) and _same(only_b["dz"], full["dz"]) and _same(none["dz"], full["dz"]), K.embed_vid(v)
    assert _same(only_g["dgamma"], full["dgamma"]) and _same(only_b["dbeta"], full["dbeta"])
    o = R.embed_reference_bounds(ops["ids"], ops["tt"], ops["word"], ops["pos"], ops["typ"], ops["gamma"], ops["beta"], v["eps"], ops["dy"])
    _note(f"embed_ln_bwd {v['dname']} dz (no dgamma / dbeta)", R.check(none["dz"], o, "dz", torch.float32, K.embed_vid(v) + " PG=false"))


# --------------------------------------------------------------------------------------------------------------- scatter
def _scatter(lib, o, dz, table, ws, accumulate):
    from pokemon_sprite_generator_amd import _lib
    N = table.N
    table.reset(o["prefill"] if accumulate else None)
    _lib.check(lib.psg_embed_scatter(_ptr(dz.view), dz.ld, _ptr(o["key"]), _ptr(o["perm"]), _ptr(table.view), o["rows"], N, o["V"], o["skip"],
                                     int(accumulate), ws.ptr(), ws.nbytes, _lib.stream_ptr()), "psg_embed_scatter")
    _sync("psg_embed_scatter")
    assert dz.unchanged() and table.guards_intact() and ws.guards_intact(), "psg_embed_scatter wrote outside the table or the workspace"
    return table.view.clone()


def _scatter_ids(chunk=32):
    return [f"{n}-N{N}-ld{ld}" for n, N, ld in K.scatter_cases(chunk)]


@pytest.mark.parametrize("case", range(len(K.scatter_cases(32))), ids=_scatter_ids())
def test_scatter_cases(lib, chunk, case):
    """Integer-valued rows: equal to the fp64 sum bit for bit; random rows: within the bound of the run's length.  A row that no
    live key names is exactly zero (accumulate = 0) or keeps the bits of the prefill (accumulate = 1)."""
    name, N, lddz = K.scatter_cases(chunk)[case]
    if name in ("long", "edges"):
        key = K.scatter_keys(K.scatter_layouts(chunk)[name][0])
        assert name != "long" or K.later_chunk_starts(key, chunk, K.HOT) >= 5
    for integer in (True, False):
        o = _dev(K.scatter_operands(name, N, chunk, integer))
        need = lib.psg_embed_scatter_workspace_bytes(o["rows"], N)
        assert need == o["rows"] * N * 4
        dz = In(o["dz"], lddz, torch.float32)
        table = Out(o["V"], N, N, torch.float32)
        for acc in (0, 1):
            got = _scatter(lib, o, dz, table, Workspace(need), acc)
            again = _scatter(lib, o, dz, table, Workspace(need), acc)
            what = f"scatter {name} N={N} lddz={lddz} {'integer' if integer else 'random'} accumulate={acc}"
            assert _same(got, again), f"{what}: a second identical launch gives other bits"
            ref, S, run, named = R.scatter_reference(o["dz"], o["key"], o["perm"], o["V"], o["skip"], prefill=o["prefill"] if acc else None)
            if acc:
                assert _same(got[~named], o["prefill"][~named]), f"{what}: a row that no key names lost the bits of the prefill"
            else:
                assert not bool(_bits(got[~named]).any()), f"{what}: a row that no key names is not exactly zero"
            if integer:
                assert torch.equal(got.double(), ref), f"{what}: not the exact sum"
                _note("embed_scatter integer (exact)", 0.0)
            else:
                _note(f"embed_scatter random accumulate={acc}", R.check_scatter(got, ref, S, run, acc, what))


# ------------------------------------------------------------------------------------------------------------ through ops
@pytest.mark.parametrize("dname", list(K.DTYPES))
def test_ops_layer_norm_on_the_class_row_view(lib, dname):
    """ops.layer_norm forward and backward on x[:, 0, :] of a [4, 50, 768] tensor (the CLIP towers' class row: ldx = 50 x 768
    reaches both launches without a copy), element-wise against the reference."""
    from pokemon_sprite_generator_amd import ops
    dt = K.DTYPES[dname]
    B, N, eps = 4, 768, 1e-5
    full = (K.h((B, K.CLASS_TOKENS, N), "ops.cls.x", 3.0) + 0.5).to(dt).to(DEV).requires_grad_(True)
    g = (1.0 + K.h((N,), "ops.cls.g", 0.3)).to(DEV).requires_grad_(True)
    b = K.h((N,), "ops.cls.b", 0.2).to(DEV).requires_grad_(True)
    dy = K.h((B, N), "ops.cls.dy").to(dt).to(DEV)
    x = full[:, 0, :]
    assert ops._rows(x.detach())[1] == K.CLASS_TOKENS * N
    copies = ops.RowCopies.bytes
    y = ops.layer_norm(x, g, b, eps)
    y.backward(dy)
    _sync("ops.layer_norm")
    assert ops.RowCopies.bytes == copies, "the class-row view was copied"
    assert y.dtype == dt and full.grad.dtype == dt and not bool(full.grad[:, 1:].any())
    o = R.reference(x.detach(), None, g.detach(), b.detach(), eps, dy=dy)
    got = dict(y=y.detach(), dz=full.grad[:, 0, :], dgamma=g.grad, dbeta=b.grad)
    for n, val in R.check_all(got, o, dt, dt, f"ops.layer_norm class row {dname}").items():
        _note(f"ops.layer_norm class row {dname}>{dname} {n}", val)


def test_ops_layer_norm_bf16_out_of_fp32(lib):
    from pokemon_sprite_generator_amd import ops
    rows, N, eps = 21, 768, 1e-12
    x = (K.h((rows, N), "ops.mix.x", 3.0) + 0.5).to(DEV).requires_grad_(True)
    g = (1.0 + K.h((N,), "ops.mix.g", 0.3)).to(DEV).requires_grad_(True)
    b = K.h((N,), "ops.mix.b", 0.2).to(DEV).requires_grad_(True)
    dy = K.h((rows, N), "ops.mix.dy").to(torch.bfloat16).to(DEV)
    y = ops.layer_norm(x, g, b, eps, out_dtype=torch.bfloat16)
    y.backward(dy)
    _sync("ops.layer_norm")
    assert y.dtype == torch.bfloat16 and x.grad.dtype == torch.float32
    o = R.reference(x.detach(), None, g.detach(), b.detach(), eps, dy=dy)
    got = dict(y=y.detach(), dz=x.grad, dgamma=g.grad, dbeta=b.grad)
    for n, val in R.check_all(got, o, torch.float32, torch.bfloat16, "ops.layer_norm f32>bf16").items():
        _note(f"ops.layer_norm f32>bf16 {n}", val)
