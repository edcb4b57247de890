"""-m gpu: every GroupNorm route and kernel variant, through the C ABI (psg_groupnorm_fwd, psg_groupnorm_bwd_res), element by
element against the fp64 reference and bounds of tests/gn_ref.py on the cases of tests/gn_cases.py.

Per launch: the route is the one the table stores (psg_groupnorm_route, asserted before the launch); y, mean, rstd, dx, dgamma
and dbeta are within their bounds at every element; outputs pre-filled with NaN hold none afterwards; the padding columns
between C and the row stride, the inputs, and the guard regions behind the statistics, the parameter gradients and the
workspace (allocated at exactly psg_groupnorm_*_workspace_bytes, NaN-filled) keep their bits; and a second identical launch
gives identical bits (the reductions are fixed-order).  The backward launch reads the reference's mean / rstd rounded to
fp32, so each direction is judged on its own."""
import os

import pytest
import torch

from tests import gn_cases as K
from tests import gn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256                                    # elements of guard behind every flat output
REPORT = os.environ.get("PSG_GN_REPORT")      # optional: append the fraction of its bound each output used to this file


def _report(line):
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    return _lib.init(0)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else (torch.int32 if t.element_size() == 4 else torch.uint8))


class Rows:
    """A [B, HW, C] operand inside a wider buffer [B * HW, ld] at column `off`: the padding holds a sentinel."""

    def __init__(self, shape, ld_off, dtype, values=None):
        B, HW, C, _ = shape
        ld, off = ld_off
        self.ld, self.C, self.off = ld, C, off
        self.buf = torch.full((B, HW, ld), -1234.5, dtype=dtype, device=DEV)
        self.view = self.buf[:, :, off:off + C]
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
        return ptr(self.view)                                   # (data_ptr of a view includes its offset)

    def padding_intact(self):
        now, was = _bits(self.buf), self.before
        return torch.equal(now[:, :, :self.off], was[:, :, :self.off]) and torch.equal(now[:, :, self.off + self.C:], was[:, :, self.off + self.C:])

    def unchanged(self):
        return torch.equal(_bits(self.buf), self.before)


class Flat:
    """n fp32 outputs followed by a guard region in the same allocation."""

    def __init__(self, n, values=None):
        self.n, self.values = n, values
        self.buf = torch.full((n + GUARD,), -4321.0, dtype=torch.float32, device=DEV)
        self.out = self.buf[:n]
        self.reset()

    def reset(self):
        if self.values is None:
            self.out.fill_(float("nan"))
        else:
            self.out.copy_(self.values)

    def guard_intact(self):
        return bool((self.buf[self.n:] == -4321.0).all())


class Workspace:
    """Exactly `nbytes` of NaN-filled workspace, a guard region behind it."""

    def __init__(self, nbytes):
        assert nbytes % 4 == 0
        self.buf = torch.full((nbytes // 4 + GUARD,), -4321.0, dtype=torch.float32, device=DEV)
        self.n = nbytes // 4
        self.reset()

    def reset(self):
        self.buf[:self.n].fill_(float("nan"))

    def guard_intact(self):
        return bool((self.buf[self.n:] == -4321.0).all())


def _dev(ops):
    return {k: (tuple(t.to(DEV) for t in v) if isinstance(v, tuple) else v.to(DEV)) for k, v in ops.items()}


def _forward(lib, shape, dname, var, ops, strides):
    """Launch the forward twice; returns the outputs of the first launch after the invariants held."""
    from pokemon_sprite_generator_amd import _lib
    B, HW, C, G = shape
    dtype = K.DTYPES[dname]
    x = Rows(shape, strides["x"], dtype, ops["x"])
    y = Rows(shape, strides["y"], dtype)
    gamma, beta = ops["gamma"].contiguous(), ops["beta"].contiguous()
    mean, rstd = Flat(B * G), Flat(B * G)
    ws = Workspace(lib.psg_groupnorm_fwd_workspace_bytes(B, G))
    runs = []
    for _ in range(2):
        for o in (y, mean, rstd, ws):
            o.reset()
        _lib.check(lib.psg_groupnorm_fwd(x.ptr(), x.ld, y.ptr(), y.ld, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(mean.out), _lib.ptr(rstd.out),
                                         B, HW, C, G, float(var["eps"]), int(var["silu"]), K.DTYPE_CODE[dname], _lib.ptr(ws.buf),
                                         _lib.stream_ptr()), "psg_groupnorm_fwd")
        torch.cuda.synchronize()
        runs.append(dict(y=y.view.clone(), mean=mean.out.clone().reshape(B, G), rstd=rstd.out.clone().reshape(B, G)))
    assert x.unchanged(), "the forward wrote into x"
    assert y.padding_intact(), "the forward wrote into y's padding columns"
    assert mean.guard_intact() and rstd.guard_intact() and ws.guard_intact(), "the forward wrote behind mean / rstd / the workspace"
    for n, t in runs[0].items():
        assert not bool(torch.isnan(t).any()), f"{n} still holds NaN"
        assert torch.equal(_bits(t), _bits(runs[1][n])), f"{n}: a second identical launch gives other bits"
    return runs[0]


def _backward(lib, shape, dname, var, ops, strides, ref):
    from pokemon_sprite_generator_amd import _lib
    B, HW, C, G = shape
    dtype = K.DTYPES[dname]
    x = Rows(shape, strides["x"], dtype, ops["x"])
    dy = Rows(shape, strides["dy"], dtype, ops["dy"])
    dres = Rows(shape, strides["dres"], dtype, ops["dres"]) if var["dres"] else None
    dx = Rows(shape, strides["dx"], dtype)
    gamma, beta = ops["gamma"].contiguous(), ops["beta"].contiguous()
    mean, rstd = ref.mean.float().reshape(-1).contiguous(), ref.rstd.float().reshape(-1).contiguous()
    pre = ops["prefill"] if var["accumulate"] else (None, None)
    dgamma, dbeta = Flat(C, pre[0]), Flat(C, pre[1])
    ws = Workspace(lib.psg_groupnorm_bwd_workspace_bytes(B, C))
    runs = []
    for _ in range(2):
        for o in (dx, dgamma, dbeta, ws):
            o.reset()
        _lib.check(lib.psg_groupnorm_bwd_res(dy.ptr(), dy.ld, x.ptr(), x.ld, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(mean), _lib.ptr(rstd),
                                             dres.ptr() if dres else None, dres.ld if dres else 0, dx.ptr(), dx.ld, _lib.ptr(dgamma.out),
                                             _lib.ptr(dbeta.out), B, HW, C, G, int(var["silu"]), int(var["accumulate"]), K.DTYPE_CODE[dname],
                                             _lib.ptr(ws.buf), _lib.stream_ptr()), "psg_groupnorm_bwd_res")
        torch.cuda.synchronize()
        runs.append(dict(dx=dx.view.clone(), dgamma=dgamma.out.clone(), dbeta=dbeta.out.clone()))
    assert x.unchanged() and dy.unchanged() and (dres is None or dres.unchanged()), "the backward wrote into an input"
    assert dx.padding_intact(), "the backward wrote into dx's padding columns"
    assert dgamma.guard_intact() and dbeta.guard_intact() and ws.guard_intact(), "the backward wrote behind dgamma / dbeta / the workspace"
    for n, t in runs[0].items():
        assert not bool(torch.isnan(t).any()), f"{n} still holds NaN"
        assert torch.equal(_bits(t), _bits(runs[1][n])), f"{n}: a second identical launch gives other bits"
    return runs[0]


def _assert_route(lib, shape, dname, backward, dres):
    rc, got = K.query_route(lib, backward, dname, *shape, dres)
    want = K.expected_route(shape, dname, backward, dres)
    assert rc == 0 and got == want, f"route of {shape} {dname} backward={backward} dres={dres}: {dict(zip(K.ROUTE_FIELDS, got))}, " \
                                    f"table {dict(zip(K.ROUTE_FIELDS, want))}"
    rt = dict(zip(K.ROUTE_FIELDS, got))
    return f"fused/N{rt['N']}/R{rt['R']}" if rt["fused"] else f"split/NS{rt['NS']}"


_IDS = [i for i, _ in K.case_ids()]
_SHAPES = [s for _, s in K.case_ids()]


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("dname", list(K.DTYPES))
@pytest.mark.parametrize("shape", _SHAPES, ids=_IDS)
def test_groupnorm_routes(lib, shape, dname, variant):
    var = K.variants(shape)[variant]
    dtype = K.DTYPES[dname]
    fwd_route = _assert_route(lib, shape, dname, False, False)
    bwd_route = _assert_route(lib, shape, dname, True, var["dres"])
    ops = _dev(K.operands(shape, dname))
    strides = K.strides(shape, dname, var["strided"])
    ref = R.reference(ops["x"], ops["gamma"], ops["beta"], shape[3], var["eps"], var["silu"], dy=ops["dy"],
                      dres=ops["dres"] if var["dres"] else None, prefill=ops["prefill"] if var["accumulate"] else None,
                      bf16=dname == "bf16")
    what = f"{shape} {dname} {var}"
    got = _forward(lib, shape, dname, var, ops, strides)
    ratios = R.check_all(got, ref, dtype, f"{what} forward {fwd_route}")
    got = _backward(lib, shape, dname, var, ops, strides, ref)
    ratios.update(R.check_all(got, ref, dtype, f"{what} backward {bwd_route}"))
    _report(f"gpu {'x'.join(map(str, shape))} {dname} v{variant} fwd:{fwd_route} bwd:{bwd_route}{'+dres' if var['dres'] else ''} "
            + " ".join(f"{n}={v:.3g}" for n, v in ratios.items()))


@pytest.mark.parametrize("dname", list(K.DTYPES))
@pytest.mark.parametrize("shape,extra", [(s, e) for s in _SHAPES for e in K.extra_forwards(s)],
                         ids=[f"{i}-{e}" for i, s in K.case_ids() for e in K.extra_forwards(s)])
def test_groupnorm_extra_forward(lib, shape, extra, dname):
    """Forward only: one sample constant (var = 0: rstd = 1 / sqrt(eps), y = [silu](beta) up to the bound)."""
    var = K.variants(shape)[0]
    fwd_route = _assert_route(lib, shape, dname, False, False)
    ops = _dev(K.operands(shape, dname, extra))
    ref = R.reference(ops["x"], ops["gamma"], ops["beta"], shape[3], var["eps"], var["silu"], bf16=dname == "bf16")
    got = _forward(lib, shape, dname, var, ops, K.strides(shape, dname, var["strided"]))
    ratios = R.check_all(got, ref, K.DTYPES[dname], f"{shape} {dname} {extra} forward {fwd_route}")
    _report(f"gpu {'x'.join(map(str, shape))} {dname} {extra} fwd:{fwd_route} " + " ".join(f"{n}={v:.3g}" for n, v in ratios.items()))
