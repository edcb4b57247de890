"""-m gpu: how the backward nodes of `ops` deliver PARAMETER gradients - to autograd (`.grad`) or, for a parameter registered
with `ops.GradSink`, straight into its fp32 gradient view (written on first use in a step, accumulated on later uses).

Every node that produces a parameter gradient is run at the smallest shape that reaches its code, in fp32 and bf16:
  1. sink delivery is autograd delivery: same bits, `.grad` untouched, entry written, `on_ready` once per parameter
     (also with only the bias / beta trainable: the column-sum / single-output paths);
  2. a second backward in the same step accumulates: the views hold 2 * g0;
  3. gamma and beta of a normalisation whose sink entries disagree on `written` (one accumulate flag per launch), or of
     which only one has a sink;
  4. which nodes hop to the second stream when `SideStream.enabled` is set, and that their result is the same bits.

Bounds of 2. and 3.: |view - expected| / max|g0|.  Measured at the commit before the delivery code was unified: the second
backward gave exactly 2 * g0 in every case and both dtypes (worst 0.0), so 2. asserts equality; the already-written half of 3.
measured 3.3e-08 .. 6.1e-08 (layer_norm, bert_embed; one fp32 rounding of a + g0 with |a + g0| <= 2 max|g0|), so its bound is
the floor 2**-23 = 1.19e-07 (4x the worst accumulate figure, 0, lies below it), and the other half is exactly g0.
"""
import functools

import pytest
import torch

from pokemon_sprite_generator_amd._lib import ACT_GELU, ACT_SILU

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
FLOOR = 2.0 ** -23


@pytest.fixture(scope="module")
def ops():
    from pokemon_sprite_generator_amd import _lib, ops as m
    _lib.init(0)
    yield m
    m.GradSink.unregister_all()
    m.WeightCache.clear()


def _u(shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return ((torch.rand(shape, device=DEV, generator=g) * 2 - 1) * scale).to(dtype)


def _p(shape, seed, scale=0.2, shift=0.0):
    return (_u(shape, seed, scale) + shift).requires_grad_(True)


# ---------------------------------------------------------------------------------------------------------------- the cases
# each: (ops, dtype) -> (parameters by name, names of the bias / beta parameters, run): run() is one forward + backward on
# fixed inputs, seeds and output gradient
def _conv(ks, cin=16, cout=24, **kw):
    def make(ops, dt):
        P = {"w": _p((cout, cin, ks, ks), 1), "b": _p((cout,), 2)}
        x, dy = _u((2, 5, 5, cin), 3, 1.0, dt), _u((2, 5, 5, cout), 4, 1.0, dt)
        return P, ("b",), lambda: ops.conv2d(x, P["w"], P["b"], **kw).backward(dy)
    return make


def _linear(ops, dt):
    P = {"w": _p((48, 32), 1), "b": _p((48,), 2)}
    x, dy = _u((10, 32), 3, 1.0, dt), _u((10, 48), 4, 1.0, dt)
    return P, ("b",), lambda: ops.linear(x, P["w"], P["b"], act=ACT_GELU, drop_p=0.25, seed=1234).backward(dy)


def _qkv(ops, dt):
    P = {n: _p((32, 32) if n[0] == "w" else (32,), i) for i, n in enumerate(("wq", "bq", "wk", "bk", "wv", "bv"))}
    x, dy = _u((12, 32), 7, 1.0, dt), _u((12, 96), 8, 1.0, dt)
    packed = ops.prep_qkv(P["wq"], P["wk"], P["wv"], P["bq"], P["bk"], P["bv"], dt, True)
    return P, ("bq", "bk", "bv"), lambda: ops.qkv_linear(x, *P.values(), packed).backward(dy)


def _ffn(ops, dt):
    P = {"w1": _p((64, 32), 1), "b1": _p((64,), 2), "w2": _p((32, 64), 3), "b2": _p((32,), 4)}
    x, dy = _u((12, 32), 5, 1.0, dt), _u((12, 32), 6, 1.0, dt)
    return P, ("b1", "b2"), lambda: ops.ffn(x, *P.values(), 0.6, drop_p=0.1, seed1=11, seed2=12).backward(dy)


def _cross(ops, dt):
    P = {"w": _p((96, 32), 1), "b": _p((96,), 2)}
    xn, tp = _u((2, 9, 32), 3, 1.0, dt), _u((2, 4, 32), 4, 1.0, dt)
    dq, dkv = _u((2, 9, 32), 5, 1.0, dt), _u((2, 4, 64), 6, 1.0, dt)
    return P, ("b",), lambda: torch.autograd.backward(ops.cross_in_proj(xn, tp, P["w"], P["b"]), (dq, dkv))


def _gn(split, silu):
    def make(ops, dt):
        P = {"gamma": _p((32,), 1, shift=1.0), "beta": _p((32,), 2)}
        x, dy, dp = _u((2, 3, 3, 32), 3, 2.0, dt).requires_grad_(True), _u((2, 3, 3, 32), 4, 1.0, dt), _u((2, 3, 3, 32), 5, 1.0, dt)
        if split:
            return P, ("beta",), lambda: torch.autograd.backward(ops.group_norm_split(x, P["gamma"], P["beta"], 8, silu=silu), (dy, dp))
        return P, ("beta",), lambda: ops.group_norm(x, P["gamma"], P["beta"], 8, silu=silu).backward(dy)
    return make


def _ln(res):
    def make(ops, dt):
        P = {"gamma": _p((64,), 1, shift=1.0), "beta": _p((64,), 2)}
        x, r, dy = _u((6, 64), 3, 2.0, dt), (_u((6, 64), 4, 1.0, dt) if res else None), _u((6, 64), 5, 1.0, dt)
        return P, ("beta",), lambda: ops.layer_norm(x, P["gamma"], P["beta"], 1e-5, residual=r).backward(dy)
    return make


def _embed(ops, dt):
    P = {"word": _p((11, 64), 1), "pos": _p((8, 64), 2), "typ": _p((2, 64), 3), "gamma": _p((64,), 4, shift=1.0), "beta": _p((64,), 5)}
    ids = torch.tensor([[3, 10, 0, 7, 3], [1, 0, 9, 9, 5]], dtype=torch.int64, device=DEV)          # 0 is the pad id
    tt = torch.tensor([[0, 0, 1, 1, 0], [1, 0, 0, 1, 1]], dtype=torch.int64, device=DEV)
    dy = _u((10, 64), 6, 1.0, dt)
    return P, ("beta",), lambda: ops.bert_embed(ids, tt, *P.values(), 1e-12, 0, dt).backward(dy)


CASES = {
    "conv3x3": _conv(3), "conv1x1_alpha": _conv(1, alpha=0.6), "conv1x1_silu": _conv(1, act=ACT_SILU),
    "linear": _linear, "qkv_linear": _qkv, "ffn": _ffn, "cross_in_proj": _cross,
    "group_norm": _gn(False, False), "group_norm_silu": _gn(False, True), "group_norm_split": _gn(True, False),
    "group_norm_split_silu": _gn(True, True), "layer_norm": _ln(False), "layer_norm_res": _ln(True), "bert_embed": _embed,
}
AFFINE = ("group_norm", "layer_norm", "bert_embed")
ALL = [(c, dt) for c in CASES for dt in DTYPES]
IDS = [f"{c}-{'fp32' if dt == torch.float32 else 'bf16'}" for c, dt in ALL]


@functools.lru_cache(maxsize=None)
def _case(ops, name, dt, bias_only=False):
    """(parameters, run, g0): the case with the gradients autograd delivers when no sink is registered (computed once)."""
    P, biases, run = CASES[name](ops, dt)
    if bias_only:
        for n, p in P.items():
            p.requires_grad_(n in biases)
    run()
    g0 = {n: p.grad.clone() for n, p in P.items() if p.requires_grad}
    assert g0 and all(torch.isfinite(g).all() for g in g0.values())
    for p in P.values():
        p.grad = None
    return P, run, g0


class _Sinks:
    """NaN-filled fp32 views registered for every parameter of the case (trainable or not; or for `names` only), with a counting
    on_ready."""

    def displaced(self, param):
        pass

    def __init__(self, ops, P, names=None):
        self.ops, self.ready = ops, {}
        self.names = list(P) if names is None else list(names)
        self.view = {n: torch.full_like(P[n], float("nan")) for n in self.names}
        self.entry = {n: ops.GradSink.register(P[n], self.view[n], i, on_ready=self._count, owner=self) for i, n in enumerate(self.names)}

    def _count(self, index):
        self.ready[index] = self.ready.get(index, 0) + 1

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ops.GradSink.unregister(self)


def _rel(view, expect, g0):
    return float((view.double() - expect.double()).abs().max() / g0.abs().max().double())


def _check_delivered(P, s, g0):
    torch.cuda.synchronize()
    for n in g0:
        i = s.names.index(n)
        assert torch.equal(s.view[n], g0[n]), f"{n}: the sink view differs from autograd's gradient"
        assert P[n].grad is None, f"{n}: .grad was set although the parameter has a sink"
        assert s.entry[n].written, f"{n}: sink entry not marked written"
        assert s.ready.get(i, 0) == 1, f"{n}: on_ready fired {s.ready.get(i, 0)} times"


# ------------------------------------------------------------------------------------------------------------------ 1 and 2
@pytest.mark.parametrize("name,dt", ALL, ids=IDS)
def test_sink_delivery_is_autograd_delivery(ops, name, dt):
    P, run, g0 = _case(ops, name, dt)
    with _Sinks(ops, P) as s:
        run()
        _check_delivered(P, s, g0)


@pytest.mark.parametrize("name,dt", ALL, ids=IDS)
def test_sink_delivery_bias_only(ops, name, dt):
    """Weight / gamma (and the embedding tables) frozen: the bias or beta gradient alone.  g0 is deliberately this variant's
    own no-sink gradient, not the all-trainable run's: the test pins sink delivery against autograd delivery on the column-sum
    path.  That path and the fused bias of the weight-gradient launch sum in different orders (they differ by ~1e-7 relative
    in fp32, before and after the delivery code was unified), so equality of the two is not something either tree offers."""
    P, run, g0 = _case(ops, name, dt, True)
    with _Sinks(ops, P) as s:
        run()
        _check_delivered(P, s, g0)


@pytest.mark.parametrize("name,dt", ALL, ids=IDS)
def test_second_backward_accumulates(ops, name, dt):
    """No begin_step between two backwards: the views hold 2 * g0 (bounds: module docstring)."""
    P, run, g0 = _case(ops, name, dt)
    with _Sinks(ops, P) as s:
        run()
        run()
        torch.cuda.synchronize()
        for i, n in enumerate(s.names):
            print(f"accumulate {name} {dt} {n}: |view - 2 g0| / max|g0| = {_rel(s.view[n], 2 * g0[n], g0[n]):.3e}")
            assert torch.equal(s.view[n], 2 * g0[n]), f"{n}: not exactly twice the single gradient"
            assert P[n].grad is None and s.ready.get(i, 0) == 2, n


# ------------------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("first", ["gamma", "beta"])
@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", AFFINE)
def test_mixed_written_flags(ops, name, dt, first):
    """`first`'s entry was already written this step (it holds a known tensor a), the other's was not (NaN): one becomes
    a + g0, the other exactly g0, both are marked written and neither parameter gets a `.grad`.  Before the delivery code was
    unified the `group_norm` instance of this test FAILED (the node abandoned the sink when the flags differed: both parameters
    got a `.grad` and their entries stayed unwritten, which a data-parallel reducer waits on forever); layer_norm and
    bert_embed passed."""
    P, run, g0 = _case(ops, name, dt)
    other = "beta" if first == "gamma" else "gamma"
    with _Sinks(ops, P) as s:
        a = _u(g0[first].shape, 9) * g0[first].abs().max()            # |a + g0| <= 2 max|g0|: one rounding of the sum is <= FLOOR
        s.view[first].copy_(a)
        s.entry[first].written = True
        run()
        torch.cuda.synchronize()
        err = _rel(s.view[first], a.double() + g0[first].double(), g0[first])
        print(f"mixed {name} {dt} first={first}: |view - (a + g0)| / max|g0| = {err:.3e}")
        assert err <= FLOOR, (name, dt, first, err)
        assert torch.equal(s.view[other], g0[other]), f"{other}: not the plain gradient"
        for n in ("gamma", "beta"):
            assert s.entry[n].written and P[n].grad is None, n


@pytest.mark.parametrize("only", ["gamma", "beta"])
@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", AFFINE)
def test_one_of_the_pair_has_a_sink(ops, name, dt, only):
    """Only `only` is registered: it is delivered to its view, the other parameter (and, for bert_embed, the tables) through
    autograd, same bits both ways.  Before the delivery code was unified the `group_norm` instance of this test FAILED for the
    same reason as the one above (the sink was used only when both entries existed and agreed); layer_norm and bert_embed
    passed."""
    P, run, g0 = _case(ops, name, dt)
    try:
        with _Sinks(ops, P, [only]) as s:
            run()
            _check_delivered(P, s, {only: g0[only]})
            for n in g0:
                if n != only:
                    assert P[n].grad is not None and torch.equal(P[n].grad, g0[n]), f"{n}: autograd's gradient changed"
    finally:
        for p in P.values():
            p.grad = None


# ------------------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("name,hops", [("qkv_linear", False), ("cross_in_proj", False), ("conv3x3", True), ("ffn", True)])
def test_side_stream_users(ops, name, hops, dt):
    """With the second stream enabled the conv and FFN weight gradients run on it (same bits after the join); the packed
    projections stay on the main stream."""
    P, run, g0 = _case(ops, name, dt)
    dev = next(iter(P.values())).device
    saved = ops.SideStream.enabled
    ops.SideStream.join(dev)
    try:
        ops.SideStream.enabled = True
        with _Sinks(ops, P) as s:
            run()
            assert ops.SideStream.used == hops
            assert bool(ops.SideStream._pending) == hops
            ops.SideStream.join(dev)
            _check_delivered(P, s, g0)
    finally:
        ops.SideStream.enabled = saved
        ops.SideStream.join(dev)
