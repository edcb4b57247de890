"""-m gpu: psg_attn_bwd_longq - the attention backward for few keys and very many queries (the VAE decoder's text
cross-attention under stage 3) - against an fp64 torch softmax-attention on the same inputs, against psg_attn_bwd, and its
contract: deterministic bits, argument errors, and no trace in psg_attn_path_counts.

Bars are the library's own (tests.util.TOL): o within TOL[dtype], dq / dk / dv within 2 x TOL[dtype], max-abs over max-abs -
the bar of the varlen pair test."""
import math

import pytest
import torch

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
