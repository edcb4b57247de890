"""-m gpu: the gradient kernels of the VAE encoder's 4x4 stride-2 convolutions (csrc/conv4s2.hip) through the C ABI, bf16 and
fp32, element by element against fp64 on the operands the kernel read, at tests/gemm_ref.check's bound
(r_out |ref| + c_acc(K) S + A_FLOOR; K = 4 Cout for the data gradient, M for the weight gradient).

Shapes (tests/conv4s2_ref.py): channel tails, a K step that crosses a tap, more pixels per parity class than one workgroup,
a 1x1 output, uneven M splits, both master layouts, cin_real < Cin, strided rows - and the three real layers at batch 1 with
the plan's own splits.  Results and workspace sit inside NaN guards (every element written, nothing outside); every
weight-gradient launch runs twice and must give the same bits.  tests/test_conv4s2_cpu.py holds the same bound against torch's
fp32 kernels and planted defects.  A device error ends the run."""
import pytest
import torch

from tests import conv4s2_ref as R
from tests import gemm_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
GUARD = 64
NAN = float("nan")
W_OIHW, W_OHWI = 0, 1


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    lib = _lib.init(0)
    yield lib
    lib.psg_conv4s2_wgrad_set_splits(0)


def _sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                   # a device error: nothing more runs on this GPU
        pytest.exit(f"{what}: {e}", returncode=3)


def _guarded(shape, dtype, fill=None):
    """A tensor of `shape` inside NaN guards: (flat buffer, view)."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * GUARD,), NAN, dtype=dtype, device=DEV)
    view = flat[GUARD:GUARD + n].view(shape)
    if fill is not None:
        view.copy_(fill.to(DEV, dtype))
    return flat, view


def _guards_intact(flat, what):
    assert bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[-GUARD:]).all()), f"{what}: written outside the result"


def _prep_wd(lib, w, dt):
    """The data-gradient operand of psg_prep_weight for an OIHW fp32 w: [Cin][kpad(16 Cout)]."""
    from pokemon_sprite_generator_amd import _lib
    O, I = w.shape[0], w.shape[1]
    code = _lib.dtype_code(dt)
    src = w.to(DEV).contiguous(memory_format=torch.channels_last)
    wd = torch.empty((I, lib.psg_kpad(16 * O, code)), dtype=dt, device=DEV)
    _lib.check(lib.psg_prep_weight(_lib.ptr(src), 0, W_OHWI, None, _lib.ptr(wd), O, I, 4, code, _lib.stream_ptr()), "psg_prep_weight")
    return wd


def _run_dgrad(lib, what, g, w, Hi, Wi, pad, dt, extra):
    from pokemon_sprite_generator_amd import _lib
    B, Ho, Wo, Cout = g.shape
    Cin = w.shape[1]
    ref, S = gemm_ref.conv_dgrad(g.to(DEV), w.to(DEV), (Hi, Wi), stride=2, pad=pad)
    gd = R.strided(g.to(DEV, dt), extra)
    wd = _prep_wd(lib, w, dt)
    flat, dx = _guarded((B, Hi, Wi, Cin), dt)
    _lib.check(lib.psg_conv4s2_dgrad(_lib.ptr(gd), gd.stride(-2), _lib.ptr(wd), _lib.ptr(dx), Cin, B, Hi, Wi, Cin, Ho, Wo, Cout, pad,
                                     _lib.dtype_code(dt), _lib.stream_ptr()), what)
    _sync(what)
    _guards_intact(flat, what)
    worst = gemm_ref.check(dx, ref, S, dt, what, 4 * Cout)        # (a NaN left in dx - an element not written - fails here)
    print(f"{what}: worst err/bound {worst:.3f}")
    return worst


@pytest.mark.parametrize("dn", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(R.DGRAD_CASES))
def test_dgrad(lib, name, dn):
    B, Hi, Wi, pad, Cin, Cout, extra = R.DGRAD_CASES[name]
    g, w = R.dgrad_inputs(name, DTYPES[dn])
    _run_dgrad(lib, f"conv4s2_dgrad {name}.{dn}", g, w, Hi, Wi, pad, DTYPES[dn], extra)


def _run_wgrad(lib, what, x, g, pad, cin_real, dt, extra, dbias, pin, layout, accumulate, ref4):
    """One configuration, launched twice: bound against fp64, NaN guards, identical bits.  Returns the worst err / bound."""
    from pokemon_sprite_generator_amd import _lib
    B, Hi, Wi, Cin = x.shape
    _, Ho, Wo, Cout = g.shape
    M = B * Ho * Wo
    code = _lib.dtype_code(dt)
    ref, S, bref, bS = ref4
    ref, S = ref[:, :cin_real], S[:, :cin_real]
    dw0 = db0 = None
    if accumulate:
        dw0 = 0.5 * R.h((Cout, cin_real, 4, 4), what + ".dw0").to(DEV)
        db0 = 0.5 * R.h((Cout,), what + ".db0").to(DEV)
        ref, S = ref + dw0.double(), S + dw0.double().abs()
        bref, bS = bref + db0.double(), bS + db0.double().abs()
    if layout == W_OHWI:
        ref_m, S_m = ref.permute(0, 2, 3, 1).contiguous(), S.permute(0, 2, 3, 1).contiguous()
    else:
        ref_m, S_m = ref, S
    xd, gd = R.strided(x.to(DEV, dt), extra), g.to(DEV, dt).contiguous()
    lib.psg_conv4s2_wgrad_set_splits(pin)
    try:
        need = int(lib.psg_conv4s2_wgrad_workspace_bytes(B, Ho, Wo, Cin, Cout, code))
        assert need > 0 and need % 4 == 0
        if pin:
            assert need == pin * (Cout * 16 * Cin + Cout) * 4, f"{what}: the pin did not give {pin} slabs"
        outs = []
        for rep in range(2):
            wflat, dw = _guarded(tuple(ref_m.shape), torch.float32, None if dw0 is None else (dw0 if layout == W_OIHW else dw0.permute(0, 2, 3, 1)))
            bflat, db = _guarded((Cout,), torch.float32, db0) if dbias else (None, None)
            ws = torch.full((need // 4 + GUARD,), NAN, dtype=torch.float32, device=DEV)
            _lib.check(lib.psg_conv4s2_wgrad(_lib.ptr(xd), xd.stride(-2), _lib.ptr(gd), Cout, _lib.ptr(dw), layout, cin_real, _lib.ptr(db), B, Hi, Wi,
                                             Cin, Ho, Wo, Cout, pad, int(accumulate), int(accumulate), code, _lib.ptr(ws), need,
                                             _lib.stream_ptr()), what)
            _sync(what)
            _guards_intact(wflat, what)
            assert bool(torch.isnan(ws[need // 4:]).all()), f"{what}: written behind the workspace the query reports"
            if dbias:
                _guards_intact(bflat, what + " dbias")
            outs.append((dw.clone(), db.clone() if dbias else None))
    finally:
        lib.psg_conv4s2_wgrad_set_splits(0)
    worst = gemm_ref.check(outs[0][0], ref_m, S_m, torch.float32, what + " dw", M)
    if dbias:
        worst = max(worst, gemm_ref.check(outs[0][1], bref, bS, torch.float32, what + " dbias", M))
        assert torch.equal(outs[0][1], outs[1][1]), f"{what}: dbias differs between two identical launches"
    assert torch.equal(outs[0][0], outs[1][0]), f"{what}: dw differs between two identical launches"
    return worst


def _refs(x, g, pad):
    ref, S = R.wgrad_ref(x.to(DEV), g.to(DEV), pad)
    bref, bS = gemm_ref.bias_grad(g.to(DEV))
    return ref, S, bref, bS


@pytest.mark.parametrize("dn", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(R.WGRAD_CASES))
def test_wgrad(lib, name, dn):
    B, Hi, Wi, pad, Cin, cin_real, Cout, extra, dbias, pins, layouts = R.WGRAD_CASES[name]
    dt = DTYPES[dn]
    x, g = R.wgrad_inputs(name, dt)
    ref4 = _refs(x, g, pad)                                       # one fp64 reference for every configuration of the case
    worst = 0.0
    for pin in tuple(pins) + (0,):
        for layout in layouts:
            for accumulate in (False, True):
                what = f"conv4s2_wgrad {name}.{dn} splits={pin} {layout}{' acc' if accumulate else ''}"
                worst = max(worst, _run_wgrad(lib, what, x, g, pad, cin_real, dt, extra, dbias, pin, W_OHWI if layout == "ohwi" else W_OIHW,
                                              accumulate, ref4))
    print(f"conv4s2_wgrad {name}.{dn}: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("dn", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(R.REAL_CASES))
def test_real_layers_batch1(lib, name, dn):
    """215 -> 107 (Cin 8 of which 3, Cout 32), 107 -> 53 (32 -> 64), 53 -> 27 pad 2 (64 -> 128): the odd sizes and the pad-2 layer
    at their true extents, the plan's own splits.  The image layer has no data gradient in the encoder; it runs here all the same."""
    Hi, pad, Cin, cin_real, Cout = R.REAL_CASES[name]
    dt = DTYPES[dn]
    x, g, w = R.real_inputs(name, dt)
    wd = _run_dgrad(lib, f"conv4s2_dgrad {name}.{dn}", g, w, Hi, Hi, pad, dt, 0)
    ww = _run_wgrad(lib, f"conv4s2_wgrad {name}.{dn}", x, g, pad, cin_real, dt, 0, True, 0, W_OIHW, False, _refs(x, g, pad))
    print(f"{name}.{dn}: worst err/bound dgrad {wd:.3f}, wgrad {ww:.3f}")
