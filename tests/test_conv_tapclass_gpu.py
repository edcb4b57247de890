"""Border-class order of the stride-1 3x3 convolutions (csrc/conv_gemm_kernel.h, TapCls): the tiles walk only the filter
taps their class of output positions can reach, so with finite inputs the forward and the data gradient must be the SAME
BITS as the plain 9-tap walk - every epilogue form the U-Net's 3x3 layers use, the training shapes and ragged ones."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    lib = _lib.init(0)
    yield lib
    _lib.check(lib.psg_conv_set_tapclass(1), "psg_conv_set_tapclass")


def _set(lib, mode):
    from pokemon_sprite_generator_amd import _lib
    _lib.check(lib.psg_conv_set_tapclass(mode), "psg_conv_set_tapclass")


def _run(B, H, W, Cin, Cout, seed):
    """conv1 form (bias + per-sample add), conv2 form (bias + residual), and the data gradient of each"""
    from pokemon_sprite_generator_amd import ops
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(B, H, W, Cin, device=DEV, generator=g).bfloat16()
    w = torch.randn(Cout, Cin, 3, 3, device=DEV, generator=g) * math.sqrt(1.0 / (9 * Cin))
    b = torch.randn(Cout, device=DEV, generator=g) * 0.3
    ra = torch.randn(B, Cout, device=DEV, generator=g).bfloat16()
    res = torch.randn(B, H, W, Cout, device=DEV, generator=g).bfloat16()
    gy = torch.randn(B, H, W, Cout, device=DEV, generator=g).bfloat16()
    outs = []
    for kw in ({"rowadd": ra}, {"residual": res}):
        xs = x.clone().requires_grad_(True)
        y = ops.conv2d(xs, w.clone().requires_grad_(True), b.clone().requires_grad_(True), **kw)
        y.backward(gy)
        outs += [y.detach(), xs.grad.clone()]
    torch.cuda.synchronize()
    return outs


def _compare(lib, B, H, W, Cin, Cout, seed=0):
    _set(lib, 0)
    c0 = int(lib.psg_conv_tapclass_launches())
    ref = _run(B, H, W, Cin, Cout, seed)
    assert int(lib.psg_conv_tapclass_launches()) == c0
    _set(lib, 2)
    got = _run(B, H, W, Cin, Cout, seed)
    took = int(lib.psg_conv_tapclass_launches()) - c0
    _set(lib, 1)
    for i, (a, b) in enumerate(zip(ref, got)):
        assert torch.isfinite(a.float()).all()
        assert torch.equal(a, b), f"output {i} differs (B={B} {H}x{W} {Cin}->{Cout})"
    return took


# every stride-1 3x3 layer shape of the U-Net at batch 256 (_LEVELS: 27x27 320 ch, 14x14 640, 7x7 1280, 4x4 1280)
UNET = [(27, 320, 320), (27, 640, 320), (14, 640, 640), (14, 1280, 640), (7, 1280, 1280), (7, 2560, 1280), (4, 1280, 1280), (4, 2560, 1280)]


@pytest.mark.parametrize("H,Cin,Cout", UNET)
def test_tapclass_is_bitwise_the_plain_walk_unet_shapes(lib, H, Cin, Cout):
    took = _compare(lib, 256, H, H, Cin, Cout, seed=H * 7 + Cin)
    assert took == 4          # the two forwards and the two data gradients all ran in class order


# (64 channels in and out: 9 K steps, too short a K axis for a split-K plan, so every launch is one the class form applies to)
@pytest.mark.parametrize("B,H,W,Cin,Cout", [(3, 7, 7, 64, 64), (37, 7, 7, 64, 64), (5, 5, 7, 64, 64), (37, 5, 7, 64, 64),
                                            (4, 3, 3, 64, 64), (37, 3, 3, 64, 64), (9, 14, 14, 64, 64), (37, 27, 27, 64, 64)])
def test_tapclass_is_bitwise_the_plain_walk_ragged(lib, B, H, W, Cin, Cout):
    took = _compare(lib, B, H, W, Cin, Cout, seed=B + H + W)
    assert took == 4


@pytest.mark.parametrize("B,H,W", [(8, 2, 2), (8, 1, 9), (8, 9, 1), (3, 2, 7)])
def test_tapclass_does_not_apply_below_3x3(lib, B, H, W):
    assert _compare(lib, B, H, W, 64, 64, seed=B * H * W) == 0


def test_tapclass_plan_at_batch_256(lib):
    """with the default setting the tile plan runs the 7x7 layers in class order (forward and data gradient); the 4x4 layers,
    one round of workgroups, stay on the plain walk (measured slower in class order)"""
    from pokemon_sprite_generator_amd import ops
    _set(lib, 1)
    for H, Cin, Cout, want in [(7, 1280, 1280, 2), (7, 2560, 1280, 2), (4, 1280, 1280, 0)]:
        x = torch.randn(256, H, H, Cin, device=DEV).bfloat16().requires_grad_(True)
        w = (torch.randn(Cout, Cin, 3, 3, device=DEV) * 0.01).requires_grad_(True)
        c0 = int(lib.psg_conv_tapclass_launches())
        y = ops.conv2d(x, w, None)
        y.backward(torch.randn_like(y))
        torch.cuda.synchronize()
        assert int(lib.psg_conv_tapclass_launches()) - c0 == want, (H, Cin, Cout)
