"""Cases, inputs and fp64 references for the gradients of the VAE encoder's 4x4 stride-2 convolutions (psg_conv4s2_dgrad /
psg_conv4s2_wgrad) and for the trainable VAEEncoder (test infrastructure shared by tests/test_conv4s2_cpu.py,
tests/test_conv4s2_gpu.py and tests/test_vae_encoder_train_gpu.py; not a conftest).

Kernel level: the references are fp64 on the operands the kernel really reads (bf16-representable in the bf16 cases), with
S = sum |a * b| over the same products, for tests/gemm_ref.check.  The data gradient is gemm_ref.conv_dgrad (explicit pad);
the weight gradient is restated here on F.unfold because gemm_ref.conv_wgrad assumes pad = ks // 2.

Module level: fp64 autograd of oracle.vae_oracle.vae_encode under loss = mean(latent * G) + KL(mu, logvar)."""
import json
import os

import torch
import torch.nn.functional as F

from oracle import hashgen, vae_oracle as V
from tests.util import h

GOLDEN_BF16 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vae_encoder_grad_bf16.json")

# name: (B, Hi, Wi, pad, Cin, Cout, extra row stride of g)
DGRAD_CASES = {
    "D1": (3, 7, 9, 1, 24, 40, 8),      # channel tails (Cin 24: half a column tile, Cout 40: a K step crosses a tap), ldg = Cout + 8
    "D2": (2, 5, 8, 2, 32, 64, 0),
    "D3": (1, 6, 6, 2, 64, 128, 0),
    "D4": (2, 13, 11, 1, 8, 8, 0),      # 84 pixels in the largest parity class: more than one workgroup
    "D5": (5, 2, 3, 1, 8, 16, 0),       # 1x1 output: one tap per pixel
}
# name: (B, Hi, Wi, pad, Cin, cin_real, Cout, extra row stride of x, with dbias, split pins, layouts)
WGRAD_CASES = {
    "W1": (3, 7, 9, 1, 8, 3, 32, 0, True, (1, 2), ("oihw",)),
    "W2": (5, 13, 11, 1, 32, 32, 64, 16, True, (1, 3), ("oihw", "ohwi")),
    "W3": (2, 5, 8, 2, 64, 64, 128, 0, False, (1,), ("oihw",)),
    "W4": (3, 7, 9, 2, 24, 24, 40, 0, True, (1,), ("oihw",)),
}
# the three layers of the encoder at their true extents, batch 1: (Hi, pad, Cin, cin_real, Cout)
REAL_CASES = {"R1": (215, 1, 8, 3, 32), "R2": (107, 1, 32, 32, 64), "R3": (53, 2, 64, 64, 128)}


def out_hw(Hi, Wi, pad):
    return (Hi + 2 * pad - 4) // 2 + 1, (Wi + 2 * pad - 4) // 2 + 1


def _rounded(t, dtype):
    """fp32 values every one of which `dtype` represents exactly."""
    return t.to(dtype).float()


def strided(t, extra):
    """A copy of channels-last t whose rows are `extra` elements longer than its channels (the padding holds NaN-free junk)."""
    if not extra:
        return t.contiguous()
    buf = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + extra,), 7.0, dtype=t.dtype, device=t.device)
    buf[..., :t.shape[-1]] = t
    return buf[..., :t.shape[-1]]


def dgrad_inputs(name, dtype):
    """(g [B,Ho,Wo,Cout] fp32 values exact in dtype, w [Cout,Cin,4,4] alike) on the CPU."""
    B, Hi, Wi, pad, Cin, Cout, _ = DGRAD_CASES[name]
    Ho, Wo = out_hw(Hi, Wi, pad)
    g = _rounded(h((B, Ho, Wo, Cout), f"c4s2.{name}.g", 1.5), dtype)
    w = _rounded(h((Cout, Cin, 4, 4), f"c4s2.{name}.w", 1.0), dtype)
    return g, w


def wgrad_inputs(name, dtype, cases=None):
    """(x [B,Hi,Wi,Cin], g [B,Ho,Wo,Cout]) fp32 values exact in dtype, on the CPU.  The channels of x beyond cin_real are NOT
    zero: a kernel that reads the wrong channel is seen."""
    B, Hi, Wi, pad, Cin, _, Cout = (cases or WGRAD_CASES)[name][:7]
    Ho, Wo = out_hw(Hi, Wi, pad)
    x = _rounded(h((B, Hi, Wi, Cin), f"c4s2.{name}.x", 1.5), dtype)
    g = _rounded(h((B, Ho, Wo, Cout), f"c4s2.{name}.g", 1.0), dtype)
    return x, g


def real_inputs(name, dtype):
    Hi, pad, Cin, cin_real, Cout = REAL_CASES[name]
    Ho, Wo = out_hw(Hi, Hi, pad)
    x = _rounded(h((1, Hi, Hi, Cin), f"c4s2.{name}.x", 1.5), dtype)
    x[..., cin_real:] = 0                                                   # as the encoder pads the image
    g = _rounded(h((1, Ho, Wo, Cout), f"c4s2.{name}.g", 1.0), dtype)
    w = _rounded(h((Cout, Cin, 4, 4), f"c4s2.{name}.w", 1.0), dtype)
    return x, g, w


def wgrad_ref(x, g, pad, rows=None):
    """dw[o, c, kh, kw] = sum_{b, oh, ow} g[b, oh, ow, o] x[b, 2 oh - pad + kh, 2 ow - pad + kw, c] in fp64 and S = the same
    sum over |g| |x|.  x [B,H,W,C], g [B,Ho,Wo,O] on any device, any row stride.  `rows` (a slice of the M = B Ho Wo output
    pixels) restricts the sum: what a kernel that drops a split computes.  Returns ([O,C,4,4], [O,C,4,4])."""
    B, H, W_, C = x.shape
    O = g.shape[-1]
    cols = F.unfold(x.detach().permute(0, 3, 1, 2).double(), 4, padding=pad, stride=2)      # [B, C*16, L], k = (c, kh, kw)
    cols = cols.transpose(1, 2).reshape(-1, C * 16)
    gb = g.detach().double().reshape(-1, O)
    assert cols.shape[0] == gb.shape[0], "gradient grid inconsistent with the input grid"
    if rows is not None:
        cols, gb = cols[rows], gb[rows]
    return (gb.t() @ cols).reshape(O, C, 4, 4), (gb.abs().t() @ cols.abs()).reshape(O, C, 4, 4)


# --------------------------------------------------------------------------------------------------------- module level
ENC_SEED = 31
ENC_SHAPE = (2, 3, 23, 27)                        # -> 11x13 -> 5x6 -> 3x4
ZERO_GRAD = "encoder.2.conv1.bias"                # exactly zero in exact arithmetic: GroupNorm(32, 32) removes a per-channel constant
ZERO_GRAD_SIBLING = "encoder.2.conv2.bias"


def encoder_state(shapes, seed=ENC_SEED):
    """hashgen 'stress' weights for a VAEEncoder state_dict's {name: shape}."""
    return hashgen.fill_unet_state({k: tuple(v) for k, v in shapes.items()}, seed, "stress")


def encoder_inputs(shape=ENC_SHAPE, latent_hw=(3, 4)):
    """(image, eps, G) on the CPU in fp32: the inputs of the module-level tests."""
    B = shape[0]
    img = h(shape, "vaeenc.img", 1.0)
    eps = h((B, 8) + tuple(latent_hw), "vaeenc.eps", 1.7)
    G = h((B, 8) + tuple(latent_hw), "vaeenc.G", 1.0)
    return img, eps, G


def encoder_loss(latent, mu, logvar, G):
    return (latent * G).mean() + -0.5 * torch.mean(1 + logvar - mu.pow(2) - logvar.exp())


def oracle_run(sd, img, eps, G, dtype, only=None, device="cpu"):
    """Autograd of oracle.vae_oracle.vae_encode in `dtype` on `device`: ({name: gradient}, (latent, mu, logvar)), all returned
    in fp64.  `only`: the parameter names whose gradients are wanted (default: all)."""
    p = {k: v.detach().to(device, dtype).requires_grad_(only is None or k in only) for k, v in sd.items()}
    latent, mu, logvar = V.vae_encode(p, img.to(device, dtype), eps.to(device, dtype))
    encoder_loss(latent, mu, logvar, G.to(device, dtype)).backward()
    grads = {k: v.grad.detach().double() for k, v in p.items() if v.grad is not None}
    return grads, tuple(t.detach().double() for t in (latent, mu, logvar))


def load_bf16_golden():
    with open(GOLDEN_BF16) as f:
        return json.load(f)
