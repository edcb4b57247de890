"""Cases, inputs and references for the trainable VAE decoder (test infrastructure shared by
tests/test_vae_decoder_train_cpu.py, tests/test_vae_decoder_train_gpu.py and tools/make_golden_vae_decoder.py; not a conftest).

The reference is autograd of oracle.vae_oracle.vae_decode (asserted equal to the reference decoder's own backward by
tools/make_golden_final.py) under loss = tests.final_cases.recon_loss(decode(latent, text), img), on the stress weights of
tests.final_cases.decoder_state.  The decoder always ends at 215x215, so the cases are small in batch and tokens, not pixels."""
import json
import os

import torch

from oracle import vae_oracle as V
from tests import final_cases as FC
from tests.util import h

GOLDEN_BF16 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vae_decoder_grad_bf16.json")

# name -> (batch, text tokens, latent grid).  s20: S divides no channel count (the [B,S,C] -> [C][S] reinterpretation's hard
# case; the inputs are final_cases' own "s20").  b2: batch > 1 and non-square interior grids (5x6 -> 10x12 -> 20x24 -> 215x215).
CASES = {"s20": (1, 20, (27, 27)), "b2": (2, 32, (5, 6))}
TAG = "vae_decoder_ref/1: s20=(1,20,27x27) b2=(2,32,5x6); weights final_cases.decoder_state; loss final_cases.recon_loss"

# conv biases whose gradient is exactly zero in exact arithmetic: they feed GroupNorm(32, 32), where every group is one channel
# and the mean subtraction removes a per-channel constant.  Checked absolutely, on the scale of the sibling conv2.bias.
ZERO_GRAD = {"block5_resnet1.conv1.bias": "block5_resnet1.conv2.bias", "block5_resnet2.conv1.bias": "block5_resnet2.conv2.bias"}


def decoder_state(module):
    """final_cases' stress weights for a VAEDecoder (or anything with its state_dict)."""
    return FC.decoder_state({k: tuple(v.shape) for k, v in module.state_dict().items()})


def inputs(case):
    """(latent [B,8,h,w], text [B,S,256], image [B,3,215,215]) on the CPU in fp32."""
    B, S, (lh, lw) = CASES[case]
    if case == "s20":
        return FC.inputs("s20")
    return (h((B, 8, lh, lw), f"vaedec.{case}.lat", 3.0 ** 0.5), h((B, S, 256), f"vaedec.{case}.text", 3.0 ** 0.5),
            h((B, 3, 215, 215), f"vaedec.{case}.img", 1.0))


def oracle_run(sd, lat, text, img, dtype, device="cpu"):
    """Autograd of vae_decode in `dtype` on `device`: ({parameter name: gradient}, d latent, d text, image), all in fp64."""
    p = {k: v.detach().to(device, dtype).requires_grad_(True) for k, v in sd.items()}
    lat = lat.detach().to(device, dtype).requires_grad_(True)
    text = text.detach().to(device, dtype).requires_grad_(True)
    out = V.vae_decode(p, lat, text)
    FC.recon_loss(out, img.to(device, dtype))[0].backward()
    return {k: v.grad.detach().double() for k, v in p.items()}, lat.grad.double(), text.grad.double(), out.detach().double()


def zero_grad_names(ref):
    """The conv1 biases whose fp64 gradient is below 1e-12 of their conv2.bias sibling's: what ZERO_GRAD must list."""
    out = set()
    for n in ref:
        if n.endswith(".conv1.bias"):
            sib = n.replace(".conv1.bias", ".conv2.bias")
            if float(ref[n].abs().max()) < 1e-12 * float(ref[sib].abs().max()):
                out.add(n)
    return out


def param_error(name, got, ref):
    """rel-L2 of a gradient against the fp64 one; for a ZERO_GRAD bias max |g| over its sibling's fp64 max-abs."""
    if name in ZERO_GRAD:
        return float(got.detach().double().abs().max()) / float(ref[ZERO_GRAD[name]].abs().max())
    a, b = got.detach().double().cpu(), ref[name].cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def load_bf16_golden():
    with open(GOLDEN_BF16) as f:
        return json.load(f)
