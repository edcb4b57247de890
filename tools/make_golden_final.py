#!/usr/bin/env python3
"""Generate tests/golden/final_grad.npz FROM THE REFERENCE VAE decoder's forward AND backward (stage 3's frozen half).

A sibling of tools/make_golden_text_grad.py: src/models/vae_decoder.py imports only torch, so the reference module is loaded
by file path, filled with the 'stress' weights of tests/final_cases.py (oracle.hashgen) and run on the CPU in fp32:
image = VAEDecoder(latent, text), loss = L1 + 0.1 * MSE against the images (final_trainer.py:425-440), backward to the text
embeddings and the latent.  oracle.vae_oracle.vae_decode under autograd is asserted to agree with the reference within 1e-5
(max-abs over max-abs) on the loss, d loss / d text and d loss / d latent.  OUTPUTS ONLY are written: the three loss scalars
and the two gradients per case.

    python tools/make_golden_final.py --ref <reference checkout> [--out tests/golden]
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import vae_oracle as V  # noqa: E402
from tests import final_cases as FC  # noqa: E402
from tests.util import maxrel  # noqa: E402


def run(decode, lat, text, img):
    lat, text = lat.clone().requires_grad_(True), text.clone().requires_grad_(True)
    losses = FC.recon_loss(decode(lat, text), img)
    losses[0].backward()
    return torch.stack([t.detach() for t in losses]), text.grad, lat.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    torch.set_num_threads(8)
    spec = importlib.util.spec_from_file_location("ref_vae", os.path.join(args.ref, "src", "models", "vae_decoder.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    dec = R.VAEDecoder(8, 256, 3).eval()
    sd = FC.decoder_state({k: v.shape for k, v in dec.state_dict().items()})
    dec.load_state_dict(sd)
    for p in dec.parameters():
        p.requires_grad = False
    out = {}
    for case in FC.CASES:
        lat, text, img = FC.inputs(case)
        ref = run(dec, lat, text, img)
        ora = run(lambda l, t: V.vae_decode(sd, l, t), lat, text, img)
        errs = [maxrel(a, b) for a, b in zip(ora, ref)]
        print(f"case {case}: loss {ref[0].tolist()}, |dtext| {float(ref[1].norm()):.6e}, |dlatent| {float(ref[2].norm()):.6e}; "
              f"oracle vs reference max-abs/max-abs: loss {errs[0]:.2e}, dtext {errs[1]:.2e}, dlatent {errs[2]:.2e}")
        assert max(errs) < 1e-5, errs
        out[f"{case}_loss"] = ref[0].numpy().astype(np.float32)
        out[f"{case}_dtext"] = ref[1].numpy().astype(np.float32)
        out[f"{case}_dlatent"] = ref[2].numpy().astype(np.float32)
    np.savez_compressed(os.path.join(args.out, "final_grad.npz"), **out)


if __name__ == "__main__":
    main()
