"""One stage-3 train step (FinalStepper.train_step: text encoder -> frozen VAE encoder -> frozen VAE decoder, differentiable ->
L1 + 0.1 MSE -> backward -> clip -> AdamW) at batch 4 (the reference's configured batch) and 16 in bf16: wall time per step
(host clock around a synchronised window) and, from psg_profile_*, the kernel-family time of the decoder's forward, of its
backward and of the text encoder (forward + backward) measured as separate passes.  The text encoder is BERT-base's shape
(12 layers, 'minimal') with hash-generated weights over the fixture vocabulary; S = 32 tokens.  Prints one JSON line per batch.

    python tools/final_step_bench.py [steps=10]
"""
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pokemon_sprite_generator_amd as psg  # noqa: E402
from pokemon_sprite_generator_amd import _lib, ops  # noqa: E402
from tests import text_cases as TC  # noqa: E402

KINDS = ("conv_fwd", "conv_dgrad", "wgrad", "attn", "gn")


def profiled(lib, fn):
    _lib.check(lib.psg_profile_begin(), "psg_profile_begin")
    fn()
    torch.cuda.synchronize()
    n = len(KINDS)
    ms, work, cnt = (C.c_double * n)(), (C.c_double * n)(), (C.c_int64 * n)()
    _lib.check(lib.psg_profile_end(ms, work, cnt, n), "psg_profile_end")
    return round(sum(ms), 3)


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    lib = _lib.init(0)
    dt = torch.bfloat16
    torch.manual_seed(0)
    te = psg.TextEncoder(bert_config=TC.bert_config(12), hidden_dim=256, finetune_strategy="minimal", compute_dtype=dt, trainable=True)
    te.load_state_dict(TC.state_dict(te))
    gen = psg.FinalPokemonGenerator(psg.VAEEncoder(compute_dtype=dt), psg.VAEDecoder(compute_dtype=dt), None, te).cuda()
    st = psg.FinalStepper(gen, lr=1e-5)
    for B in (4, 16):
        images = torch.rand(B, 3, 215, 215, device="cuda") * 2 - 1
        ids = torch.randint(5, TC.bert_config(1)["vocab_size"], (B, 32), device="cuda")
        mask = torch.ones(B, 32, dtype=torch.int64, device="cuda")
        for _ in range(3):
            st.train_step(images, ids, mask)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            r = st.train_step(images, ids, mask)
        torch.cuda.synchronize()
        step_ms = (time.perf_counter() - t0) / steps * 1e3
        # the split, as separate profiled passes over the same tensors
        latent = gen.vae_encoder(images)[0]
        emb = te.encode_ids(ids, mask).detach().requires_grad_(True)
        box = {}
        dec_fwd = profiled(lib, lambda: box.update(loss=ops.recon_loss(gen.vae_decoder(latent, emb), images)[0]))
        dec_bwd = profiled(lib, lambda: box["loss"].backward())
        g = emb.grad
        text = profiled(lib, lambda: te.encode_ids(ids, mask).backward(g))
        for p in te.parameters():
            p.grad = None
        print(json.dumps({"tool": "final_step_bench", "dtype": "bf16", "B": B, "steps": steps, "step_ms": round(step_ms, 2), "loss": round(float(r["loss"]), 4),
                          "kernel_ms": {"decoder_fwd": dec_fwd, "decoder_bwd": dec_bwd, "text_encoder_fwd_bwd": text}}), flush=True)


if __name__ == "__main__":
    main()
