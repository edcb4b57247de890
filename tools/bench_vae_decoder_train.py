#!/usr/bin/env python3
"""Forward + backward time of the VAE decoder (stage 1, src/training/vae_trainer.py): VAEDecoder(trainable=True) - all 144
parameter gradients - next to the frozen decoder's forward + backward (data gradients only, stage 3's path) on the same box
in the same run: the difference is what the weight gradients cost.  bf16 also with the slim weight-gradient route switched off
(every launch through psg_conv_wgrad).  No target, a record: one JSON line per (dtype, batch).

Method: synthetic inputs from a seed, loss = ops.recon_loss; every variant is warmed up, then the variants are timed in
alternating rounds of REPS steps between two HIP events; the line gives each variant's median and the spread of its rounds.

    python tools/bench_vae_decoder_train.py [--batches 4 16] [--rounds 5] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pokemon_sprite_generator_amd as psg
    from pokemon_sprite_generator_amd import _lib, ops
    _lib.init(0)
    dev = "cuda"
    slim_on = ops._WGRAD_SLIM                       # (PSG_WGRAD_SLIM=0 in the environment switches the route off for the whole run)
    lines = []
    for dt, dn in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        for B in args.batches:
            gen = torch.Generator(device=dev).manual_seed(B)
            lat = torch.randn((B, 8, 27, 27), device=dev, generator=gen)
            text = torch.randn((B, args.tokens, 256), device=dev, generator=gen)
            img = torch.rand((B, 3, 215, 215), device=dev, generator=gen) * 2 - 1
            torch.manual_seed(0)
            train = psg.VAEDecoder(8, 256, 3, compute_dtype=dt, trainable=True).to(dev)
            frozen = psg.VAEDecoder(8, 256, 3, compute_dtype=dt).to(dev)
            frozen.load_state_dict(train.state_dict())

            def step(dec, slim):
                ops._WGRAD_SLIM = slim
                dec.zero_grad(set_to_none=True)
                l, t = lat.clone().requires_grad_(True), text.clone().requires_grad_(True)
                ops.recon_loss(dec(l, t), img)[0].backward()

            variants = {"frozen": lambda: step(frozen, slim_on), "trainable": lambda: step(train, slim_on)}
            if dt == torch.bfloat16 and slim_on:
                variants["trainable_no_slim"] = lambda: step(train, False)
            for fn in variants.values():
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in variants}
            for _ in range(args.rounds):
                for k, fn in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.reps):
                        fn()
                    e1.record()
                    e1.synchronize()
                    times[k].append(e0.elapsed_time(e1) / args.reps)
            ops._WGRAD_SLIM = slim_on
            line = {"dtype": dn, "B": B, "tokens": args.tokens, "rounds": args.rounds, "reps": args.reps}
            for k, v in times.items():
                med = statistics.median(v)
                line[k + "_ms"] = round(med, 3)
                line[k + "_spread"] = round((max(v) - min(v)) / med, 3)
            line["weight_grad_cost_ms"] = round(line["trainable_ms"] - line["frozen_ms"], 3)
            print(json.dumps(line), flush=True)
            lines.append(line)
            del train, frozen
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
