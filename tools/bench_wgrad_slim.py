#!/usr/bin/env python3
"""psg_conv_wgrad_slim against psg_conv_wgrad ON THE SAME DESCRIPTOR, for every distinct weight-gradient shape of the VAE
decoder's blocks 4 and 5 and its image convolution (bf16, with dbias, OIHW master layout) at batch 4 and 16.

Method: both entries are warmed up, then timed in ROUNDS alternating rounds (A B A B ...), each round REPS back-to-back
launches between two HIP events.  Per shape the line gives the median per-launch time of either entry, the spread of each
entry's rounds ((max - min) / median: what the same code does from round to round in this session) and whether the slim kernel
wins by more than the larger of the two spreads - the adoption rule of DESIGN.md section 19.  The two results are compared on
the timed operands (max |a - b| / max |a|).  One JSON line per shape.

    python tools/bench_wgrad_slim.py [--batches 4 16] [--rounds 7] [--reps 20] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import wgrad_cases as W  # noqa: E402
from tests.wgrad_slim_cases import mk  # noqa: E402

# (H = W, Cin, Cout, ks): vae_decoder.py:163-175 - block 4 at 108 x 108 (128 -> 64, then 64 wide), block 5 at 215 x 215
# (64 -> 32, then 32 wide), the ResNet 3x3 convs, the 1x1 shortcuts and q / proj, and the 32 -> 3 (in 8) image conv
SHAPES = [(108, 128, 64, 3), (108, 64, 64, 3), (108, 128, 64, 1), (108, 64, 64, 1),
          (215, 64, 32, 3), (215, 32, 32, 3), (215, 64, 32, 1), (215, 32, 32, 1), (215, 32, 8, 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pokemon_sprite_generator_amd import _lib
    lib = _lib.init(0)
    dev = "cuda"
    lines = []
    for B in args.batches:
        for (H, Cin, Cout, ks) in SHAPES:
            c = mk(f"b{B}.{H}.i{Cin}.o{Cout}.k{ks}", B=B, H=H, Cin=Cin, Cout=Cout, ks=ks, dbias=True, layout="oihw")
            g = W.geom(c)
            gen = torch.Generator(device=dev).manual_seed(1)
            x = torch.randn((g["M"], Cin), device=dev, generator=gen).to(torch.bfloat16)
            dy = torch.randn((g["M"], Cout), device=dev, generator=gen).to(torch.bfloat16)
            outs, launch = {}, {}
            for name, entry, query in (("wgrad", lib.psg_conv_wgrad, lib.psg_conv_wgrad_workspace_bytes),
                                       ("slim", lib.psg_conv_wgrad_slim, lib.psg_conv_wgrad_slim_workspace_bytes)):
                need = int(query(ctypes.byref(W.make_desc(c, "bf16"))))
                assert need >= 0, lib.psg_last_error()
                ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
                dw = torch.empty(Cout * g["Q"], dtype=torch.float32, device=dev)
                db = torch.empty(Cout, dtype=torch.float32, device=dev)
                d = W.make_desc(c, "bf16", dict(x=x.data_ptr(), dy=dy.data_ptr(), dw=dw.data_ptr(), dbias=db.data_ptr()), ws.data_ptr() if need else 0, need)
                outs[name] = (dw, db, ws, d)
                launch[name] = lambda entry=entry, d=d, name=name: _lib.check(entry(ctypes.byref(d), _lib.stream_ptr()), name)
            for name in launch:
                for _ in range(5):
                    launch[name]()
            torch.cuda.synchronize()
            times = {"wgrad": [], "slim": []}
            for _ in range(args.rounds):
                for name in ("wgrad", "slim"):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.reps):
                        launch[name]()
                    e1.record()
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1) * 1e3 / args.reps)
            med = {k: statistics.median(v) for k, v in times.items()}
            spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
            a, b = outs["wgrad"], outs["slim"]
            diff = max(float((a[i] - b[i]).abs().max() / a[i].abs().max()) for i in (0, 1))
            gain = 1.0 - med["slim"] / med["wgrad"]
            operand_mb = (g["M"] * (Cin + Cout) * 2) / 1e6
            line = {"B": B, "H": H, "Cin": Cin, "Cout": Cout, "ks": ks, "M": g["M"], "operand_MB": round(operand_mb, 1),
                    "wgrad_us": round(med["wgrad"], 1), "slim_us": round(med["slim"], 1), "wgrad_spread": round(spread["wgrad"], 3),
                    "slim_spread": round(spread["slim"], 3), "slim_gain": round(gain, 3), "slim_wins": bool(gain > max(spread.values())),
                    "max_rel_diff": diff, "rounds": args.rounds, "reps": args.reps}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
