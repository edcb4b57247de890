"""The optimizer phase with and without an EMA of the weights, on the full-width arena (640 488 456 floats, bf16 shadow on),
three variants timed in ONE process, interleaved round by round:

  (a) psg_adamw_dev_f32                                  30 bytes per parameter
  (b) psg_adamw_dev_ema_f32 (the EMA in the same pass)   38
  (c) (a) followed by ema.lerp_(flat, 1 - d)             30 + 12

Every round times each variant once (device events around `--iters` back-to-back calls); the table gives the median, the
minimum and the maximum over the rounds, the bytes-per-time figure, and (b) / (a), (b) / (c).  DESIGN.md §25 quotes it.

    python tools/adamw_ema_bench.py [--n N] [--rounds R] [--iters I] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pokemon_sprite_generator_amd import _lib  # noqa: E402
from pokemon_sprite_generator_amd._lib import check, ptr, stream_ptr  # noqa: E402

FULL_WIDTH = 640_488_456
DECAY = 0.999


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=FULL_WIDTH)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adamw_ema_bench needs a GPU: there is nothing to time without one")
    n = a.n // 8 * 8
    lib = _lib.init(0)
    dev = "cuda"
    p, g, m, v, ema = (torch.randn(n, device=dev) * 0.01 for _ in range(5))
    v.abs_()
    shadow = torch.empty(n, dtype=torch.bfloat16, device=dev)
    lr, step, nsq, flag = torch.full((1,), 1e-4, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), torch.ones(1, device=dev), \
        torch.zeros(1, dtype=torch.int32, device=dev)
    head = lambda: (ptr(p), ptr(g), ptr(m), ptr(v), n, ptr(lr), None, 1, 0.9, 0.999, 1e-6, 0.01, ptr(step), ptr(nsq), 1.0, ptr(flag), ptr(shadow))

    def plain():
        check(lib.psg_adamw_dev_f32(*head(), stream_ptr()), "psg_adamw_dev_f32")

    def fused():
        check(lib.psg_adamw_dev_ema_f32(*head(), ptr(ema), DECAY, 1, stream_ptr()), "psg_adamw_dev_ema_f32")

    def separate():
        plain()
        ema.lerp_(p, 1.0 - DECAY)

    variants = [("a adamw_dev", plain, 30), ("b adamw_dev_ema", fused, 38), ("c adamw_dev + lerp_", separate, 42)]
    times = {name: [] for name, _, _ in variants}
    for _, fn, _ in variants:                          # warm-up: code objects loaded, every buffer touched
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, fn, _ in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.iters)
    lines = [f"optimizer phase, n = {n} floats, bf16 shadow on, decay {DECAY} with warm-up; {a.rounds} interleaved rounds x {a.iters} calls, "
             f"ms per call ({torch.cuda.get_device_name(0)})",
             f"{'variant':24s} {'median':>8s} {'min':>8s} {'max':>8s} {'bytes/param':>12s} {'TB/s':>7s}"]
    med = {}
    for name, _, bpp in variants:
        t = times[name]
        med[name] = statistics.median(t)
        lines.append(f"{name:24s} {med[name]:8.3f} {min(t):8.3f} {max(t):8.3f} {bpp:12d} {n * bpp / 1e9 / med[name]:7.2f}")
    A, B, Cc = (med[name] for name, _, _ in variants)
    lines.append(f"b / a = {B / A:.3f} (by bytes 38 / 30 = {38 / 30:.3f});  b / c = {B / Cc:.3f};  b is {'faster' if B < Cc else 'NOT faster'} than c")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
