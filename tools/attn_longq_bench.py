"""psg_attn_bwd (the routing every other caller keeps) against psg_attn_bwd_longq on the five text cross-attentions of the VAE
decoder (S = 32 keys, 8 heads) at batch 4 (stage 3's configured batch) and 16, bf16 and fp32.  The two entries are timed with
HIP events on the same tensors, interleaved in one process: warm-up, then the median of N timings each.  Prints one JSON line.

    python tools/attn_longq_bench.py [N=60]
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pokemon_sprite_generator_amd import _lib  # noqa: E402

SHAPES = [(64, 729), (32, 729), (16, 2916), (8, 11664), (4, 46225)]      # (head_dim, queries) of decoder blocks 1..5
HEADS, S = 8, 32


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    lib = _lib.init(0)
    rows = []
    for dt in (torch.bfloat16, torch.float32):
        for B in (4, 16):
            for d, L in SHAPES:
                E = HEADS * d
                g = torch.Generator(device="cuda").manual_seed(d + L)
                u = lambda shape, a: ((torch.rand(shape, device="cuda", generator=g) * 2 - 1) * a).to(dt)
                q, k, v, do = u((B, L, E), 2.45), u((B, S, E), 2.45), u((B, S, E), 1.0), u((B, L, E), 1.0)
                o, dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
                lse = torch.empty((B, HEADS, L), dtype=torch.float32, device="cuda")
                delta = torch.empty_like(lse)
                code, st = _lib.dtype_code(dt), _lib.stream_ptr()
                p = _lib.ptr
                _lib.check(lib.psg_attn_fwd(p(q), E, p(k), E, p(v), E, p(o), E, p(lse), B, HEADS, L, S, d, d ** -0.5, 0.0, 0, code, st), "fwd")
                args = [p(q), E, p(k), E, p(v), E, p(o), E, p(do), E, p(lse), p(delta), p(dq), E, p(dk), E, p(dv), E, B, HEADS, L, S, d, d ** -0.5,
                        0.0, 0, code]
                need = lib.psg_attn_bwd_longq_workspace_bytes(B, HEADS, L, S, d)
                ws = torch.empty(need, dtype=torch.uint8, device="cuda")
                legs = {"attn_bwd": lambda: _lib.check(lib.psg_attn_bwd(*args, st), "psg_attn_bwd"),
                        "longq": lambda: _lib.check(lib.psg_attn_bwd_longq(*args, p(ws), need, st), "psg_attn_bwd_longq")}
                times = {name: [] for name in legs}
                for it in range(5 + n):
                    for name, fn in legs.items():
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        fn()
                        b.record()
                        b.synchronize()
                        if it >= 5:
                            times[name].append(a.elapsed_time(b) * 1e3)
                row = {"dtype": str(dt).split(".")[-1], "B": B, "d": d, "L": L, "attn_bwd_us": round(statistics.median(times["attn_bwd"]), 1),
                       "longq_us": round(statistics.median(times["longq"]), 1)}
                rows.append(row)
                print(f"# {row}", flush=True)
    sums = {}
    for r in rows:
        key = f"{r['dtype']}_B{r['B']}"
        s = sums.setdefault(key, [0.0, 0.0])
        s[0] += r["attn_bwd_us"]
        s[1] += r["longq_us"]
    print(json.dumps({"tool": "attn_longq_bench", "n": n, "rows": rows, "sum_us": {k: [round(a, 1), round(b, 1)] for k, (a, b) in sums.items()}}))


if __name__ == "__main__":
    main()
