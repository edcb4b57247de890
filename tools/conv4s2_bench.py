"""The gradient launches of the VAE encoder's three 4x4 stride-2 convolutions (psg_conv4s2_dgrad, psg_conv4s2_wgrad) at the
stage-1 geometries, batch 32, bf16 and fp32, and the encoder's forward and forward + backward at the same batch.

Per launch: 5 warm-up launches, then `samples` samples of `reps` back-to-back launches between two device events (one event
pair around a single 20-200 us launch would time the events); the median, fastest and slowest per-launch time are reported
beside the ALGORITHMIC bytes (x, g and the weight read once, the result written once) and the fraction of 8 TB/s they imply.
The operands of one launch (up to 24 MB) stay in the 256 MB Infinity Cache between repetitions: the figures say what the
launch costs in a train step that has just produced its operands, not what it would cost from cold HBM.  One JSON line per leg.

    python tools/conv4s2_bench.py [samples=20] [reps=10]
"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pokemon_sprite_generator_amd as psg  # noqa: E402
from pokemon_sprite_generator_amd import _lib, ops  # noqa: E402
from pokemon_sprite_generator_amd._lib import check, dtype_code, ptr, stream_ptr  # noqa: E402

B = 32
# (name, Hi, pad, Cin, cin_real, Cout)
LAYERS = (("conv0 215->107", 215, 1, 8, 3, 32), ("conv3 107->53", 107, 1, 32, 32, 64), ("conv6 53->27", 53, 2, 64, 64, 128))
HBM = 8e12


def timed(fn, samples, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(samples):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1000.0 / reps)
    return {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}


def leg(kind, name, dn, us, nbytes, **more):
    print(json.dumps({"tool": "conv4s2_bench", "launch": kind, "layer": name, "B": B, "dtype": dn, "us": us, "algorithmic_MB": round(nbytes / 1e6, 3),
                      "fraction_of_8TBps": round(nbytes / (us["median"] * 1e-6) / HBM, 4), **more}), flush=True)


def main():
    samples = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    lib = _lib.init(0)
    torch.manual_seed(0)
    for dt, dn in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        es, code = (2 if dt == torch.bfloat16 else 4), dtype_code(dt)
        for name, Hi, pad, Cin, cin_real, Cout in LAYERS:
            Ho = (Hi + 2 * pad - 4) // 2 + 1
            x = (torch.rand(B, Hi, Hi, Cin, device="cuda") * 2 - 1).to(dt)
            g = (torch.rand(B, Ho, Ho, Cout, device="cuda") * 2 - 1).to(dt)
            w = torch.rand(Cout, cin_real, 4, 4, device="cuda") * 0.2 - 0.1
            _, wd = ops.WeightCache.get(w, dt, True, pad_in=Cin - cin_real)
            dx = torch.empty_like(x)
            dw, db = torch.empty_like(w), torch.empty(Cout, device="cuda")
            need = lib.psg_conv4s2_wgrad_workspace_bytes(B, Ho, Ho, Cin, Cout, code)
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            slab = (Cout * 16 * Cin + Cout) * 4

            def dgrad():
                check(lib.psg_conv4s2_dgrad(ptr(g), Cout, ptr(wd), ptr(dx), Cin, B, Hi, Hi, Cin, Ho, Ho, Cout, pad, code, stream_ptr()), "dgrad")

            def wgrad():
                check(lib.psg_conv4s2_wgrad(ptr(x), Cin, ptr(g), Cout, ptr(dw), 0, cin_real, ptr(db), B, Hi, Hi, Cin, Ho, Ho, Cout, pad, 0, 0, code,
                                            ptr(ws), need, stream_ptr()), "wgrad")
            leg("dgrad", name, dn, timed(dgrad, samples, reps), (g.numel() + Cin * 16 * Cout + dx.numel()) * es)
            leg("wgrad", name, dn, timed(wgrad, samples, reps), (x.numel() + g.numel()) * es + (dw.numel() + Cout) * 4,
                splits=need // slab, workspace_MB=round(need / 1e6, 3))
    for dt, dn in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        enc = psg.VAEEncoder(3, 8, compute_dtype=dt, trainable=True).cuda()
        img = torch.rand(B, 3, 215, 215, device="cuda") * 2 - 1
        eps = torch.randn(B, 8, 27, 27, device="cuda")
        G = torch.randn(B, 8, 27, 27, device="cuda")

        def fwd():
            with torch.no_grad():
                enc(img, eps=eps)

        def fwd_bwd():
            for p in enc.parameters():
                p.grad = None
            latent, mu, logvar = enc(img, eps=eps)
            ((latent * G).mean() + ops.kl_loss(mu, logvar)).backward()
        f, fb = timed(fwd, samples, 1), timed(fwd_bwd, samples, 1)
        print(json.dumps({"tool": "conv4s2_bench", "launch": "VAEEncoder", "B": B, "dtype": dn, "forward_us": f, "forward_backward_us": fb,
                          "ratio": round(fb["median"] / f["median"], 2),
                          "grads_finite": all(bool(torch.isfinite(p.grad).all()) for p in enc.parameters())}), flush=True)


if __name__ == "__main__":
    main()
