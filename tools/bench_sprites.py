"""Sprite batches: images/s of psg_sprite_contrast_mean + psg_sprite_augment at B = 256, S = 215 (device events), the cost
of drawing the parameter rows, and the reference's PIL chain in ms per image on one thread of this host.

    python tools/bench_sprites.py [--iters 200] [--pil-images 64]

Informational (DESIGN.md quotes the numbers); the resident set is the 8 fixture sprites repeated to the real dataset's 898."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pokemon_sprite_generator_amd import _lib, data as D    # noqa: E402
from tests import sprite_ref as R                            # noqa: E402  (the one statement of the PIL chain)


def events_ms(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--pil-images", type=int, default=64)
    args = ap.parse_args()
    B, S, N = 256, 215, 898
    res = {"B": B, "S": S, "N": N}

    # ---- the reference's chain, one thread
    imgs = R.fixture_images(S)
    p = D.draw_params(args.pil_images, S, generator=torch.Generator().manual_seed(0)).double()
    ang = torch.rad2deg(torch.atan2(p[:, 4], p[:, 1])).tolist()
    t0 = time.perf_counter()
    for k in range(args.pil_images):
        r = p[k].tolist()
        R.pil_chain(imgs[k % len(imgs)], S, flip=int(r[0]), angle=ang[k], order=R.ORDERS[int(r[7])], b=r[8], c=r[9], s=r[10], hue=r[11],
                    crop=tuple(int(v) for v in r[12:16]))
    res["pil_ms_per_image"] = (time.perf_counter() - t0) * 1e3 / args.pil_images

    if not torch.cuda.is_available():
        raise SystemExit("bench_sprites needs a GPU for the kernel timings (PIL chain: %.2f ms per image)" % res["pil_ms_per_image"])
    _lib.init(0)
    dev = torch.device("cuda", 0)
    src = torch.from_numpy(np.array(R.fixture_array(S))).to(dev).repeat(N // 8 + 1, 1, 1, 1)[:N].contiguous()
    gen = torch.Generator(device=dev).manual_seed(0)
    idx = torch.randint(0, N, (B,), device=dev, generator=gen)
    params = D.draw_params(B, S, gen, dev)
    mean = D.contrast_mean(src, idx, params)
    ms_mean = events_ms(lambda: D.contrast_mean(src, idx, params), args.iters)
    ms_aug = events_ms(lambda: D.augment(src, idx, params, mean=mean), args.iters)
    ms_both = events_ms(lambda: D.augment(src, idx, params), args.iters)
    ms_ident = events_ms(lambda: D.augment(src, idx, D.identity_params(B, S, dev), mean=mean), args.iters)
    ms_draw = events_ms(lambda: D.draw_params(B, S, gen, dev), 50)
    out_bytes = B * 3 * S * S * 4
    res.update({"contrast_mean_ms": ms_mean, "augment_ms": ms_aug, "mean_plus_augment_ms": ms_both,
                "images_per_s": B / (ms_both * 1e-3), "augment_store_GBps": out_bytes / (ms_aug * 1e-3) / 1e9,
                "identity_augment_ms": ms_ident, "draw_params_ms": ms_draw,
                "pil_ms_per_batch_one_thread": res["pil_ms_per_image"] * B})
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
