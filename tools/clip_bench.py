"""The CLIP loss of stage 3 at full size: ViT-B/32 (12 layers, 768 wide) with random weights, forward + image gradient of
`CLIPLoss.forward_features` on 215 x 215 images with the text side cached (`text_features` once, outside the timed window), at
batch 4 (stage 3's configured batch), 16 and 64 in fp32 and bf16.  Per leg: 3 warm-up iterations, then `iters` iterations timed one by one with device events;
the median, the fastest and the slowest are reported (the spread says what a difference is worth).  Also the one-off time of the
cached text side (77 tokens).  Prints one JSON line per leg.

    python tools/clip_bench.py [iters=10]
"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pokemon_sprite_generator_amd as psg  # noqa: E402
from pokemon_sprite_generator_amd import _lib  # noqa: E402

VIT_B32 = dict(projection_dim=512,
               vision_config=dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, image_size=224,
                                  patch_size=32, layer_norm_eps=1e-5),
               text_config=dict(vocab_size=49408, hidden_size=512, intermediate_size=2048, num_hidden_layers=12, num_attention_heads=8,
                                max_position_embeddings=77, layer_norm_eps=1e-5, eos_token_id=2))


def timed(fn, iters):
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    _lib.init(0)
    torch.manual_seed(0)
    clip = psg.CLIPLoss(VIT_B32).cuda()
    params = sum(p.numel() for p in clip.parameters())
    for dt, name in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        clip.compute_dtype = dt
        for B in (4, 16, 64):
            images = (torch.rand(B, 3, 215, 215, device="cuda") * 2 - 1).requires_grad_(True)
            ids = torch.randint(3, 49000, (B, 77), device="cuda")
            ids[:, -1] = 49407
            text_ms = timed(lambda: clip.text_features(ids), 4)
            te = clip.text_features(ids)
            box = {}

            def step():
                images.grad = None
                box["loss"] = clip.forward_features(images, te)
                box["loss"].backward()
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            ms = timed(step, iters)
            print(json.dumps({"tool": "clip_bench", "model": "ViT-B/32, random weights", "params": params, "dtype": name, "B": B, "iters": iters,
                              "fwd_bwd_ms": {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)},
                              "text_features_ms_last": round(text_ms[-1], 3), "loss": round(float(box["loss"]), 5),
                              "grad_finite": bool(torch.isfinite(images.grad).all())}), flush=True)


if __name__ == "__main__":
    main()
