"""The imaging end of the generation path beside what it replaces, one JSON line:

  * `pil_to_tensor` for 475 x 475 and 2048 x 2048 RGB uploads - host clock around upload + psg_resample_u8, ending in a device
    synchronise - beside the reference's host path on the same machine (PIL LANCZOS resize + numpy + `.to(device)`,
    gradio_app.py:440-454), and the kernels alone on a resident image (device events);
  * `to_uint8` for a [8, 3, 215, 215] batch beside the torch-op chain of trainer.generate_samples brought to the same uint8
    HWC result (device events), and both with the copy to the host (one copy per batch here, one per image there).

    python tools/bench_imaging.py [--iters 200] [--host-iters 20]

Informational (DESIGN.md quotes the numbers)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pokemon_sprite_generator_amd import _lib, imaging    # noqa: E402


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


def host_ms(fn, iters):
    """Host clock around `iters` calls, each ending in a device synchronise."""
    for _ in range(3):
        fn()
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def reference_pil_to_tensor(pil, dev):
    from PIL import Image
    image = pil.resize((215, 215), Image.Resampling.LANCZOS)
    t = torch.from_numpy(np.array(image)).float() / 255.0
    return ((t.permute(2, 0, 1) - 0.5) * 2).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_imaging needs a GPU")
    from PIL import Image
    _lib.init(0)
    dev = torch.device("cuda", 0)
    res = {}
    rng = np.random.default_rng(0)
    for S in (475, 2048):
        arr = rng.integers(0, 256, (S, S, 3), dtype=np.uint8)
        pil = Image.fromarray(arr, "RGB")
        got, ref = imaging.pil_to_tensor(pil, device=dev), reference_pil_to_tensor(pil, dev)
        res[f"in{S}_bitwise_equal"] = bool(torch.equal(got, ref))
        resident = torch.from_numpy(arr).to(dev)
        res[f"in{S}_pil_to_tensor_ms"] = host_ms(lambda: imaging.pil_to_tensor(pil, device=dev), args.host_iters)
        res[f"in{S}_pil_to_tensor_from_array_ms"] = host_ms(lambda: imaging.pil_to_tensor(arr, device=dev), args.host_iters)
        res[f"in{S}_reference_host_path_ms"] = host_ms(lambda: reference_pil_to_tensor(pil, dev), args.host_iters)
        res[f"in{S}_kernels_only_ms"] = events_ms(lambda: imaging.resize_lanczos(resident, (215, 215)), args.iters)

    img = torch.rand(8, 3, 215, 215, device=dev) * 2.4 - 1.2

    def torch_chain(x):
        return (torch.clamp((x + 1.0) / 2.0, 0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    res["to_uint8_bitwise_equal"] = bool(torch.equal(imaging.to_uint8(img), torch_chain(img)))
    res["to_uint8_ms"] = events_ms(lambda: imaging.to_uint8(img), args.iters)
    res["torch_chain_ms"] = events_ms(lambda: torch_chain(img), args.iters)
    res["to_uint8_plus_one_copy_ms"] = host_ms(lambda: imaging.to_uint8(img).cpu(), args.host_iters * 5)
    res["generate_samples_clamp_plus_copy_per_image_ms"] = host_ms(lambda: [i.cpu() for i in torch.clamp((img + 1.0) / 2.0, 0, 1)],
                                                                   args.host_iters * 5)
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
