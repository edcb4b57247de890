"""One denoising step of four samplers on the full-width bf16 U-Net at n latents, timed in ONE process, interleaved round by round:

  (a) one step of today's SamplerRun (psg_ddpm_update_f32), batch n
  (b) one unguided DDIM step (psg_guided_update_f32, eps_u = NULL), batch n
  (c) one guided DDIM step: ONE forward at batch 2n plus the fused update (combine, step, copy into the second half)
  (d) the same guidance the plain way: two batch-n forwards (text, null text) plus torch elementwise ops for the combine, the
      clamp and the step

Every variant runs its step body eagerly (no hipGraph) so that the four are compared like for like.  Every round times each
variant once (device events around `--iters` back-to-back steps); the table gives the median, the minimum and the maximum over
the rounds, then (c) / (d), (c) / (a), and the cost of a whole chain per n latents: 1000 steps of (a) against 50 steps of (c).
DESIGN.md §26 quotes it.

    python tools/bench_guided_sampler.py [--n N] [--rounds R] [--iters I] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pokemon_sprite_generator_amd as psg  # noqa: E402
from pokemon_sprite_generator_amd.trainer import SamplerRun  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_guided_sampler needs a GPU: there is nothing to time without one")
    dev, n, w, clip = torch.device("cuda", 0), a.n, 2.0, 3.0
    torch.manual_seed(0)
    with torch.device(dev):
        unet = psg.UNet(compute_dtype=torch.bfloat16)
    unet.eval()
    st = psg.DiffusionStepper(unet, psg.NoiseScheduler(), distributed=False)
    text, null = torch.randn(n, 32, 256, device=dev), torch.randn(32, 256, device=dev)
    abar = st.noise_scheduler.alphas_cumprod
    k = 50
    # the chains are re-armed before every timed block (index back to a middle step), so any number of steps can be timed
    ddpm = SamplerRun(st, text, n, False, None, 8, 27, False, None)
    plain = psg.DdimRun(unet, text, abar, num_steps=k, use_graph=False)
    guided = psg.DdimRun(unet, text, abar, num_steps=k, guidance_scale=w, null_text=null, use_graph=False)
    tab = guided.tab
    x_d = torch.randn(n, 8, 27, 27, device=dev)
    tv = torch.full((n,), 500, device=dev, dtype=torch.long)
    null_n = null.unsqueeze(0).expand(n, -1, -1).contiguous()

    def arm(run, length):
        run.i = length // 2

    @torch.no_grad()
    def two_forwards():
        """(d): what guidance costs without the 2n forward and the fused launch."""
        ec, eu = unet(x_d, tv, text).float(), unet(x_d, tv, null_n).float()
        e = eu + w * (ec - eu)
        s0, s1, p0, p1 = tab[0, 25], tab[1, 25], tab[2, 25], tab[3, 25]
        x0 = (x_d - s1 * e) / s0
        c = x0.clamp(-clip, clip)
        e = torch.where(c != x0, (x_d - s0 * c) / s1, e)
        x_d.copy_(p0 * c + p1 * e)

    def step_of(run, length):
        def fn():
            if run.remaining() < 1:
                arm(run, length)
            run.step()
        return fn

    variants = [("a SamplerRun step (n)", step_of(ddpm, 1000)), ("b DDIM step (n)", step_of(plain, k)),
                ("c guided DDIM step (2n, fused)", step_of(guided, k)), ("d guided, 2 forwards + torch ops", two_forwards)]
    times = {name: [] for name, _ in variants}
    for run, length in ((ddpm, 1000), (plain, k), (guided, k)):
        arm(run, length)
    for _, fn in variants:                             # warm-up: workspaces sized, prepared weights cached
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.iters)
    lines = [f"one denoising step, full-width bf16 U-Net, n = {n} latents, guidance scale {w}, clip {clip}, eager step bodies; "
             f"{a.rounds} interleaved rounds x {a.iters} steps, ms per step ({torch.cuda.get_device_name(0)})",
             f"{'variant':34s} {'median':>8s} {'min':>8s} {'max':>8s}"]
    med = {}
    for name, _ in variants:
        t = times[name]
        med[name] = statistics.median(t)
        lines.append(f"{name:34s} {med[name]:8.3f} {min(t):8.3f} {max(t):8.3f}")
    A, Bv, Cv, Dv = (med[name] for name, _ in variants)
    lines.append(f"c / d = {Cv / Dv:.3f};  c / a = {Cv / A:.3f};  b / a = {Bv / A:.3f}")
    lines.append(f"per {n} latents: 1000-step chain of (a) {1000 * A:.0f} ms;  guided DDIM at 50 steps (c) {50 * Cv:.0f} ms;  "
                 f"unguided DDIM at 50 steps (b) {50 * Bv:.0f} ms")
    text_out = "\n".join(lines)
    print(text_out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text_out + "\n")
    st.close()


if __name__ == "__main__":
    main()
