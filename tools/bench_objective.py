"""The loss phase of a train step at batch 256 and one DDIM step at n latents under v-prediction + Min-SNR, timed in
ONE process, variants interleaved round by round:

  loss phase, on tensors of the U-Net's output shape [256, 8, 27, 27] fp32 (loss and dL/dpred, as the stepper asks for them):
  (a) today's psg_smooth_l1_f32 against the noise
  (b) the fused v + gamma launch psg_diffusion_loss_f32 (target and weight built in the kernel)
  (c) the same objective the plain way: torch elementwise ops for the clamp and the v target, psg_smooth_l1_f32 for the
      gradient, torch ops for the per-sample weight of the gradient and for the weighted loss

  one denoising step of guidance.DdimRun on the full-width bf16 U-Net (eager step body, unguided):
  (d) eps-prediction (psg_guided_update_f32)      (e) v-prediction (psg_guided_update_pred_f32)

Every round times each variant once (device events around `--iters` back-to-back calls); the table gives the median, the minimum
and the maximum over the rounds.

    python tools/bench_objective.py [--batch B] [--n N] [--rounds R] [--iters I] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pokemon_sprite_generator_amd as psg  # noqa: E402
from pokemon_sprite_generator_amd import objective  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_objective needs a GPU: there is nothing to time without one")
    dev, B, n, gamma, beta = torch.device("cuda", 0), a.batch, a.n, 5.0, 0.1
    torch.manual_seed(0)
    with torch.device(dev):
        unet = psg.UNet(compute_dtype=torch.bfloat16)
    unet.eval()
    st = psg.DiffusionStepper(unet, psg.NoiseScheduler(), distributed=False)
    sch = st.noise_scheduler.to(dev)
    lat, noise = 2.0 * torch.randn(B, 8, 27, 27, device=dev), torch.randn(B, 8, 27, 27, device=dev)
    t = torch.randint(0, 1000, (B,), device=dev)
    wtab = psg.min_snr_weights(sch.alphas_cumprod, gamma, "v_prediction").to(dev)
    pred = objective.v_target(lat, noise, t, sch) + 0.1 * torch.randn_like(noise)
    loss = torch.zeros(1, device=dev)

    def today():
        return st.smooth_l1(pred, noise)

    def fused():
        return objective.diffusion_loss(pred, lat, noise, t, sch, "v_prediction", wtab, beta, True, True, st.flag, loss_out=loss)

    def plain():
        A, Bc, w = (v[t].view(-1, 1, 1, 1) for v in (sch.sqrt_alphas_cumprod, sch.sqrt_one_minus_alphas_cumprod, wtab))
        target = A * noise - Bc * lat.clamp(-3.0, 3.0)
        _, g = st.smooth_l1(pred, target)
        d = pred - target
        ad = d.abs()
        lw = (w * torch.where(ad < beta, 0.5 * d * d / beta, ad - 0.5 * beta)).mean()
        return lw, g * w

    text = torch.randn(n, 32, 256, device=dev)
    abar, k = sch.alphas_cumprod, 50
    run_e = psg.DdimRun(unet, text, abar, num_steps=k, use_graph=False)
    run_v = psg.DdimRun(unet, text, abar, num_steps=k, use_graph=False, prediction="v_prediction")

    def step_of(run):
        def fn():
            if run.remaining() < 1:
                run.i = k // 2
            run.step()
        return fn

    variants = [("a smooth_l1 (today)", today), ("b fused v + gamma loss", fused), ("c v + gamma, torch ops + smooth_l1", plain),
                ("d DDIM step, eps", step_of(run_e)), ("e DDIM step, v", step_of(run_v))]
    times = {name: [] for name, _ in variants}
    run_e.i = run_v.i = k // 2
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
    lines = [f"loss phase at batch {B} ([{B}, 8, 27, 27] fp32, loss + gradient) and one unguided DDIM step at n = {n} on the full-width bf16 "
             f"U-Net; {a.rounds} interleaved rounds x {a.iters} calls, ms per call ({torch.cuda.get_device_name(0)})",
             f"{'variant':38s} {'median':>8s} {'min':>8s} {'max':>8s}"]
    med = {}
    for name, _ in variants:
        v = times[name]
        med[name] = statistics.median(v)
        lines.append(f"{name:38s} {med[name]:8.4f} {min(v):8.4f} {max(v):8.4f}")
    A, Bv, Cv, Dv, Ev = (med[name] for name, _ in variants)
    lines.append(f"b / a = {Bv / A:.3f};  b / c = {Bv / Cv:.3f};  e / d = {Ev / Dv:.4f}")
    text_out = "\n".join(lines)
    print(text_out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text_out + "\n")
    st.close()


if __name__ == "__main__":
    main()
