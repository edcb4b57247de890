"""One stage-3 JOINT train step (FinalStepper.train_step after switch_to_joint_training: text encoder -> frozen VAE encoder -> VAE
decoder -> L1 + 0.1 MSE -> backward -> the gradient norms -> ONE clip + AdamW over the text encoder's and the decoder's param
groups) at batch 4 (the reference config's) and batch 16, update="grouped" (one norm pass + one update launch over the arena,
psg_adamw_groups_sets_f32) against update="torch" (torch.optim.AdamW + one clip_grad_norm_ over the separate tensors, the
reference's own sequence).  Both steppers live in ONE process over their own copies of the same modules and are timed in
alternating rounds; every figure is a host clock around a window that ends in a device synchronise, reported as median and min
over the rounds.

  step_ms        the whole joint train step
  opt_ms         the optimizer phase alone (FinalStepper.optimizer_phase on the gradients of the last backward, with both
                 learning rates set to 0 for the window so that the repeats leave the weights where the steps put them: the
                 kernels do the same work)
  opt_launches   device-side events of the optimizer phase (torch.profiler; "not measured" where the profiler is unavailable)

The text encoder is BERT-base's shape (12 layers, 'minimal') with hash-generated weights over the fixture vocabulary, S = 32
tokens; there is no U-Net (the training forward never calls it).  Prints one JSON line per batch size.

    python tools/bench_final_step.py [rounds=7] [steps=5] [dtype=bf16|fp32]
"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pokemon_sprite_generator_amd as psg  # noqa: E402
from pokemon_sprite_generator_amd import _lib  # noqa: E402
from oracle import hashgen  # noqa: E402
from tests import text_cases as TC  # noqa: E402

UPDATES = ("grouped", "torch")
OPT_REPEATS = 20


def build(update, dt, vae_sd, te_sd):
    enc, dec = psg.VAEEncoder(3, 8, compute_dtype=dt), psg.VAEDecoder(8, 256, 3, compute_dtype=dt, trainable=True)
    enc.load_state_dict({k[8:]: v for k, v in vae_sd.items() if k.startswith("encoder.")})
    dec.load_state_dict({k[8:]: v for k, v in vae_sd.items() if k.startswith("decoder.")})
    te = psg.TextEncoder(bert_config=TC.bert_config(12), hidden_dim=256, finetune_strategy="minimal", compute_dtype=dt, trainable=True)
    te.load_state_dict(te_sd)
    st = psg.FinalStepper(psg.FinalPokemonGenerator(enc, dec, None, te).cuda(), lr=1e-5, update=update)
    st.switch_to_joint_training()
    return st


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n if n > 0 else "not measured"
    except Exception as e:                                 # (a measurement that cannot be taken is reported as such, never guessed)
        return f"not measured ({type(e).__name__})"


def stats(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3)}


class zero_lr:
    """Both learning rates 0 inside the window."""

    def __init__(self, optimizer):
        self.groups = optimizer.param_groups

    def __enter__(self):
        self.lrs = [g["lr"] for g in self.groups]
        for g in self.groups:
            g["lr"] = 0.0

    def __exit__(self, *exc):
        for g, lr in zip(self.groups, self.lrs):
            g["lr"] = lr


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[sys.argv[3] if len(sys.argv) > 3 else "bf16"]
    _lib.init(0)
    probe = psg.PokemonVAE(8, 256)
    vae_sd = hashgen.fill_unet_state({k: tuple(v.shape) for k, v in probe.state_dict().items()}, 77, "stress")
    te_probe = psg.TextEncoder(bert_config=TC.bert_config(12), hidden_dim=256, finetune_strategy="minimal", trainable=True)
    te_sd = TC.state_dict(te_probe)
    del probe, te_probe
    st = {u: build(u, dt, vae_sd, te_sd) for u in UPDATES}
    n_tensors = len(st["grouped"].text_params) + len(st["grouped"].decoder_params)
    for B in (4, 16):
        gen = torch.Generator(device="cuda").manual_seed(B)
        images = torch.rand(B, 3, 215, 215, device="cuda", generator=gen) * 2 - 1
        ids = torch.randint(5, TC.bert_config(1)["vocab_size"], (B, 32), device="cuda", generator=gen)
        mask = torch.ones(B, 32, dtype=torch.int64, device="cuda")
        step = {u: (lambda s=st[u]: s.train_step(images, ids, mask)) for u in UPDATES}
        opt = {u: st[u].optimizer_phase for u in UPDATES}
        first = {}
        for u in UPDATES:                                  # warm-up: every shape of the timed window
            first[u] = round(float(step[u]()["loss"]), 4)
            for _ in range(2):
                step[u]()
        step_ms, opt_ms = {u: [] for u in UPDATES}, {u: [] for u in UPDATES}
        for r in range(rounds):
            for u in (UPDATES if r % 2 == 0 else UPDATES[::-1]):
                step_ms[u].append(timed(step[u], steps))
            for u in (UPDATES if r % 2 == 0 else UPDATES[::-1]):
                with zero_lr(st[u].optimizer):
                    opt_ms[u].append(timed(opt[u], OPT_REPEATS))
        launches = {}
        for u in UPDATES:
            with zero_lr(st[u].optimizer):
                launches[u] = count_launches(opt[u])
        loss = {u: round(float(step[u]()["loss"]), 4) for u in UPDATES}
        print(json.dumps({"tool": "bench_final_step", "phase": "joint", "dtype": str(dt).split(".")[-1], "B": B, "rounds": rounds,
                          "steps_per_round": steps, "stepped_tensors": n_tensors, "arena_floats": st["grouped"].param_arena.numel,
                          "step_ms": {u: stats(step_ms[u]) for u in UPDATES}, "opt_ms": {u: stats(opt_ms[u]) for u in UPDATES},
                          "opt_launches": launches, "first_loss": first, "last_loss": loss}), flush=True)


if __name__ == "__main__":
    main()
