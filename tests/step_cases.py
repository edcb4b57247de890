"""The case tables of the step-kernel tests (tests/step_ref.py has the references): sizes, scalars and hash-generated inputs
(test infrastructure, not a conftest).  tests/test_step_ref_cpu.py runs the references and planted mistakes over them;
tests/test_step_kernels_gpu.py launches them.

Sizes: one case well below every grid cap with a ragged last block (1001), and per cap G one of 2 G + 333 elements: some
lanes take three trips of the grid-stride loop, the others two, and the last block is ragged."""
import numpy as np
import torch

from tests import step_ref as R
from tests.util import h

GUARD = 64                     # guard words before and after every device buffer (256 bytes: 16-byte alignment is kept)
N_SMALL = 1001


def past(cap):
    return 2 * cap + 333


N_GRID, N_RED, N_SUMSQ, N_SCALAR = past(R.GRID_CAP), past(R.RED_CAP), past(R.SUMSQ_CAP), past(R.SCALAR_CAP)
STREAM_N = [N_SMALL, N_GRID]
RED_N = [N_SMALL, N_RED]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
DTYPE_CODE = {"f32": 0, "bf16": 1}


def hn(n, name, scale=1.0):
    """n hash-generated fp32 values in [-scale, scale) as a numpy array."""
    return h((n,), name, scale).numpy()


def ulps(x, k):
    """The fp32 value k units in the last place from x."""
    v = np.float32(x)
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return v


# ------------------------------------------------------------------------------------------------------------ noise_add
NUM_T = 1000
NOISE_SHAPES = [(7, 143), (1000, 1049)]                 # 1001 elements; 1 049 000 = two full grids and 424


def noise_tables():
    from oracle import unet_oracle as O
    tb = O.cosine_clipped_tables(NUM_T)
    return tb["sqrt_alphas_cumprod"].numpy().astype(np.float32), tb["sqrt_one_minus_alphas_cumprod"].numpy().astype(np.float32)


def noise_inputs(B, chw, t_range):
    """x0 beyond +-3 in places, +-3 exactly, one NaN; t spread over the whole table; t_range: one pair outside it."""
    x0 = hn(B * chw, f"step.noise.x0.{B}", 4.0).reshape(B, chw)
    noise = hn(B * chw, f"step.noise.z.{B}", 2.0).reshape(B, chw)
    x0[0, :6] = [3.0, -3.0, ulps(3.0, 1), ulps(-3.0, -1), -5.0, np.nan]
    t = (np.arange(B, dtype=np.int64) * (NUM_T - 1)) // (B - 1)
    if t_range:
        t[1], t[B - 2] = -1, NUM_T
    return x0, noise, t


def fallback_inputs(n, bad):
    x0, noise = hn(n, f"step.fb.x0.{n}", 4.0), hn(n, f"step.fb.z.{n}", 2.0)
    x0[:4] = [3.0, ulps(3.0, 1), -7.0, 0.0]
    if bad:
        x0[n - 1] = np.nan                  # NaN survives the clamp (an infinity would not): the rescued batch is still bad
    return x0, noise


# --------------------------------------------------------------------------------------------------- sampler updates
DDPM_T = [0, 5]
DDPM_LEN = 10
SAMPLER = [(1, True), (1, False), (2, False), (3, True), (3, False)]      # (mode, z given)
SAMPLER_C = (1.0101, 0.02, 0.7, 0.1)


def ddpm_tables():
    return (1.0 + np.abs(hn(DDPM_LEN, "step.ddpm.c1", 0.1)), np.abs(hn(DDPM_LEN, "step.ddpm.c2", 0.2)) + 0.01, np.abs(hn(DDPM_LEN, "step.ddpm.sg", 0.15)) + 0.01)


def xez(n, tag):
    return hn(n, f"step.{tag}.x.{n}", 2.0), hn(n, f"step.{tag}.e.{n}", 1.5), hn(n, f"step.{tag}.z.{n}", 1.0)


# --------------------------------------------------------------------------------------------------------------- layout
# (B, C, HW): 1005 elements; 1 048 915 (2 G + 333 is prime: the next size with a channel count above 1)
LAYOUT_SHAPES = [(3, 5, 67), (1, 7, 149845)]
LD_EXTRA = [0, 8]
TEXT_POOL = [(S, D) for S in (1, 32) for D in (40, 256, 300)]
TEXT_B = 3
SIN_B, SIN_HALF, SIN_T = 3, [5, 64], [0, 999, 37]

# ------------------------------------------------------------------------------------------------------------ reparam
def reparam_inputs(n):
    return h((n,), f"step.rp.mu.{n}", 2.0), h((n,), f"step.rp.lv.{n}", 4.0), h((n,), f"step.rp.eps.{n}", 3.0)


# --------------------------------------------------------------------------------------------------------------- losses
SL1_BETA, SL1_SCALE = 0.1, 0.37
SL1_ULPS = [1, 2, 8]
RECON_W = [(1.0, 0.1), (0.0, 0.1), (1.0, 0.0)]


def smooth_l1_inputs(n):
    """|d| up to 0.6 around beta = 0.1: both branches.  Planted at the front, with target 0 so that d is exact: |d| 1, 2 and 8
    ulps below and above beta in both signs, |d| = beta, and d = 0."""
    pred, target = h((n,), f"step.sl1.p.{n}", 0.3), h((n,), f"step.sl1.t.{n}", 0.3)
    b = np.float32(SL1_BETA)
    plant = [b, -b] + [s * ulps(b, k * sg) for k in SL1_ULPS for sg in (1, -1) for s in (1, -1)]
    pred[:len(plant)] = torch.tensor(np.array(plant, dtype=np.float32))
    target[:len(plant)] = 0.0
    pred[len(plant)] = target[len(plant)] = 0.25
    return pred, target


def recon_inputs(n):
    """d = 0 at eight places (sign(0) = 0), spread so that several blocks see one."""
    pred, target = h((n,), f"step.rec.p.{n}", 1.0), h((n,), f"step.rec.t.{n}", 1.0)
    idx = torch.arange(8) * (n // 8)
    target[idx] = pred[idx]
    return pred, target


SUMSQ_N = [1000, 1001, 1003, N_SUMSQ]        # n % 4 = 0, 1, 3; past the cap (n % 4 = 1)
SUMSQ_PREV = 12.5


# ------------------------------------------------------------------------------------------------------- clip and AdamW
# (normsq, max_norm): clearly below (every bit stays); above; the norm within an ulp of max_norm from either side
CLIP = {"below": (0.25, 1.0), "above": (4e-4, 0.01), "at": (1.0, 1.0), "just-under": (0.999998, 1.0)}
CLIP_N = [N_SMALL, N_SCALAR]

ADAM = dict(lr=0.05, beta1=0.9, beta2=0.999, eps=1e-6, wd=0.01)
NORM_ABOVE, NORM_BELOW = (4e-4, 0.01), (4e-4, 1.0)            # (normsq, max_norm): coefficient 0.49998 / 1
# id: n, step, (normsq, max_norm) or None, overrides
ADAM_CASES = {
    "vec-step1": (1000, 1, NORM_ABOVE, {}),
    "vec-step2": (1000, 2, NORM_ABOVE, {}),
    "vec-step1000": (1000, 1000, NORM_ABOVE, {}),
    "vec-no-normsq": (1000, 2, None, {}),
    "vec-clip-below": (1000, 2, NORM_BELOW, {}),
    "vec-wd0": (1000, 2, NORM_ABOVE, {"wd": 0.0}),
    "scalar-1001": (1001, 2, NORM_ABOVE, {}),
    "scalar-past-cap": (N_SCALAR, 2, NORM_ABOVE, {}),
}
SCHED_LR = [0.05, 0.04, 0.03, 0.02]
SCHED_B1 = [0.95, 0.9, 0.85, 0.8]
SCHED_CALLS = 6                                               # *step_dev 0..5: entries 0, 1, 2, 3, 3, 3
SKIP_BITS = [1, 2, 4, 8, 32]
NO_SKIP_BITS = [16, 64]


def adam_kw(over):
    return dict(ADAM, **over)


def adam_inputs(n):
    """p, g, m, v (v >= 0) as fp32 tensors."""
    return (h((n,), f"step.adam.p.{n}", 1.0), h((n,), f"step.adam.g.{n}", 0.5), h((n,), f"step.adam.m.{n}", 0.1),
            h((n,), f"step.adam.v.{n}", 0.02).abs())
