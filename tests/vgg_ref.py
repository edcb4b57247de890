"""fp64 restatement of the stage-1 loss (reference: src/models/losses.py), generated VGG16 weights and inputs, the case table
and the recorded precision baseline for the perceptual-loss tests (test infrastructure, not a conftest; the style of
tests/gn_ref.py and tests/attn_ref.py).

`perceptual` / `combined` restate the reference on plain torch functions (clamp, F.interpolate, conv2d, relu, max_pool2d,
l1_loss, the KL formula) in ANY dtype: in float64 they are the reference every test compares against; in float32 / bfloat16 on
the CPU they are the yardstick - BASELINE_ERR records their error against float64 per case (tests/test_vgg_ref_cpu.py
re-measures and asserts the table), and the GPU tests allow the kernels four times that (`bar`).  Only the layers up to
max(feature_layers) run; a map recorded at a convolution's index is the one after the following ReLU (the reference's ReLUs are
in-place).
"""
import functools
import math

import torch
import torch.nn.functional as F

from oracle import hashgen

SEED = 1607
CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CONV_WIDTH = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
POOL_INDEX = (4, 9, 16, 23, 30)
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)

# name -> image shape and VGGPerceptualLoss arguments
CASES = {
    "odd": dict(shape=(2, 3, 23, 21), min_size=0, resize_to=224, feature_layers=(8, 15), weights=(1.0, 1.0)),       # pools 23x21 -> 11x10 -> 5x5
    "even": dict(shape=(1, 3, 16, 24), min_size=0, resize_to=224, feature_layers=(8, 15), weights=(1.0, 1.0)),      # nothing dropped
    "resize": dict(shape=(2, 3, 13, 15), min_size=200, resize_to=32, feature_layers=(8, 15), weights=(1.0, 1.0)),   # the resize leg, H != W
    "sprite": dict(shape=(1, 3, 215, 215), min_size=200, resize_to=224, feature_layers=(8, 15), weights=(1.0, 1.0)),  # production: 215 -> 107 -> 53
    "weights": dict(shape=(2, 3, 23, 21), min_size=0, resize_to=224, feature_layers=(3, 8), weights=(0.5, 2.0)),    # non-default constructor
}
LAST_RUN = max(max(c["feature_layers"]) for c in CASES.values())      # the deepest layer any case runs
COMBINED_CASE = "odd"
LATENT_SHAPE = (2, 8, 3, 3)
COMBINED_WEIGHTS = (1.0, 0.1, 0.01)          # reconstruction, perceptual, kl: CombinedLoss's defaults

# Error of the torch CPU pipeline in a precision against float64: (case, "fp32" | "bf16") -> {quantity: error}.  `loss` (and the
# combined case's parts) by relative error, gradients by rel-L2.  Filled from tests/test_vgg_ref_cpu.py's own run on 4 threads (it asserts
# that a re-measurement in that configuration gives every value within 25 %); the bars of tests/test_perceptual_gpu.py are derived from here alone.
BASELINE_ERR = {
    ("odd", "fp32"): dict(loss=3.230e-08, grad=3.235e-07),
    ("odd", "bf16"): dict(loss=1.008e-03, grad=1.512e-01),
    ("even", "fp32"): dict(loss=5.397e-08, grad=2.813e-07),
    ("even", "bf16"): dict(loss=4.367e-03, grad=1.576e-01),
    ("resize", "fp32"): dict(loss=2.254e-08, grad=1.125e-03),
    ("resize", "bf16"): dict(loss=3.198e-03, grad=1.017e-01),
    ("sprite", "fp32"): dict(loss=6.405e-08, grad=7.565e-04),
    ("sprite", "bf16"): dict(loss=1.492e-03, grad=1.728e-01),
    ("weights", "fp32"): dict(loss=5.318e-08, grad=2.440e-07),
    ("weights", "bf16"): dict(loss=1.593e-03, grad=1.249e-01),
    ("combined", "fp32"): dict(total=9.835e-09, reconstruction=1.623e-10, perceptual=6.087e-08, kl=8.990e-09, grad=8.437e-08, dmu=3.471e-08,
                               dlogvar=6.157e-08),
    ("combined", "bf16"): dict(total=5.291e-04, reconstruction=2.131e-03, perceptual=4.238e-03, kl=2.467e-04, grad=4.947e-02, dmu=3.499e-03,
                               dlogvar=4.517e-03),
}
BAR_FACTOR, BAR_FLOOR = 4.0, 1e-6


def bar(case, prec, what):
    """The GPU tests' bound for a quantity: four times the torch CPU error in the same precision, floored at 1e-6.  The factor
    allows for another summation order in the convolutions and the few ReLU / pool / sign decisions that flip when a value lies
    within rounding of a tie."""
    return max(BAR_FACTOR * BASELINE_ERR[(case, prec)][what], BAR_FLOOR)


def bf16_exact(t):
    return t.to(torch.bfloat16).to(torch.float32)


@functools.lru_cache(maxsize=None)
def vgg_state_dict(prefix="vgg_features."):
    """The 26 tensors of torchvision's vgg16().features, generated: He-scaled weights (uniform, variance 2 / fan_in),
    biases in +-0.1, all bf16-representable (a bf16 launch then reads exactly these values)."""
    sd, cin = {}, 3
    for i, cout in zip(CONV_INDEX, CONV_WIDTH):
        kw, kb = f"{prefix}{i}.weight", f"{prefix}{i}.bias"
        lim = math.sqrt(3.0) * math.sqrt(2.0 / (cin * 9))
        if i <= LAST_RUN:
            u = hashgen.uniform((cout, cin, 3, 3), SEED, hashgen.name_id(kw))
        else:                                    # never run by a case (only loaded): torch's seeded CPU generator is quicker for 14 M values
            u = torch.rand((cout, cin, 3, 3), generator=torch.Generator().manual_seed(SEED + i)) * 2.0 - 1.0
        sd[kw] = bf16_exact(u * lim)
        sd[kb] = bf16_exact(hashgen.uniform((cout,), SEED, hashgen.name_id(kb)) * 0.1)
        cin = cout
    return sd


def _plant(x, lo, hi):
    """Every 17th value exactly `lo`, the one after it exactly `hi`: the clamp's inclusive edges."""
    f = x.reshape(-1)
    f[0::17] = lo
    f[1::17] = hi
    return x


def images(case, unit=True):
    """(generated, target) fp32, independent draws.  unit: the [0, 1] entry point, values in about [-0.3, 1.3] with pixels exactly
    0 and 1; else CombinedLoss's [-1, 1] convention, values in [-1.3, 1.3] with pixels exactly -1 and 1."""
    shape = CASES[case]["shape"]
    out = []
    for which in ("generated", "target"):
        u = hashgen.uniform(shape, SEED, hashgen.name_id(f"{case}.{which}.{int(unit)}"))
        out.append(_plant(0.5 + 0.8 * u, 0.0, 1.0) if unit else _plant(1.3 * u, -1.0, 1.0))
    return out[0], out[1]


def latents():
    mu = hashgen.uniform(LATENT_SHAPE, SEED, hashgen.name_id("mu")) * 1.5
    logvar = hashgen.uniform(LATENT_SHAPE, SEED, hashgen.name_id("logvar")) * 2.0
    return mu, logvar


def _prep(x, a, b, min_size, resize_to, dtype):
    v = torch.clamp(a * x + b, 0, 1) if (a, b) != (1.0, 0.0) else torch.clamp(x, 0, 1)
    if v.shape[-1] < min_size:
        v = F.interpolate(v, size=(resize_to, resize_to), mode="bilinear", align_corners=False)
    mean = torch.tensor(MEAN, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    return (v - mean) / std


def feature_maps(x, sd, feature_layers, dtype, prefix="vgg_features."):
    """Maps at `feature_layers` (ascending) of a normalised image x, layers 0..max(feature_layers) only."""
    got, i, last = {}, 0, max(feature_layers)
    while i <= last:
        if i in POOL_INDEX:
            x = F.max_pool2d(x, 2, 2)
            hit = (i,)
            i += 1
        else:
            x = F.relu(F.conv2d(x, sd[f"{prefix}{i}.weight"].to(dtype), sd[f"{prefix}{i}.bias"].to(dtype), padding=1))
            hit = (i, i + 1)
            i += 2
        for j in hit:
            if j in feature_layers:
                got[j] = x
    return [got[j] for j in sorted(set(feature_layers))]


def _leaf(t, dtype):
    """The tensor the gradient is taken at: the fp32 input (float64 for the float64 restatement, whose gradient is not rounded)."""
    return t.detach().to(torch.float64 if dtype == torch.float64 else torch.float32).clone().requires_grad_(True)


def perceptual(generated, target, sd, case, dtype=torch.float64, a=1.0, b=0.0):
    """VGGPerceptualLoss.forward(a * generated + b, a * target + b) in `dtype` on the CPU.  Returns (loss, d loss / d generated)
    as float64 tensors."""
    c = CASES[case]
    g = _leaf(generated, dtype)
    loss = _perceptual_term(g, target, sd, c, dtype, a, b)
    loss.backward()
    return loss.detach().double(), g.grad.double()


def _perceptual_term(g, target, sd, c, dtype, a, b):
    fg = feature_maps(_prep(g.to(dtype), a, b, c["min_size"], c["resize_to"], dtype), sd, c["feature_layers"], dtype)
    with torch.no_grad():
        ft = feature_maps(_prep(target.to(dtype), a, b, c["min_size"], c["resize_to"], dtype), sd, c["feature_layers"], dtype)
    loss = 0.0
    for x, y, w in zip(fg, ft, c["weights"]):
        loss = loss + w * F.l1_loss(x, y)
    return loss


def kl(mu, logvar):
    return -0.5 * torch.sum(1 + logvar - mu.pow(2) - logvar.exp()) / mu.numel()


def combined(generated, target, mu, logvar, sd, case=COMBINED_CASE, dtype=torch.float64, weights=COMBINED_WEIGHTS):
    """CombinedLoss.forward in `dtype` on the CPU: a dict of float64 values - total, reconstruction, perceptual, kl and the
    gradients grad (generated), dmu, dlogvar of the total."""
    g, m, lv = _leaf(generated, dtype), _leaf(mu, dtype), _leaf(logvar, dtype)
    gd, td = g.to(dtype), target.to(dtype)
    rec = F.l1_loss(gd, td)
    perc = _perceptual_term(g, target, sd, CASES[case], dtype, 0.5, 0.5)
    k = kl(m.to(dtype), lv.to(dtype))
    total = weights[0] * rec + weights[1] * perc + weights[2] * k
    total.backward()
    d = dict(total=total, reconstruction=rec, perceptual=perc, kl=k, grad=g.grad, dmu=m.grad, dlogvar=lv.grad)
    return {n: v.detach().double() for n, v in d.items()}


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm())
