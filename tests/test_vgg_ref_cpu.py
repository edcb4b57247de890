"""CPU suite of the stage-1 loss: tests/vgg_ref.py's fp64 restatement against the reference's own logic on torch.nn modules,
the state-dict surface, the recorded precision baseline the GPU bars come from, torch's max-pool tie rule, and the argument
validation of every new psg_* entry (no launch without a GPU)."""
import ctypes as C
import functools
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import vgg_ref as R

PRECISIONS = {"fp32": torch.float32, "bf16": torch.bfloat16}


# ---- the reference's logic (src/models/losses.py) on torch.nn modules, fp64 --------------------------------------------------
class RefVGGPerceptualLoss(nn.Module):
    """losses.py:12-92 with vgg16().features rebuilt from plain containers (torchvision's layout, in-place ReLUs) instead of
    the torchvision download, a float64 accumulator, and the layer loop ended after the last recorded map; min_size / resize_to
    stand for the literals 200 / 224."""

    def __init__(self, feature_layers, weights, min_size=200, resize_to=224):
        super().__init__()
        self.feature_layers, self.weights, self.min_size, self.resize_to = list(feature_layers), list(weights), min_size, resize_to
        layers, cin = [], 3
        for i in range(31):
            if i in R.POOL_INDEX:
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            elif i in R.CONV_INDEX:
                cout = R.CONV_WIDTH[R.CONV_INDEX.index(i)]
                layers.append(nn.Conv2d(cin, cout, kernel_size=3, padding=1))
                cin = cout
            else:
                layers.append(nn.ReLU(inplace=True))
        self.vgg_features = nn.Sequential(*layers)
        for p in self.vgg_features.parameters():
            p.requires_grad = False

    def extract_features(self, x):
        mean_tensor = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1).to(x.dtype)
        std_tensor = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1).to(x.dtype)
        x = (x - mean_tensor) / std_tensor
        features = []
        for i, layer in enumerate(self.vgg_features.children()):
            x = layer(x)
            if i in self.feature_layers:
                features.append(x)
            if i == max(self.feature_layers):      # the reference runs on through all 31 layers and drops the results; the small
                break                               # test images do not survive five pools
        return features

    def forward(self, generated, target):
        generated = torch.clamp(generated, 0, 1)
        target = torch.clamp(target, 0, 1)
        if generated.shape[-1] < self.min_size:
            generated = F.interpolate(generated, size=(self.resize_to, self.resize_to), mode="bilinear", align_corners=False)
            target = F.interpolate(target, size=(self.resize_to, self.resize_to), mode="bilinear", align_corners=False)
        gen_features = self.extract_features(generated)
        target_features = self.extract_features(target)
        loss = torch.tensor(0.0, dtype=generated.dtype)
        for gen_feat, target_feat, weight in zip(gen_features, target_features, self.weights):
            loss = loss + weight * F.l1_loss(gen_feat, target_feat)
        return loss


class RefCombinedLoss(nn.Module):
    """losses.py:95-162."""

    def __init__(self, perceptual, reconstruction_weight=1.0, perceptual_weight=0.1, kl_weight=0.01):
        super().__init__()
        self.reconstruction_weight, self.perceptual_weight, self.kl_weight = reconstruction_weight, perceptual_weight, kl_weight
        self.l1_loss = nn.L1Loss()
        self.perceptual_loss = perceptual

    def forward(self, generated, target, mu, logvar):
        generated_norm = (generated + 1.0) / 2.0
        target_norm = (target + 1.0) / 2.0
        recon_loss = self.l1_loss(generated, target)
        perceptual_loss = self.perceptual_loss(generated_norm, target_norm)
        kl_loss = -0.5 * torch.sum(1 + logvar - mu.pow(2) - logvar.exp())
        kl_loss = kl_loss / (mu.numel())
        total_loss = self.reconstruction_weight * recon_loss + self.perceptual_weight * perceptual_loss + self.kl_weight * kl_loss
        return total_loss, dict(reconstruction=recon_loss, perceptual=perceptual_loss, kl=kl_loss)


def _ref_module(case):
    c = R.CASES[case]
    m = RefVGGPerceptualLoss(c["feature_layers"], c["weights"], c["min_size"], c["resize_to"])
    m.load_state_dict(R.vgg_state_dict())
    return m.double()


@functools.lru_cache(maxsize=None)
def _f64(case):
    g, t = R.images(case)
    return R.perceptual(g, t, R.vgg_state_dict(), case, torch.float64)


@functools.lru_cache(maxsize=None)
def _f64_combined():
    g, t = R.images(R.COMBINED_CASE, unit=False)
    mu, lv = R.latents()
    return R.combined(g, t, mu, lv, R.vgg_state_dict())


def _rel_close(got, ref, tol, what):
    err = R.rel(got, ref)
    assert err <= tol, f"{what}: relative error {err:.3e} > {tol:.1e}"


@pytest.mark.parametrize("case", list(R.CASES))
def test_restatement_equals_reference_logic(case):
    g, t = R.images(case)
    loss, grad = _f64(case)
    gd = g.double().requires_grad_(True)
    ref = _ref_module(case)(gd, t.double())
    ref.backward()
    _rel_close(loss, ref, 1e-12, f"{case} loss")
    _rel_close(grad, gd.grad, 1e-12, f"{case} image gradient")
    assert float(grad.abs().max()) > 0


def test_restatement_equals_reference_logic_combined():
    g, t = R.images(R.COMBINED_CASE, unit=False)
    mu, lv = R.latents()
    mine = _f64_combined()
    gd, md, ld = (v.double().requires_grad_(True) for v in (g, mu, lv))
    total, parts = RefCombinedLoss(_ref_module(R.COMBINED_CASE))(gd, t.double(), md, ld)
    total.backward()
    _rel_close(mine["total"], total, 1e-12, "total")
    for n, v in parts.items():
        _rel_close(mine[n], v, 1e-12, n)
    for n, v in (("grad", gd), ("dmu", md), ("dlogvar", ld)):
        _rel_close(mine[n], v.grad, 1e-12, n)


def test_planted_pixels_sit_on_the_clamp_edges():
    """The inputs exercise the clamp mask and its inclusive edges: pixels exactly 0 and 1 (-1 and 1 for CombinedLoss), values
    outside on both sides, and a gradient of exactly 0 outside."""
    g, _ = R.images("odd")
    assert int((g == 0).sum()) > 50 and int((g == 1).sum()) > 50 and float(g.min()) < -0.2 and float(g.max()) > 1.2
    grad = _f64("odd")[1]
    assert float(grad[(g < 0) | (g > 1)].abs().max()) == 0.0
    assert float(grad[(g == 0) | (g == 1)].abs().min()) > 0.0, "torch.clamp's gradient is 1 on the edges"
    gc, _ = R.images("odd", unit=False)
    assert int((gc == -1).sum()) > 50 and int((gc == 1).sum()) > 50


# ---- the module's surface ------------------------------------------------------------------------------------------------
VGG16_KEYS = [f"vgg_features.{i}.{p}" for i in (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28) for p in ("weight", "bias")]


def test_state_dict_is_torchvisions_vgg16_features():
    import pokemon_sprite_generator_amd as psg
    sd = R.vgg_state_dict()
    assert list(sd) == VGG16_KEYS and len(VGG16_KEYS) == 26
    m = psg.VGGPerceptualLoss(state_dict=sd)
    got = m.state_dict()
    assert list(got) == VGG16_KEYS
    cin = 3
    for i, cout in zip(R.CONV_INDEX, R.CONV_WIDTH):
        assert tuple(got[f"vgg_features.{i}.weight"].shape) == (cout, cin, 3, 3) and tuple(got[f"vgg_features.{i}.bias"].shape) == (cout,)
        assert torch.equal(got[f"vgg_features.{i}.weight"], sd[f"vgg_features.{i}.weight"])
        cin = cout
    assert len(m.vgg_features) == 31 and not any(p.requires_grad for p in m.parameters())
    c = psg.CombinedLoss()
    assert list(c.state_dict()) == ["perceptual_loss." + k for k in VGG16_KEYS]
    assert (c.reconstruction_weight, c.perceptual_weight, c.kl_weight) == (1.0, 0.1, 0.01)
    assert isinstance(c.l1_loss, nn.L1Loss) and isinstance(c.perceptual_loss, psg.VGGPerceptualLoss)
    assert not any(p.requires_grad for p in c.parameters())
    c.load_state_dict({"perceptual_loss." + k: v for k, v in sd.items()})


def test_losses_refuse_cpu_tensors():
    import pokemon_sprite_generator_amd as psg
    from pokemon_sprite_generator_amd import ops
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(psg.PsgError):
        psg.VGGPerceptualLoss()(x, x)
    with pytest.raises(psg.PsgError):
        psg.CombinedLoss()(x, x, torch.zeros(1, 8, 3, 3), torch.zeros(1, 8, 3, 3))
    for call in (lambda: ops.max_pool2x2(torch.zeros(1, 4, 4, 8)), lambda: ops.image_prep(x), lambda: ops.kl_loss(torch.zeros(4), torch.zeros(4)),
                 lambda: ops.feature_l1(torch.zeros(2, 8), torch.zeros(2, 8))):
        with pytest.raises(psg.PsgError):
            call()


# ---- the precision baseline -------------------------------------------------------------------------------------------------
PINNED_THREADS = 4        # the configuration BASELINE_ERR was recorded in: the CPU convolutions' summation order depends on it
REL_TOL = 0.25            # another CPU may give other low bits; an entry is an error figure of one or two significant digits


def measure_baseline(case, prec):
    """{quantity: error against float64} of the torch CPU pipeline in one precision, on PINNED_THREADS threads."""
    dtype, sd = PRECISIONS[prec], R.vgg_state_dict()
    before = torch.get_num_threads()
    torch.set_num_threads(PINNED_THREADS)
    try:
        if case == "combined":
            g, t = R.images(R.COMBINED_CASE, unit=False)
            mu, lv = R.latents()
            got, ref = R.combined(g, t, mu, lv, sd, dtype=dtype), _f64_combined()
            return {n: R.rel(got[n], ref[n]) for n in ref}
        g, t = R.images(case)
        loss, grad = R.perceptual(g, t, sd, case, dtype)
        rl, rg = _f64(case)
        return {"loss": R.rel(loss, rl), "grad": R.rel(grad, rg)}
    finally:
        torch.set_num_threads(before)


@pytest.mark.parametrize("prec", list(PRECISIONS))
@pytest.mark.parametrize("case", list(R.CASES) + ["combined"])
def test_baseline_err_is_torchs_own_error(case, prec):
    """Every recorded value, the ones under the bars' floor included, against a re-measurement: |measured - recorded| <=
    REL_TOL * recorded."""
    got = measure_baseline(case, prec)
    print(f"BASELINE {case} {prec} " + " ".join(f"{n}={v:.3e}" for n, v in got.items()))
    rec = R.BASELINE_ERR[(case, prec)]
    assert set(rec) == set(got)
    for n, v in got.items():
        assert abs(v - rec[n]) <= REL_TOL * rec[n], f"{case} {prec} {n}: measured {v:.3e}, recorded {rec[n]:.3e}"
        assert R.bar(case, prec, n) == max(4.0 * rec[n], 1e-6)


# ---- torch's tie rule -----------------------------------------------------------------------------------------------------
def test_max_pool_ties_go_to_the_first_tap():
    """torch.max_pool2d on the CPU replaces the running maximum only by a strictly greater value: among equal maxima the first
    tap in row-major order is recorded and receives the whole gradient.  psg_maxpool2x2_fwd / _bwd follow this rule."""
    x = torch.tensor([[[[1.0, 1.0, 0.0, 2.0, 9.0],
                        [1.0, 1.0, 2.0, 2.0, 9.0],
                        [3.0, 0.0, -1.0, -1.0, 9.0],
                        [0.0, 3.0, -1.0, -2.0, 9.0],
                        [7.0, 7.0, 7.0, 7.0, 9.0]]]], requires_grad=True)
    y, idx = F.max_pool2d(x, 2, 2, return_indices=True)
    assert y.tolist() == [[[[1.0, 2.0], [3.0, -1.0]]]]
    assert idx.tolist() == [[[[0, 3], [10, 12]]]]                       # flat h * 5 + w: all-equal -> tap 0; (0,3) before (1,2), (1,3)
    dy = torch.tensor([[[[10.0, 20.0], [30.0, 40.0]]]])
    y.backward(dy)
    want = torch.zeros(5, 5)
    want[0, 0], want[0, 3], want[2, 0], want[2, 2] = 10.0, 20.0, 30.0, 40.0
    assert torch.equal(x.grad[0, 0], want)                                # the dropped last row and column get zeros


# ---- argument validation of the new entries -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


P = 0x1000          # a 16-byte aligned address nothing dereferences on the host
ARG, SHAPE, DTYPE, ALIGN, WS = -6, -1, -2, -3, -4


def test_maxpool_argument_validation(lib):
    f = lib.psg_maxpool2x2_fwd
    assert f(None, 8, P, 8, P, 1, 4, 6, 8, 1, None) == ARG and b"null" in lib.psg_last_error()
    assert f(P, 8, None, 8, P, 1, 4, 6, 8, 1, None) == ARG
    assert f(P, 8, P, 8, P, 1, 4, 6, 8, 7, None) == DTYPE
    assert f(P, 8, P, 8, P, 0, 4, 6, 8, 1, None) == SHAPE
    assert f(P, 8, P, 8, P, 1, 1, 6, 8, 1, None) == SHAPE                 # Hi < 2: no output row
    assert f(P, 12, P, 12, P, 1, 4, 6, 12, 1, None) == SHAPE              # C not a multiple of 8 for bf16
    assert f(P, 12, P, 8, P, 1, 4, 6, 8, 1, None) == SHAPE and b"ld" in lib.psg_last_error()
    assert f(P, 4, P, 8, P, 1, 4, 6, 8, 0, None) == SHAPE                 # ld < C
    assert f(P + 4, 8, P, 8, P, 1, 4, 6, 8, 0, None) == ALIGN
    assert f(P, 8, P, 8, P + 4, 1, 4, 6, 8, 0, None) == ALIGN             # tap
    b = lib.psg_maxpool2x2_bwd
    assert b(None, 8, P, P, 8, 1, 4, 6, 8, 1, None) == ARG
    assert b(P, 8, None, P, 8, 1, 4, 6, 8, 1, None) == ARG                # the taps are not optional in backward
    assert b(P, 8, P, None, 8, 1, 4, 6, 8, 1, None) == ARG
    assert b(P, 8, P, P, 8, 1, 4, 6, 8, 5, None) == DTYPE
    assert b(P, 8, P, P, 8, 1, 4, 0, 8, 1, None) == SHAPE
    assert b(P, 8, P, P, 20, 1, 4, 6, 8, 1, None) == SHAPE                # lddx not a multiple of 8
    assert b(P, 8, P, P + 8, 8, 1, 4, 6, 8, 1, None) == ALIGN


def test_image_prep_argument_validation(lib):
    f = lib.psg_image_prep_fwd
    assert f(None, P, 8, 1, 4, 4, 4, 4, 1.0, 0.0, 0, None) == ARG
    assert f(P, None, 8, 1, 4, 4, 4, 4, 1.0, 0.0, 0, None) == ARG
    assert f(P, P, 8, 1, 4, 4, 4, 4, 1.0, 0.0, 2, None) == DTYPE
    assert f(P, P, 8, 1, 0, 4, 4, 4, 1.0, 0.0, 0, None) == SHAPE
    assert f(P, P, 8, 1, 4, 4, 4, -1, 1.0, 0.0, 0, None) == SHAPE
    assert f(P, P, 4, 1, 4, 4, 4, 4, 1.0, 0.0, 0, None) == SHAPE          # ld < 8 columns
    assert f(P, P, 12, 1, 4, 4, 4, 4, 1.0, 0.0, 1, None) == SHAPE         # bf16 rows are whole 8-element chunks
    assert f(P, P + 8, 8, 1, 4, 4, 4, 4, 1.0, 0.0, 0, None) == ALIGN
    b = lib.psg_image_prep_bwd
    assert b(None, P, 8, P, 1, 4, 4, 4, 4, 1.0, 0.0, 0, None) == ARG
    assert b(P, None, 8, P, 1, 4, 4, 4, 4, 1.0, 0.0, 0, None) == ARG
    assert b(P, P, 8, None, 1, 4, 4, 4, 4, 1.0, 0.0, 0, None) == ARG
    assert b(P, P, 8, P, 1, 4, 4, 4, 4, 1.0, 0.0, 9, None) == DTYPE
    assert b(P, P, 8, P, 1, 4, 0, 4, 4, 1.0, 0.0, 0, None) == SHAPE
    assert b(P, P, 8, P, 1, 4, 4, 0, 4, 1.0, 0.0, 0, None) == SHAPE
    assert b(P, P, 6, P, 1, 4, 4, 4, 4, 1.0, 0.0, 0, None) == SHAPE
    assert b(P, P + 2, 8, P, 1, 4, 4, 4, 4, 1.0, 0.0, 1, None) == ALIGN


def test_feat_l1_and_kl_argument_validation(lib):
    need = lib.psg_feat_l1_workspace_bytes()
    assert need > 0
    f = lib.psg_feat_l1
    assert f(None, 8, P, 8, None, 0, P, 4, 8, 1.0, 0, P, need, None) == ARG
    assert f(P, 8, None, 8, None, 0, P, 4, 8, 1.0, 0, P, need, None) == ARG
    assert f(P, 8, P, 8, None, 0, None, 4, 8, 1.0, 0, P, need, None) == ARG
    assert f(P, 8, P, 8, None, 0, P, 4, 8, 1.0, 0, None, need, None) == ARG
    assert f(P, 8, P, 8, None, 0, P, 4, 8, 1.0, 3, P, need, None) == DTYPE
    assert f(P, 8, P, 8, None, 0, P, 0, 8, 1.0, 0, P, need, None) == SHAPE
    assert f(P, 6, P, 6, None, 0, P, 4, 6, 1.0, 0, P, need, None) == SHAPE            # cols not a whole chunk
    assert f(P, 8, P, 4, None, 0, P, 4, 8, 1.0, 0, P, need, None) == SHAPE            # ldb < cols
    assert f(P, 8, P, 8, P, 12, P, 4, 8, 1.0, 1, P, need, None) == SHAPE              # ld of grad
    assert f(P, 8, P + 4, 8, None, 0, P, 4, 8, 1.0, 0, P, need, None) == ALIGN
    assert f(P, 8, P, 8, None, 0, P, 4, 8, 1.0, 0, P, need - 1, None) == WS
    k = lib.psg_kl_f32
    kneed = lib.psg_kl_workspace_bytes()
    assert kneed > 0
    assert k(None, P, None, None, P, 7, P, kneed, None) == ARG
    assert k(P, None, None, None, P, 7, P, kneed, None) == ARG
    assert k(P, P, None, None, None, 7, P, kneed, None) == ARG
    assert k(P, P, None, None, P, 7, None, kneed, None) == ARG
    assert k(P, P, None, None, P, 0, P, kneed, None) == SHAPE
    assert k(P, P, None, None, P, 7, P + 4, kneed, None) == ALIGN
    assert k(P, P, None, None, P, 7, P, kneed - 1, None) == WS
