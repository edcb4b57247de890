"""Stage 1's loss on the MI355X kernels (reference: src/models/losses.py; used by vae_trainer.py:214,249-286).

`CombinedLoss` = L1 + 0.1 * `VGGPerceptualLoss` + kl_weight * KL.  Same classes, constructor and forward signatures and
state-dict keys as the reference; torchvision is not imported and no pretrained file is fetched: the VGG16 weights come from
a state dict (`state_dict=` or `load_state_dict`, a torchvision `vgg16().features` dict under the prefix `vgg_features.`).

Data flow of the perceptual term, channels-last in `compute_dtype`:

    generated [B,3,H,W] fp32 --ops.image_prep--> [B,H',W',8] --(ops.conv2d + ReLU | ops.max_pool2x2)* --> feature maps
    target, once, under no_grad, on the inference launches (ops.conv_infer with prepared weights, no saved pre-activations)
    loss = sum_i weights[i] * ops.feature_l1(gen_i, target_i)                       (fp32 device scalar)

Only the layers 0..max(feature_layers) run (the reference runs all 31 and uses two).  The reference's ReLUs are in-place,
so the map it records at a convolution's index is the one after the ReLU that follows; conv + ReLU is one launch here and
serves both indices.  The resize happens only for images narrower than `min_size` (200): the 215-pixel sprites run VGG at
215 x 215, pooled 215 -> 107 -> 53 (floor).  Gradients reach `generated` only; the VGG parameters are frozen containers.
"""
from typing import List

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import ACT_RELU
from .ops import conv_infer as _conv, prep_weight as _prep, prepared as _prepared

# torchvision's VGG16 ("D") feature extractor: 13 convolutions at indices 0,2,5,7,10,12,14,17,19,21,24,26,28 of 31 entries
_VGG16_CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")


def _vgg16_features():
    layers, cin = [], 3
    for v in _VGG16_CFG:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    return nn.Sequential(*layers)


class VGGPerceptualLoss(nn.Module):
    """L1 between VGG16 feature maps of the generated and the target image (losses.py:12-92).  Images in [0, 1]."""

    def __init__(self, feature_layers: List[int] = [8, 15], weights: List[float] = [1.0, 1.0], state_dict=None,
                 compute_dtype: torch.dtype = torch.float32, min_size: int = 200, resize_to: int = 224):
        super().__init__()
        self.feature_layers = list(feature_layers)
        self.weights = list(weights)
        self.compute_dtype = compute_dtype
        self.min_size, self.resize_to = int(min_size), int(resize_to)
        self.vgg_features = _vgg16_features()
        if not self.feature_layers or min(self.feature_layers) < 0 or max(self.feature_layers) >= len(self.vgg_features):
            raise ValueError(f"feature_layers {self.feature_layers} outside VGG16's 0..{len(self.vgg_features) - 1}")
        if state_dict is not None:
            self.load_state_dict(state_dict)
        for p in self.vgg_features.parameters():
            p.requires_grad = False
        # launches: ("conv", index of the Conv2d; its ReLU is index + 1) or ("pool", index), up to the last recorded map
        self._plan, i, last = [], 0, max(self.feature_layers)
        while i <= last:
            if isinstance(self.vgg_features[i], nn.Conv2d):
                self._plan.append(("conv", i))
                i += 2
            else:
                self._plan.append(("pool", i))
                i += 1
        self._cache = {}

    # ---- the two forwards ---------------------------------------------------------------------------------------
    def _size(self, img):
        return (self.resize_to, self.resize_to) if img.shape[-1] < self.min_size else None

    def _maps(self, x, grad):
        """Feature maps (channels-last) at `feature_layers`, in the reference's order (ascending layer index), from the prepared
        image x [B,H,W,8].  grad: the autograd nodes of `ops`; else the inference launches."""
        dt = self.compute_dtype
        got = {}
        for kind, i in self._plan:
            if kind == "pool":
                x = ops.max_pool2x2(x)
                hit = (i,)
            else:
                m = self.vgg_features[i]
                pin = (-m.in_channels) % 8                       # 3 image channels in one 16-byte chunk, zero weight columns
                if grad:
                    w = m.weight if not pin else _prepared(self._cache, ("pad", i), [m.weight], lambda m=m, pin=pin: torch.nn.functional.pad(
                        m.weight.detach().float(), (0, 0, 0, 0, 0, pin)).contiguous())
                    x = ops.conv2d(x, w, m.bias, act=ACT_RELU)
                else:
                    wf = _prepared(self._cache, (i, dt), [m.weight], lambda m=m, pin=pin: _prep(m.weight, dt, pad_in=pin))
                    x = _conv(x, wf, m.bias, m.in_channels + pin, m.out_channels, 3, 1, 1, act=ACT_RELU)
                hit = (i, i + 1)
            for j in hit:
                if j in self.feature_layers:
                    got[j] = x
        return [got[j] for j in sorted(set(self.feature_layers))]

    def _check(self, *imgs):
        for t in imgs:
            if not t.is_cuda:
                raise _lib.PsgError("VGGPerceptualLoss (MI355X build) needs GPU tensors; there is no CPU fallback")
            if t.dim() != 4 or t.shape[1] != 3:
                raise _lib.PsgError(f"VGGPerceptualLoss: expected [B,3,H,W] images, got {tuple(t.shape)}")

    def extract_features(self, x: torch.Tensor) -> List[torch.Tensor]:
        """losses.py:40-61 for an image in [0, 1] (values outside are clamped): the recorded maps as fp32 NCHW tensors."""
        self._check(x)
        h = ops.image_prep(x, 1.0, 0.0, None, self.compute_dtype)
        return [ops.nhwc_to_nchw(f) for f in self._maps(h, torch.is_grad_enabled() and x.requires_grad)]

    def prepared(self, generated: torch.Tensor, target: torch.Tensor, a: float = 1.0, b: float = 0.0) -> torch.Tensor:
        """forward(a * generated + b, a * target + b) with the affine map folded into the preprocessing pass (CombinedLoss's
        (x + 1) / 2 is a = b = 0.5)."""
        self._check(generated, target)
        if generated.shape != target.shape:
            raise _lib.PsgError(f"VGGPerceptualLoss: shapes {tuple(generated.shape)} and {tuple(target.shape)} differ")
        dt, size = self.compute_dtype, self._size(generated)
        with torch.no_grad():
            tmaps = self._maps(ops.image_prep(target, a, b, size, dt), False)
        want = torch.is_grad_enabled() and generated.requires_grad
        gmaps = self._maps(ops.image_prep(generated, a, b, size, dt), want)
        loss = None
        for g, t, w in zip(gmaps, tmaps, self.weights):
            term = ops.feature_l1(g, t, w)
            loss = term if loss is None else loss + term
        return loss

    def forward(self, generated: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return self.prepared(generated, target, 1.0, 0.0)


class CombinedLoss(nn.Module):
    """reconstruction_weight * L1 + perceptual_weight * VGG perceptual + kl_weight * KL (losses.py:95-162); `generated` and
    `target` in [-1, 1].  Gradients reach `generated`, `mu` and `logvar`."""

    PARTS = ("total_loss", "reconstruction_loss", "perceptual_loss", "kl_loss")

    def __init__(self, reconstruction_weight: float = 1.0, perceptual_weight: float = 0.1, kl_weight: float = 0.01,
                 state_dict=None, compute_dtype: torch.dtype = torch.float32):
        super().__init__()
        self.reconstruction_weight = reconstruction_weight
        self.perceptual_weight = perceptual_weight
        self.kl_weight = kl_weight              # (vae_trainer.py:264-273 rewrites the three weights between batches)
        self.l1_loss = nn.L1Loss()
        self.perceptual_loss = VGGPerceptualLoss(compute_dtype=compute_dtype)
        if state_dict is not None:
            self.load_state_dict(state_dict)

    def forward_tensors(self, generated, target, mu, logvar):
        """(total, parts): parts = fp32 device tensor [total, reconstruction, perceptual, kl] (detached).  No host
        synchronisation: the call can sit inside a captured graph."""
        if not generated.is_cuda:
            raise _lib.PsgError("CombinedLoss (MI355X build) needs GPU tensors; there is no CPU fallback")
        rec = ops.recon_loss(generated, target, w_l1=1.0, w_mse=0.0)[0]
        perc = self.perceptual_loss.prepared(generated, target, 0.5, 0.5)
        kl = ops.kl_loss(mu, logvar)
        total = self.reconstruction_weight * rec + self.perceptual_weight * perc + self.kl_weight * kl
        return total, torch.stack([total.detach(), rec.detach(), perc.detach(), kl.detach()])

    def forward(self, generated, target, mu, logvar):
        total, parts = self.forward_tensors(generated, target, mu, logvar)
        return total, dict(zip(self.PARTS, parts.tolist()))
