"""VAE encoder / decoder on the MI355X kernels (reference: src/models/vae_decoder.py).

The VAE sits either side of the U-Net path: stage 2 encodes every image batch with the FROZEN encoder before the train
step (improved_diffusion_trainer.py:198-208,357-358) and decodes sampled latents for monitoring (:598); stage 3 and the
demo decode with it.  By default its parameters are never trained here (they are containers with the reference's names and
shapes, so `load_state_dict` takes a stage-1 checkpoint's 'vae_state_dict' halves unchanged), and the encoder runs under
`torch.no_grad()`.

One forward per module.  Every module has ONE body, written on the autograd nodes of `ops` (`ops.conv2d`, `ops.linear`,
`ops.conv4s2_relu` for the encoder's three 4x4 stride-2 convolutions, `ops.group_norm[_split]`, `ops.attention_cross_longq`,
`ops.reparam`, `ops.image_out`); the public `forward`s only decide the grad mode.  Under no_grad a node issues its forward launch
and keeps nothing, so inference and training run the same launches in the same order.  Every prepared weight comes from
`ops.WeightCache` under its one stamp (storage pointer, version counter, the epoch that `WeightCache.invalidate()` bumps for
optimizers writing through raw pointers, dtype): a block called through its own `forward` sees an update of either kind, as
the whole encoder / decoder does.  The padded operands enter the same cache: the first convolution's Cin 3 -> 8 as
`WeightCache.get(..., pad_in=)`, the image convolution's Cout 3 -> 4 | 8 as `WeightCache.derived` copies
(`VAEDecoder._image_conv`).  A module's entries are released when it is collected (`_release_on_collect`).

What is trainable, opt-in: `VAEEncoder(..., trainable=True)` has parameters that require grad and, called with grad mode on,
gradients reach all 70 of them (stage 1, src/training/vae_trainer.py; psg_conv4s2_dgrad / psg_conv4s2_wgrad, csrc/conv4s2.hip).
`VAEDecoder(..., trainable=True)` likewise: every one of its 144 parameters receives a gradient - the convolutions' and the
k / v Linears' through psg_conv_wgrad or, for the high-resolution layers of blocks 4 and 5 in bf16, psg_conv_wgrad_slim
(`ops._deliver_gemm_grads`, `ops._wgrad_slim_route`), the GroupNorms' from psg_groupnorm_bwd_res; the 3-channel image
convolution is computed in 8 output columns and its gradients come back at the parameter's own [3,32,3,3] / [3] shapes
(`ops.pad_rows`).  `PokemonVAE(..., trainable=True)` builds both halves trainable and its `forward` carries the graph encoder
-> latent -> decoder.  The steppers are `vae_stepper.VAEStepper` (stage 1) and `final.FinalStepper` (stage 3, whose joint
phase unfreezes a `trainable=True` decoder: `VAEDecoder.live_weights`).

A default DECODER is frozen (a parameter switched to requires_grad by hand raises, `_require_frozen`) but differentiable with
respect to its inputs: stage 3 trains the text encoder through it (final_trainer.py:215-236), so when grad mode is on and
`text_emb` or `latent` requires grad, `VAEDecoder.forward` keeps grad mode on (data gradients only; the cross-attention
backward is psg_attn_bwd_longq).  Every other call runs under no_grad.

Same classes / constructor and forward signatures as the reference: `ResNetBlock`, `CrossAttentionBlock`, `VAEEncoder`,
`VAEDecoder`, `PokemonVAE`.  Everything runs channels-last in `compute_dtype` on the kernels of the U-Net path:
3x3 / 1x1 convolutions and the encoder's 4x4 stride-2 convolutions (psg_conv_fwd, fused bias / ReLU / Tanh / residual),
GroupNorm+SiLU, bilinear upsampling and the attention core.  Reference quirks kept, not fixed: the decoder's
cross-attention reshapes the [B, S, C] key / value projections straight to [B, heads, head_dim, S]
(vae_decoder.py:56-57 - a reinterpretation of memory, not a transpose), and the encoder returns a SAMPLED latent.
"""
import weakref

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import ACT_TANH


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _release_on_collect(module):
    """`ops.WeightCache` entries keep their parameter alive: a module's are dropped when the module is collected."""
    weakref.finalize(module, ops.WeightCache.drop, list(module.parameters()))


def _require_frozen(module):
    """The differentiable path produces data gradients only: a trainable VAE parameter would silently get none."""
    for n, p in module.named_parameters():
        if p.requires_grad:
            raise _lib.PsgError(f"{type(module).__name__}: parameter {n} has requires_grad=True, but VAE weight gradients (stage 1, "
                                "and the joint phase of stage 3) are not built; freeze the VAE")


class ResNetBlock(nn.Module):
    """vae_decoder.py:8-32."""

    def __init__(self, in_channels: int, out_channels: int, groups: int = 32, dropout: float = 0.0):
        super().__init__()
        self.norm1 = nn.GroupNorm(groups, in_channels)
        self.conv1 = nn.Conv2d(in_channels, out_channels, kernel_size=3, padding=1)
        self.norm2 = nn.GroupNorm(groups, out_channels)
        self.conv2 = nn.Conv2d(out_channels, out_channels, kernel_size=3, padding=1)
        self.dropout = nn.Dropout(dropout)
        self.shortcut = nn.Conv2d(in_channels, out_channels, kernel_size=1) if in_channels != out_channels else nn.Identity()
        _release_on_collect(self)

    def nhwc(self, x):
        """x [B,H,W,C] in the compute dtype, on the nodes of `ops`: with grad mode on, data gradients and the gradient of every
        parameter that requires one."""
        h, xs = ops.group_norm_split(x, self.norm1.weight, self.norm1.bias, self.norm1.num_groups, self.norm1.eps, silu=True)
        h = ops.conv2d(h, self.conv1.weight, self.conv1.bias)
        h = ops.group_norm(h, self.norm2.weight, self.norm2.bias, self.norm2.num_groups, self.norm2.eps, silu=True)
        skip = ops.conv2d(xs, self.shortcut.weight, self.shortcut.bias) if isinstance(self.shortcut, nn.Conv2d) else xs
        return ops.conv2d(h, self.conv2.weight, self.conv2.bias, residual=skip)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        dt = getattr(self, "compute_dtype", torch.float32)
        if _wants_grad(x):
            _require_frozen(self)
            return ops.nhwc_to_nchw(self.nhwc(ops.nchw_to_nhwc_grad(x, dt)))
        with torch.no_grad():
            return ops.nhwc_to_nchw(self.nhwc(ops.nchw_to_nhwc(x, dt)))


class CrossAttentionBlock(nn.Module):
    """vae_decoder.py:33-65 - the decoder's hand-rolled text cross-attention."""

    def __init__(self, channels: int, text_dim: int, num_heads: int = 8):
        super().__init__()
        self.channels, self.text_dim, self.num_heads = channels, text_dim, num_heads
        self.head_dim = channels // num_heads
        self.norm = nn.GroupNorm(32, channels)
        self.q = nn.Conv2d(channels, channels, kernel_size=1)
        self.k = nn.Linear(text_dim, channels)
        self.v = nn.Linear(text_dim, channels)
        self.proj = nn.Conv2d(channels, channels, kernel_size=1)
        _release_on_collect(self)

    def nhwc(self, x, text):
        """x [B,H,W,C], text [B,S,text_dim] in the compute dtype, on the nodes of `ops`; the attention core's backward is
        psg_attn_bwd_longq."""
        B, H, W, C = x.shape
        S = text.shape[1]
        xn, xs = ops.group_norm_split(x, self.norm.weight, self.norm.bias, self.norm.num_groups, self.norm.eps)
        q = ops.conv2d(xn, self.q.weight, self.q.bias).reshape(B, H * W, C)
        k = ops.linear(text, self.k.weight, self.k.bias)
        v = ops.linear(text, self.v.weight, self.v.bias)
        # vae_decoder.py:56-57: `.reshape(b, heads, head_dim, -1)` of a [b, S, C] tensor reads its memory as [C][S]:
        # key token s' of channel c is element c*S + s' of the projection's buffer.  The attention kernel wants [S][C] rows:
        # a reshape + transpose of views, differentiated by autograd as such.
        kv = torch.cat([k.reshape(B, C, S).transpose(1, 2), v.reshape(B, C, S).transpose(1, 2)], dim=-1).contiguous()
        o = ops.attention_cross_longq(q, kv, self.num_heads)
        return ops.conv2d(o.reshape(B, H, W, C), self.proj.weight, self.proj.bias, residual=xs)

    def forward(self, x: torch.Tensor, text_emb: torch.Tensor) -> torch.Tensor:
        dt = getattr(self, "compute_dtype", torch.float32)
        if _wants_grad(x, text_emb):
            _require_frozen(self)
            xin = ops.nchw_to_nhwc_grad(x, dt) if x.requires_grad else ops.nchw_to_nhwc(x, dt)
            return ops.nhwc_to_nchw(self.nhwc(xin, text_emb.to(dt).contiguous()))
        with torch.no_grad():
            return ops.nhwc_to_nchw(self.nhwc(ops.nchw_to_nhwc(x, dt), text_emb.to(dt).contiguous()))


class VAEEncoder(nn.Module):
    """vae_decoder.py:68-125: 215 -> 107 -> 53 -> 27 by three 4x4 stride-2 convolutions (+ReLU, ResNetBlock), four more
    ResNetBlocks up to 512 channels, mu / logvar 3x3 projections, reparameterised sample."""

    def __init__(self, input_channels: int = 3, latent_dim: int = 8, compute_dtype: torch.dtype = torch.float32, trainable: bool = False):
        super().__init__()
        self.latent_dim = latent_dim
        self.trainable = bool(trainable)
        self.encoder = nn.Sequential(
            nn.Conv2d(input_channels, 32, kernel_size=4, stride=2, padding=1), nn.ReLU(), ResNetBlock(32, 32),
            nn.Conv2d(32, 64, kernel_size=4, stride=2, padding=1), nn.ReLU(), ResNetBlock(64, 64),
            nn.Conv2d(64, 128, kernel_size=4, stride=2, padding=2), nn.ReLU(), ResNetBlock(128, 128),
            ResNetBlock(128, 256), ResNetBlock(256, 256), ResNetBlock(256, 512), ResNetBlock(512, 512),
        )
        self.mu_proj = nn.Conv2d(512, latent_dim, kernel_size=3, padding=1)
        self.logvar_proj = nn.Conv2d(512, latent_dim, kernel_size=3, padding=1)
        self.compute_dtype = compute_dtype
        for p in self.parameters():                  # frozen unless asked
            p.requires_grad_(self.trainable)
        _release_on_collect(self)

    def forward(self, x: torch.Tensor, eps: torch.Tensor = None, generator: torch.Generator = None):
        """x [B,3,H,W] -> (latent, mu, logvar), each [B,latent_dim,h,w] fp32 (215 -> 27).  `eps` (default: randn of mu's
        shape, from `generator` when given - a data-parallel rank's own stream) is the reparameterisation noise the
        reference draws with randn_like (:121).  A `trainable` encoder called with grad mode on returns outputs that carry
        gradients to all its parameters; every other call runs under no_grad."""
        if not x.is_cuda:
            raise _lib.PsgError("VAEEncoder (MI355X build) needs GPU tensors; there is no CPU fallback")
        if self.trainable and torch.is_grad_enabled():
            if x.requires_grad:
                raise _lib.PsgError("VAEEncoder: the image has requires_grad=True, but nothing differentiates with respect to the image "
                                    "(the first convolution's data gradient is never computed); detach it")
            return self._forward(x, eps, generator)
        with torch.no_grad():
            return self._forward(x, eps, generator)

    def _draw_eps(self, mu, eps, generator):
        if eps is None:
            eps = torch.randn_like(mu) if generator is None else torch.randn(mu.shape, dtype=mu.dtype, device=mu.device, generator=generator)
        return eps.detach().to(device=mu.device, dtype=torch.float32).contiguous()

    def _forward(self, x, eps, generator):
        """The three 4x4 stride-2 convolutions (+ the ReLU after each) are `ops.conv4s2_relu` (own gradient kernels, stage 1,
        vae_trainer.py), everything else the nodes the decoder and the U-Net use."""
        dt = self.compute_dtype
        Cin = x.shape[1]
        # image -> channels-last with the channel count padded to one 16-byte chunk (zeros; conv4s2_relu pads the weight alike)
        h = ops.nchw_to_nhwc(x, dt, width=Cin + (-Cin) % 8)
        for m in self.encoder:
            if isinstance(m, nn.Conv2d):
                h = ops.conv4s2_relu(h, m.weight, m.bias, m.padding[0])
            elif isinstance(m, ResNetBlock):
                h = m.nhwc(h)                    # (called directly: ResNetBlock.forward guards its own, frozen, entry)
        mu = ops.nhwc_to_nchw(ops.conv2d(h, self.mu_proj.weight, self.mu_proj.bias))
        logvar = ops.nhwc_to_nchw(ops.conv2d(h, self.logvar_proj.weight, self.logvar_proj.bias))
        return ops.reparam(mu, logvar, self._draw_eps(mu, eps, generator)), mu, logvar


class VAEDecoder(nn.Module):
    """vae_decoder.py:128-222: 27 -> 54 -> 108 -> 215 with a text cross-attention in every block."""

    def __init__(self, latent_dim: int = 8, text_dim: int = 256, output_channels: int = 3, compute_dtype: torch.dtype = torch.float32,
                 trainable: bool = False):
        super().__init__()
        self.latent_dim, self.text_dim = latent_dim, text_dim
        self.trainable = bool(trainable)
        self.latent_proj = nn.Conv2d(latent_dim, 512, kernel_size=3, padding=1)
        chans = [(512, 512), (512, 256), (256, 128), (128, 64), (64, 32)]
        for i, (cin, cout) in enumerate(chans, start=1):
            setattr(self, f"block{i}_resnet1", ResNetBlock(cin, cout))
            setattr(self, f"block{i}_attn", CrossAttentionBlock(cout, text_dim))
            setattr(self, f"block{i}_resnet2", ResNetBlock(cout, cout))
            if i in (2, 3):
                setattr(self, f"block{i}_upsample", nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False))
            elif i == 4:
                setattr(self, f"block{i}_upsample", nn.Upsample(size=(215, 215), mode="bilinear", align_corners=False))
        self.final_conv = nn.Sequential(nn.GroupNorm(8, 32), nn.SiLU(), nn.Conv2d(32, output_channels, kernel_size=3, padding=1), nn.Tanh())
        self.compute_dtype = compute_dtype
        for p in self.parameters():                  # frozen unless asked
            p.requires_grad_(self.trainable)
        _release_on_collect(self)

    def forward(self, latent: torch.Tensor, text_emb: torch.Tensor) -> torch.Tensor:
        """latent [B,latent_dim,h,w], text_emb [B,S,text_dim] -> image [B,3,215,215] fp32.  A `trainable` decoder whose
        parameters require grad (`live_weights`), called with grad mode on, returns an image that carries gradients to all its
        parameters (stage 1, vae_trainer.py; stage 3's joint phase) and to `latent` / `text_emb` when they ask; a frozen one carries the inputs' gradients when an input requires grad (data gradients only:
        `_require_frozen`); every other call runs under no_grad."""
        if not latent.is_cuda:
            raise _lib.PsgError("VAEDecoder (MI355X build) needs GPU tensors; there is no CPU fallback")
        if (self.live_weights() and torch.is_grad_enabled()) or _wants_grad(latent, text_emb):
            if not self.trainable:
                _require_frozen(self)
            return self._forward(latent, text_emb)
        with torch.no_grad():
            return self._forward(latent, text_emb)

    def live_weights(self) -> bool:
        """Whether a call with grad mode on differentiates with respect to the parameters: a `trainable` decoder whose
        parameters currently require grad.  Stage 3 freezes a trainable decoder for its text-encoder phase
        (`FinalPokemonGenerator.freeze_vae_decoder`): it is then a default decoder launch for launch - data gradients only, no
        weight-gradient launch, every prepared operand from `WeightCache` - until `unfreeze_vae_decoder` switches it back."""
        return self.trainable and any(p.requires_grad for p in self.parameters())

    def _image_conv(self, grad):
        """(w, b) of the image convolution: its 3 channels computed in 4 output columns (zero rows of weight), or in 8 when a
        gradient is wanted - the data gradient gathers 16-byte chunks of dY; `image_out` reads the width off the result.  The padded fp32 copies follow the
        parameters' WeightCache stamp; a `trainable` decoder's are differentiable and made from the live parameters on every
        call: the [8,32,3,3] / [8] gradients of the node come back as [3,32,3,3] / [3]."""
        conv = self.final_conv[2]
        width = 8 if grad else 4
        extra = (-conv.out_channels) % width
        live = grad and self.live_weights()
        pad = (lambda p: ops.pad_rows(p, extra)) if live else (
            lambda p: torch.nn.functional.pad(p.detach().float(), (0, 0) * (p.dim() - 1) + (0, extra)).contiguous())
        return [ops.WeightCache.derived(p, width, lambda: pad(p), fresh=live) for p in (conv.weight, conv.bias)]

    def _forward(self, latent, text_emb):
        """The blocks' `nhwc` are called directly: their own `forward`s guard the frozen entry."""
        dt = self.compute_dtype
        text = text_emb.to(device=latent.device, dtype=dt).contiguous()
        lat = ops.nchw_to_nhwc_grad(latent, dt) if _wants_grad(latent) else ops.nchw_to_nhwc(latent, dt)
        x = ops.conv2d(lat, self.latent_proj.weight, self.latent_proj.bias)
        for i in range(1, 6):
            x = getattr(self, f"block{i}_resnet1").nhwc(x)
            x = getattr(self, f"block{i}_attn").nhwc(x, text)
            x = getattr(self, f"block{i}_resnet2").nhwc(x)
            up = getattr(self, f"block{i}_upsample", None)
            if up is not None:
                size = up.size if up.size is not None else (int(x.shape[1] * up.scale_factor), int(x.shape[2] * up.scale_factor))
                x = ops.upsample_bilinear(x, size)
        gn, conv = self.final_conv[0], self.final_conv[2]
        x = ops.group_norm(x, gn.weight, gn.bias, gn.num_groups, gn.eps, silu=True)
        w, b = self._image_conv(torch.is_grad_enabled())
        y = ops.conv2d(x, w, b, act=ACT_TANH)
        return ops.image_out(y, conv.out_channels)  # d tanh rides the conv node's epilogue backward; the padding columns get zeros


class PokemonVAE(nn.Module):
    """vae_decoder.py:225-291."""

    def __init__(self, latent_dim: int = 8, text_dim: int = 256, compute_dtype: torch.dtype = torch.float32, trainable: bool = False):
        super().__init__()
        self.latent_dim, self.text_dim = latent_dim, text_dim
        self.trainable = bool(trainable)
        self.encoder = VAEEncoder(input_channels=3, latent_dim=latent_dim, compute_dtype=compute_dtype, trainable=self.trainable)
        self.decoder = VAEDecoder(latent_dim=latent_dim, text_dim=text_dim, output_channels=3, compute_dtype=compute_dtype,
                                  trainable=self.trainable)

    def forward(self, images: torch.Tensor, text_emb: torch.Tensor, mode: str = "train", eps: torch.Tensor = None) -> dict:
        """vae_decoder.py:236-269.  A `trainable` VAE called with grad mode on (stage 1, vae_trainer.py) returns
        `reconstructed`, `latent`, `mu`, `logvar` with a graph to the parameters of both halves; every other call runs under
        no_grad, as the frozen VAE always did.  `eps`: the encoder's reparameterisation noise (default: drawn)."""
        if self.trainable and torch.is_grad_enabled():
            return self._forward(images, text_emb, mode, eps)
        with torch.no_grad():
            return self._forward(images, text_emb, mode, eps)

    def _forward(self, images, text_emb, mode, eps):
        if mode == "sample" or images is None:
            latent = torch.randn(text_emb.size(0), self.latent_dim, 27, 27, device=text_emb.device)
            mu = logvar = None
        else:
            latent, mu, logvar = self.encoder(images, eps=eps)
            if mode == "generate":
                latent = mu
        return {"reconstructed": self.decoder(latent, text_emb), "latent": latent, "mu": mu, "logvar": logvar}

    def encode(self, images, eps: torch.Tensor = None):
        return self.encoder(images, eps=eps)

    def decode(self, latent, text_emb):
        return self.decoder(latent, text_emb)

    def sample(self, batch_size: int, text_emb: torch.Tensor, device: torch.device) -> torch.Tensor:
        return self.decoder(torch.randn(batch_size, self.latent_dim, 27, 27, device=device), text_emb)
