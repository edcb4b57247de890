"""VAE encoder / decoder on the MI355X kernels (reference: src/models/vae_decoder.py).

The VAE sits either side of the U-Net path: stage 2 encodes every image batch with the FROZEN encoder before the train
step (improved_diffusion_trainer.py:198-208,357-358) and decodes sampled latents for monitoring (:598); stage 3 and the
demo decode with it.  By default its parameters are never trained here (they are containers with the reference's names and
shapes, so `load_state_dict` takes a stage-1 checkpoint's 'vae_state_dict' halves unchanged), and the encoder runs under
`torch.no_grad()`.

What is trainable: the ENCODER, opt-in.  `VAEEncoder(..., trainable=True)` has parameters that require grad and, with grad mode
on, runs the autograd nodes of `ops`: `ops.conv4s2_relu` for the three 4x4 stride-2 convolutions (psg_conv4s2_dgrad /
psg_conv4s2_wgrad, csrc/conv4s2.hip), `ResNetBlock.nhwc_grad`, `ops.conv2d` for the mu / logvar projections and `ops.reparam`
for the sample - gradients reach all 70 of its parameters (stage 1, src/training/vae_trainer.py).  The DECODER, opt-in as
well: `VAEDecoder(..., trainable=True)` runs the same nodes with grad mode on and every one of its 144 parameters receives a
gradient - the convolutions' and the k / v Linears' through psg_conv_wgrad or, for the high-resolution layers of blocks 4 and 5
in bf16, psg_conv_wgrad_slim (`ops._deliver_gemm_grads`, `ops._wgrad_slim_route`), the GroupNorms' from psg_groupnorm_bwd_res; the 3-channel image convolution is computed in 8 output columns and its gradients come back at the
parameter's own [3,32,3,3] / [3] shapes (`ops.pad_rows`).  `PokemonVAE(..., trainable=True)` builds both halves trainable and
its `forward` carries the graph encoder -> latent -> decoder.  What is still missing: the stage-1 stepper (two learning
rates, two clip norms, KL annealing, the arena / FusedAdamW wiring for the VAE) and the joint phase of stage 3
(`FinalPokemonGenerator.unfreeze_vae_decoder` keeps raising).

A default DECODER is frozen (a parameter switched to requires_grad by hand raises, `_require_frozen`) but differentiable with
respect to its inputs: stage 3 trains the text encoder through it (final_trainer.py:215-236), so when grad mode is on and
`text_emb` or `latent` requires grad, `VAEDecoder.forward` runs the autograd nodes of `ops` (data gradients only; the
cross-attention backward is psg_attn_bwd_longq).  Every other call runs the inference launches, unchanged.

Same classes / constructor and forward signatures as the reference: `ResNetBlock`, `CrossAttentionBlock`, `VAEEncoder`,
`VAEDecoder`, `PokemonVAE`.  Everything runs channels-last in `compute_dtype` on the kernels of the U-Net path:
3x3 / 1x1 convolutions and the encoder's 4x4 stride-2 convolutions (psg_conv_fwd, fused bias / ReLU / Tanh / residual),
GroupNorm+SiLU, bilinear upsampling and the attention core.  Reference quirks kept, not fixed: the decoder's
cross-attention reshapes the [B, S, C] key / value projections straight to [B, heads, head_dim, S]
(vae_decoder.py:56-57 - a reinterpretation of memory, not a transpose), and the encoder returns a SAMPLED latent.
"""
import math

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import ACT_NONE, ACT_RELU, ACT_SILU, ACT_TANH, check, ptr, stream_ptr
from .ops import conv_infer as _conv, prep_weight as _prep, prepared as _prepared


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


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
        self._cache = {}

    def nhwc(self, x):
        dt = x.dtype
        cin, cout = self.conv1.in_channels, self.conv1.out_channels
        w1 = _prepared(self._cache, ("c1", dt), [self.conv1.weight], lambda: _prep(self.conv1.weight, dt))
        w2 = _prepared(self._cache, ("c2", dt), [self.conv2.weight], lambda: _prep(self.conv2.weight, dt))
        h = ops.group_norm(x, self.norm1.weight, self.norm1.bias, self.norm1.num_groups, self.norm1.eps, silu=True)
        h = _conv(h, w1, self.conv1.bias, cin, cout, 3, 1, 1)
        h = ops.group_norm(h, self.norm2.weight, self.norm2.bias, self.norm2.num_groups, self.norm2.eps, silu=True)
        if isinstance(self.shortcut, nn.Conv2d):
            ws = _prepared(self._cache, ("sc", dt), [self.shortcut.weight], lambda: _prep(self.shortcut.weight, dt))
            skip = _conv(x, ws, self.shortcut.bias, cin, cout, 1, 1, 0)
        else:
            skip = x
        return _conv(h, w2, self.conv2.bias, cout, cout, 3, 1, 1, residual=skip)

    def nhwc_grad(self, x):
        """`nhwc` on the autograd nodes of `ops`: data gradients, and the gradient of every parameter that requires one."""
        h, xs = ops.group_norm_split(x, self.norm1.weight, self.norm1.bias, self.norm1.num_groups, self.norm1.eps, silu=True)
        h = ops.conv2d(h, self.conv1.weight, self.conv1.bias)
        h = ops.group_norm(h, self.norm2.weight, self.norm2.bias, self.norm2.num_groups, self.norm2.eps, silu=True)
        skip = ops.conv2d(xs, self.shortcut.weight, self.shortcut.bias) if isinstance(self.shortcut, nn.Conv2d) else xs
        return ops.conv2d(h, self.conv2.weight, self.conv2.bias, residual=skip)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        dt = getattr(self, "compute_dtype", torch.float32)
        if _wants_grad(x):
            _require_frozen(self)
            return ops.nhwc_to_nchw(self.nhwc_grad(ops.nchw_to_nhwc_grad(x, dt)))
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
        self._cache = {}

    def nhwc(self, x, text):
        """x [B,H,W,C], text [B,S,text_dim] in the compute dtype."""
        dt = x.dtype
        B, H, W, C = x.shape
        S = text.shape[1]
        wq = _prepared(self._cache, ("q", dt), [self.q.weight], lambda: _prep(self.q.weight, dt))
        wp = _prepared(self._cache, ("p", dt), [self.proj.weight], lambda: _prep(self.proj.weight, dt))
        wk = _prepared(self._cache, ("k", dt), [self.k.weight], lambda: _prep(self.k.weight[:, :, None, None], dt))
        wv = _prepared(self._cache, ("v", dt), [self.v.weight], lambda: _prep(self.v.weight[:, :, None, None], dt))
        xn = ops.group_norm(x, self.norm.weight, self.norm.bias, self.norm.num_groups, self.norm.eps)
        q = _conv(xn, wq, self.q.bias, C, C, 1, 1, 0).reshape(B, H * W, C)
        t4 = text.reshape(B, S, 1, self.text_dim)
        k = _conv(t4, wk, self.k.bias, self.text_dim, C, 1, 1, 0).reshape(B, S, C)
        v = _conv(t4, wv, self.v.bias, self.text_dim, C, 1, 1, 0).reshape(B, S, C)
        # vae_decoder.py:56-57: `.reshape(b, heads, head_dim, -1)` of a [b, S, C] tensor reads its memory as [C][S]:
        # key token s' of channel c is element c*S + s' of the projection's buffer.  The attention kernel wants [S][C] rows.
        kv = torch.cat([k.reshape(B, C, S).transpose(1, 2), v.reshape(B, C, S).transpose(1, 2)], dim=-1).contiguous()
        o = ops.attention_cross(q, kv, self.num_heads)             # softmax(q^T k / sqrt(head_dim)) v, per head
        y = _conv(o.reshape(B, H, W, C), wp, self.proj.bias, C, C, 1, 1, 0, residual=x)
        return y

    def nhwc_grad(self, x, text):
        """`nhwc` on the autograd nodes of `ops`.  The [B,S,C] -> [C][S] reinterpretation is a reshape + transpose of views,
        differentiated by autograd as such; the attention core's backward is psg_attn_bwd_longq."""
        B, H, W, C = x.shape
        S = text.shape[1]
        xn, xs = ops.group_norm_split(x, self.norm.weight, self.norm.bias, self.norm.num_groups, self.norm.eps)
        q = ops.conv2d(xn, self.q.weight, self.q.bias).reshape(B, H * W, C)
        k = ops.linear(text, self.k.weight, self.k.bias)
        v = ops.linear(text, self.v.weight, self.v.bias)
        kv = torch.cat([k.reshape(B, C, S).transpose(1, 2), v.reshape(B, C, S).transpose(1, 2)], dim=-1).contiguous()
        o = ops.attention_cross_longq(q, kv, self.num_heads)
        return ops.conv2d(o.reshape(B, H, W, C), self.proj.weight, self.proj.bias, residual=xs)

    def forward(self, x: torch.Tensor, text_emb: torch.Tensor) -> torch.Tensor:
        dt = getattr(self, "compute_dtype", torch.float32)
        if _wants_grad(x, text_emb):
            _require_frozen(self)
            xin = ops.nchw_to_nhwc_grad(x, dt) if x.requires_grad else ops.nchw_to_nhwc(x, dt)
            return ops.nhwc_to_nchw(self.nhwc_grad(xin, text_emb.to(dt).contiguous()))
        with torch.no_grad():
            return ops.nhwc_to_nchw(self.nhwc(ops.nchw_to_nhwc(x, dt), text_emb.to(dt)))


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
        self._cache = {}
        self._epoch = ops.WeightCache.epoch
        for p in self.parameters():                  # frozen unless asked: gradients exist only on the trainable path
            p.requires_grad_(self.trainable)

    def forward(self, x: torch.Tensor, eps: torch.Tensor = None, generator: torch.Generator = None):
        """x [B,3,H,W] -> (latent, mu, logvar), each [B,latent_dim,h,w] fp32 (215 -> 27).  `eps` (default: randn of mu's
        shape, from `generator` when given - a data-parallel rank's own stream) is the reparameterisation noise the
        reference draws with randn_like (:121).  A `trainable` encoder called with grad mode on runs the autograd nodes of
        `ops` and its outputs carry gradients to all its parameters; every other call runs the inference launches."""
        if not x.is_cuda:
            raise _lib.PsgError("VAEEncoder (MI355X build) needs GPU tensors; there is no CPU fallback")
        if self.trainable and torch.is_grad_enabled():
            return self._forward_train(x, eps, generator)
        with torch.no_grad():
            return self._forward_infer(x, eps, generator)

    def _draw_eps(self, mu, eps, generator):
        if eps is None:
            eps = torch.randn_like(mu) if generator is None else torch.randn(mu.shape, dtype=mu.dtype, device=mu.device, generator=generator)
        return eps.detach().to(device=mu.device, dtype=torch.float32).contiguous()

    def _forward_train(self, x, eps, generator):
        """The encoder on the autograd nodes of `ops` (stage 1, vae_trainer.py): the three 4x4 stride-2 convolutions are
        `ops.conv4s2_relu` (own gradient kernels), everything else the nodes the decoder and the U-Net already use."""
        if x.requires_grad:
            raise _lib.PsgError("VAEEncoder: the image has requires_grad=True, but nothing differentiates with respect to the image "
                                "(the first convolution's data gradient is never computed); detach it")
        dt = self.compute_dtype
        Cin = x.shape[1]
        cpad = (-Cin) % 8
        h = ops.nchw_to_nhwc(x, dt, width=Cin + cpad)
        for i, m in enumerate(self.encoder):
            if isinstance(m, nn.Conv2d):
                h = ops.conv4s2_relu(h, m.weight, m.bias, m.padding[0], self._cache, (i, dt, "train"))
            elif isinstance(m, ResNetBlock):
                h = m.nhwc_grad(h)               # (called directly: ResNetBlock.forward guards its own, frozen, entry)
        mu = ops.nhwc_to_nchw(ops.conv2d(h, self.mu_proj.weight, self.mu_proj.bias))
        logvar = ops.nhwc_to_nchw(ops.conv2d(h, self.logvar_proj.weight, self.logvar_proj.bias))
        return ops.reparam(mu, logvar, self._draw_eps(mu, eps, generator)), mu, logvar

    def _forward_infer(self, x, eps, generator):
        if self.trainable and self._epoch != ops.WeightCache.epoch:
            # an optimizer wrote the parameters through raw pointers (WeightCache.invalidate): version counters did not move
            self._cache.clear()
            for m in self.encoder:
                if isinstance(m, ResNetBlock):
                    m._cache.clear()
            self._epoch = ops.WeightCache.epoch
        dt = self.compute_dtype
        Cin = x.shape[1]
        # image -> channels-last with the channel count padded to one 16-byte chunk (zeros; the weights are padded alike)
        cpad = (-Cin) % 8
        h = ops.nchw_to_nhwc(x, dt, width=Cin + cpad)
        for i, m in enumerate(self.encoder):
            if isinstance(m, nn.Conv2d):
                pin = cpad if i == 0 else 0
                wf = _prepared(self._cache, (i, dt), [m.weight], lambda m=m, pin=pin: _prep(m.weight, dt, pad_in=pin))
                h = _conv(h, wf, m.bias, m.in_channels + pin, m.out_channels, 4, 2, m.padding[0], act=ACT_RELU)   # Conv2d + the ReLU after it
            elif isinstance(m, ResNetBlock):
                h = m.nhwc(h)
        wm = _prepared(self._cache, ("mu", dt), [self.mu_proj.weight], lambda: _prep(self.mu_proj.weight, dt))
        wl = _prepared(self._cache, ("lv", dt), [self.logvar_proj.weight], lambda: _prep(self.logvar_proj.weight, dt))
        mu = ops.nhwc_to_nchw(_conv(h, wm, self.mu_proj.bias, 512, self.latent_dim, 3, 1, 1))
        logvar = ops.nhwc_to_nchw(_conv(h, wl, self.logvar_proj.bias, 512, self.latent_dim, 3, 1, 1))
        if eps is None:
            eps = torch.randn_like(mu) if generator is None else torch.randn(mu.shape, dtype=mu.dtype, device=mu.device, generator=generator)
        eps = eps.to(device=mu.device, dtype=torch.float32).contiguous()
        latent = torch.empty_like(mu)
        check(ops._lib_for(mu).psg_reparam_f32(ptr(mu), ptr(logvar), ptr(eps), ptr(latent), mu.numel(), stream_ptr()), "psg_reparam_f32")
        return latent, mu, logvar


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
        self._cache = {}
        self._epoch = ops.WeightCache.epoch
        self._fc_padded = None
        for p in self.parameters():                  # frozen unless asked: weight gradients exist only on the trainable path
            p.requires_grad_(self.trainable)

    def forward(self, latent: torch.Tensor, text_emb: torch.Tensor) -> torch.Tensor:
        """latent [B,latent_dim,h,w], text_emb [B,S,text_dim] -> image [B,3,215,215] fp32.  A `trainable` decoder called with
        grad mode on runs the autograd nodes of `ops` and its output carries gradients to all its parameters (and to `latent`
        / `text_emb` when they ask); a frozen one runs them when an input requires grad; every other call runs the inference
        launches."""
        if not latent.is_cuda:
            raise _lib.PsgError("VAEDecoder (MI355X build) needs GPU tensors; there is no CPU fallback")
        if (self.trainable and torch.is_grad_enabled()) or _wants_grad(latent, text_emb):
            return self._forward_grad(latent, text_emb)
        with torch.no_grad():
            return self._forward_infer(latent, text_emb)

    def _forward_grad(self, latent, text_emb):
        """The decoder on the autograd nodes of `ops`: gradients reach `text_emb` and `latent`, and - `trainable` only - every
        parameter (stage 1, vae_trainer.py).  The blocks' `nhwc_grad` are called directly: their own `forward`s guard the
        frozen entry."""
        if not self.trainable:
            _require_frozen(self)
        dt = self.compute_dtype
        text = text_emb.to(device=latent.device, dtype=dt).contiguous()
        lat = ops.nchw_to_nhwc_grad(latent, dt) if latent.requires_grad else ops.nchw_to_nhwc(latent, dt)
        x = ops.conv2d(lat, self.latent_proj.weight, self.latent_proj.bias)
        for i in range(1, 6):
            x = getattr(self, f"block{i}_resnet1").nhwc_grad(x)
            x = getattr(self, f"block{i}_attn").nhwc_grad(x, text)
            x = getattr(self, f"block{i}_resnet2").nhwc_grad(x)
            up = getattr(self, f"block{i}_upsample", None)
            if up is not None:
                size = up.size if up.size is not None else (int(x.shape[1] * up.scale_factor), int(x.shape[2] * up.scale_factor))
                x = ops.upsample_bilinear(x, size)
        gn, conv = self.final_conv[0], self.final_conv[2]
        x = ops.group_norm(x, gn.weight, gn.bias, gn.num_groups, gn.eps, silu=True)
        cout = conv.out_channels
        opad = (-cout) % 8          # 3 image channels in 8 columns (zero rows of weight): the data gradient gathers 16-byte chunks of dY
        if self.trainable:
            # Padded from the live parameters on every call - so an update of either kind (version counter, or raw pointers +
            # WeightCache.invalidate) is always seen - and differentiable: the [8,32,3,3] / [8] gradients of the node come
            # back as [3,32,3,3] / [3].  The previous call's padded weight leaves the WeightCache with it.
            if self._fc_padded is not None:
                ops.WeightCache.drop([self._fc_padded])
            w8, b8 = ops.pad_rows(conv.weight, opad), ops.pad_rows(conv.bias, opad)
            self._fc_padded = w8
        else:
            w8, b8 = _prepared(self._cache, ("fc_grad",), [conv.weight, conv.bias],
                               lambda: (torch.nn.functional.pad(conv.weight.detach().float(), (0, 0, 0, 0, 0, 0, 0, opad)).contiguous(),
                                        torch.nn.functional.pad(conv.bias.detach().float(), (0, opad)).contiguous()))
        y = ops.conv2d(x, w8, b8, act=ACT_TANH)
        return ops.image_out(y, cout)               # d tanh rides the conv node's epilogue backward; the padding columns get zeros

    def _forward_infer(self, latent, text_emb):
        if self.trainable and self._epoch != ops.WeightCache.epoch:
            # an optimizer wrote the parameters through raw pointers (WeightCache.invalidate): version counters did not move
            self._cache.clear()
            for m in self.modules():
                if isinstance(m, (ResNetBlock, CrossAttentionBlock)):
                    m._cache.clear()
            self._epoch = ops.WeightCache.epoch
        dt = self.compute_dtype
        text = text_emb.detach().to(device=latent.device, dtype=dt).contiguous()
        wl = _prepared(self._cache, ("lp", dt), [self.latent_proj.weight], lambda: _prep(self.latent_proj.weight, dt))
        x = _conv(ops.nchw_to_nhwc(latent, dt), wl, self.latent_proj.bias, self.latent_dim, 512, 3, 1, 1)
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
        cout = conv.out_channels
        opad = (-cout) % 4                                           # 3 image channels -> 4 output columns (zero rows of weight)
        wf = _prepared(self._cache, ("fc", dt), [conv.weight, conv.bias],
                       lambda: (_prep(conv.weight, dt, pad_out=opad), torch.nn.functional.pad(conv.bias.detach().float(), (0, opad)).contiguous()))
        y = _conv(x, wf[0], wf[1], conv.in_channels, cout + opad, 3, 1, 1, act=ACT_TANH)
        return ops.nhwc_rows_to_nchw(y, cout + opad, cout)


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

    def encode(self, images):
        return self.encoder(images)

    def decode(self, latent, text_emb):
        return self.decoder(latent, text_emb)

    def sample(self, batch_size: int, text_emb: torch.Tensor, device: torch.device) -> torch.Tensor:
        return self.decoder(torch.randn(batch_size, self.latent_dim, 27, 27, device=device), text_emb)
