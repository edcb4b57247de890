"""Stage 3's text-image alignment loss on the MI355X kernels (reference: src/models/clip_loss.py; used by
final_trainer.py:469-473 as `clip_weight * CLIPLoss(reconstructed, descriptions)`).

`CLIPLoss` = -mean_b cos(image_embeds[b], text_embeds[b]) of a frozen CLIP (openai/clip-vit-base-patch32: ViT-B/32 and a causal
text transformer, quick-GELU, pre-LayerNorm blocks).  Same attribute name as the reference (`self.model`) and transformers'
`CLIPModel` state-dict keys under it, so a `CLIPModel.state_dict()` loads unchanged (`...embeddings.position_ids` buffers that
some transformers versions save are ignored).  transformers is needed by `from_pretrained` alone, on the host, with
`local_files_only=True`: nothing is ever fetched.

Data flow, in `compute_dtype`:

    image [B,3,H,H] fp32 in [-1, 1] --ops.clip_prep--> patch rows [B, 49, 3072]      ((x + 1) / 2, resize to 224, normalise)
      --ops.linear (patch embedding)--> [class ; patches] + positions --pre_layrnorm--> N x block --> post_layernorm(class row)
      --visual_projection--> image_embeds [B, 512]
    input_ids [B,S] --token + position rows--> N x block (ops.attention_causal) --> final_layer_norm --> EOS row
      --text_projection--> text_embeds [B, 512]                                       (always under no_grad: a constant)
    loss = ops.cosine_loss(image_embeds, text_embeds)                                 (fp32 device scalar)

    block(x): h = LN1(x); x = x + out_proj(attention(qkv(h))); h = LN2(x); x = x + fc2(quick_gelu(fc1(h)))
              ops.layer_norm, ops.qkv_linear, ops.attention_self | ops.attention_causal, ops.linear(residual= / act=)

The resize SPECIFICATION is the image processor's float path, F.interpolate(mode='bicubic', align_corners=False,
antialias=True) - not its PIL path, which goes through uint8, clips the overshoot and cannot take a batch that requires grad
(see psg_clip_prep_fwd).  Square images no larger than the model's image size only.  The token and class rows are torch indexing
on the device (plumbing: three small gathers).  All parameters are frozen: the nodes deliver data gradients only, and when the
image asks for none the whole call runs under no_grad.  `logit_scale` is a container only (the loss does not use it).
"""
import os

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import ACT_QUICK_GELU
from .ops import prepared as _prepared

VISION_KEYS = ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "image_size", "patch_size")
TEXT_KEYS = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "max_position_embeddings")
MASK_WORDS = ("[MASK]", "[NAME]")          # clip_loss.py:49
MAX_TEXT = 128                             # psg_attn_fwd_causal's limit (CLIP: 77 positions)


def clean_text(text):
    """clip_loss.py:47-49: the words [MASK] / [NAME] dropped from each description (split on single spaces, as the reference)."""
    return [" ".join(w for w in t.split(" ") if w not in MASK_WORDS) for t in text]


def config_dict(cfg):
    """A transformers CLIPConfig (or a dict with `vision_config`, `text_config`, `projection_dim`) -> the plain dict this class
    takes; rejects what the kernels do not compute."""
    get = (lambda o, k, d=None: o.get(k, d)) if isinstance(cfg, dict) else (lambda o, k, d=None: getattr(o, k, d))
    sub = (lambda o, k, d=None: o.get(k, d)) if isinstance(get(cfg, "vision_config"), dict) else (lambda o, k, d=None: getattr(o, k, d))
    out = {"projection_dim": int(get(cfg, "projection_dim"))}
    for name, keys in (("vision_config", VISION_KEYS), ("text_config", TEXT_KEYS)):
        src = get(cfg, name)
        d = {k: int(sub(src, k)) for k in keys}
        d["layer_norm_eps"] = float(sub(src, "layer_norm_eps", 1e-5))
        act = sub(src, "hidden_act", "quick_gelu")
        if act != "quick_gelu":
            raise _lib.PsgError(f"CLIPLoss computes CLIP with hidden_act='quick_gelu' (got {act!r} in {name})")
        if d["hidden_size"] % d["num_attention_heads"]:
            raise _lib.PsgError(f"{name}: hidden_size must be a multiple of num_attention_heads")
        out[name] = d
    eos = sub(get(cfg, "text_config"), "eos_token_id", 2)
    out["text_config"]["eos_token_id"] = 2 if eos is None else int(eos)
    v = out["vision_config"]
    if v["image_size"] % v["patch_size"]:
        raise _lib.PsgError("vision_config: image_size must be a multiple of patch_size")
    return out


# containers with transformers' attribute names (state-dict keys only; nothing here runs torch math)
class _Attention(nn.Module):
    def __init__(self, W):
        super().__init__()
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = nn.Linear(W, W), nn.Linear(W, W), nn.Linear(W, W), nn.Linear(W, W)


class _MLP(nn.Module):
    def __init__(self, W, I):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(W, I), nn.Linear(I, W)


class _Layer(nn.Module):
    def __init__(self, c):
        super().__init__()
        W = c["hidden_size"]
        self.self_attn = _Attention(W)
        self.layer_norm1 = nn.LayerNorm(W, eps=c["layer_norm_eps"])
        self.mlp = _MLP(W, c["intermediate_size"])
        self.layer_norm2 = nn.LayerNorm(W, eps=c["layer_norm_eps"])


class _Encoder(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(c) for _ in range(c["num_hidden_layers"])])


class _VisionEmbeddings(nn.Module):
    def __init__(self, c):
        super().__init__()
        W, P = c["hidden_size"], c["patch_size"]
        self.class_embedding = nn.Parameter(torch.randn(W))
        self.patch_embedding = nn.Conv2d(3, W, kernel_size=P, stride=P, bias=False)
        self.position_embedding = nn.Embedding((c["image_size"] // P) ** 2 + 1, W)


class _VisionModel(nn.Module):
    def __init__(self, c):
        super().__init__()
        W, eps = c["hidden_size"], c["layer_norm_eps"]
        self.embeddings = _VisionEmbeddings(c)
        self.pre_layrnorm = nn.LayerNorm(W, eps=eps)               # (transformers' own spelling)
        self.encoder = _Encoder(c)
        self.post_layernorm = nn.LayerNorm(W, eps=eps)


class _TextEmbeddings(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.token_embedding = nn.Embedding(c["vocab_size"], c["hidden_size"])
        self.position_embedding = nn.Embedding(c["max_position_embeddings"], c["hidden_size"])


class _TextModel(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.embeddings = _TextEmbeddings(c)
        self.encoder = _Encoder(c)
        self.final_layer_norm = nn.LayerNorm(c["hidden_size"], eps=c["layer_norm_eps"])


class _CLIP(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.config = c
        self.text_model = _TextModel(c["text_config"])
        self.vision_model = _VisionModel(c["vision_config"])
        self.visual_projection = nn.Linear(c["vision_config"]["hidden_size"], c["projection_dim"], bias=False)
        self.text_projection = nn.Linear(c["text_config"]["hidden_size"], c["projection_dim"], bias=False)
        self.logit_scale = nn.Parameter(torch.tensor(2.6592))


def _drop_position_ids(state_dict, prefix, *_):
    for k in [k for k in state_dict if k.startswith(prefix) and k.endswith("embeddings.position_ids")]:
        del state_dict[k]


class CLIPLoss(nn.Module):
    """-mean cosine similarity between CLIP's embeddings of `image` ([B,3,H,H] in [-1, 1]) and of the texts (clip_loss.py:12-69)."""

    def __init__(self, config, state_dict=None, tokenizer=None, compute_dtype: torch.dtype = torch.float32, device=None):
        super().__init__()
        self.compute_dtype = compute_dtype
        self.tokenizer = tokenizer
        self.model = _CLIP(config_dict(config))
        self._register_load_state_dict_pre_hook(_drop_position_ids)
        if state_dict is not None:
            self.load_state_dict(state_dict)
        for p in self.model.parameters():
            p.requires_grad = False
        self._cache = {}
        if device is not None:
            self.to(device)

    @classmethod
    def from_pretrained(cls, path_or_name="openai/clip-vit-base-patch32", tokenizer=None, compute_dtype=torch.float32, device=None,
                        load_tokenizer=True):
        """Configuration, weights and (when its files are there) the tokenizer of a CLIPModel directory or cached name - host
        side only, `local_files_only=True`."""
        from transformers import CLIPModel
        m = CLIPModel.from_pretrained(path_or_name, local_files_only=True)
        cfg = config_dict(m.config)
        sd = {"model." + k: v.detach().clone().float() for k, v in m.state_dict().items()}
        del m
        has_files = not os.path.isdir(path_or_name) or any(os.path.exists(os.path.join(path_or_name, f)) for f in ("vocab.json", "tokenizer.json"))
        if tokenizer is None and load_tokenizer and has_files:       # (a directory without tokenizer files: token ids only)
            from transformers import CLIPTokenizer
            tokenizer = CLIPTokenizer.from_pretrained(path_or_name, local_files_only=True)     # a broken one raises here
        return cls(cfg, state_dict=sd, tokenizer=tokenizer, compute_dtype=compute_dtype, device=device)

    # ---- the two towers -------------------------------------------------------------------------------------------
    def _block(self, x, lay, heads, key, causal, need_wd):
        """One pre-LN block on [B, L, W] (the reference's CLIPEncoderLayer) through the nodes of `ops`."""
        dt = self.compute_dtype
        B, L, W = x.shape
        sa, eps = lay.self_attn, lay.layer_norm1.eps
        ps = [sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight, sa.q_proj.bias, sa.k_proj.bias, sa.v_proj.bias]
        packed = _prepared(self._cache, (key, dt, need_wd), ps, lambda: ops.prep_qkv(*ps, dt, need_wd))
        h = ops.layer_norm(x, lay.layer_norm1.weight, lay.layer_norm1.bias, eps)
        qkv = ops.qkv_linear(h, ps[0], ps[3], ps[1], ps[4], ps[2], ps[5], packed)
        a = ops.attention_causal(qkv, heads) if causal else ops.attention_self(qkv, heads)
        x = ops.linear(a, sa.out_proj.weight, sa.out_proj.bias, residual=x)
        h = ops.layer_norm(x, lay.layer_norm2.weight, lay.layer_norm2.bias, eps)
        u = ops.linear(h, lay.mlp.fc1.weight, lay.mlp.fc1.bias, act=ACT_QUICK_GELU)
        return ops.linear(u, lay.mlp.fc2.weight, lay.mlp.fc2.bias, residual=x)

    def _image_embeds(self, image):
        c, vm, dt = self.model.config["vision_config"], self.model.vision_model, self.compute_dtype
        emb = vm.embeddings
        W, P, B = c["hidden_size"], c["patch_size"], image.shape[0]
        rows = ops.clip_prep(image, c["image_size"], P, 0.5, 0.5, dt)
        w2d = _prepared(self._cache, "patch2d", [emb.patch_embedding.weight], lambda: emb.patch_embedding.weight.detach().view(W, 3 * P * P))
        pos = emb.position_embedding.weight
        patches = (ops.linear(rows, w2d).float() + pos[1:]).to(dt)
        x = torch.cat([(emb.class_embedding + pos[0]).to(dt).expand(B, 1, W), patches], 1)
        x = ops.layer_norm(x, vm.pre_layrnorm.weight, vm.pre_layrnorm.bias, vm.pre_layrnorm.eps)
        for i, lay in enumerate(vm.encoder.layers):
            x = self._block(x, lay, c["num_attention_heads"], ("v", i), False, True)
        pooled = ops.layer_norm(x[:, 0, :], vm.post_layernorm.weight, vm.post_layernorm.bias, vm.post_layernorm.eps)
        return ops.linear(pooled, self.model.visual_projection.weight)

    def text_features(self, input_ids):
        """text_embeds [B, projection_dim] in compute_dtype (CLIPModel's, not normalised) of token ids [B, S]: the constant
        side of the loss, which a caller may compute once per caption batch and hand to `forward_features`."""
        c, tm, dt = self.model.config["text_config"], self.model.text_model, self.compute_dtype
        dev = self.model.text_projection.weight.device
        if dev.type != "cuda":
            raise _lib.PsgError("CLIPLoss (MI355X build) needs its parameters on a GPU; there is no CPU fallback")
        if input_ids.dim() != 2 or input_ids.dtype != torch.int64:
            raise _lib.PsgError(f"CLIPLoss: token ids must be an int64 [B, S] tensor, got {input_ids.dtype} {tuple(input_ids.shape)}")
        B, S = input_ids.shape
        if S > min(c["max_position_embeddings"], MAX_TEXT):
            raise _lib.PsgError(f"CLIPLoss: {S} tokens, more than {min(c['max_position_embeddings'], MAX_TEXT)} positions")
        ids = input_ids.to(dev)
        with torch.no_grad():
            emb = tm.embeddings
            x = (emb.token_embedding.weight[ids] + emb.position_embedding.weight[:S]).to(dt)
            for i, lay in enumerate(tm.encoder.layers):
                x = self._block(x, lay, c["num_attention_heads"], ("t", i), True, False)
            x = ops.layer_norm(x, tm.final_layer_norm.weight, tm.final_layer_norm.bias, tm.final_layer_norm.eps)
            # transformers' pooling: the highest id is EOS in the original vocabulary (eos_token_id == 2 is that legacy
            # configuration, the real checkpoint's); otherwise the first position that holds eos_token_id.  On the device.
            eos = c["eos_token_id"]
            at = ids.argmax(-1) if eos == 2 else (ids == eos).int().argmax(-1)
            pooled = x[torch.arange(B, device=dev), at]
            return ops.linear(pooled, self.model.text_projection.weight)

    def _check_image(self, image):
        if not image.is_cuda:
            raise _lib.PsgError("CLIPLoss (MI355X build) needs GPU tensors; there is no CPU fallback")
        if image.dim() != 4 or image.shape[1] != 3:
            raise _lib.PsgError(f"CLIPLoss: expected [B,3,H,W] images, got {tuple(image.shape)}")

    def forward_features(self, image, text_embeds):
        """The loss against text embeddings from `text_features` (a constant: no gradient reaches them)."""
        self._check_image(image)
        if text_embeds.shape[0] != image.shape[0]:
            raise _lib.PsgError(f"CLIPLoss: {image.shape[0]} images and {text_embeds.shape[0]} texts")
        if torch.is_grad_enabled() and image.requires_grad:
            return ops.cosine_loss(self._image_embeds(image), text_embeds.detach())
        with torch.no_grad():
            return ops.cosine_loss(self._image_embeds(image), text_embeds)

    def forward_ids(self, image, input_ids):
        self._check_image(image)
        return self.forward_features(image, self.text_features(input_ids))

    def tokenize(self, text):
        """Cleaned descriptions -> int64 [B, S] token ids through the caller's tokenizer (CLIPProcessor's text half:
        padding=True, truncation=True)."""
        if self.tokenizer is None:
            raise _lib.PsgError("CLIPLoss: no tokenizer was given - pass token ids, or construct with tokenizer=")
        enc = self.tokenizer(clean_text(text), return_tensors="pt", padding=True, truncation=True,
                             max_length=self.model.config["text_config"]["max_position_embeddings"])
        return enc["input_ids"].to(torch.int64)

    def forward(self, image, text):
        """image [B,3,H,H] in [-1, 1]; text: a list of B descriptions (needs the tokenizer) or an int64 [B, S] tensor of token ids."""
        self._check_image(image)
        if not torch.is_tensor(text):
            text = self.tokenize(list(text))
        return self.forward_ids(image, text)
