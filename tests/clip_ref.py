"""fp64 restatement of the stage-3 CLIP loss (reference: src/models/clip_loss.py = transformers' CLIPProcessor + CLIPModel),
generated weights and inputs, the case tables and the recorded precision baseline for the CLIP tests (test infrastructure, not
a conftest; the style of tests/vgg_ref.py).

`prep`, `block`, `vision`, `text`, `loss` restate the reference on plain torch functions in ANY dtype: in float64 they are the
reference every test compares against; in float32 / bfloat16 on the CPU they are the yardstick - BASELINE_ERR records their
error against float64 per case (tests/test_clip_ref_cpu.py re-measures and asserts the table) and the GPU tests allow the
kernels four times that (`bar`), floored at 1e-6.  The state dicts carry transformers' CLIPModel keys.

The resize is the image processor's float path, F.interpolate(mode='bicubic', align_corners=False, antialias=True), restated as
one dense matrix per axis (`resize_matrix`); tests/test_clip_ref_cpu.py holds it against F.interpolate in float64.  The three
keyword arguments `cubic_a`, `causal`, `act` exist so the CPU test can plant a defect and see the comparator reject it.

The last section holds what the element-wise tests of the four kernels need (cases: tests/clip_cases.py): fp64 references with
the magnitude each bound scales with, the constants of the bounds, and fp32 evaluations in the order the header describes.
"""
import functools
import math
import types

import numpy as np
import torch
import torch.nn.functional as F

from oracle import hashgen
from tests.gemm_ref import BF16_ROUND, F32_ROUND, c_acc

SEED = 3207
MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
PRECISIONS = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _cfg(pd, v, t):
    vk = ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "image_size", "patch_size")
    tk = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "max_position_embeddings", "eos_token_id")
    return dict(projection_dim=pd, vision_config=dict(zip(vk, v), layer_norm_eps=1e-5, hidden_act="quick_gelu"),
                text_config=dict(zip(tk, t), layer_norm_eps=1e-5, hidden_act="quick_gelu"))


# name -> CLIP configuration.  tiny: 17 vision tokens, text sequences of 8 in 16 positions; real1: every launch shape of
# ViT-B/32 and its text tower once (one layer each, vocabulary cut to 1000); hook: the 215-pixel images of stage 3 on a narrow
# tower; eos: the second EOS-pooling rule (eos_token_id != 2: the first position that holds it)
CONFIGS = {
    "tiny": _cfg(32, (64, 128, 2, 2, 64, 16), (64, 32, 64, 2, 2, 16, 2)),
    "real1": _cfg(512, (768, 3072, 1, 12, 224, 32), (1000, 512, 2048, 1, 8, 77, 2)),
    "hook": _cfg(32, (64, 128, 1, 2, 224, 32), (64, 32, 64, 1, 2, 16, 2)),
    "eos": _cfg(32, (64, 128, 1, 2, 64, 16), (64, 32, 64, 1, 2, 16, 40)),
}
# loss cases: name -> (config, batch, input image side, text length)
LOSS_CASES = {"tiny": ("tiny", 2, 57, 8), "real1": ("real1", 2, 215, 12)}
PREP_CASES = ((13, 16, 8), (7, 16, 8), (16, 16, 8), (215, 224, 32))          # (Hi, S, P)
PREP_BATCHES = (1, 2)
CAUSAL_CASES = tuple((L, d) for L in (1, 8, 17, 77) for d in (16, 64))       # 2 heads, B = 2
COSINE_CASES = ((1, 32, "none"), (3, 512, "none"), (3, 512, "u"), (3, 512, "v"))   # (B, D, which operand has a zero row 1)
QGELU_SHAPE = (17, 64, 128)                                                   # rows, Cin, Cout

# Error of the torch CPU computation in a precision against float64: key -> {quantity: error}.  Scalars by relative error,
# tensors by rel-L2 (the cosine gradient: the worst row's rel-L2 - a zero row of u has a gradient of 1e12).  Filled from
# `measure` on 4 threads; tests/test_clip_ref_cpu.py asserts that a re-measurement gives every value within 25 %.  The bars of
# the GPU tests are derived from here alone.
BASELINE_ERR = {
    ('prep', 13, 16, 8, 1, 'fp32'): dict(fwd=1.252e-07, bwd=6.803e-08),
    ('prep', 13, 16, 8, 1, 'bf16'): dict(fwd=8.326e-03, bwd=4.354e-03),
    ('prep', 13, 16, 8, 2, 'fp32'): dict(fwd=1.265e-07, bwd=6.945e-08),
    ('prep', 13, 16, 8, 2, 'bf16'): dict(fwd=8.493e-03, bwd=4.419e-03),
    ('prep', 7, 16, 8, 1, 'fp32'): dict(fwd=1.420e-07, bwd=9.548e-08),
    ('prep', 7, 16, 8, 1, 'bf16'): dict(fwd=7.645e-03, bwd=4.073e-03),
    ('prep', 7, 16, 8, 2, 'fp32'): dict(fwd=1.436e-07, bwd=8.788e-08),
    ('prep', 7, 16, 8, 2, 'bf16'): dict(fwd=8.184e-03, bwd=4.445e-03),
    ('prep', 16, 16, 8, 1, 'fp32'): dict(fwd=7.105e-08, bwd=4.318e-08),
    ('prep', 16, 16, 8, 1, 'bf16'): dict(fwd=5.903e-03, bwd=2.747e-03),
    ('prep', 16, 16, 8, 2, 'fp32'): dict(fwd=7.177e-08, bwd=4.340e-08),
    ('prep', 16, 16, 8, 2, 'bf16'): dict(fwd=5.833e-03, bwd=2.701e-03),
    ('prep', 215, 224, 32, 1, 'fp32'): dict(fwd=1.408e-07, bwd=7.624e-08),
    ('prep', 215, 224, 32, 1, 'bf16'): dict(fwd=8.109e-03, bwd=4.089e-03),
    ('prep', 215, 224, 32, 2, 'fp32'): dict(fwd=1.409e-07, bwd=7.627e-08),
    ('prep', 215, 224, 32, 2, 'bf16'): dict(fwd=8.120e-03, bwd=4.089e-03),
    ('causal', 1, 16, 'fp32'): dict(out=0.000e+00),
    ('causal', 1, 16, 'bf16'): dict(out=0.000e+00),
    ('causal', 1, 64, 'fp32'): dict(out=0.000e+00),
    ('causal', 1, 64, 'bf16'): dict(out=0.000e+00),
    ('causal', 8, 16, 'fp32'): dict(out=4.860e-08),
    ('causal', 8, 16, 'bf16'): dict(out=1.508e-03),
    ('causal', 8, 64, 'fp32'): dict(out=5.704e-08),
    ('causal', 8, 64, 'bf16'): dict(out=1.635e-03),
    ('causal', 17, 16, 'fp32'): dict(out=7.344e-08),
    ('causal', 17, 16, 'bf16'): dict(out=1.754e-03),
    ('causal', 17, 64, 'fp32'): dict(out=7.573e-08),
    ('causal', 17, 64, 'bf16'): dict(out=1.680e-03),
    ('causal', 77, 16, 'fp32'): dict(out=1.015e-07),
    ('causal', 77, 16, 'bf16'): dict(out=1.904e-03),
    ('causal', 77, 64, 'fp32'): dict(out=1.062e-07),
    ('causal', 77, 64, 'bf16'): dict(out=1.912e-03),
    ('cosine', 1, 32, 'none', 'fp32'): dict(loss=4.474e-08, du=6.720e-08),
    ('cosine', 1, 32, 'none', 'bf16'): dict(loss=2.332e-03, du=3.328e-03),
    ('cosine', 3, 512, 'none', 'fp32'): dict(loss=1.037e-07, du=1.457e-07),
    ('cosine', 3, 512, 'none', 'bf16'): dict(loss=4.301e-03, du=8.223e-03),
    ('cosine', 3, 512, 'u', 'fp32'): dict(loss=1.033e-07, du=1.457e-07),
    ('cosine', 3, 512, 'u', 'bf16'): dict(loss=1.325e-03, du=8.223e-03),
    ('cosine', 3, 512, 'v', 'fp32'): dict(loss=1.033e-07, du=1.457e-07),
    ('cosine', 3, 512, 'v', 'bf16'): dict(loss=1.325e-03, du=8.223e-03),
    ('qgelu', 'fp32'): dict(fwd=6.044e-08, dx=2.276e-07, dw=9.765e-08, db=8.530e-08),
    ('qgelu', 'bf16'): dict(fwd=2.753e-03, dx=3.256e-03, dw=3.212e-03, db=3.035e-03),
    ('loss', 'tiny', 'fp32'): dict(loss=1.420e-07, grad=2.744e-06),
    ('loss', 'tiny', 'bf16'): dict(loss=4.205e-03, grad=5.419e-02),
    ('loss', 'real1', 'fp32'): dict(loss=1.196e-07, grad=1.727e-06),
    ('loss', 'real1', 'bf16'): dict(loss=4.547e-04, grad=2.834e-02),
}
BAR_FACTOR, BAR_FLOOR = 4.0, 1e-6


def bar(key, what):
    """The GPU tests' bound for a quantity: four times the torch CPU error in the same precision, floored at 1e-6."""
    return max(BAR_FACTOR * BASELINE_ERR[key][what], BAR_FLOOR)


def bf16_exact(t):
    return t.to(torch.bfloat16).to(torch.float32)


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm())


def rel_rows(got, ref):
    """The worst row's rel-L2; a row whose reference is exactly zero must be exactly zero."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    worst = 0.0
    for g, r in zip(got, ref):
        n = float(r.norm())
        worst = max(worst, float((g - r).norm()) / n if n > 0 else (0.0 if float(g.abs().max()) == 0.0 else math.inf))
    return worst


def u(shape, name, scale=1.0):
    return hashgen.uniform(tuple(shape), SEED, hashgen.name_id(name)) * scale


# ---------------------------------------------------------------------------------------------------------------
# generated weights and inputs
# ---------------------------------------------------------------------------------------------------------------
def state_shapes(cfg):
    """{key: shape} of transformers' CLIPModel(cfg).state_dict(), in its order (without the position_ids buffers)."""
    v, t, pd = cfg["vision_config"], cfg["text_config"], cfg["projection_dim"]
    out = {"logit_scale": ()}

    def tower(p, c):
        W, I = c["hidden_size"], c["intermediate_size"]
        for i in range(c["num_hidden_layers"]):
            q = f"{p}.encoder.layers.{i}."
            for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
                out[q + f"self_attn.{n}.weight"], out[q + f"self_attn.{n}.bias"] = (W, W), (W,)
            out[q + "layer_norm1.weight"], out[q + "layer_norm1.bias"] = (W,), (W,)
            out[q + "mlp.fc1.weight"], out[q + "mlp.fc1.bias"] = (I, W), (I,)
            out[q + "mlp.fc2.weight"], out[q + "mlp.fc2.bias"] = (W, I), (W,)
            out[q + "layer_norm2.weight"], out[q + "layer_norm2.bias"] = (W,), (W,)

    Wt, Wv, P = t["hidden_size"], v["hidden_size"], v["patch_size"]
    out["text_model.embeddings.token_embedding.weight"] = (t["vocab_size"], Wt)
    out["text_model.embeddings.position_embedding.weight"] = (t["max_position_embeddings"], Wt)
    tower("text_model", t)
    out["text_model.final_layer_norm.weight"], out["text_model.final_layer_norm.bias"] = (Wt,), (Wt,)
    out["vision_model.embeddings.class_embedding"] = (Wv,)
    out["vision_model.embeddings.patch_embedding.weight"] = (Wv, 3, P, P)
    out["vision_model.embeddings.position_embedding.weight"] = ((v["image_size"] // P) ** 2 + 1, Wv)
    out["vision_model.pre_layrnorm.weight"], out["vision_model.pre_layrnorm.bias"] = (Wv,), (Wv,)
    tower("vision_model", v)
    out["vision_model.post_layernorm.weight"], out["vision_model.post_layernorm.bias"] = (Wv,), (Wv,)
    out["visual_projection.weight"], out["text_projection.weight"] = (pd, Wv), (pd, Wt)
    return out


@functools.lru_cache(maxsize=None)
def state_dict(name):
    """Generated CLIPModel weights of CONFIGS[name], all bf16-representable (a bf16 launch then reads exactly these values):
    matrices with variance 1 / fan_in, biases in +-0.1, LayerNorm weights 1 +- 0.2, embeddings +-0.5.  Tensors of more than
    65536 values (real1) come from torch's seeded CPU generator: the hash generator would take seconds for 13 M values."""
    sd = {}
    for k, shape in state_shapes(CONFIGS[name]).items():
        n = math.prod(shape)
        if n > 65536:
            x = torch.rand(shape, generator=torch.Generator().manual_seed(SEED + hashgen.name_id(k) % 100000)) * 2.0 - 1.0
        else:
            x = u(shape, f"{name}.{k}") if shape else torch.tensor(0.0)
        if k == "logit_scale":
            x = torch.tensor(2.6592)
        elif k.endswith("norm.weight") or k.endswith("norm1.weight") or k.endswith("norm2.weight"):
            x = 1.0 + 0.2 * x
        elif k.endswith(".bias"):
            x = 0.1 * x
        elif "embedding" in k and "patch" not in k:
            x = 0.5 * x
        else:
            x = x * math.sqrt(3.0 / math.prod(shape[1:]))
        sd[k] = bf16_exact(x)
    return sd


def token_ids(name, B, S):
    """int64 [B, S]: ordinary ids in [3, vocab - 2] (never the EOS), then the EOS (the highest id, or the config's eos_token_id
    when that is not 2) at another place in every sample, then padding: EOS again in even samples (CLIP's tokenizer pads with it), 0 in odd."""
    t = CONFIGS[name]["text_config"]
    V, eos = t["vocab_size"], t["eos_token_id"]
    top = V - 1 if eos == 2 else eos
    ids = hashgen.randint((B, S), SEED, hashgen.name_id(f"{name}.ids"), 3, V - 1)
    if eos != 2:
        ids[ids == eos] = eos + 1                # ordinary ids lie on both sides of this EOS: the two pooling rules disagree
    for b in range(B):
        e = max(1, S - 1 - 3 * b)
        ids[b, e] = top
        ids[b, e + 1:] = top if b % 2 == 0 else 0
    return ids


def image(name, B, H):
    """fp32 [B,3,H,H] in about [-1.2, 1.2]: nothing clamps, so values outside [-1, 1] must pass through."""
    return u((B, 3, H, H), f"{name}.image") * 1.2


# ---------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------
def keys_cubic(x, a):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


@functools.lru_cache(maxsize=None)
def resize_matrix(n_in, n_out, a=-0.5):
    """float64 [n_out, n_in]: antialiased bicubic up-scaling of one axis (ATen's _compute_indices_min_size_weights_aa for
    scale = n_in / n_out <= 1): Keys cubic at (sample + 0.5 - centre), centre = scale (o + 0.5), over
    [trunc(centre - 1.5), trunc(centre + 2.5)) clipped to the axis, renormalised."""
    assert n_in <= n_out
    scale = n_in / n_out
    M = torch.zeros(n_out, n_in, dtype=torch.float64)
    for o in range(n_out):
        c = scale * (o + 0.5)
        lo, hi = max(int(c - 1.5), 0), min(int(c + 2.5), n_in)
        w = [keys_cubic(j + 0.5 - c, a) for j in range(lo, hi)]
        tot = sum(w)
        M[o, lo:hi] = torch.tensor([x / tot for x in w], dtype=torch.float64)
    return M


def prep(img, S, dtype=torch.float64, cubic_a=-0.5):
    """clip_loss.py:52 + CLIPImageProcessor (do_rescale=False): (img + 1) / 2, resize to S x S, normalise -> pixel_values."""
    v = 0.5 * img.to(dtype) + 0.5
    H = v.shape[-1]
    if H != S:
        M = resize_matrix(H, S, cubic_a).to(dtype)
        v = torch.einsum("oh,bchw,pw->bcop", M, v, M)
    cast = (lambda c: torch.tensor(c, dtype=torch.float64)) if dtype == torch.float64 else (lambda c: torch.tensor(c, dtype=torch.float32).to(dtype))
    return (v - cast(MEAN).view(1, 3, 1, 1)) / cast(STD).view(1, 3, 1, 1)


def patch_rows(pixel_values, P):
    """[B,3,S,S] -> [B, (S/P)^2, 3 P P]: the rows the patch embedding's flattened Conv2d weight multiplies (F.unfold's order)."""
    return F.unfold(pixel_values, P, stride=P).transpose(1, 2)


def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def block(x, sd, p, heads, eps, causal, act="quick_gelu"):
    """CLIPEncoderLayer: pre-LN attention and MLP, both with a residual."""
    B, L, W = x.shape
    d = W // heads
    lin = lambda t, n: F.linear(t, sd[p + n + ".weight"].to(x.dtype), sd[p + n + ".bias"].to(x.dtype))
    ln = lambda t, n: F.layer_norm(t, (W,), sd[p + n + ".weight"].to(x.dtype), sd[p + n + ".bias"].to(x.dtype), eps)
    split = lambda t: t.view(B, L, heads, d).transpose(1, 2)
    h = ln(x, "layer_norm1")
    q, k, v = split(lin(h, "self_attn.q_proj")), split(lin(h, "self_attn.k_proj")), split(lin(h, "self_attn.v_proj"))
    s = (q * d ** -0.5) @ k.transpose(-1, -2)
    if causal:
        s = s.masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), float("-inf"))
    x = x + lin((torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, L, W), "self_attn.out_proj")
    h = lin(ln(x, "layer_norm2"), "mlp.fc1")
    return x + lin(quick_gelu(h) if act == "quick_gelu" else F.gelu(h), "mlp.fc2")


def vision(pixel_values, sd, cfg, act="quick_gelu"):
    """CLIPModel.get_image_features: image_embeds [B, projection_dim] of pixel_values [B,3,S,S] (in their dtype)."""
    c, dt = cfg["vision_config"], pixel_values.dtype
    W, P, eps, e = c["hidden_size"], c["patch_size"], c["layer_norm_eps"], "vision_model.embeddings."
    B = pixel_values.shape[0]
    x = patch_rows(pixel_values, P) @ sd[e + "patch_embedding.weight"].to(dt).reshape(W, -1).t()
    x = torch.cat([sd[e + "class_embedding"].to(dt).expand(B, 1, W), x], 1) + sd[e + "position_embedding.weight"].to(dt)
    ln = lambda t, n: F.layer_norm(t, (W,), sd[f"vision_model.{n}.weight"].to(dt), sd[f"vision_model.{n}.bias"].to(dt), eps)
    x = ln(x, "pre_layrnorm")
    for i in range(c["num_hidden_layers"]):
        x = block(x, sd, f"vision_model.encoder.layers.{i}.", c["num_attention_heads"], eps, False, act)
    return F.linear(ln(x[:, 0], "post_layernorm"), sd["visual_projection.weight"].to(dt))


def eos_index(ids, eos_token_id):
    """transformers' pooling position: argmax of the ids when eos_token_id == 2, else the first position equal to it."""
    return ids.argmax(-1) if eos_token_id == 2 else (ids == eos_token_id).int().argmax(-1)


def text(ids, sd, cfg, dtype=torch.float64, causal=True, act="quick_gelu", key_mask=None):
    """CLIPModel.get_text_features: text_embeds [B, projection_dim].  `key_mask` (bool [B,S], True = attend) restates the
    processor's padding mask, only to show that it cannot change the result."""
    return _text(ids, sd, cfg, dtype, causal, act, key_mask, sd["text_projection.weight"])


def _text(ids, sd, cfg, dtype, causal, act, key_mask, projection):
    """`text`; projection None: the pooled EOS row in front of text_projection."""
    c = cfg["text_config"]
    W, eps, e = c["hidden_size"], c["layer_norm_eps"], "text_model.embeddings."
    B, S = ids.shape
    x = sd[e + "token_embedding.weight"].to(dtype)[ids] + sd[e + "position_embedding.weight"].to(dtype)[:S]
    for i in range(c["num_hidden_layers"]):
        p = f"text_model.encoder.layers.{i}."
        if key_mask is None:
            x = block(x, sd, p, c["num_attention_heads"], eps, causal, act)
        else:
            x = _block_masked(x, sd, p, c["num_attention_heads"], eps, key_mask)
    x = F.layer_norm(x, (W,), sd["text_model.final_layer_norm.weight"].to(dtype), sd["text_model.final_layer_norm.bias"].to(dtype), eps)
    pooled = x[torch.arange(B), eos_index(ids, c["eos_token_id"])]
    return pooled if projection is None else F.linear(pooled, projection.to(dtype))


def _block_masked(x, sd, p, heads, eps, key_mask):
    """`block` with the causal mask AND a key-padding mask (keys where key_mask is False take no part)."""
    B, L, W = x.shape
    d = W // heads
    lin = lambda t, n: F.linear(t, sd[p + n + ".weight"].to(x.dtype), sd[p + n + ".bias"].to(x.dtype))
    ln = lambda t, n: F.layer_norm(t, (W,), sd[p + n + ".weight"].to(x.dtype), sd[p + n + ".bias"].to(x.dtype), eps)
    split = lambda t: t.view(B, L, heads, d).transpose(1, 2)
    h = ln(x, "layer_norm1")
    q, k, v = split(lin(h, "self_attn.q_proj")), split(lin(h, "self_attn.k_proj")), split(lin(h, "self_attn.v_proj"))
    s = (q * d ** -0.5) @ k.transpose(-1, -2)
    dead = torch.ones(L, L, dtype=torch.bool).triu(1)[None, None] | ~key_mask[:, None, None, :]
    x = x + lin((torch.softmax(s.masked_fill(dead, float("-inf")), -1) @ v).transpose(1, 2).reshape(B, L, W), "self_attn.out_proj")
    return x + lin(quick_gelu(lin(ln(x, "layer_norm2"), "mlp.fc1")), "mlp.fc2")


def loss_inputs(case):
    """(image, token ids) of a loss case."""
    name, B, H, S = LOSS_CASES[case]
    return image(case, B, H), token_ids(name, B, S)


@functools.lru_cache(maxsize=None)
def loss_state_dict(case):
    """state_dict(config) of a loss case with ONE tensor rebuilt, text_projection, so that the case's own texts and images
    agree as a trained CLIP's do: W = 0.5 W0 + IE^T (T T^T)^-1 T with IE the float64 image embeddings [B, pd] of the case's
    images and T the pooled text rows [B, width], so W t_b = 0.5 W0 t_b + ie_b.  With generated weights alone the two
    embeddings are unrelated, the cosines scatter around 0 and the loss (-0.003, 0.017) is what their cancellation leaves:
    its relative error then measures the cancellation.  Here the loss is of order -0.5 ... -0.9 and its relative error
    measures the arithmetic.  Rounded to bf16 like every generated weight."""
    name, B, H, S = LOSS_CASES[case]
    cfg, sd = CONFIGS[name], dict(state_dict(name))
    img, ids = loss_inputs(case)
    with torch.no_grad():
        ie = vision(prep(img, cfg["vision_config"]["image_size"]), sd, cfg)
        t = _text(ids, sd, cfg, torch.float64, True, "quick_gelu", None, None)
        w = 0.5 * sd["text_projection.weight"].double() + ie.t() @ torch.linalg.solve(t @ t.t(), t)
    sd["text_projection.weight"] = bf16_exact(w.float())
    return sd


def cosine(ie, te):
    """clip_loss.py:60-67."""
    return -(F.normalize(ie, dim=-1) * F.normalize(te, dim=-1)).sum(-1).mean()


def loss(img, ids, sd, cfg, dtype=torch.float64, cubic_a=-0.5, causal=True, act="quick_gelu"):
    """CLIPLoss.forward(img, ids) in `dtype` on the CPU: (loss, d loss / d img) as float64 tensors.  The gradient is taken at
    the fp32 image (float64 for the float64 restatement, whose gradient is not rounded)."""
    g = img.detach().to(torch.float64 if dtype == torch.float64 else torch.float32).clone().requires_grad_(True)
    ie = vision(prep(g, cfg["vision_config"]["image_size"], dtype, cubic_a), sd, cfg, act)
    with torch.no_grad():
        te = text(ids, sd, cfg, dtype, causal, act)
    out = cosine(ie, te)
    out.backward()
    return out.detach().double(), g.grad.double()


# ---------------------------------------------------------------------------------------------------------------
# kernel-level cases: inputs and the torch computation in a dtype
# ---------------------------------------------------------------------------------------------------------------
def prep_inputs(Hi, S, P, B):
    G = S // P
    return image(f"prep.{Hi}.{S}", B, Hi), bf16_exact(u((B, G * G, 3 * P * P), f"prep.dy.{Hi}.{S}.{B}"))


def prep_torch(img, dy, S, P, dtype):
    """(patch rows, d sum(rows * dy) / d img) in `dtype`; the gradient at the fp32 (float64) image."""
    g = img.detach().to(torch.float64 if dtype == torch.float64 else torch.float32).clone().requires_grad_(True)
    rows = patch_rows(prep(g, S, dtype), P)
    (rows * dy.to(dtype)).sum().backward()
    return rows.detach(), g.grad


def causal_inputs(L, d, B=2, heads=2):
    return bf16_exact(u((B, L, 3 * heads * d), f"causal.{L}.{d}") * 1.5)


def causal_torch(qkv, heads, dtype):
    B, L, E3 = qkv.shape
    E = E3 // 3
    q, k, v = (t.view(B, L, heads, E // heads).transpose(1, 2) for t in qkv.to(dtype).split(E, -1))
    return F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(B, L, E)


def cosine_inputs(B, D, zero):
    v = u((B, D), f"cos.v.{B}.{D}")
    x = bf16_exact(0.6 * v + 0.8 * u((B, D), f"cos.u.{B}.{D}"))
    v = bf16_exact(v)
    if zero == "u":
        x[1] = 0.0
    if zero == "v":
        v[1] = 0.0
    return x, v


def cosine_torch(x, v, dtype):
    g = x.to(dtype).clone().requires_grad_(True)
    out = cosine(g, v.to(dtype))
    out.backward()
    return out.detach(), g.grad


def qgelu_inputs():
    M, I, O = QGELU_SHAPE
    return (bf16_exact(u((M, I), "qg.x") * 2.0), bf16_exact(u((O, I), "qg.w") * math.sqrt(3.0 / I)), bf16_exact(u((O,), "qg.b") * 0.5),
            bf16_exact(u((M, O), "qg.dy")))


def qgelu_torch(x, w, b, dy, dtype):
    """y = quick_gelu(x w^T + b) and the gradients of sum(y * dy): dict(fwd, dx, dw, db)."""
    xs, ws, bs = (t.to(dtype).clone().requires_grad_(True) for t in (x, w, b))
    y = quick_gelu(F.linear(xs, ws, bs))
    (y * dy.to(dtype)).sum().backward()
    return dict(fwd=y.detach(), dx=xs.grad, dw=ws.grad, db=bs.grad)


def _err(got, ref):
    return {k: (abs(float(got[k]) - float(ref[k])) / abs(float(ref[k])) if ref[k].dim() == 0 else rel(got[k], ref[k])) for k in ref}


def baseline_keys():
    keys = [("prep", *c, B) for c in PREP_CASES for B in PREP_BATCHES] + [("causal", *c) for c in CAUSAL_CASES]
    keys += [("cosine", *c) for c in COSINE_CASES] + [("qgelu",)] + [("loss", n) for n in LOSS_CASES]
    return [k + (p,) for k in keys for p in PRECISIONS]


@functools.lru_cache(maxsize=None)
def reference(key):
    """The float64 values of a case (key without the precision): {quantity: tensor}."""
    return _compute(key, torch.float64)


def _compute(key, dtype):
    kind = key[0]
    if kind == "prep":
        _, Hi, S, P, B = key
        fwd, bwd = prep_torch(*prep_inputs(Hi, S, P, B), S, P, dtype)
        return dict(fwd=fwd, bwd=bwd)
    if kind == "causal":
        _, L, d = key
        return dict(out=causal_torch(causal_inputs(L, d), 2, dtype))
    if kind == "cosine":
        _, B, D, zero = key
        out, du = cosine_torch(*cosine_inputs(B, D, zero), dtype)
        return dict(loss=out, du=du)
    if kind == "qgelu":
        return qgelu_torch(*qgelu_inputs(), dtype)
    out, grad = loss(*loss_inputs(key[1]), loss_state_dict(key[1]), CONFIGS[LOSS_CASES[key[1]][0]], dtype)
    return dict(loss=out, grad=grad)


def errors(got, key):
    """{quantity: error of `got` against the float64 reference of the case}: scalars by relative error, tensors by rel-L2, the
    cosine gradient by its worst row."""
    ref = reference(key)
    out = _err(got, ref)
    if key[0] == "cosine":
        out["du"] = rel_rows(got["du"], ref["du"])
    return out


def measure(key_with_prec, threads=4):
    """BASELINE_ERR's entry for a key, re-measured: the torch CPU computation in the precision against float64, on `threads`
    threads (the CPU GEMMs' summation order depends on the count)."""
    *key, prec = key_with_prec
    before = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        return errors(_compute(tuple(key), PRECISIONS[prec]), tuple(key))
    finally:
        torch.set_num_threads(before)


# ---------------------------------------------------------------------------------------------------------------
# element-wise references and bounds of the kernels of csrc/clip.hip (cases: tests/clip_cases.py)
# ---------------------------------------------------------------------------------------------------------------
# Every bound below is per element and leaves out no element; `check_bound` is the one comparator.  The causal attention is
# checked by tests/attn_ref.py (reference(causal=True), check) with the constant C_CAUSAL measured here.
TWO24 = 2.0 ** -24
A_FLOOR = 2.0 ** -126
COS_EPS = 1e-12                      # F.normalize's eps

# Constants of the bounds: measured on the CPU over every case of tests/clip_cases.py, never against a kernel
# (tests/test_clip_ref_cpu.py re-measures each within 25 %; tests/golden/REPORT_clip_kernels.txt lists them per case class).
#   C_CAUSAL_TORCH  smallest c (attn_ref.smallest_c, o and lse) at which torch's fp32 masked softmax + matmul passes
#   C_CAUSAL_SEQ    the same for `causal_seq_f32`: the header's description of psg_attn_fwd_causal evaluated in numpy fp32 -
#                   one query at a time, keys in ascending order, running maximum, exp(m - m_new) rescale, one division
#   C_CAUSAL        4 x the larger: the project's margin for "a different but fixed order" (attn_ref.C_ATTN was measured on
#                   tree-ordered kernels; this one adds up to 128 keys one after the other, rescaling at every new maximum)
#   C_COS_TORCH     smallest c at which torch's fp32 evaluation of clip_loss.py:60-67 (autograd) passes cosine_ref's bounds
#   C_COS           4 x that
C_CAUSAL_TORCH = 0.0385               # f32.d64.L77.hot
C_CAUSAL_SEQ = 0.0343                 # f32.d64.L77.hot
C_CAUSAL = 4.0 * max(C_CAUSAL_TORCH, C_CAUSAL_SEQ)
C_COS_TORCH = 0.0291                  # bf16.B9.D516.neg
C_COS = 4.0 * C_COS_TORCH
# psg_clip_prep_fwd: the fp32 roundings on the path of ONE term w_y w_x (a x + b) of an output, counted from the header's
# description ("centre and weights in fp64, each weight rounded once, the taps combined in fp32, rows first") and the kernel:
#    2  the two weights, each rounded once to fp32
#    2  a * x, then + b
#    1  w_x * (a x + b)
#    4  the adds of a window row (at most 4 taps; the first, onto 0, is exact and is counted all the same)
#    1  w_y * row
#    4  the adds over the window's rows
#    2  - mean, * inv_std
#    1  the constant's own rounding: the kernel's mean is fp32(mean) where the reference takes the decimal value
#       (inv_std is fp32(1 / std) on both sides, as the header states it)
#   17  each at most 2^-24 of a partial result that the sum of the magnitudes bounds; the fp32 store is exact.
K_PREP = 17


def _f32(x):
    return float(np.float32(x))


def _inv_std():
    return [float(np.float32(1.0) / np.float32(s)) for s in STD]


def check_bound(got, ref, bound, what):
    """Assert |got - ref| <= bound for every element (a NaN in got fails); returns the worst err / bound."""
    g = got.detach().to(device=ref.device, dtype=torch.float64)
    assert g.shape == ref.shape, f"{what}: shape {tuple(g.shape)} vs reference {tuple(ref.shape)}"
    err = (g - ref).abs()
    ratio = err / bound
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if not worst <= 1.0:
        i = int(ratio.argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
        raise AssertionError(f"{what}: {int((ratio > 1.0).sum())} of {ratio.numel()} elements out of bound; worst at {idx}: got "
                             f"{float(g.reshape(-1)[i]):.9g}, ref {float(ref.reshape(-1)[i]):.9g}, |err| {float(err.reshape(-1)[i]):.3g} > bound "
                             f"{float(bound.reshape(-1)[i]):.3g} (err/bound {worst:.3g})")
    return worst


def smallest_c(got, ref, mag, r_out):
    """The smallest c at which |got - ref| <= r_out |ref| + c 2^-24 mag + A_FLOOR holds everywhere."""
    err = (got.detach().double() - ref).abs()
    over = (err - r_out * ref.abs() - A_FLOOR).clamp_min(0.0)
    c = torch.where(over > 0, over / (TWO24 * mag), torch.zeros_like(over))
    c = torch.where(torch.isnan(c), torch.full_like(c, math.inf), c)
    return float(c.max())


# ---- image processor ----------------------------------------------------------------------------------------------
def _axis_matrix(Hi, S, cubic_a=-0.5):
    return resize_matrix(Hi, S, cubic_a) if Hi != S else torch.eye(S, dtype=torch.float64)


def rows_of(pixels, P):
    """[B,3,S,S] -> [B (S/P)^2, 3 P P]."""
    r = patch_rows(pixels, P)
    return r.reshape(-1, r.shape[-1])


def pixels_of(rows, B, S, P):
    """The inverse of rows_of: [B (S/P)^2, 3 P P] -> [B,3,S,S]."""
    G = S // P
    return F.fold(rows.reshape(B, G * G, 3 * P * P).transpose(1, 2), (S, S), P, stride=P)


def prep_fwd_ref(img, S, P, a, b, W=None):
    """psg_clip_prep_fwd in fp64 on the fp32 image: y = (W (a img + b) W^T - mean) inv_std with W clip_ref.resize_matrix (fp64
    weights; the identity when Hi == S), CLIP's mean and fp32(1 / std), a and b as the C floats the entry takes - as patch rows
    [B (S/P)^2, 3 P P] - and the magnitude of the same shape,
        Mag = (sum |Wy| |Wx| (|a x| + |b|) + mean_c) inv_std_c
    (the cubic has negative lobes: the sum of the magnitudes is the scale of the roundings, not |ref|).  The bound is
    K_PREP 2^-24 Mag + A_FLOOR (prep_fwd_bound).  `W` replaces the axis matrix (the CPU test plants defects with it)."""
    a, b = _f32(a), _f32(b)
    x = img.detach().double()
    W = _axis_matrix(x.shape[-1], S) if W is None else W
    Wy, Wx = W if isinstance(W, tuple) else (W, W)
    mean = torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    inv = torch.tensor(_inv_std(), dtype=torch.float64).view(1, 3, 1, 1)
    v = torch.einsum("oh,bchw,pw->bcop", Wy, a * x + b, Wx)
    m = torch.einsum("oh,bchw,pw->bcop", Wy.abs(), (a * x).abs() + abs(b), Wx.abs())
    return rows_of((v - mean) * inv, P), rows_of((m + mean) * inv, P)


def prep_fwd_bound(mag):
    return K_PREP * TWO24 * mag + A_FLOOR


def prep_bwd_ref(dy_rows, B, Hi, S, P, a, W=None):
    """psg_clip_prep_bwd in fp64: dimg[b,c] = a inv_std_c W^T dy[b,c] W with dy the patch rows read back as [B,3,S,S], and M, the
    same sum over |dy|, |a| and |W|.  Bound: 4 2^-24 M + A_FLOOR (prep_bwd_bound) - the kernel forms the sum in fp64 and rounds
    once, with its two constant factors, exactly as psg_image_prep_bwd, which tests/test_imaging_gpu.py holds to this bound."""
    a = _f32(a)
    g = pixels_of(dy_rows.detach().double(), B, S, P)
    W = _axis_matrix(Hi, S) if W is None else W
    inv = torch.tensor(_inv_std(), dtype=torch.float64).view(1, 3, 1, 1)
    ref = a * inv * torch.einsum("oh,bcop,pw->bchw", W, g, W)
    M = abs(a) * inv * torch.einsum("oh,bcop,pw->bchw", W.abs(), g.abs(), W.abs())
    return ref, M


def prep_bwd_bound(M):
    return 4.0 * TWO24 * M + A_FLOOR


def prep_fwd_f32(img, S, P, a, b):
    """The header's description of psg_clip_prep_fwd evaluated in numpy fp32: weights from fp64 rounded once, v = a x + b, the
    taps of each window row first, then the rows, - mean, * inv_std.  Patch rows, fp32."""
    x = img.detach().numpy().astype(np.float32)
    B, _, Hi, _ = x.shape
    a, b = np.float32(a), np.float32(b)
    mean = np.array(MEAN, dtype=np.float32)
    inv = np.float32(1.0) / np.array(STD, dtype=np.float32)
    W = _axis_matrix(Hi, S).numpy()
    out = np.zeros((B, 3, S, S), dtype=np.float32)
    v = a * x + b
    taps = [np.nonzero(W[o])[0] for o in range(S)]
    for oy in range(S):
        for ox in range(S):
            acc = np.zeros((B, 3), dtype=np.float32)
            for iy in taps[oy]:
                row = np.zeros((B, 3), dtype=np.float32)
                for ix in taps[ox]:
                    row = row + np.float32(W[ox, ix]) * v[:, :, iy, ix]
                acc = acc + np.float32(W[oy, iy]) * row
            out[:, :, oy, ox] = (acc - mean) * inv
    return rows_of(torch.from_numpy(out), P)


# ---- cosine loss ------------------------------------------------------------------------------------------------------
def cosine_ref(u, v):
    """clip_loss.py:60-67 with F.normalize's clamp in fp64, its gradient, and the magnitudes of their bounds
        |got - ref| <= r_out |ref| + C_COS 2^-24 M + A_FLOOR.
    Per row r, nu = ||u_r||, nu' = max(nu, eps) (nv, nv' alike), cos_r = u_r . v_r / (nu' nv'), out = -mean_r cos_r,
        du[r, c] = -(v_c / (nu' nv') - [nu > eps] cos_r u_c / nu^2) / B.
    With sq(n) = gemm_ref.c_acc(n) / 2^-24 the factor of an fp32 reduction over n terms, in units of 2^-24:
      e_r    = sum_c |u_c v_c| / (nu' nv')                 the dot product's error scale
      Ecos_r = sq(D) (e_r + 2 |cos_r|) + 4                 u . v, the two norms (a square root halves a relative error: sq(D) / 2
                                                           each, taken whole), the product, the division, the clamp
      out    M = (1/B) sum_r Ecos_r + sq(B) (1/B) sum_r |cos_r|          the cosines, then their sum over the rows
      du     M = (1/B) ((2 sq(D) + 4) |v_c| / (nu' nv') + (Ecos_r + |cos_r| (2 sq(D) + 4)) |u_c| / nu^2)
             the first term's factor 1 / (nu' nv'), the second's cos_r / nu^2 (cos_r's own error plus the squared norm's), the
             two products and the add; the second term is absent where nu <= eps.
    Returns a namespace: loss, loss_mag (0-d), du, du_mag [B, D], cos [B], nu [B]."""
    u, v = u.detach().double(), v.detach().double()
    B, D = u.shape
    sqD, sqB = c_acc(D) / TWO24, c_acc(B) / TWO24
    nu, nv = u.norm(dim=-1, keepdim=True), v.norm(dim=-1, keepdim=True)
    den = nu.clamp_min(COS_EPS) * nv.clamp_min(COS_EPS)
    cos = (u * v).sum(-1, keepdim=True) / den
    gate = nu > COS_EPS
    nu2 = torch.where(gate, nu * nu, torch.ones_like(nu))
    e = (u * v).abs().sum(-1, keepdim=True) / den
    Ecos = sqD * (e + 2.0 * cos.abs()) + 4.0
    r = types.SimpleNamespace(cos=cos.squeeze(-1), nu=nu.squeeze(-1))
    r.loss = -cos.mean()
    r.loss_mag = Ecos.mean() + sqB * cos.abs().mean()
    r.du = -(v / den - torch.where(gate, cos * u / nu2, torch.zeros_like(u))) / B
    r.du_mag = ((2.0 * sqD + 4.0) * v.abs() / den + torch.where(gate, (Ecos + cos.abs() * (2.0 * sqD + 4.0)) * u.abs() / nu2, torch.zeros_like(u))) / B
    return r


def cosine_bound(ref, mag, out_dtype, c=None):
    c = C_COS if c is None else c
    return (BF16_ROUND if out_dtype == torch.bfloat16 else F32_ROUND) * ref.abs() + c * TWO24 * mag + A_FLOOR


# ---- causal attention -------------------------------------------------------------------------------------------------
def causal_seq_f32(q, k, v, heads, scale):
    """include/psg_hip.h's description of psg_attn_fwd_causal evaluated in numpy fp32: one query row at a time, its keys
    s = 0..l in ascending order with a running maximum m - p = exp(s - m_new), sum and the output row rescaled by exp(m - m_new)
    at every key - one division at the end, lse = m + log(sum).  q, k, v: [B, L, heads d] fp32.  Returns (o [B, L, heads d],
    lse [B, heads, L]) as fp32 tensors."""
    B, L, E = q.shape
    d = E // heads
    Q, K, V = (t.detach().reshape(B, L, heads, d).permute(0, 2, 1, 3).contiguous().numpy().astype(np.float32) for t in (q, k, v))
    s = np.zeros((B, heads, L, L), dtype=np.float32)
    for c in range(d):
        s = s + Q[:, :, :, None, c] * K[:, :, None, :, c]
    s = s * np.float32(scale)
    m = np.full((B, heads, L), -np.inf, dtype=np.float32)
    tot = np.zeros((B, heads, L), dtype=np.float32)
    acc = np.zeros((B, heads, L, d), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(L):                                   # key j, for the queries l >= j
            sj = s[:, :, j:, j]
            mn = np.maximum(m[:, :, j:], sj)
            corr = np.exp(m[:, :, j:] - mn)
            p = np.exp(sj - mn)
            tot[:, :, j:] = tot[:, :, j:] * corr + p
            acc[:, :, j:] = acc[:, :, j:] * corr[..., None] + V[:, :, j, None, :] * p[..., None]
            m[:, :, j:] = mn
    o = acc * (np.float32(1.0) / tot)[..., None]
    lse = m + np.log(tot)
    return torch.from_numpy(o).permute(0, 2, 1, 3).reshape(B, L, E), torch.from_numpy(lse)


def causal_torch_f32(q, k, v, heads, scale):
    """torch's own fp32 masked softmax and matmul: (o, lse)."""
    B, L, E = q.shape
    d = E // heads
    Q, K, V = (t.detach().float().reshape(B, L, heads, d).permute(0, 2, 1, 3) for t in (q, k, v))
    s = (Q @ K.transpose(2, 3)) * torch.tensor(scale, dtype=torch.float32)
    s = s.masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), -math.inf)
    return (torch.softmax(s, -1) @ V).permute(0, 2, 1, 3).reshape(B, L, E), torch.logsumexp(s, -1)
