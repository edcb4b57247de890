"""BERT text encoder on the MI355X kernels, frozen or fine-tuned in its last layers (reference: src/models/text_encoder.py).

The reference wraps a transformers `BertModel` (+ `projection`, Linear or Identity, + `layer_norm`) and returns the
normalised `last_hidden_state` [B, S, hidden_dim] of a right-padded token batch.  Stage 2 calls it for every training
and validation batch and every monitoring sample (improved_diffusion_trainer.py:155,202-208,352,461,583) with the model
frozen; stages 1 and 3 train it under `finetune_strategy`.  This class computes the forward on the library's kernels:

  psg_bert_embed_ln        word + token-type + position embeddings, LayerNorm                   1 launch
  per layer (post-LN):     QKV Linear over one packed [3H][H] prepared weight (fp32 bias)        7 launches
                           psg_attn_fwd_varlen (key length per sample = attention_mask.sum(1))
                           out-proj Linear + bias + residual, psg_layernorm
                           FFN-1 Linear + bias + erf-GELU, FFN-2 Linear + bias + residual, psg_layernorm
  projection Linear (hidden_dim != BERT width), final psg_layernorm written in fp32             1-2 launches

Right padding makes the key-length vector exactly the reference's additive `finfo.min` mask: a padded key's probability
is 0 there too, and outputs at padded positions (which the U-Net cross-attends to) are computed like the reference's.

Parameters carry the reference module's names and shapes (`bert.embeddings.*`, `bert.encoder.layer.N.*`, `bert.pooler.*`,
`projection.*` when present, `layer_norm.*`), so a stage-1 checkpoint's 'text_encoder_state_dict' loads unchanged.  The
pooler is kept for checkpoint interchange only: the reference returns `last_hidden_state`, never the pooled output.

By default (`trainable=False`) the class is inference only: every parameter frozen, `torch.no_grad()`, `.train()` ignored;
`finetune_strategy` is validated and otherwise unused.  With `trainable=True` the strategy is applied as the reference
applies it ('none': BERT frozen; 'minimal': last 2 encoder layers + pooler; 'partial': last 4 + pooler; `projection` and
`layer_norm` always trainable; 'full' raises unless `train_embeddings=True` is passed as well: then every `bert.*` parameter
trains, the word / position / token-type tables and their LayerNorm through `ops.bert_embed`, whose backward is
psg_bert_embed_ln_bwd + one atomic-free psg_embed_scatter per table; row `pad_token_id` of the word table - an optional
`bert_config` key, default 0 - gets no gradient, as nn.Embedding's padding_idx).  When grad mode is on, the frozen
prefix runs under no_grad on the inference launches and the trainable suffix through the autograd nodes of `ops`
(`qkv_linear`, `attention_self(kv_len=)`, `linear`, `layer_norm`): autograd stops at the first trainable layer's input, and
nothing of the prefix is kept.  Parameters and gradients are fp32 (`p.grad`), the activations `compute_dtype`.  `.train()`
draws BERT's dropouts (hidden_dropout_prob after the embedding LayerNorm and the two output denses of every layer,
attention_probs_dropout_prob on the probabilities - `bert_config` keys of those names, default 0.1) in frozen and trainable
layers alike, with per-site seeds from the stream the U-Net's attention blocks use.  The pooler's parameters are trainable
under 'minimal' / 'partial' as in the reference and, as there, never receive a gradient: `last_hidden_state` is returned.

`transformers` is used on the host only, to load a pretrained tokenizer / config / state dict (`model_name`) and to
tokenize (`forward`); `encode_ids` needs neither it nor any host synchronisation.
"""
import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import ACT_GELU
from .unet import _SeedStream
from .ops import prep_weight as _prep, prepared as _prepared

# keys of a `bert_config` dict (transformers.BertConfig attribute names)
CONFIG_KEYS = ("hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "vocab_size",
               "max_position_embeddings", "type_vocab_size", "layer_norm_eps")
FINETUNE_STRATEGIES = ("none", "minimal", "partial", "full")
DROPOUT_KEYS = ("hidden_dropout_prob", "attention_probs_dropout_prob")      # optional `bert_config` keys (BertConfig defaults: 0.1)
PAD_KEY = "pad_token_id"            # optional `bert_config` key (BertConfig default: 0): word_embeddings.padding_idx
MAX_LENGTH = 256                    # the reference tokenizer call's max_length (text_encoder.py forward)


def config_dict(cfg):
    """A transformers BertConfig (or a dict) -> the plain dict this class takes; rejects what the kernels do not compute."""
    get = (lambda k: cfg[k]) if isinstance(cfg, dict) else (lambda k: getattr(cfg, k))
    out = {k: get(k) for k in CONFIG_KEYS}
    for k in DROPOUT_KEYS:
        v = cfg.get(k) if isinstance(cfg, dict) else getattr(cfg, k, None)
        if v is not None:
            out[k] = float(v)
    v = cfg.get(PAD_KEY) if isinstance(cfg, dict) else getattr(cfg, PAD_KEY, None)
    if v is not None:
        out[PAD_KEY] = int(v)
    out["layer_norm_eps"] = float(out["layer_norm_eps"])
    for k in CONFIG_KEYS[:-1]:
        out[k] = int(out[k])
    if not isinstance(cfg, dict):
        act = getattr(cfg, "hidden_act", "gelu")
        pet = getattr(cfg, "position_embedding_type", "absolute") or "absolute"
        if act != "gelu" or pet != "absolute":
            raise _lib.PsgError(f"TextEncoder computes BERT with hidden_act='gelu' and absolute positions (got {act!r}, {pet!r})")
    if out["hidden_size"] % out["num_attention_heads"]:
        raise _lib.PsgError("hidden_size must be a multiple of num_attention_heads")
    return out


def _from_pretrained(model_name):
    """(tokenizer, config dict, BertModel state dict) from the local transformers cache - host side only."""
    from transformers import BertModel, BertTokenizer
    tok = BertTokenizer.from_pretrained(model_name)
    m = BertModel.from_pretrained(model_name)
    cfg = config_dict(m.config)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    del m
    return tok, cfg, sd


# containers with transformers' attribute names (state-dict keys only; nothing here runs torch math)
class _SelfAttention(nn.Module):
    def __init__(self, H):
        super().__init__()
        self.query, self.key, self.value = nn.Linear(H, H), nn.Linear(H, H), nn.Linear(H, H)


class _DenseLN(nn.Module):
    def __init__(self, i, o, eps):
        super().__init__()
        self.dense = nn.Linear(i, o)
        self.LayerNorm = nn.LayerNorm(o, eps=eps)


class _Attention(nn.Module):
    def __init__(self, H, eps):
        super().__init__()
        self.self = _SelfAttention(H)
        self.output = _DenseLN(H, H, eps)


class _Intermediate(nn.Module):
    def __init__(self, H, I):
        super().__init__()
        self.dense = nn.Linear(H, I)


class _Layer(nn.Module):
    def __init__(self, c):
        super().__init__()
        H, I, eps = c["hidden_size"], c["intermediate_size"], c["layer_norm_eps"]
        self.attention = _Attention(H, eps)
        self.intermediate = _Intermediate(H, I)
        self.output = _DenseLN(I, H, eps)


class _Encoder(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.layer = nn.ModuleList([_Layer(c) for _ in range(c["num_hidden_layers"])])


class _Embeddings(nn.Module):
    def __init__(self, c):
        super().__init__()
        H = c["hidden_size"]
        self.word_embeddings = nn.Embedding(c["vocab_size"], H, padding_idx=c.get(PAD_KEY, 0))
        self.position_embeddings = nn.Embedding(c["max_position_embeddings"], H)
        self.token_type_embeddings = nn.Embedding(c["type_vocab_size"], H)
        self.LayerNorm = nn.LayerNorm(H, eps=c["layer_norm_eps"])


class _Pooler(nn.Module):
    def __init__(self, H):
        super().__init__()
        self.dense = nn.Linear(H, H)


class _Bert(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.config = dict(c)
        self.embeddings = _Embeddings(c)
        self.encoder = _Encoder(c)
        self.pooler = _Pooler(c["hidden_size"])


def layer_norm(x, weight, bias, eps, residual=None, out_dtype=None):
    """y = LayerNorm(x [+ residual]) * weight + bias over the last dimension (psg_layernorm); x [..., N] contiguous."""
    return ops.layer_norm_fwd(x, weight, bias, eps, residual, out_dtype)[0]


def attention_varlen(qkv, kv_len, heads):
    """Self-attention of packed projections qkv [B, S, 3E] with the keys of sample b limited to kv_len[b] (int32, device)."""
    return ops.attention_fwd(qkv, None, heads, kv_len=kv_len, want_lse=False)[0]


class TextEncoder(nn.Module):
    """src/models/text_encoder.py:TextEncoder (same constructor arguments, same state-dict keys, same forward): frozen, or
    with `trainable=True` fine-tuned under `finetune_strategy`."""

    def __init__(self, model_name='google-bert/bert-base-uncased', hidden_dim=768, finetune_strategy='minimal', *,
                 compute_dtype=torch.float32, tokenizer=None, bert_config=None, trainable=False, train_embeddings=False):
        super().__init__()
        if finetune_strategy not in FINETUNE_STRATEGIES:
            raise ValueError(f"Unknown finetune_strategy: {finetune_strategy}")
        if trainable and finetune_strategy == "full" and not train_embeddings:
            raise _lib.PsgError("TextEncoder(trainable=True, finetune_strategy='full'): the embedding gradients (word / position / "
                                "token-type tables and their LayerNorm) are not built; use 'none', 'minimal' or 'partial', or pass "
                                "train_embeddings=True to train the embedding tables too")
        state = None
        if bert_config is None:                          # pretrained weights and tokenizer from the local HF cache
            tok, cfg, state = _from_pretrained(model_name)
            tokenizer = tokenizer if tokenizer is not None else tok
        else:
            cfg = config_dict(bert_config)
        self.model_name, self.finetune_strategy = model_name, finetune_strategy
        self.compute_dtype = compute_dtype
        self.trainable = bool(trainable)
        self.train_embeddings = bool(train_embeddings)
        self.pad_token_id = int(cfg.get(PAD_KEY, 0))
        self.hidden_dropout_prob = float(cfg.get("hidden_dropout_prob", 0.1))
        self.attention_probs_dropout_prob = float(cfg.get("attention_probs_dropout_prob", 0.1))
        self.tokenizer = tokenizer
        self.bert = _Bert(cfg)
        self.bert_hidden_size = cfg["hidden_size"]
        self.hidden_dim = hidden_dim
        self.projection = nn.Linear(self.bert_hidden_size, hidden_dim) if self.bert_hidden_size != hidden_dim else nn.Identity()
        self.layer_norm = nn.LayerNorm(hidden_dim)
        if state is not None:
            own = self.bert.state_dict()
            self.bert.load_state_dict({k: v for k, v in state.items() if k in own}, strict=True)
        self._cache = {}
        self._apply_finetune_strategy()
        self.eval()

    def _apply_finetune_strategy(self):
        """Set requires_grad as the reference's method of this name and its __init__ do (frozen class: everything off)."""
        for p in self.parameters():
            p.requires_grad = False
        if not self.trainable:
            return
        if self.finetune_strategy == "full":         # (reached with train_embeddings=True only) the reference unfreezes all of bert
            for p in self.parameters():
                p.requires_grad = True
            return
        n = len(self.bert.encoder.layer)
        last = {"none": 0, "minimal": 2, "partial": 4}[self.finetune_strategy]
        for i in range(max(0, n - last), n):
            for p in self.bert.encoder.layer[i].parameters():
                p.requires_grad = True
        if last:
            for p in self.bert.pooler.parameters():
                p.requires_grad = True
        for p in list(self.projection.parameters()) + list(self.layer_norm.parameters()):
            p.requires_grad = True

    def first_trainable_layer(self):
        """Index of the first encoder layer with a trainable parameter (the layer count when BERT is frozen)."""
        for i, lay in enumerate(self.bert.encoder.layer):
            if any(p.requires_grad for p in lay.parameters()):
                return i
        return len(self.bert.encoder.layer)

    def train(self, mode=True):
        """Honoured when trainable; the frozen class stays in eval mode."""
        return super().train(mode and self.trainable)

    @classmethod
    def from_reference(cls, enc, compute_dtype=torch.float32, trainable=False, train_embeddings=False):
        """A reference TextEncoder instance -> this class with its tokenizer, configuration and weights (copied)."""
        obj = cls(hidden_dim=enc.layer_norm.normalized_shape[0], finetune_strategy=getattr(enc, "finetune_strategy", "minimal"),
                  compute_dtype=compute_dtype, tokenizer=enc.tokenizer, bert_config=config_dict(enc.bert.config), trainable=trainable,
                  train_embeddings=train_embeddings)
        own = obj.state_dict()
        obj.load_state_dict({k: v.detach().clone() for k, v in enc.state_dict().items() if k in own}, strict=True)
        return obj.to(next(enc.parameters()).device)

    # -- prepared weights (rebuilt when a parameter changes: load_state_dict, .to()) --------------------------------
    def _layer_weights(self, i, dt):
        lay = self.bert.encoder.layer[i]
        sa, ao, it, ou = lay.attention.self, lay.attention.output.dense, lay.intermediate.dense, lay.output.dense
        qkv = [sa.query.weight, sa.key.weight, sa.value.weight]
        return (
            _prepared(self._cache, ("qkv", i, dt), qkv + [sa.query.bias, sa.key.bias, sa.value.bias],
                      lambda: (_prep(torch.cat(qkv, 0)[:, :, None, None], dt),
                               torch.cat([sa.query.bias, sa.key.bias, sa.value.bias]).detach().float().contiguous())),
            _prepared(self._cache, ("o", i, dt), [ao.weight], lambda: _prep(ao.weight[:, :, None, None], dt)),
            _prepared(self._cache, ("f1", i, dt), [it.weight], lambda: _prep(it.weight[:, :, None, None], dt)),
            _prepared(self._cache, ("f2", i, dt), [ou.weight], lambda: _prep(ou.weight[:, :, None, None], dt)),
        )

    def drop_prepared(self):
        """Forget the packed operands of the trainable layers and the projection.  `_prepared` stamps them with the parameters'
        storage and version counters; an optimizer that writes through raw pointers (optim.GroupedAdamW) moves neither, so its
        stepper calls this after every update.  The frozen prefix keeps its operands."""
        first = self.first_trainable_layer()
        for k in [k for k in self._cache if k[0] == "proj" or k[1] >= first]:
            del self._cache[k]

    def launches_per_call(self):
        """Kernel launches of one encode_ids call."""
        return 1 + 7 * len(self.bert.encoder.layer) + (1 if isinstance(self.projection, nn.Linear) else 0) + 1

    def _qkv_packed(self, i, dt):
        """(wf, bias, wd) of layer i for ops.qkv_linear: the inference path's packed forward weight + the data-gradient one."""
        sa = self.bert.encoder.layer[i].attention.self
        ps = [sa.query.weight, sa.key.weight, sa.value.weight, sa.query.bias, sa.key.bias, sa.value.bias]
        return _prepared(self._cache, ("qkv_train", i, dt), ps, lambda: ops.prep_qkv(*ps, dt, True))

    def _embed(self, ids, tt, dt, drop_p=0.0, seed=0):
        """BertEmbeddings on the inference launches (the embedding dropout in place when drop_p > 0)."""
        emb = self.bert.embeddings
        return ops.bert_embed_fwd(ids, tt, emb.word_embeddings.weight, emb.position_embeddings.weight, emb.token_type_embeddings.weight,
                                  emb.LayerNorm.weight, emb.LayerNorm.bias, self.bert.config["layer_norm_eps"], dt, drop_p, seed)

    def _layer_infer(self, i, x, kv_len, B, S):
        """Encoder layer i on the inference launches (nothing kept for a backward)."""
        c = self.bert.config
        dt = self.compute_dtype
        H, heads, I, eps = c["hidden_size"], c["num_attention_heads"], c["intermediate_size"], c["layer_norm_eps"]
        lay = self.bert.encoder.layer[i]
        (wqkv, bqkv), wo, w1, w2 = self._layer_weights(i, dt)
        ao, it, ou = lay.attention.output, lay.intermediate.dense, lay.output
        qkv = ops.conv_infer(x, wqkv, bqkv, H, 3 * H)
        ctx = attention_varlen(qkv.view(B, S, 3 * H), kv_len, heads).view(B * S, H)
        h = layer_norm(ops.conv_infer(ctx, wo, ao.dense.bias, H, H, residual=x), ao.LayerNorm.weight, ao.LayerNorm.bias, eps)
        u = ops.conv_infer(h, w1, it.bias, H, I, act=ACT_GELU)
        return layer_norm(ops.conv_infer(u, w2, ou.dense.bias, I, H, residual=h), ou.LayerNorm.weight, ou.LayerNorm.bias, eps)

    def _layer_autograd(self, i, x, kv_len, B, S, ph, pa):
        """Encoder layer i through the autograd nodes of `ops` (dropouts ph / pa drawn when > 0)."""
        c = self.bert.config
        dt = self.compute_dtype
        H, heads, eps = c["hidden_size"], c["num_attention_heads"], c["layer_norm_eps"]
        lay = self.bert.encoder.layer[i]
        sa, ao, it, ou = lay.attention.self, lay.attention.output, lay.intermediate.dense, lay.output
        s_attn = _SeedStream.next() if pa > 0 else 0
        s_o, s_f = (_SeedStream.next(), _SeedStream.next()) if ph > 0 else (0, 0)
        qkv = ops.qkv_linear(x, sa.query.weight, sa.query.bias, sa.key.weight, sa.key.bias, sa.value.weight, sa.value.bias,
                             self._qkv_packed(i, dt))
        ctx = ops.attention_self(qkv.view(B, S, 3 * H), heads, drop_p=pa, seed=s_attn, kv_len=kv_len).view(B * S, H)
        # BertSelfOutput / BertOutput: LayerNorm(dropout(dense(.)) + input) - dropout and residual ride the GEMM epilogue, as on
        # the inference launches (same bits in eval mode)
        h = ops.layer_norm(ops.linear(ctx, ao.dense.weight, ao.dense.bias, residual=x, drop_p=ph, seed=s_o), ao.LayerNorm.weight,
                           ao.LayerNorm.bias, eps)
        u = ops.linear(h, it.weight, it.bias, act=ACT_GELU)
        return ops.layer_norm(ops.linear(u, ou.dense.weight, ou.dense.bias, residual=h, drop_p=ph, seed=s_f), ou.LayerNorm.weight,
                              ou.LayerNorm.bias, eps)

    def encode_ids(self, input_ids, attention_mask, token_type_ids=None):
        """Token ids [B, S] + attention mask [B, S] (right padding: ones then zeros) -> [B, S, hidden_dim] fp32."""
        dev = self.layer_norm.weight.device
        if dev.type != "cuda":
            raise _lib.PsgError("TextEncoder (MI355X build) needs its parameters on the GPU; there is no CPU fallback")
        ids = input_ids.to(device=dev, dtype=torch.int64).contiguous()
        kv_len = attention_mask.to(dev).sum(1, dtype=torch.int32).contiguous()      # stays on the device
        tt = None if token_type_ids is None else token_type_ids.to(device=dev, dtype=torch.int64).contiguous()
        drop = self.trainable and self.training and (self.hidden_dropout_prob > 0 or self.attention_probs_dropout_prob > 0)
        if not (self.trainable and (torch.is_grad_enabled() or drop)):
            with torch.no_grad():
                return self._encode_frozen(ids, kv_len, tt)
        return self._encode_train(ids, kv_len, tt, drop)

    def _encode_frozen(self, ids, kv_len, tt):
        dt = self.compute_dtype
        B, S = ids.shape
        x = self._embed(ids, tt, dt)
        for i in range(len(self.bert.encoder.layer)):
            x = self._layer_infer(i, x, kv_len, B, S)
        if isinstance(self.projection, nn.Linear):
            wp = _prepared(self._cache, ("proj", dt), [self.projection.weight], lambda: _prep(self.projection.weight[:, :, None, None], dt))
            x = ops.conv_infer(x, wp, self.projection.bias, self.bert_hidden_size, self.hidden_dim)
        y = layer_norm(x, self.layer_norm.weight, self.layer_norm.bias, self.layer_norm.eps, out_dtype=torch.float32)
        return y.view(B, S, self.hidden_dim)

    def _encode_train(self, ids, kv_len, tt, drop):
        dt = self.compute_dtype
        B, S = ids.shape
        ph, pa = (self.hidden_dropout_prob, self.attention_probs_dropout_prob) if drop else (0.0, 0.0)
        first = self.first_trainable_layer()
        emb = self.bert.embeddings
        emb_params = [emb.word_embeddings.weight, emb.position_embeddings.weight, emb.token_type_embeddings.weight, emb.LayerNorm.weight,
                      emb.LayerNorm.bias]
        train_emb = torch.is_grad_enabled() and any(p.requires_grad for p in emb_params)
        if train_emb:                               # 'full': the embedding is a node too (same launches, same seed draw, same bits)
            first = 0                               # (every layer carries its gradient, trainable or not)
            x = ops.bert_embed(ids, tt, *emb_params, self.bert.config["layer_norm_eps"], self.pad_token_id, dt, ph,
                               _SeedStream.next() if ph > 0 else 0)
        with torch.no_grad():                       # the frozen prefix: no graph, no saved activation
            if not train_emb:
                x = self._embed(ids, tt, dt, ph, _SeedStream.next() if ph > 0 else 0)
            for i in range(first):
                x = self._layer_autograd(i, x, kv_len, B, S, ph, pa) if drop else self._layer_infer(i, x, kv_len, B, S)
        for i in range(first, len(self.bert.encoder.layer)):
            x = self._layer_autograd(i, x, kv_len, B, S, ph, pa)
        if isinstance(self.projection, nn.Linear):
            x = ops.linear(x, self.projection.weight, self.projection.bias)
        y = ops.layer_norm(x, self.layer_norm.weight, self.layer_norm.bias, self.layer_norm.eps, out_dtype=torch.float32)
        return y.view(B, S, self.hidden_dim)

    def tokenize(self, text_list):
        """The reference's tokenizer call (padding to the longest text, truncation at 256 tokens), right padding enforced."""
        if self.tokenizer is None:
            raise _lib.PsgError("TextEncoder built from bert_config= without tokenizer=: call encode_ids with token ids")
        self.tokenizer.padding_side = "right"          # the key-length form of the mask assumes it (BERT's default)
        return self.tokenizer(list(text_list), return_tensors="pt", padding=True, truncation=True, max_length=MAX_LENGTH)

    def forward(self, text_list):
        inputs = self.tokenize(text_list)
        return self.encode_ids(inputs["input_ids"], inputs["attention_mask"], inputs.get("token_type_ids"))
