"""Cases of the text-encoder fixtures (tests/golden/text_encoder.npz, made by tools/make_golden_text.py from the reference
module): BERT configurations, the texts, and the hash-generated weights - rebuilt here bit for bit from oracle.hashgen,
so that neither the weights nor `transformers` are needed where the fixture is checked."""
import math
import os

import torch

from oracle import hashgen

VOCAB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text_vocab.txt")
SEED_W = 909
STD = 0.02                                    # BERT's initializer_range
U_STD = math.sqrt(3.0)                        # hashgen.uniform is uniform in [-1, 1): std 1/sqrt(3)


def vocab_words():
    return [w for w in open(VOCAB).read().split("\n") if w]


def bert_config(layers):
    """BERT-base widths (768, 12 heads, 3072) with `layers` layers over the fixture vocabulary."""
    return {"hidden_size": 768, "num_hidden_layers": layers, "num_attention_heads": 12, "intermediate_size": 3072,
            "vocab_size": len(vocab_words()), "max_position_embeddings": 512, "type_vocab_size": 2, "layer_norm_eps": 1e-12}


def _text(n, tid):
    """n words of the vocabulary (specials and word pieces excluded), picked by hash."""
    words = [w for w in vocab_words() if not w.startswith("[") and not w.startswith("##")]
    idx = hashgen.randint((n,), SEED_W + 1, tid, 0, len(words)).tolist()
    return " ".join(words[i] for i in idx)


# A: 2 layers, projection 768 -> 256 on, three texts of very different lengths
# B: all 12 layers, hidden_dim 768 (Identity: the shipped config), one text past the 256-token truncation
CASES = {
    "A": {"layers": 2, "hidden_dim": 256, "texts": [_text(4, 1), _text(37, 2), _text(95, 3)]},
    "B": {"layers": 12, "hidden_dim": 768, "texts": [_text(300, 4), _text(21, 5)]},
}
COL_STRIDE = {"A": 4, "B": 12}                 # the fixture keeps every position, every k-th feature column


def weight(key, shape):
    """The fixture value of state-dict entry `key`: std 0.02 for weights, embeddings and biases; LayerNorm gamma near 1."""
    u = hashgen.uniform(tuple(shape), SEED_W, hashgen.name_id(key))
    if key.endswith("LayerNorm.weight") or key == "layer_norm.weight":
        return 1.0 + 0.1 * u
    return u * (STD * U_STD)


def state_dict(module):
    """Hash-generated values for every entry of `module`'s state dict (reference or this package's TextEncoder)."""
    return {k: weight(k, v.shape) for k, v in module.state_dict().items()}


def key_shapes(module):
    """'key:d0xd1' strings in state-dict order - the layout a checkpoint carries."""
    return ["%s:%s" % (k, "x".join(str(s) for s in v.shape)) for k, v in module.state_dict().items()]
