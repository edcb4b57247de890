"""Cases of the text-encoder gradient fixture (tests/golden/text_encoder_grad.npz, made by tools/make_golden_text_grad.py
from the reference module's own forward + backward): strategy, size and texts per case, the weights (tests/text_cases.py's,
with the query / key projections sharpened) and the loss's cotangent - all rebuilt here from oracle.hashgen."""
import torch

from oracle import hashgen
from tests import text_cases as TC

# N: BERT frozen (projection + layer_norm train); M: 'minimal' over 3 layers (layer 0 frozen); P: 'partial' over 5 layers
# (layer 0 frozen), hidden_dim 768 (Identity projection), one text truncated at 256 tokens
CASES = {
    "N": {"strategy": "none", "layers": 2, "hidden_dim": 256, "texts": TC.CASES["A"]["texts"]},
    "M": {"strategy": "minimal", "layers": 3, "hidden_dim": 256, "texts": TC.CASES["A"]["texts"]},
    "P": {"strategy": "partial", "layers": 5, "hidden_dim": 768, "texts": TC.CASES["B"]["texts"]},
}
COL_STRIDE = {"N": 8, "M": 8, "P": 12}         # the fixture keeps every position, every k-th feature column of the output
GRAD_SAMPLE = 512                              # elements of the strided sample kept per gradient tensor (tests.util.digest)
SEED_G = 1717                                  # hashgen seed of the cotangent G of the loss L = sum(y * G)
# At the fixture's std 0.02 the scaled attention scores have std 0.3: a near-uniform softmax, under which a wrong softmax
# backward passes.  x4 on W_q and W_k puts every layer's score std inside SCORE_STD_WINDOW (the generator measures and
# asserts it); x8 gives std 20, too peaked for a bf16 comparison.  Change the factor, not the window.
QK_FACTOR = 4.0
SCORE_STD_WINDOW = (2.0, 8.0)


def weight(key, shape):
    w = TC.weight(key, shape)
    if key.endswith("attention.self.query.weight") or key.endswith("attention.self.key.weight"):
        w = w * QK_FACTOR
    return w


def state_dict(module):
    return {k: weight(k, v.shape) for k, v in module.state_dict().items()}


def cotangent(case, shape):
    """G of L = sum(y * G), every position (padded ones included)."""
    return hashgen.uniform(tuple(shape), SEED_G, hashgen.name_id("G_" + case))


def trainable_names(module):
    return sorted(n for n, p in module.named_parameters() if p.requires_grad)
