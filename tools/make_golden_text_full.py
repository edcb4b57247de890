#!/usr/bin/env python3
"""Generate tests/golden/text_encoder_full_grad.npz FROM THE REFERENCE text encoder under finetune_strategy 'full'.

A sibling of tools/make_golden_text_grad.py: the reference module (src/models/text_encoder.py) is loaded by file path and
built without `from_pretrained`, its own `_apply_finetune_strategy` is run with 'full', and its own `forward` is run
unchanged - with the tokenizer replaced by a callable that returns the prepared input_ids / attention_mask / token_type_ids
of tests/text_full_cases.py, so that the ids (many distinct ones, one hot id, token type 1, [UNK], vocab-1, right padding)
are the case's and not what the fixture vocabulary tokenizes to.  fp32, CPU, eval mode, L = sum(y * G).  Beyond what
text_encoder_grad.npz stores per case, the fp64 norm of every row of the three embedding-table gradients is stored: a strided
sample alone cannot tell which row a contribution landed in.  The same module run in fp64 measures the reference's own
fp32 error (written into the report).

    python tools/make_golden_text_full.py --ref <reference checkout> [--out tests/golden]
"""
import argparse
import copy
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tests import text_full_cases as FC  # noqa: E402
from tests.util import digest  # noqa: E402
from make_golden_text_grad import score_stds  # noqa: E402


class PreparedTokenizer:
    """Stands where the reference keeps its BertTokenizer: returns the case's tensors whatever the texts."""

    def __init__(self, ids, mask, tt):
        self.out = {"input_ids": ids, "attention_mask": mask, "token_type_ids": tt}

    def __call__(self, text_list, **kw):
        assert len(text_list) == self.out["input_ids"].shape[0]
        return {k: v.clone() for k, v in self.out.items()}


def reference_encoder(mod, tokenizer):
    from transformers import BertConfig, BertModel
    enc = object.__new__(mod.TextEncoder)
    nn.Module.__init__(enc)
    enc.finetune_strategy = "full"
    enc.tokenizer = tokenizer
    enc.bert = BertModel(BertConfig(**FC.bert_config(), hidden_act="gelu", hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1))
    for p in enc.bert.parameters():                      # so that the flags below are the method's doing
        p.requires_grad = False
    enc._apply_finetune_strategy()                       # the reference's own method
    enc.bert_hidden_size = enc.bert.config.hidden_size
    enc.projection = nn.Linear(enc.bert_hidden_size, FC.HIDDEN_DIM)
    enc.layer_norm = nn.LayerNorm(FC.HIDDEN_DIM)
    for p in list(enc.projection.parameters()) + list(enc.layer_norm.parameters()):      # __init__ lines 54-57
        p.requires_grad = True
    enc.load_state_dict(FC.state_dict(enc), strict=True)
    return enc.eval()


def run(enc, texts, dtype):
    enc.zero_grad(set_to_none=True)
    y = enc(texts)                                       # the reference's forward, unchanged
    (y * FC.cotangent(y.shape).to(dtype)).sum().backward()
    return y.detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    torch.set_num_threads(8)
    spec = importlib.util.spec_from_file_location("ref_text_encoder", os.path.join(args.ref, "src", "models", "text_encoder.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    c = FC.CASE
    ids, mask, tt = FC.inputs()
    vocab = FC.bert_config()["vocab_size"]
    facts = FC.id_facts(ids, mask, tt, vocab)
    FC.check_id_facts(facts)
    enc = reference_encoder(mod, PreparedTokenizer(ids, mask, tt))
    with torch.no_grad():
        stds = score_stds(enc, {"input_ids": ids, "attention_mask": mask, "token_type_ids": tt})
    lo, hi = FC.SCORE_STD_WINDOW
    assert all(lo <= s <= hi for s in stds), f"score std {stds} outside [{lo}, {hi}]"
    texts = ["-"] * FC.B
    y = run(enc, texts, torch.float32)
    out = {f"{c}_input_ids": ids.numpy(), f"{c}_attention_mask": mask.numpy(), f"{c}_token_type_ids": tt.numpy(),
           f"{c}_out_cols": y[:, :, ::FC.COL_STRIDE].contiguous().numpy().astype(np.float32),
           f"{c}_out_stats": np.array([float(y.double().norm()), float(y.double().sum())]),
           f"{c}_out_shape": np.array(y.shape, dtype=np.int64),
           f"{c}_requires_grad": np.array(sorted(n for n, p in enc.named_parameters() if p.requires_grad))}
    none, have, grads = [], [], {}
    for n, p in sorted(enc.named_parameters()):
        if not p.requires_grad:
            continue
        if p.grad is None:
            none.append(n)
            continue
        have.append(n)
        grads[n] = p.grad.detach().clone()
        out[f"{c}_grad_d::{n}"], out[f"{c}_grad_s::{n}"] = digest(p.grad, max_elems=FC.GRAD_SAMPLE)
    out[f"{c}_grad_none"], out[f"{c}_grad_names"] = np.array(none), np.array(have)
    for n in FC.EMBED_TABLES:
        out[f"{c}_row_norms::{n}"] = grads[n].double().norm(dim=1).numpy()
    word = grads[FC.EMBED_TABLES[0]]
    assert not word[FC.PAD].any(), "the reference's gradient of word row 0 (padding_idx) must be exactly zero"
    # the reference's own fp32 error: the same module in fp64
    enc64 = copy.deepcopy(enc).double()
    y64 = run(enc64, texts, torch.float64)
    e_out = float((y.double() - y64).abs().max() / y64.abs().max())
    e_par, e_name = 0.0, ""
    for n, p in enc64.named_parameters():
        if n in grads and not n.endswith("attention.self.key.bias"):          # key biases: identically zero, rounding noise only
            e = float((grads[n].double() - p.grad).abs().max() / p.grad.abs().max())
            if e > e_par:
                e_par, e_name = e, n
    np.savez_compressed(os.path.join(args.out, "text_encoder_full_grad.npz"), **out)
    rows = {n: int((out[f"{c}_row_norms::{n}"] > 0).sum()) for n in FC.EMBED_TABLES}
    lines = [
        "tests/golden/text_encoder_full_grad.npz: reference src/models/text_encoder.py under finetune_strategy 'full', forward + "
        "backward of L = sum(y * G) (transformers BertModel, fp32, CPU, eval), driven by the ids of tests/text_full_cases.py",
        f"case {c}: layers {FC.LAYERS}, hidden_dim {FC.HIDDEN_DIM}, out {tuple(y.shape)}, token counts {mask.sum(1).tolist()}, "
        f"|y| {float(y.norm()):.6f}, requires_grad {len(out[f'{c}_requires_grad'])}, gradients {len(have)}, grad None {len(none)}",
        f"ids: distinct {facts['distinct']}, hot id {facts['hot_id']} x {facts['hot_count']} over {facts['hot_samples']} samples, "
        f"unused vocabulary rows {facts['unused']}, token type 1 on {facts['type1']} of {facts['live']} live positions, "
        f"padded {facts['padded']} of {facts['positions']}, [UNK] {facts['has_unk']}, vocab-1 {facts['has_last']}",
        "score std per layer " + " ".join(f"{s:.3f}" for s in stds) + " (window [%g, %g])" % (lo, hi),
        "non-zero gradient rows: word %d, position %d, token type %d; word row 0 exactly zero: True" % tuple(rows[n] for n in FC.EMBED_TABLES),
        f"fp32 vs the same module in fp64: output max-rel {e_out:.2e}, worst gradient max-rel {e_par:.2e} ({e_name}; key biases excluded)",
    ]
    with open(os.path.join(args.out, "REPORT_text_full_grad.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
