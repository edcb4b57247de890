#!/usr/bin/env python3
"""Generate tests/golden/text_encoder_grad.npz FROM THE REFERENCE text encoder's forward AND backward.

A sibling of tools/make_golden_text.py: the reference module (src/models/text_encoder.py) is loaded by file path and built
without `from_pretrained`; the fine-tuning strategy is applied by the reference's own `_apply_finetune_strategy` and the
`requires_grad` lines of its __init__.  Weights come from tests/text_grad_cases.py (oracle.hashgen).  fp32, CPU, eval mode
(dropout off), loss L = sum(y * G).  OUTPUTS ONLY are written: ids and masks, the output at every COL_STRIDE-th column, the
names with requires_grad, the names whose .grad is None after backward, and per remaining gradient its norm, sum and a
strided sample (tests.util.digest).  The scaled attention scores' std is measured per layer and asserted to lie in
SCORE_STD_WINDOW.

    python tools/make_golden_text_grad.py --ref <reference checkout> [--out tests/golden]
"""
import argparse
import importlib.util
import math
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import text_cases as TC  # noqa: E402
from tests import text_grad_cases as GC  # noqa: E402
from tests.util import digest  # noqa: E402


def reference_encoder(mod, case):
    from transformers import BertConfig, BertModel, BertTokenizer
    cfg = TC.bert_config(case["layers"])
    enc = object.__new__(mod.TextEncoder)
    nn.Module.__init__(enc)
    enc.finetune_strategy = case["strategy"]
    enc.tokenizer = BertTokenizer(vocab_file=TC.VOCAB, do_lower_case=True)
    enc.bert = BertModel(BertConfig(**cfg, hidden_act="gelu", hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1))
    enc._apply_finetune_strategy()                       # the reference's own method
    enc.bert_hidden_size = enc.bert.config.hidden_size
    hd = case["hidden_dim"]
    enc.projection = nn.Linear(enc.bert_hidden_size, hd) if enc.bert_hidden_size != hd else nn.Identity()
    enc.layer_norm = nn.LayerNorm(hd)
    for p in enc.projection.parameters():                # __init__ lines 54-57
        p.requires_grad = True
    for p in enc.layer_norm.parameters():
        p.requires_grad = True
    enc.load_state_dict(GC.state_dict(enc), strict=True)
    return enc.eval()


def score_stds(enc, inputs):
    """std of the scaled scores q.k/sqrt(d) over the unmasked (query, key) pairs, per layer."""
    out = enc.bert(**inputs, output_hidden_states=True)
    mask = inputs["attention_mask"].bool()
    heads = enc.bert.config.num_attention_heads
    stds = []
    for i, lay in enumerate(enc.bert.encoder.layer):
        x = out.hidden_states[i]
        B, S, H = x.shape
        d = H // heads
        q = lay.attention.self.query(x).view(B, S, heads, d).transpose(1, 2)
        k = lay.attention.self.key(x).view(B, S, heads, d).transpose(1, 2)
        sc = (q @ k.transpose(-1, -2)) / math.sqrt(d)
        pair = (mask[:, None, :, None] & mask[:, None, None, :]).expand_as(sc)
        stds.append(float(sc[pair].std()))
    return stds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    torch.set_num_threads(8)
    spec = importlib.util.spec_from_file_location("ref_text_encoder", os.path.join(args.ref, "src", "models", "text_encoder.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out, report = {}, []
    for name, case in GC.CASES.items():
        enc = reference_encoder(mod, case)
        inputs = enc.tokenizer(case["texts"], return_tensors="pt", padding=True, truncation=True, max_length=256)
        with torch.no_grad():
            stds = score_stds(enc, inputs)
        lo, hi = GC.SCORE_STD_WINDOW
        assert all(lo <= s <= hi for s in stds), f"case {name}: score std {stds} outside [{lo}, {hi}]: change QK_FACTOR"
        y = enc(case["texts"])                           # the reference's forward, unchanged
        G = GC.cotangent(name, y.shape)
        (y * G).sum().backward()
        st = GC.COL_STRIDE[name]
        out[f"{name}_input_ids"] = inputs["input_ids"].numpy().astype(np.int64)
        out[f"{name}_attention_mask"] = inputs["attention_mask"].numpy().astype(np.int64)
        out[f"{name}_token_type_ids"] = inputs["token_type_ids"].numpy().astype(np.int64)
        out[f"{name}_out_cols"] = y.detach()[:, :, ::st].contiguous().numpy().astype(np.float32)
        out[f"{name}_out_stats"] = np.array([float(y.detach().double().norm()), float(y.detach().double().sum())])
        out[f"{name}_out_shape"] = np.array(y.shape, dtype=np.int64)
        out[f"{name}_requires_grad"] = np.array(GC.trainable_names(enc))
        none, have = [], []
        for n, p in sorted(enc.named_parameters()):
            if not p.requires_grad:
                continue
            if p.grad is None:
                none.append(n)
                continue
            have.append(n)
            d, s = digest(p.grad, max_elems=GC.GRAD_SAMPLE)
            out[f"{name}_grad_d::{n}"], out[f"{name}_grad_s::{n}"] = d, s
        out[f"{name}_grad_none"] = np.array(none)
        out[f"{name}_grad_names"] = np.array(have)
        lens = inputs["attention_mask"].sum(1).tolist()
        report.append(f"case {name}: strategy {case['strategy']}, layers {case['layers']}, hidden_dim {case['hidden_dim']}, "
                      f"out {tuple(y.shape)}, token counts {lens}, |y| {float(y.detach().norm()):.6f}, requires_grad {len(out[f'{name}_requires_grad'])}, "
                      f"gradients {len(have)}, grad None {len(none)}, score std per layer " + " ".join(f"{s:.3f}" for s in stds))
    np.savez_compressed(os.path.join(args.out, "text_encoder_grad.npz"), **out)
    with open(os.path.join(args.out, "REPORT_text_grad.txt"), "w") as f:
        f.write("tests/golden/text_encoder_grad.npz: reference src/models/text_encoder.py forward + backward of L = sum(y * G) "
                "(transformers BertModel, fp32, CPU, eval)\n")
        f.write("weights: tests/text_grad_cases.py (tests/text_cases.py's, query / key weights x %g); score std window [%g, %g]\n"
                % (GC.QK_FACTOR, *GC.SCORE_STD_WINDOW))
        f.write("\n".join(report) + "\n")
    print("\n".join(report))


if __name__ == "__main__":
    main()
