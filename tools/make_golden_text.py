#!/usr/bin/env python3
"""Generate tests/golden/text_encoder.npz FROM THE REFERENCE text encoder (src/models/text_encoder.py).

The reference module is loaded by file path and instantiated without `from_pretrained` (no model download): a
`BertModel(BertConfig(...))` of the case's size, a `BertTokenizer` over tests/golden/text_vocab.txt, and `projection` /
`layer_norm` as its __init__ makes them.  Weights come from tests/text_cases.py (oracle.hashgen); the reference's own
forward(text_list) runs unchanged on the CPU in fp32, eval mode.  OUTPUTS ONLY are written: token ids, masks, the
state-dict layout, and every position of the output at every COL_STRIDE-th feature column (+ its full norm and sum).

    python tools/make_golden_text.py --ref <reference checkout> [--out tests/golden]
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import text_cases as TC  # noqa: E402


def reference_encoder(mod, layers, hidden_dim):
    from transformers import BertConfig, BertModel, BertTokenizer
    cfg = TC.bert_config(layers)
    enc = object.__new__(mod.TextEncoder)
    nn.Module.__init__(enc)
    enc.finetune_strategy = "none"
    enc.tokenizer = BertTokenizer(vocab_file=TC.VOCAB, do_lower_case=True)
    enc.bert = BertModel(BertConfig(**cfg, hidden_act="gelu", hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1))
    enc.bert_hidden_size = enc.bert.config.hidden_size
    enc.projection = nn.Linear(enc.bert_hidden_size, hidden_dim) if enc.bert_hidden_size != hidden_dim else nn.Identity()
    enc.layer_norm = nn.LayerNorm(hidden_dim)
    enc.load_state_dict(TC.state_dict(enc), strict=True)
    return enc.eval()


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
    for name, case in TC.CASES.items():
        enc = reference_encoder(mod, case["layers"], case["hidden_dim"])
        inputs = enc.tokenizer(case["texts"], return_tensors="pt", padding=True, truncation=True, max_length=256)
        with torch.no_grad():
            y = enc(case["texts"])                       # the reference's forward, unchanged
        st = TC.COL_STRIDE[name]
        out[f"{name}_input_ids"] = inputs["input_ids"].numpy().astype(np.int64)
        out[f"{name}_attention_mask"] = inputs["attention_mask"].numpy().astype(np.int64)
        out[f"{name}_token_type_ids"] = inputs["token_type_ids"].numpy().astype(np.int64)
        out[f"{name}_out_cols"] = y[:, :, ::st].contiguous().numpy().astype(np.float32)
        out[f"{name}_out_stats"] = np.array([float(y.double().norm()), float(y.double().sum())])
        out[f"{name}_out_shape"] = np.array(y.shape, dtype=np.int64)
        out[f"{name}_state_dict"] = np.array(TC.key_shapes(enc))
        lens = inputs["attention_mask"].sum(1).tolist()
        report.append(f"case {name}: layers {case['layers']}, hidden_dim {case['hidden_dim']}, out {tuple(y.shape)}, "
                      f"token counts {lens}, |y| {float(y.norm()):.6f}, state-dict entries {len(out[f'{name}_state_dict'])}")
    np.savez_compressed(os.path.join(args.out, "text_encoder.npz"), **out)
    with open(os.path.join(args.out, "REPORT_text.txt"), "w") as f:
        f.write("tests/golden/text_encoder.npz: reference src/models/text_encoder.py forward (transformers BertModel, fp32, CPU, eval)\n")
        f.write("weights: tests/text_cases.py (hashgen seed %d, std %.3g, LayerNorm gamma 1 + 0.1 u)\n" % (TC.SEED_W, TC.STD))
        f.write("\n".join(report) + "\n")
    print("\n".join(report))


if __name__ == "__main__":
    main()
