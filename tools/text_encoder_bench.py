#!/usr/bin/env python3
"""Frozen BERT-base text encoder forward: this package's kernels against a torch-ROCm restatement with the same weights.

For B in {1, 64, 256}, S in {32, 128, 256}, bf16 and fp32: device-event time per call after warm-up, TFLOP/s by the
formula 12 layers x (2 x (768*2304 + 768*768 + 2*768*3072) + 4*S*768) FLOP per token (GEMMs + attention; the
embeddings, LayerNorms and the projection-free final LayerNorm are not counted), launches per call, the attention kernel
family the call took (psg_attn_path_counts), and the same for the torch leg: F.linear / F.scaled_dot_product_attention
with the additive finfo.min padding mask / F.layer_norm in the same dtype.  Every sample is full length (kv_len = S).

    python tools/text_encoder_bench.py [--iters 20] [--warmup 3] [--json out.json] [--check]

--check: also compares the two legs' outputs (rel-L2) on a ragged batch, so the restatement is known to compute the same.
--train: instead of the frozen forward, forward + backward of `TextEncoder(trainable=True)` under 'minimal' and 'partial'
         (eval mode, a fixed cotangent, gradients into p.grad) next to torch autograd over the same restatement and weights;
         FLOP = the forward's + 2x the trainable layers' (data and weight gradients; the first trainable layer's QKV data
         gradient is not computed and not counted).
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BERT_BASE = {"hidden_size": 768, "num_hidden_layers": 12, "num_attention_heads": 12, "intermediate_size": 3072,
             "vocab_size": 30522, "max_position_embeddings": 512, "type_vocab_size": 2, "layer_norm_eps": 1e-12}


def flop_per_call(B, S, c=BERT_BASE):
    H, I, L = c["hidden_size"], c["intermediate_size"], c["num_hidden_layers"]
    return B * S * L * (2.0 * (H * 3 * H + H * H + 2 * H * I) + 4.0 * S * H)


def torch_forward(enc, ids, mask, tt=None, dtype=torch.float32):
    """The reference computation restated with torch functional ops on enc's weights (BertModel eval forward + projection +
    LayerNorm); returns fp32 [B, S, hidden_dim]."""
    c = enc.bert.config
    H, nh = c["hidden_size"], c["num_attention_heads"]
    d, eps = H // nh, c["layer_norm_eps"]
    B, S = ids.shape
    e = enc.bert.embeddings
    tt = torch.zeros_like(ids) if tt is None else tt
    x = (e.word_embeddings.weight[ids] + e.token_type_embeddings.weight[tt]) + e.position_embeddings.weight[:S][None]
    x = F.layer_norm(x, (H,), e.LayerNorm.weight, e.LayerNorm.bias, eps).to(dtype)
    amask = ((1.0 - mask[:, None, None, :].to(dtype)) * torch.finfo(dtype).min)          # transformers' additive padding mask
    w = lambda t: t.to(dtype)                                                           # noqa: E731
    for lay in enc.bert.encoder.layer:
        sa, ao = lay.attention.self, lay.attention.output
        heads = lambda t: t.view(B, S, nh, d).transpose(1, 2)                           # noqa: E731
        q, k, v = (heads(F.linear(x, w(m.weight), w(m.bias))) for m in (sa.query, sa.key, sa.value))
        ctx = F.scaled_dot_product_attention(q, k, v, attn_mask=amask).transpose(1, 2).reshape(B, S, H)
        h = F.layer_norm(F.linear(ctx, w(ao.dense.weight), w(ao.dense.bias)) + x, (H,), w(ao.LayerNorm.weight), w(ao.LayerNorm.bias), eps)
        u = F.gelu(F.linear(h, w(lay.intermediate.dense.weight), w(lay.intermediate.dense.bias)))
        x = F.layer_norm(F.linear(u, w(lay.output.dense.weight), w(lay.output.dense.bias)) + h, (H,), w(lay.output.LayerNorm.weight),
                         w(lay.output.LayerNorm.bias), eps)
    if isinstance(enc.projection, torch.nn.Linear):
        x = F.linear(x, w(enc.projection.weight), w(enc.projection.bias))
    return F.layer_norm(x.float(), (x.shape[-1],), enc.layer_norm.weight, enc.layer_norm.bias, enc.layer_norm.eps)


def train_flop_per_call(B, S, trained, c=BERT_BASE):
    H, I, L = c["hidden_size"], c["intermediate_size"], c["num_hidden_layers"]
    per_layer = B * S * (2.0 * (H * 3 * H + H * H + 2 * H * I) + 4.0 * S * H)
    return per_layer * (L + 2 * trained) - B * S * 2.0 * H * 3 * H


def build(dev, hidden_dim=768, **kw):
    from pokemon_sprite_generator_amd.text_encoder import TextEncoder
    enc = TextEncoder(bert_config=BERT_BASE, hidden_dim=hidden_dim, **kw).to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        for k, p in enc.named_parameters():
            if k.endswith("LayerNorm.weight") or k == "layer_norm.weight":
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, device=dev, generator=g))
            else:
                p.copy_(0.02 * torch.randn(p.shape, device=dev, generator=g))
    return enc


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def train_legs(args, lib, dev, dts, rows):
    def counts():
        m, v, f = C.c_int64(), C.c_int64(), C.c_int64()
        lib.psg_attn_path_counts(C.byref(m), C.byref(v), C.byref(f))
        return m.value, v.value, f.value

    print(f"{'strategy':8} {'dtype':5} {'B':>4} {'S':>4} {'fwd+bwd ms':>10} {'TFLOP/s':>8} {'attn family':>12} | {'torch ms':>9} {'TFLOP/s':>8} {'speedup':>7}")
    for strat in args.strategies.split(","):
        enc = build(dev, finetune_strategy=strat, trainable=True)
        trained = len(enc.bert.encoder.layer) - enc.first_trainable_layer()
        for dn in args.dtypes.split(","):
            enc.compute_dtype = dts[dn]
            for B in (int(b) for b in args.batches.split(",")):
                for S in (int(s) for s in args.seqs.split(",")):
                    ids = torch.randint(1000, 30000, (B, S), device=dev)
                    mask = torch.ones(B, S, dtype=torch.int64, device=dev)
                    G = torch.randn(B, S, enc.hidden_dim, device=dev)

                    def ours():
                        enc.zero_grad(set_to_none=True)
                        enc.encode_ids(ids, mask).backward(G)

                    def theirs():
                        enc.zero_grad(set_to_none=True)
                        torch_forward(enc, ids, mask, dtype=dts[dn]).backward(G)

                    ours()
                    c0 = counts()
                    ours()
                    torch.cuda.synchronize()
                    c1 = counts()
                    fam = ["bf16-mfma", "valu", "fp32-mfma"][max(range(3), key=lambda i: c1[i] - c0[i])]
                    ms = timed(ours, args.iters, args.warmup)
                    tms = timed(theirs, args.iters, args.warmup)
                    fl = train_flop_per_call(B, S, trained)
                    r = {"strategy": strat, "trained_layers": trained, "dtype": dn, "B": B, "S": S, "ms": ms, "tflops": fl / ms / 1e9,
                         "attn_family": fam, "attn_launches": [c1[i] - c0[i] for i in range(3)], "torch_ms": tms, "torch_tflops": fl / tms / 1e9,
                         "speedup": tms / ms}
                    rows.append(r)
                    print(f"{strat:8} {dn:5} {B:4d} {S:4d} {ms:10.3f} {r['tflops']:8.1f} {fam:>12} | {tms:9.3f} {r['torch_tflops']:8.1f} {r['speedup']:7.2f}",
                          flush=True)
        del enc
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,64,256")
    ap.add_argument("--seqs", default="32,128,256")
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--json", default=None)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--strategies", default="minimal,partial")
    args = ap.parse_args()
    from pokemon_sprite_generator_amd import _lib
    dev = torch.device("cuda", 0)
    lib = _lib.init(0)
    dts = {"bf16": torch.bfloat16, "fp32": torch.float32}
    rows = []
    if args.train:
        train_legs(args, lib, dev, dts, rows)
        if args.json:
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            with open(args.json, "w") as f:
                json.dump({"tool": "tools/text_encoder_bench.py --train", "iters": args.iters, "warmup": args.warmup, "rows": rows}, f, indent=1)
        return
    enc = build(dev)
    print(f"{'dtype':5} {'B':>4} {'S':>4} {'ms':>9} {'TFLOP/s':>8} {'launch':>6} {'attn family':>12} | {'torch ms':>9} {'TFLOP/s':>8} {'speedup':>7}")

    def counts():
        m, v, f = C.c_int64(), C.c_int64(), C.c_int64()
        lib.psg_attn_path_counts(C.byref(m), C.byref(v), C.byref(f))
        return m.value, v.value, f.value

    for dn in args.dtypes.split(","):
        enc.compute_dtype = dts[dn]
        for B in (int(b) for b in args.batches.split(",")):
            for S in (int(s) for s in args.seqs.split(",")):
                ids = torch.randint(1000, 30000, (B, S), device=dev)
                mask = torch.ones(B, S, dtype=torch.int64, device=dev)
                with torch.no_grad():
                    enc.encode_ids(ids, mask)                                     # prepares the weights of this dtype
                    c0 = counts()
                    enc.encode_ids(ids, mask)
                    torch.cuda.synchronize()
                    c1 = counts()
                    fam = ["bf16-mfma", "valu", "fp32-mfma"][max(range(3), key=lambda i: c1[i] - c0[i])]
                    ms = timed(lambda: enc.encode_ids(ids, mask), args.iters, args.warmup)
                    tms = timed(lambda: torch_forward(enc, ids, mask, dtype=dts[dn]), args.iters, args.warmup)
                fl = flop_per_call(B, S)
                r = {"dtype": dn, "B": B, "S": S, "ms": ms, "tflops": fl / ms / 1e9, "launches": enc.launches_per_call(),
                     "attn_family": fam, "torch_ms": tms, "torch_tflops": fl / tms / 1e9, "speedup": tms / ms}
                rows.append(r)
                print(f"{dn:5} {B:4d} {S:4d} {ms:9.3f} {r['tflops']:8.1f} {r['launches']:6d} {fam:>12} | {tms:9.3f} {r['torch_tflops']:8.1f} "
                      f"{r['speedup']:7.2f}", flush=True)
    if args.check:
        lens = torch.tensor([1, 17, 64, 128], device=dev)
        ids = torch.randint(1000, 30000, (4, 128), device=dev)
        mask = (torch.arange(128, device=dev)[None] < lens[:, None]).to(torch.int64)
        for dn in args.dtypes.split(","):
            enc.compute_dtype = dts[dn]
            with torch.no_grad():
                a, b = enc.encode_ids(ids, mask), torch_forward(enc, ids, mask, dtype=dts[dn])
                ref = torch_forward(enc, ids, mask, dtype=torch.float32)
            rl = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm())   # noqa: E731
            print(f"check {dn}: kernels vs torch-fp32 rel-L2 {rl(a, ref):.2e}; torch-{dn} vs torch-fp32 {rl(b, ref):.2e}")
            rows.append({"check": dn, "kernels_vs_torch_fp32": rl(a, ref), "torch_vs_torch_fp32": rl(b, ref)})
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"tool": "tools/text_encoder_bench.py", "iters": args.iters, "warmup": args.warmup, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
