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
         gradient is not computed and not counted).  `--strategies full` builds the encoder with train_embeddings=True: the
         embedding tables train too (there the first layer's QKV data gradient is computed, and counted).
--embed: the embedding backward alone at bert-base tables, (B, S) of --pairs: dropout mask, psg_bert_embed_ln_bwd, the device
         sort and the three psg_embed_scatter launches (94 MB zero-fill of the word-table gradient included) through
         `ops.bert_embed`'s backward, alternating call by call with torch autograd over F.embedding x 3 + F.layer_norm +
         F.dropout on the same tables; and, through the C ABI, the share of the kernel sequence that is the zero-fill
         (accumulate = 0 against accumulate = 1 on the word table).
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


def timed_alternating(f1, f2, iters, warmup):
    """ms per call of f1 and of f2, run in turns (f1, f2, f1, ...) so that both see the same machine state."""
    for _ in range(warmup):
        f1()
        f2()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters)]
    for a, b, c in ev:
        a.record()
        f1()
        b.record()
        f2()
        c.record()
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b, _ in ev) / iters, sum(b.elapsed_time(c) for _, b, c in ev) / iters


def embed_legs(args, lib, dev, dts, rows):
    from pokemon_sprite_generator_amd import _lib, ops
    from pokemon_sprite_generator_amd._lib import check, dtype_code, ptr, stream_ptr
    c, p, seed = BERT_BASE, 0.1, 4321
    V, P, N, eps = c["vocab_size"], c["max_position_embeddings"], c["hidden_size"], c["layer_norm_eps"]
    g = torch.Generator(device=dev).manual_seed(0)
    tabs = [0.02 * torch.randn(s, device=dev, generator=g) for s in ((V, N), (P, N), (2, N))]
    tabs += [1.0 + 0.1 * torch.randn(N, device=dev, generator=g), 0.02 * torch.randn(N, device=dev, generator=g)]
    params = [t.requires_grad_(True) for t in tabs]
    word, pos, typ, gamma, beta = params
    print(f"{'dtype':5} {'B':>4} {'S':>4} {'embed bwd ms':>12} {'torch ms':>9} {'speedup':>7} | {'kernels ms':>10} {'acc=1 ms':>9} {'zero-fill':>9}")
    for dn in args.dtypes.split(","):
        dt = dts[dn]
        for B, S in (tuple(int(v) for v in pr.split("x")) for pr in args.pairs.split(",")):
            rows_ = B * S
            ids = torch.randint(1000, 30000, (B, S), device=dev)
            ids[:, S - S // 4:] = 0                                               # a quarter of right padding
            tt = (torch.arange(S, device=dev)[None] >= S // 3).long().expand(B, S).contiguous()
            G = torch.randn(rows_, N, device=dev).to(dt)
            y = ops.bert_embed(ids, tt, word, pos, typ, gamma, beta, eps, 0, dt, p, seed)
            torch.manual_seed(0)
            z = (F.embedding(ids, word, padding_idx=0) + F.embedding(tt, typ)) + F.embedding(torch.arange(S, device=dev)[None].expand(B, S), pos)
            yt = F.dropout(F.layer_norm(z, (N,), gamma, beta, eps).to(dt), p, training=True).view(rows_, N)

            def clear():
                for q in params:
                    q.grad = None

            def ours():
                clear()
                y.backward(G, retain_graph=True)

            def theirs():
                clear()
                yt.backward(G, retain_graph=True)

            ms, tms = timed_alternating(ours, theirs, args.iters, args.warmup)
            clear()
            # the kernel sequence through the C ABI, word table written (zero-fill) or accumulated into
            need = max(lib.psg_bert_embed_ln_bwd_workspace_bytes(rows_, N), lib.psg_embed_scatter_workspace_bytes(rows_, N))
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            g2, dz = torch.empty_like(G), torch.empty(rows_, N, device=dev)
            outs = [torch.zeros_like(t) for t in tabs]
            j = torch.arange(rows_, device=dev)
            pk, pp = j // B, (j % B) * S + j // B

            def seq(acc):
                check(lib.psg_dropout_apply(ptr(G), N, ptr(g2), N, rows_, N, p, seed, 1.0 / (1.0 - p), dtype_code(dt), stream_ptr()), "dropout")
                check(lib.psg_bert_embed_ln_bwd(ptr(ids), ptr(tt), ptr(word), ptr(pos), ptr(typ), ptr(gamma), ptr(g2), N, ptr(dz), ptr(outs[3]),
                                                ptr(outs[4]), 0, B, S, N, V, P, 2, eps, dtype_code(dt), ptr(ws), need, stream_ptr()), "embed_ln_bwd")
                wk, wp = torch.sort(ids.view(-1), stable=True)
                tk, tp = torch.sort(tt.view(-1), stable=True)
                for out, key, perm, skip, a in ((outs[0], wk, wp, 0, acc), (outs[1], pk, pp, -1, 0), (outs[2], tk, tp, -1, 0)):
                    check(lib.psg_embed_scatter(ptr(dz), N, ptr(key), ptr(perm), ptr(out), rows_, N, out.shape[0], skip, a, ptr(ws), need,
                                                stream_ptr()), "embed_scatter")

            with torch.no_grad():
                k0, k1 = timed_alternating(lambda: seq(0), lambda: seq(1), args.iters, args.warmup)
            r = {"leg": "embed_bwd", "dtype": dn, "B": B, "S": S, "ms": ms, "torch_ms": tms, "speedup": tms / ms, "kernels_ms": k0,
                 "kernels_accumulate_ms": k1, "zero_fill_share": (k0 - k1) / k0}
            rows.append(r)
            print(f"{dn:5} {B:4d} {S:4d} {ms:12.3f} {tms:9.3f} {r['speedup']:7.2f} | {k0:10.3f} {k1:9.3f} {100 * r['zero_fill_share']:8.1f}%", flush=True)
            del y, yt, z


def train_legs(args, lib, dev, dts, rows):
    def counts():
        m, v, f = C.c_int64(), C.c_int64(), C.c_int64()
        lib.psg_attn_path_counts(C.byref(m), C.byref(v), C.byref(f))
        return m.value, v.value, f.value

    print(f"{'strategy':8} {'dtype':5} {'B':>4} {'S':>4} {'fwd+bwd ms':>10} {'TFLOP/s':>8} {'attn family':>12} | {'torch ms':>9} {'TFLOP/s':>8} {'speedup':>7}")
    for strat in args.strategies.split(","):
        enc = build(dev, finetune_strategy=strat, trainable=True, train_embeddings=True)      # (the keyword matters to 'full' only)
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
                    fl = train_flop_per_call(B, S, trained) + (B * S * 2.0 * 768 * 3 * 768 if strat == "full" else 0.0)
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
    ap.add_argument("--embed", action="store_true")
    ap.add_argument("--pairs", default="16x64,64x256", help="--embed: BxS pairs")
    args = ap.parse_args()
    from pokemon_sprite_generator_amd import _lib
    dev = torch.device("cuda", 0)
    lib = _lib.init(0)
    dts = {"bf16": torch.bfloat16, "fp32": torch.float32}
    rows = []
    if args.train or args.embed:
        (embed_legs if args.embed else train_legs)(args, lib, dev, dts, rows)
        if args.json:
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            with open(args.json, "w") as f:
                json.dump({"tool": "tools/text_encoder_bench.py " + ("--embed" if args.embed else "--train"), "iters": args.iters, "warmup": args.warmup, "rows": rows}, f, indent=1)
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
