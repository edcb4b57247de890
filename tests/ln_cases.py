"""The case table of the text-encoder row-kernel tests (psg_layernorm, psg_layernorm_bwd, psg_bert_embed_ln,
psg_bert_embed_ln_bwd, psg_embed_scatter): widths, row counts, dtype pairs, strides, data kinds and the key layouts of the
scatter (test infrastructure, not a conftest).  tests/test_ln_ref_cpu.py checks that the table meets its own conditions (every
CPL instantiation at both edges, every dtype pair with and without a residual, the scatter's segment loop re-entered);
tests/test_ln_kernels_gpu.py launches it."""
import zlib

import torch


def h(shape, tag, scale=1.0):
    """Uniform (-scale, scale) fp32 values from torch's CPU generator, seeded by the tag (the same on every host)."""
    g = torch.Generator().manual_seed(zlib.crc32(tag.encode()))
    return (torch.rand(tuple(shape), generator=g) * 2.0 - 1.0) * scale

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
PAIRS = [("f32", "f32"), ("bf16", "bf16"), ("bf16", "f32"), ("f32", "bf16")]      # (x, y) of the forward = (x, dy) of the backward

# both edges of every CPL instantiation (16-byte chunks per lane, CPL = ceil(N / 8 / 64)): N = 512 (c - 1) + 8 puts exactly one
# chunk (lane 0) into a lane's last slot, N = 512 c fills it; N = 8 leaves lane 0 alone; 200 and 768 are partial first slots
CPL_EDGES = [8, 512] + [n for c in range(2, 9) for n in (512 * (c - 1) + 8, 512 * c)]
WIDTHS = CPL_EDGES + [200, 768]
ROWS_ALL_N = 21                       # backward: wave 0 full, wave 1 partial, waves 2 and 3 empty; forward: 5 full workgroups + 1 row
ROWS_MORE = (1, 67, 150)              # 67: a second backward workgroup of 3 rows; 150: the geometry check (rows 37..40)
WIDTHS_MORE = (8, 520, 768, 1544, 4096)
GEOMETRY_ROWS = (37, 41)              # rows [37:41] of the 150-row launch against a 4-row launch of the same rows

KINDS = ("plain", "offset", "const", "tiny")
STRIDES = ("contiguous", "padded", "class")
CLASS_TOKENS = 50                     # the class-row view x[:, 0, :] of a [rows, 50, N] tensor: ldx = 50 N
CLASS_MAX_ELEMS = 1 << 23             # ... where that tensor stays below 8 Mi elements; wider cases run padded instead


def shapes():
    """Every (N, rows) of the LayerNorm table."""
    return [(N, ROWS_ALL_N) for N in WIDTHS] + [(N, r) for N in WIDTHS_MORE for r in ROWS_MORE]


def variants(N, rows):
    """The eight launches of a shape: every dtype pair with and without a residual; stride, data kind, eps and accumulate
    rotate with the shape so that every pair meets every kind and every stride somewhere in the table."""
    s = shapes().index((N, rows))
    out = []
    for i, (xd, od) in enumerate(PAIRS):
        for res in (0, 1):
            j = 2 * i + res
            kind = KINDS[(s + j) % 4]
            stride = STRIDES[(s // 4 + s + j + res) % 3]
            if stride == "class" and rows * CLASS_TOKENS * N > CLASS_MAX_ELEMS:
                stride = "padded"
            eps = {"const": 1e-12, "tiny": 1e-5}.get(kind, 1e-12 if (s + j // 2) % 2 else 1e-5)
            out.append(dict(N=N, rows=rows, xd=xd, od=od, res=bool(res), kind=kind, stride=stride, eps=eps, accumulate=bool((s + i + res) % 2)))
    return out


def all_variants():
    return [v for N, rows in shapes() for v in variants(N, rows)]


def vid(v):
    return f"N{v['N']}-r{v['rows']}-{v['xd']}>{v['od']}{'-res' if v['res'] else ''}-{v['kind']}-{v['stride']}-eps{v['eps']:g}"


def const_row(rows):
    return rows // 2


def _q(t, dname):
    return t.to(DTYPES[dname]).float()


def _data(shape, tag, kind, dname, res_part):
    """One operand of z = x + r.  plain: 3 u + 0.5; offset: spread 1 around 1024 (bf16: spread 16 - its spacing at 1024 is 8, a
    spread of 1 would be a constant row); tiny: around 1e-4.  With a residual x carries the level and r spreads around 0."""
    u = h(shape, tag)
    if kind in ("plain", "const"):
        return 2.0 * u if res_part else 3.0 * u + 0.5
    if kind == "offset":
        w = 16.0 if dname == "bf16" else 1.0
        return 0.5 * w * u if res_part else 1024.0 + w * u
    return 1e-4 * (0.5 * u if res_part else u + 0.5)


def operands(v):
    """CPU fp32 tensors holding the values the launch reads (x, r, dy representable in their dtypes): x, r (or None), dy
    [rows, N], gamma, beta [N], prefill (dgamma0, dbeta0)."""
    N, rows = v["N"], v["rows"]
    tag = f"ln.{N}.{rows}.{v['xd']}.{v['od']}.{int(v['res'])}"
    x = _q(_data((rows, N), tag + ".x", v["kind"], v["xd"], False), v["xd"])
    r = _q(_data((rows, N), tag + ".r", v["kind"], v["xd"], True), v["xd"]) if v["res"] else None
    if v["kind"] == "const":                         # one row of equal values (x + r too) among plain rows
        x[const_row(rows)] = 0.75
        if r is not None:
            r[const_row(rows)] = -0.25
    return dict(x=x, r=r, dy=_q(h((rows, N), tag + ".dy"), v["od"]), gamma=1.0 + h((N,), tag + ".g", 0.3), beta=h((N,), tag + ".b", 0.2),
                prefill=(h((N,), tag + ".pg", 3.0), h((N,), tag + ".pb", 3.0)))


def strides(v):
    """name -> row stride of x, r, y, dy, dz.  padded: N + 8 k with a different k per operand; class: ldx = 50 N."""
    N = v["N"]
    names = ("x", "r", "y", "dy", "dz")
    if v["stride"] == "padded":
        return {n: N + 8 * k for k, n in enumerate(names, start=1)}
    ld = {n: N for n in names}
    if v["stride"] == "class":
        ld["x"] = CLASS_TOKENS * N
    return ld


# ------------------------------------------------------------------------------------------------------------ embeddings
EMBED_V, EMBED_T = 50, 2
EMBED_SHAPES = [(N, 3, 7) for N in CPL_EDGES] + [(N, 5, 67) for N in (200, 768, 1544)]


def embed_variants():
    """Per shape and dtype (y's and dy's) a clean launch and one with ids outside the tables: an id == V, an id == -1 and (with
    token types) a type id == T, in separate rows of separate samples.  Token types alternate; ldy and lddy are padded."""
    out = []
    for s, (N, B, S) in enumerate(EMBED_SHAPES):
        for d, dname in enumerate(DTYPES):
            for bad in (False, True):
                out.append(dict(N=N, B=B, S=S, dname=dname, typed=bool((s + d + bad) % 2), bad=bad, ldy=N + 8, lddy=N + 24,
                                eps=1e-12 if (s + d) % 2 else 1e-5, accumulate=bool((s + bad) % 2)))
    return out


def embed_vid(v):
    return f"N{v['N']}-b{v['B']}s{v['S']}-{v['dname']}{'-typed' if v['typed'] else ''}{'-bad' if v['bad'] else ''}"


def embed_bad_rows(v):
    """(flat row, what) of the rows a bad launch takes out: (b, s) = (0, 2) id == V, (1, 4) id == -1, (2, 5) type id == T."""
    S = v["S"]
    rows = [(0 * S + 2, "id == V"), (1 * S + 4, "id == -1")]
    return rows + ([(2 * S + 5, "type == T")] if v["typed"] else [])


def embed_operands(v):
    N, B, S = v["N"], v["B"], v["S"]
    V, T, P = EMBED_V, EMBED_T, S + 3
    tag = f"emb.{N}.{B}.{S}.{v['dname']}"
    g = torch.Generator().manual_seed(1000 * N + 10 * B + S)
    ids = torch.randint(0, V, (B, S), generator=g)
    tt = torch.randint(0, T, (B, S), generator=g) if v["typed"] else None
    if v["bad"]:
        f = ids.view(-1)
        f[embed_bad_rows(v)[0][0]], f[embed_bad_rows(v)[1][0]] = V, -1
        if tt is not None:
            tt.view(-1)[embed_bad_rows(v)[2][0]] = T
    return dict(ids=ids, tt=tt, word=h((V, N), tag + ".w", 0.05), pos=h((P, N), tag + ".p", 0.05), typ=h((T, N), tag + ".t", 0.05),
                gamma=1.0 + h((N,), tag + ".g", 0.3), beta=h((N,), tag + ".b", 0.2), dy=_q(h((B * S, N), tag + ".dy"), v["dname"]),
                prefill=(h((N,), tag + ".pg", 3.0), h((N,), tag + ".pb", 3.0)))


# --------------------------------------------------------------------------------------------------------------- scatter
SCATTER_WIDTHS = (8, 200, 256, 264, 768, 4096)      # 264: a second slab of 8 columns; 200: a partial slab
SCATTER_V = 40
HOT = 7


def scatter_layouts(chunk):
    """name -> (segments [(key, count)] in sorted-position order, skip_key).  Keys ascend (the launch's contract is that equal
    keys are adjacent); negative keys and keys >= V are the invalid ones.  With chunk = 32:
      long   positions 16 .. 16 + 9 chunk + 2 hold HOT: a run of 9 chunk + 3 that starts in the middle of chunk 0 and reaches 9
             later chunk starts (embed_scatter_sum_kernel's loop runs 3 times: 4 + 4 + 1 segments); chunk start 0 holds a
             negative key, the last chunk start a key >= V; the skip key's run stays inside chunk 0
      edges  a run that ends on a chunk boundary, a run of exactly one chunk on a boundary, a run that starts on one and spills,
             the skip key over two chunk starts, two whole chunks of one key, a negative chunk start, keys >= V over a chunk start
    and the small ones: `rows` positions, one negative, one run through the rest, two keys >= V where they fit."""
    V = SCATTER_V
    lay = {
        "long": ([(-1, 3), (0, 5), (1, 2), (2, 1), (3, chunk // 2 - 11), (HOT, 9 * chunk + 3), (9, 4), (11, 1), (12, chunk - chunk // 2 - 8), (V + 3, 3)], 0),
        "edges": ([(-3, 2), (1, chunk - 14), (2, 12), (3, chunk), (4, chunk + 5), (5, 2 * chunk + 6), (6, 1), (8, chunk - 12), (9, chunk + 1),
                   (10, chunk - 1), (12, 2 * chunk), (V, 3)], 5),
        "r1": ([(4, 1)], -1),
        "r5": ([(-1, 1), (1, 2), (3, 1), (V, 1)], -1),
    }
    for rows in (chunk - 1, chunk, chunk + 1):
        tail = [(2, rows - 4)] if rows > chunk else [(2, rows - 6), (V + 1, 2)]        # chunk + 1: the run spills one position
        lay[f"r{rows}"] = ([(-1, 1), (1, 3)] + tail, 1 if rows == chunk else -1)
    return lay


def scatter_keys(segments):
    return torch.tensor([k for k, n in segments for _ in range(n)], dtype=torch.int64)


def scatter_cases(chunk):
    """(layout, N, lddz): the two long layouts at every width and both strides, the small ones with the stride alternating."""
    out = []
    for i, N in enumerate(SCATTER_WIDTHS):
        for name in ("long", "edges"):
            out += [(name, N, N), (name, N, N + 8)]
        for j, name in enumerate(n for n in scatter_layouts(chunk) if n.startswith("r")):
            out.append((name, N, N + 8 * ((i + j) % 2)))
    return out


def scatter_operands(name, N, chunk, integer):
    """key, perm (a permutation of the dz rows), dz [rows, N] (random, or integers with |v| <= 64), prefill [V + 1, N], V, skip."""
    segments, skip = scatter_layouts(chunk)[name]
    key = scatter_keys(segments)
    rows = key.numel()
    g = torch.Generator().manual_seed(17 * N + rows)
    perm = torch.randperm(rows, generator=g)
    if integer:
        dz = torch.randint(-64, 65, (rows, N), generator=g).float()
        pre = torch.randint(-64, 65, (SCATTER_V, N), generator=g).float()
    else:
        dz, pre = h((rows, N), f"sc.{name}.{N}.dz"), h((SCATTER_V, N), f"sc.{name}.{N}.pre", 3.0)
    return dict(key=key, perm=perm, dz=dz, prefill=pre, V=SCATTER_V, skip=skip, rows=rows)


def later_chunk_starts(key, chunk, k):
    """How many chunk starts after its first chunk the run of key k reaches (the segments embed_scatter_sum_kernel collects)."""
    pos = (key == k).nonzero().view(-1)
    first = int(pos[0])
    return sum(1 for c in range((first // chunk + 1) * chunk, key.numel(), chunk) if int(key[c]) == k)


# ----------------------------------------------------------------------------------------------- what the table launches
NULL_WIDTHS = [8] + [512 * (c - 1) + 8 for c in range(2, 9)]       # one width per CPL for the NULL-output (PG = false) launches


def null_output_variants():
    """The launches repeated with dgamma only, dbeta only and neither (the PG = false instantiation): every dtype pair with and
    without a residual at one width per CPL."""
    return [v for N in NULL_WIDTHS for v in variants(N, ROWS_ALL_N)]


def embed_null_output_variants():
    return [e for e in embed_variants() if e["N"] in NULL_WIDTHS and not e["bad"]]


def instantiations():
    """The kernel instantiations the table names: ("layernorm", x, y, CPL, RES), ("layernorm_bwd", x, dy, CPL, PG, residual),
    ("embed_ln", y, CPL), ("embed_ln_bwd", dy, CPL, PG)."""
    def cpl(N):
        return (N // 8 + 63) // 64
    out = set()
    for v in all_variants():
        out.add(("layernorm", v["xd"], v["od"], cpl(v["N"]), v["res"]))
        out.add(("layernorm_bwd", v["xd"], v["od"], cpl(v["N"]), True, v["res"]))
    for v in null_output_variants():
        out.add(("layernorm_bwd", v["xd"], v["od"], cpl(v["N"]), False, v["res"]))
    for e in embed_variants():
        out.add(("embed_ln", e["dname"], cpl(e["N"])))
        out.add(("embed_ln_bwd", e["dname"], cpl(e["N"]), True))
    for e in embed_null_output_variants():
        out.add(("embed_ln_bwd", e["dname"], cpl(e["N"]), False))
    return out
