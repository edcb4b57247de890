"""fp64 reference of BertEmbeddings' forward + backward (F.embedding x 3 with padding_idx, F.layer_norm, autograd) and the
comparator the GPU tests of psg_bert_embed_ln_bwd / psg_embed_scatter use.  tests/test_text_embed_grad_cpu.py checks the
reference against transformers' BertEmbeddings and the comparator against injected defects."""
import torch
import torch.nn.functional as F

from tests.util import maxrel

GRADS = ("dz", "word", "pos", "type", "gamma", "beta")
TABLES = ("word", "pos", "type")


def embed_reference(ids, tt, word, pos, typ, gamma, beta, eps, pad_id, dy, keep=None, p=0.0):
    """y = dropout(LN(word[ids] + type[tt] + pos[s])) and the gradients of sum(y * dy), all in fp64 from the given (already
    rounded) operands.  ids / tt: int64 [B, S] (tt None: zeros); dy: [B*S, N]; keep: bool [B*S, N] dropout mask or None.
    A row whose id is outside the table is taken out of the graph (zero dz, no contribution), as the kernels define it."""
    B, S = ids.shape
    V, N = word.shape
    dev = word.device
    tt = torch.zeros_like(ids) if tt is None else tt
    valid = ((ids >= 0) & (ids < V) & (tt >= 0) & (tt < typ.shape[0])).reshape(-1)
    w, ps, ty, g, b = (t.detach().double().requires_grad_(True) for t in (word, pos, typ, gamma, beta))
    idc, ttc = ids.clamp(0, V - 1), tt.clamp(0, typ.shape[0] - 1)
    z = F.embedding(idc, w, padding_idx=pad_id) + F.embedding(ttc, ty) + F.embedding(torch.arange(S, device=dev)[None].expand(B, S), ps)
    z = z.reshape(B * S, N)
    z.retain_grad()
    y = F.layer_norm(z, (N,), g, b, eps)
    if keep is not None:
        y = y * keep.double() / (1.0 - p)
    cot = dy.detach().double() * valid[:, None].double()
    y.backward(cot)
    return {"y": y.detach(), "dz": z.grad, "word": w.grad, "pos": ps.grad, "type": ty.grad, "gamma": g.grad, "beta": b.grad}


def zero_rows(ids, tt, V, P, T, pad_id):
    """Per table the bool mask of the rows that must be EXACTLY zero: rows no valid key names, the padding row, positions >= S."""
    B, S = ids.shape
    tt = torch.zeros_like(ids) if tt is None else tt
    valid = (ids >= 0) & (ids < V) & (tt >= 0) & (tt < T)
    zw = torch.ones(V, dtype=torch.bool)
    zw[ids[valid].cpu()] = False
    if 0 <= pad_id < V:
        zw[pad_id] = True
    zp = torch.ones(P, dtype=torch.bool)
    zp[:S] = ~valid.any(0).cpu()
    zt = torch.ones(T, dtype=torch.bool)
    zt[tt[valid].cpu()] = False
    return {"word": zw, "pos": zp, "type": zt}


def check_embed(got, ref, tol, zeros, names=GRADS):
    """Every tensor of `names` within max-rel `tol` of the fp64 reference, equal shapes, finite; the rows of `zeros` exactly
    zero.  Returns the errors; raises AssertionError with the tensor's name otherwise."""
    errs = {}
    for n in names:
        a, r = got[n], ref[n]
        assert tuple(a.shape) == tuple(r.shape), f"{n}: shape {tuple(a.shape)} vs {tuple(r.shape)}"
        assert a.dtype == torch.float32, f"{n}: dtype {a.dtype}"
        assert bool(torch.isfinite(a).all()), f"{n}: not finite"
        if n in TABLES:
            z = zeros[n].to(a.device)
            assert not bool(a[z].any()), f"{n}: a row that no key names (or the padding row, or a position >= S) is not exactly zero"
        errs[n] = maxrel(a, r)
        assert errs[n] < tol, f"{n}: max-rel {errs[n]:.3e} >= {tol}"
    return errs
