"""float64 reference of the attention core (forward and backward, key lengths, dropout), a per-element error bound for every
output of the launches - o, lse, delta, dq, dk, dv - and an integer-only restatement of the kernels' dropout mask (test
infrastructure, not a conftest; the style of tests/gn_ref.py, whose constants it shares through tests/gemm_ref.py).

The reference takes the operands as the kernel read them (bf16-representable for a bf16 launch), q / dout as [B, L, heads d]
and k / v as [B, S, heads d] views of any row stride, and computes per (sample, head) in fp64, with Se = kv_len[b] clamped to
[1, S] (S without key lengths) and keep the mask of keep_mask() (all ones at p = 0):

    s = scale q k^T                 P = softmax(s) over keys < Se      lse = log sum_{j < Se} exp(s)
    Pd = keep P / (1 - p)           O = Pd v                           delta = rowsum(dO O)
    dV = Pd^T dO                    dP = dO v^T                        g = keep dP / (1 - p)
    dS = P (g - delta)              dQ = scale dS k                    dK = scale dS^T q;    dK = dV = 0 for keys >= Se

Every bound has the shape of gn_ref.py:  |got - ref| <= r_out |ref| + C_ATTN 2^-24 M + extra,  r_out the output's own
rounding (gemm_ref.BF16_ROUND / F32_ROUND), M the sum of the absolute values of the terms added to form the element, each
weighted by the error it carries in units of 2^-24, and `extra` the analytic terms that are not summation order.  With
sq(n) = gemm_ref.c_acc(n) / 2^-24 the factor of a reduction over n terms:

  scores    an fp32 dot product over d: |ds_ij| <= 2^-24 sq(d) e_ij, e_ij = scale sum_c |q_ic| |k_jc|.
  P         P_ij = exp(s_ij - lse_i): d log P_ij = ds_ij - sum_k P_ik ds_ik, plus the roundings of s and lse themselves:
                RP_ij = sq(d) (e_ij + (P e)_i) + |s_ij| + |lse_i| + 2            (relative error of P_ij in units of 2^-24)
            and, outside the constant, the fast exponential: __expf(x) = v_exp_f32(x log2 e) rounds its argument
            (relative 2^-24, i.e. 2^-24 |x| in the result) and is itself good to 1 ulp; numerator and row sum both carry it:
                XP_ij = 2^-22 (1 + |s_ij - max_i|)                                (relative, absolute term P_ij XP_ij)
  o         M = sum_j Pd_ij |v_jc| (sq(S) + RP_ij),  extra = sum_j Pd_ij |v_jc| (XP_ij + RB)
            RB = 2^-8 on the bf16 MFMA family, whose P is rounded to bf16 (gemm_ref.BF16_ROUND: half an ulp of 8 bits) before it enters
            the second product; 0 elsewhere.
  lse       M = sq(d) (P e)_i + sq(S) + |lse_i| + |max_i|,  extra = sum_j P_ij XP_ij + 2^-22 (1 + |lse_i - max_i|) for the fast
            __logf (v_log_f32 times ln 2: 1 ulp of the logarithm plus the product's rounding).
  delta     the kernels form it from the STORED o (the launch's input, the reference's o rounded to the I/O dtype), so it is
            compared with rowsum(dO o_stored): M = sq(d) sum_c |dO_ic| |o_ic|.  A sample with masked keys (Se < S) instead
            gets sum_j Pd_ij dP_ij from the recomputed probabilities (psg_attn_bwd_varlen) - the exact delta:
            M = sum_j Pd_ij (|dP_ij| (sq(S) + RP_ij) + sq(d) a_ij), a_ij = sum_c |dO_ic| |v_jc|, extra = sum_j Pd_ij |dP_ij| XP_ij.
  dv        M = sum_i Pd_ij |dO_ic| (sq(L) + RP_ij),  extra = sum_i Pd_ij |dO_ic| (XP_ij + RB)
  dS        dS_ij = P_ij (g_ij - delta_i), to first order
                |d dS_ij| <= P_ij (|dP_ij / P_ij| |g_ij - delta_i| + |dg_ij| + |d delta_i|) + the subtraction's rounding:
                A_ij = P_ij (RP_ij |g_ij - delta_i| + sq(d) a_ij keep / (1 - p) + MD_i + |g_ij| + |delta_i|)      (units of 2^-24)
                X_ij = P_ij (XP_ij |g_ij - delta_i| + XD_i) + RB |dS_ij|                                       (absolute)
            MD_i / XD_i are delta's M / extra; where delta comes from the stored o, XD_i also holds what the exact delta
            loses by o's storage rounding: r_o sum_c |dO_ic| |o_ic| with r_o = 2^-8 (bf16) or 2^-24
            (fp32).  RB |dS| is the bf16 MFMA family's rounding of dS before the second product.
  dq        M = scale sum_j (A_ij + sq(S) |dS_ij|) |k_jc|,   extra = scale sum_j X_ij |k_jc|
  dk        M = scale sum_i (A_ij + sq(L) |dS_ij|) |q_ic|,   extra = scale sum_i X_ij |q_ic|

C_ATTN is not chosen but measured (tests/test_attn_ref_cpu.py::test_c_attn_is_four_times_torchs_own_error): over every case of
tests/attn_cases.py the smallest c at which torch's own fp32 restatement (matmul, softmax, autograd backward; for bf16 on
pre-rounded inputs, P and dS rounded to bf16 as the matrix-core kernels round them, outputs rounded to bf16) passes each
bound against this reference is C_TORCH; C_ATTN = 4 C_TORCH, one value for all outputs.  The margin covers a different
but fixed summation order, nothing else.  tests/golden/REPORT_attention_routes.txt lists the measured values per output.
"""
import math
import types

import numpy as np
import torch

from tests.drop_ref import drop_hash_pair, drop_thresh, mix32  # noqa: F401  (re-exported)
from tests.gemm_ref import A_FLOOR, BF16_ROUND, F32_ROUND, c_acc

TWO24 = 2.0 ** -24
EXP_REL = 2.0 ** -22
# largest smallest-passing c of torch's fp32 restatement over the case table (delta of an fp32 case: 0.0378; see the report).
# It is small because every reduction term of M already carries gemm_ref.c_acc's factor sqrt(max(1024, n)) = 32.
C_TORCH = 0.04
C_ATTN = 4.0 * C_TORCH

FWD_OUTPUTS = ("o", "lse")
BWD_OUTPUTS = ("delta", "dq", "dk", "dv")
OUTPUTS = FWD_OUTPUTS + BWD_OUTPUTS
MFMA_BF16, VALU, MFMA_F32 = 0, 1, 2


def _sq(n):
    return c_acc(n) / TWO24


# ------------------------------------------------------------------------------------------------- dropout mask restatement
# (mix32, drop_hash_pair, drop_thresh: tests/drop_ref.py, shared with the conv epilogue's masks in tests/gemm_ref.py)


def keep_mask(seed, BH, L, S, p):
    """The keep mask [BH, L, S] (bool) of an attention launch: element (bh, l, s) has index ((bh L + l) 2 ceil(S/2) + s); its
    pair index >> 1 is hashed once and key s takes the low (even s) or high (odd s) 16 bits, kept when >= thresh >> 16."""
    if not p > 0.0:
        return np.ones((BH, L, S), dtype=bool)
    hS = (S + 1) // 2
    rows = np.arange(BH * L, dtype=np.uint64).reshape(BH, L, 1)
    s = np.arange(S, dtype=np.uint64).reshape(1, 1, S)
    idx = rows * np.uint64(2 * hS) + s
    hh = drop_hash_pair(seed, idx >> np.uint64(1))
    half = np.where((idx & np.uint64(1)) == 1, hh >> np.uint64(16), hh & np.uint64(0xFFFF))
    return half >= np.uint64(drop_thresh(p) >> 16)


# ---------------------------------------------------------------------------------------------------------------- reference
def key_ends(kv_len, B, S):
    """Se per sample: kv_len clamped to [1, S], or S."""
    if kv_len is None:
        return [S] * B
    return [min(max(int(n), 1), S) for n in kv_len]


def _heads(t, H):
    B, N, HD = t.shape
    return t.detach().double().reshape(B, N, H, HD // H).permute(0, 2, 1, 3)       # [B, H, N, d]


def _rows(t):
    B, H, N, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, N, H * d)


def stored(t, bf16):
    """An fp64 tensor as the launch's I/O dtype stores it, back in fp64."""
    return (t.to(torch.bfloat16) if bf16 else t.to(torch.float32)).double()


def reference(q, k, v, heads, scale, family, bf16, kv_len=None, drop_p=0.0, seed=0, dout=None, causal=False):
    """fp64 reference and magnitudes (module docstring).  q, dout: [B, L, heads d]; k, v: [B, S, heads d]; kv_len: a sequence of B
    ints or None; family: MFMA_BF16 / VALU / MFMA_F32 of the launch (the bf16 MFMA extras); causal: key s takes part for query
    l iff s <= l (psg_attn_fwd_causal) - the set of live keys then differs from row to row, nothing else changes.  Returns a namespace with, per
    output name n, n (fp64), n_mag (M) and n_extra; o / dq [B, L, heads d], dk / dv [B, S, heads d], lse / delta [B, heads, L].
    o_st and lse_st are o and lse as stored (what the backward launch is given).  Backward outputs only with dout."""
    H = heads
    B, L, S = q.shape[0], q.shape[1], k.shape[1]
    d = q.shape[2] // H
    scale = float(torch.tensor(float(scale), dtype=torch.float32))
    Q, K, V = _heads(q, H), _heads(k, H), _heads(v, H)
    ends = key_ends(kv_len, B, S)
    live = torch.zeros(B, 1, 1, S, dtype=torch.bool, device=q.device)
    for b, e in enumerate(ends):
        live[b, :, :, :e] = True
    if causal:                                                                                   # [B, 1, L, S]
        live = live & torch.ones(L, S, dtype=torch.bool, device=q.device).tril()
    keep = torch.from_numpy(keep_mask(seed, B * H, L, S, drop_p)).to(q.device).reshape(B, H, L, S)
    kp = keep.double() / (1.0 - float(np.float32(drop_p)) if drop_p > 0.0 else 1.0)
    RB = BF16_ROUND if family == MFMA_BF16 else 0.0

    s = scale * (Q @ K.transpose(2, 3))
    e = scale * (Q.abs() @ K.abs().transpose(2, 3))
    sm = s.masked_fill(~live, -math.inf)
    mx = sm.amax(-1, keepdim=True)
    lse = torch.logsumexp(sm, -1, keepdim=True)
    P = torch.exp(sm - lse)
    Pd = P * kp
    Pe = (P * e).sum(-1, keepdim=True)
    RP = _sq(d) * (e + Pe) + s.abs() + lse.abs() + 2.0
    XP = EXP_REL * (1.0 + (s - mx).abs())
    RP, XP = RP.masked_fill(~live, 0.0), XP.masked_fill(~live, 0.0)

    r = types.SimpleNamespace(B=B, H=H, L=L, S=S, d=d, ends=ends, keep=keep)
    O = Pd @ V
    r.o = _rows(O)
    r.o_mag = _rows((Pd * (_sq(S) + RP)) @ V.abs())
    r.o_extra = _rows((Pd * (XP + RB)) @ V.abs())
    r.lse = lse.squeeze(-1)
    r.lse_mag = (_sq(d) * Pe + _sq(S) + lse.abs() + mx.abs()).squeeze(-1)
    r.lse_extra = ((P * XP).sum(-1, keepdim=True) + EXP_REL * (1.0 + (lse - mx).abs())).squeeze(-1)
    r.o_st, r.lse_st = stored(r.o, bf16), r.lse.float().double()
    if dout is None:
        return r

    G = _heads(dout, H)
    Ost = _heads(r.o_st, H)
    dP = G @ V.transpose(2, 3)
    a = G.abs() @ V.abs().transpose(2, 3)
    g = dP * kp
    delta = (G * O).sum(-1, keepdim=True)
    direct = torch.tensor([e_ < S for e_ in ends], device=q.device).reshape(B, 1, 1, 1) if kv_len is not None \
        else torch.zeros(B, 1, 1, 1, dtype=torch.bool, device=q.device)
    # delta as the launch forms it, its M and extra; XD adds what the exact delta loses where the stored o is used
    d_st = (G * Ost).sum(-1, keepdim=True)
    m_st = _sq(d) * (G.abs() * Ost.abs()).sum(-1, keepdim=True)
    x_lost = (BF16_ROUND if bf16 else TWO24) * (G.abs() * O.abs()).sum(-1, keepdim=True)
    m_dir = (Pd * (dP.abs() * (_sq(S) + RP) + _sq(d) * a)).sum(-1, keepdim=True)
    x_dir = (Pd * dP.abs() * XP).sum(-1, keepdim=True)
    r.delta = torch.where(direct, delta, d_st).squeeze(-1)
    MD = torch.where(direct, m_dir, m_st)
    r.delta_mag = MD.squeeze(-1)
    r.delta_extra = torch.where(direct, x_dir, torch.zeros_like(x_dir)).squeeze(-1)
    XD = torch.where(direct, x_dir, x_lost)

    dS = P * (g - delta)
    A = P * (RP * (g - delta).abs() + _sq(d) * a * kp + MD + g.abs() + delta.abs())
    X = P * (XP * (g - delta).abs() + XD) + RB * dS.abs()
    r.dv = _rows(Pd.transpose(2, 3) @ G)
    r.dv_mag = _rows((Pd * (_sq(L) + RP)).transpose(2, 3) @ G.abs())
    r.dv_extra = _rows((Pd * (XP + RB)).transpose(2, 3) @ G.abs())
    r.dq = _rows(scale * (dS @ K))
    r.dq_mag = _rows(scale * ((A + _sq(S) * dS.abs()) @ K.abs()))
    r.dq_extra = _rows(scale * (X @ K.abs()))
    r.dk = _rows(scale * (dS.transpose(2, 3) @ Q))
    r.dk_mag = _rows(scale * ((A + _sq(L) * dS.abs()).transpose(2, 3) @ Q.abs()))
    r.dk_extra = _rows(scale * (X.transpose(2, 3) @ Q.abs()))
    return r


# --------------------------------------------------------------------------------------------------------------- comparator
def _parts(got, ref, out_dtype, extra):
    g = got.detach().to(device=ref.device, dtype=torch.float64)
    assert g.shape == ref.shape, f"shape {tuple(g.shape)} vs reference {tuple(ref.shape)}"
    fixed = ref.abs() * (BF16_ROUND if out_dtype == torch.bfloat16 else F32_ROUND) + A_FLOOR
    if extra is not None:
        fixed = fixed + extra
    return g, (g - ref).abs(), fixed


def check(got, ref, mag, out_dtype, what, extra=None, c=None):
    """Assert |got - ref| <= r_out |ref| + c 2^-24 mag + extra + A_FLOOR for every element; return (worst err / bound, its index).
    A NaN in got fails.  The message names the worst element."""
    c = C_ATTN if c is None else c
    g, err, fixed = _parts(got, ref, out_dtype, extra)
    bound = fixed + c * TWO24 * mag
    ratio = err / bound
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    worst = float(ratio.max())
    if not worst <= 1.0:
        i = int(ratio.argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
        nbad = int((ratio > 1.0).sum())
        raise AssertionError(f"{what}: {nbad} of {ratio.numel()} elements out of bound; worst at {idx}: got {float(g.reshape(-1)[i]):.9g}, "
                             f"ref {float(ref.reshape(-1)[i]):.9g}, |err| {float(err.reshape(-1)[i]):.3g} > bound "
                             f"{float(bound.reshape(-1)[i]):.3g} (err/bound {worst:.3g})")
    return worst


def smallest_c(got, ref, mag, out_dtype, extra=None):
    """The smallest c at which check() passes: max over the elements of (err - r_out |ref| - extra - A_FLOOR) / (2^-24 mag)."""
    _, err, fixed = _parts(got, ref, out_dtype, extra)
    over = (err - fixed).clamp_min(0.0)
    c = torch.where(over > 0, over / (TWO24 * mag), torch.zeros_like(over))
    c = torch.where(torch.isnan(c), torch.full_like(c, math.inf), c)
    return float(c.max())


def out_dtype(name, dtype):
    """The type an output is stored in: o, dq, dk, dv in the launch's, lse and delta in fp32."""
    return dtype if name in ("o", "dq", "dk", "dv") else torch.float32


def check_all(got, r, dtype, what, names=None, c=None):
    """check() for every output in `got` (a dict name -> tensor); returns name -> worst err / bound."""
    res = {}
    for name in (names or [n for n in OUTPUTS if n in got]):
        res[name] = check(got[name], getattr(r, name), getattr(r, name + "_mag"), out_dtype(name, dtype), f"{what} {name}",
                          extra=getattr(r, name + "_extra"), c=c)
    return res
