"""CPU checks of tests/attn_ref.py and tests/attn_cases.py: the fp64 attention reference equals torch's, its per-element bounds
accept a correct fp32 / bf16 result (torch's own matmul / softmax / autograd, and a formula model that rounds P and dS as the
matrix-core kernels do) on every case of the table and reject eleven subtle kernel defects where they matter; the constant of
the bounds is what torch's own error measures; the integer restatement of the dropout mask reproduces known answers; and,
through psg_attn_route, the table takes the routes it stores and reaches every launch variant a sweep of shapes reaches."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import attn_cases as K
from tests import attn_ref as R

REPORT = os.environ.get("PSG_ATTN_REPORT")      # optional: append the measured figures to this file
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _report(line):
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def _store(t, name, dname):
    return t.to(K.DTYPES[dname]) if name in ("o", "dq", "dk", "dv") else t


def _heads(t, H):
    B, N, HD = t.shape
    return t.reshape(B, N, H, HD // H).permute(0, 2, 1, 3)


def _rows(t):
    B, H, N, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, N, H * d)


# ------------------------------------------------------------------------------------------------- correct implementations
class _RoundST(torch.autograd.Function):
    """bf16 rounding in the forward, identity in the backward."""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).float()

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundGrad(torch.autograd.Function):
    """identity in the forward, the gradient rounded to bf16 in the backward."""

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).float()


def _live(ref):
    live = torch.zeros(ref.B, 1, 1, ref.S, dtype=torch.bool)
    for b, e in enumerate(ref.ends):
        live[b, :, :, :e] = True
    return live


def torch_restatement(ops, dname, family, ref, drop_p):
    """torch's own fp32 matmul, softmax and autograd backward on the operands; on the bf16 MFMA family P and dS are rounded to
    bf16 before the second products, as the kernels round them.  Outputs stored like the launch's."""
    H, S = ref.H, ref.S
    rnd = family == R.MFMA_BF16
    q, k, v = (ops[n].clone().requires_grad_(True) for n in ("q", "k", "v"))
    Q, Kk, V, G = _heads(q, H), _heads(k, H), _heads(v, H), _heads(ops["dout"], H)
    live = _live(ref)
    s = (Q @ Kk.transpose(2, 3)) * R.stored(torch.tensor(ops["scale"]), False).float()
    if rnd:
        s = _RoundGrad.apply(s)
    s = s.masked_fill(~live, -math.inf)
    lse = torch.logsumexp(s, -1)
    P = torch.softmax(s, -1)
    kp = ref.keep.float() / (1.0 - np.float32(drop_p)) if drop_p > 0 else torch.ones_like(P)
    Pd = P * kp
    O = (_RoundST.apply(Pd) if rnd else Pd) @ V
    O.backward(G)
    direct = torch.tensor([e < S for e in ref.ends]).reshape(-1, 1, 1)
    d_st = (G * _heads(ref.o_st.float(), H)).sum(-1)
    d_dir = (Pd.detach() * (G @ V.detach().transpose(2, 3))).sum(-1)
    out = dict(o=_rows(O.detach()), lse=lse.detach(), delta=torch.where(direct, d_dir, d_st), dq=q.grad, dk=k.grad, dv=v.grad)
    return {n: _store(t, n, dname) for n, t in out.items()}


MUTATIONS = ("odd_last_key", "pad_key_zero", "lse_no_max", "dq_no_scale", "delta_neighbour", "dk_partial_missing", "last_qtile_unwritten",
             "head_stride", "mask_row_base", "masked_dkv_nonzero", "slice16")


def mutation_applies(mut, case, varlen, ref, drop_p, route):
    name, dname, d, L, S, over, i = case
    rt = dict(zip(K.ROUTE_FIELDS, route))
    if mut == "odd_last_key":
        return S % 2 == 1 and S > 1 and any(e == S for e in ref.ends)
    if mut == "pad_key_zero":
        return S % 32 != 0
    if mut == "delta_neighbour":
        return L > 1
    if mut == "dk_partial_missing":
        return rt["QW"] > 1
    if mut == "last_qtile_unwritten":
        return L % 32 != 0
    if mut == "head_stride":
        return K.layout(case)[0]["q"][0] != K.HEADS * d and L > 1
    if mut == "mask_row_base":
        return drop_p > 0 and S % 2 == 1 and L > 1
    if mut == "masked_dkv_nonzero":
        return varlen and any(e < S for e in ref.ends)
    if mut == "slice16":
        return d >= 32
    return True


def formula_model(ops, case, family, ref, drop_p, seed, route, mut=None):
    """The forward and the backward written out in fp32 torch operations the way the kernels compute them (P from the stored
    lse, delta from the stored o or, for a sample with masked keys, from the recomputed probabilities; on the bf16 MFMA family P
    and scale dS rounded to bf16) - a correct implementation when mut is None, and with `mut` one of MUTATIONS that defect."""
    name, dname, d, L, S, over, i = case
    H, B = ref.H, ref.B
    rt = dict(zip(K.ROUTE_FIELDS, route))
    rnd = family == R.MFMA_BF16
    r16 = (lambda t: t.to(torch.bfloat16).float()) if rnd else (lambda t: t)
    scale = R.stored(torch.tensor(ops["scale"]), False).float()
    q = ops["q"]
    if mut == "head_stride":         # rows of q read at stride heads d out of a buffer whose rows are ld apart
        ld, off = K.layout(case)[0]["q"]
        buf = torch.zeros(B, L, ld)
        buf[:, :, off:off + H * d] = q
        flat = buf.reshape(B, L * ld)
        q = torch.stack([flat[:, off + l * H * d: off + (l + 1) * H * d] for l in range(L)], 1)
    Q, Kk, V, G = _heads(q, H), _heads(ops["k"], H), _heads(ops["v"], H), _heads(ops["dout"], H)
    live = _live(ref).clone()
    if mut == "odd_last_key":
        for b, e in enumerate(ref.ends):
            if e == S:
                live[b, :, :, S - 1] = False
    s = scale * (Q @ Kk.transpose(2, 3))
    if mut == "slice16":
        c0 = 16 * ((d // 16) // 2)
        s = s - scale * (Q[..., c0:c0 + 16] @ Kk[..., c0:c0 + 16].transpose(2, 3))
    keep = ref.keep
    if mut == "mask_row_base":
        hh = R.drop_hash_pair(seed, (np.arange(B * H * L, dtype=np.uint64).reshape(-1, 1) * np.uint64(S) + np.arange(S, dtype=np.uint64)) >> np.uint64(1))
        idx = np.arange(B * H * L, dtype=np.uint64).reshape(-1, 1) * np.uint64(S) + np.arange(S, dtype=np.uint64)
        half = np.where((idx & np.uint64(1)) == 1, hh >> np.uint64(16), hh & np.uint64(0xFFFF))
        keep = torch.from_numpy(half >= np.uint64(R.drop_thresh(drop_p) >> 16)).reshape(B, H, L, S)
    kp = keep.float() / (1.0 - np.float32(drop_p)) if drop_p > 0 else torch.ones(B, H, L, S)
    # forward: online-softmax form
    sm = s.masked_fill(~live, -math.inf)
    mx = sm.amax(-1, keepdim=True)
    ex = torch.exp(sm - mx)
    tot = ex.sum(-1, keepdim=True)
    if mut == "pad_key_zero":
        tot = tot + torch.exp(-mx)
    O = (r16(ex * kp) @ V) / tot
    lse = (torch.log(tot) if mut == "lse_no_max" else mx + torch.log(tot)).squeeze(-1)
    if mut == "last_qtile_unwritten":
        O = O.clone()
        O[:, :, L - L % 32:] = 0.0
    # backward from the stored lse and o
    lse_st = ref.lse_st.float().unsqueeze(-1)
    if mut == "pad_key_zero":
        lse_st = torch.logaddexp(lse_st, torch.zeros(()))
    P = torch.exp(sm - lse_st)
    Pd = P * kp
    dP = G @ V.transpose(2, 3)
    g = dP * kp
    direct = torch.tensor([e < S for e in ref.ends]).reshape(-1, 1, 1, 1)
    delta = torch.where(direct, (Pd * dP).sum(-1, keepdim=True), (G * _heads(ref.o_st.float(), H)).sum(-1, keepdim=True))
    dl = torch.roll(delta, 1, 2) if mut == "delta_neighbour" else delta
    dS = P * (g - dl)
    dSs = r16(dS * scale)
    dQ = dSs @ Kk
    if mut == "dq_no_scale":
        dQ = r16(dS) @ Kk
    dSk = dSs
    if mut == "dk_partial_missing":          # the query tiles of the last query group never reach dK
        dSk = dSs.clone()
        for qt in range(rt["QW"] - 1, (L + 31) // 32, rt["QW"]):
            dSk[:, :, 32 * qt:32 * qt + 32] = 0.0
    dK = dSk.transpose(2, 3) @ Q
    dV = r16(Pd).transpose(2, 3) @ G
    if mut == "masked_dkv_nonzero":          # the rows of masked keys computed like live ones instead of stored as zeros
        dV = dV + r16(torch.exp(s - lse_st) * kp * (~live)).transpose(2, 3) @ G
    out = dict(o=_rows(O), lse=lse, delta=delta.squeeze(-1), dq=_rows(dQ), dk=_rows(dK), dv=_rows(dV))
    return {n: _store(t, n, dname) for n, t in out.items()}


# ------------------------------------------------------------------------------------------------------ per-case fixture
def _runs(case):
    """The two launch pairs of a case - plain (psg_attn_fwd / psg_attn_bwd) and with key lengths (psg_attn_fwd_varlen_train /
    psg_attn_bwd_varlen) - with operands, the backward route and the fp64 reference."""
    name, dname, d, L, S, over, i = case
    var = K.variations(case)
    ops = K.operands(case)
    p = K.DROP_P if var["drop"] else 0.0
    out = []
    for varlen, pb in ((False, K.BWD), (True, K.BWD_VARLEN)):
        route = K.expected_route(case, pb)
        ref = R.reference(ops["q"], ops["k"], ops["v"], K.HEADS, ops["scale"], route[0], dname == "bf16", kv_len=var["kv_len"] if varlen else None,
                          drop_p=p, seed=var["seed"], dout=ops["dout"])
        out.append((varlen, route, ops, ref, p, var["seed"]))
    return out


@pytest.fixture(scope="module", params=K.CASES, ids=K.IDS)
def case(request):
    return request.param, _runs(request.param)


_measured = {}       # case name -> {(dname, output): smallest c of torch's restatement}


def _measure(case, runs=None):
    if case[0] not in _measured:
        m = {}
        for varlen, route, ops, ref, p, seed in (runs or _runs(case)):
            got = torch_restatement(ops, case[1], route[0], ref, p)
            for name in R.OUTPUTS:
                c = R.smallest_c(got[name], getattr(ref, name), getattr(ref, name + "_mag"), R.out_dtype(name, K.DTYPES[case[1]]),
                                 extra=getattr(ref, name + "_extra"))
                m[(case[1], name)] = max(m.get((case[1], name), 0.0), c)
        _measured[case[0]] = m
    return _measured[case[0]]


# ------------------------------------------------------------------------------------------------------ reference == torch
def test_reference_matches_torch_fp64():
    g = torch.Generator().manual_seed(7)
    B, H, L, S, d = 3, 3, 11, 13, 8
    qb = torch.randn(B, L, H * d + 8, dtype=torch.float64, generator=g)
    q = qb[..., 4:4 + H * d]                                                       # a strided view
    k, v = torch.randn(B, S, H * d, dtype=torch.float64, generator=g), torch.randn(B, S, H * d, dtype=torch.float64, generator=g)
    do = torch.randn(B, L, H * d, dtype=torch.float64, generator=g)
    kv = [0, 5, 20]
    p, seed = 0.3, 99
    r = R.reference(q, k, v, H, 0.37, R.VALU, False, kv_len=kv, drop_p=p, seed=seed, dout=do)
    assert r.ends == [1, 5, 13]
    qn, kn, vn = (t.clone().contiguous().requires_grad_(True) for t in (q, k, v))
    sc = float(torch.tensor(0.37, dtype=torch.float32))
    s = sc * (_heads(qn, H) @ _heads(kn, H).transpose(2, 3))
    live = torch.zeros(B, 1, 1, S, dtype=torch.bool)
    for b, e in enumerate(r.ends):
        live[b, :, :, :e] = True
    s = s.masked_fill(~live, -math.inf)
    keep = torch.from_numpy(R.keep_mask(seed, B * H, L, S, p)).reshape(B, H, L, S)
    O = (torch.softmax(s, -1) * keep / (1.0 - float(np.float32(p)))) @ _heads(vn, H)
    O.backward(_heads(do, H))
    for a, b, what in ((r.o, _rows(O.detach()), "o"), (r.lse, torch.logsumexp(s, -1).detach(), "lse"), (r.dq, qn.grad, "dq"), (r.dk, kn.grad, "dk"),
                       (r.dv, vn.grad, "dv")):
        assert float((a - b).abs().max() / b.abs().max()) < 1e-12, what
    assert float(r.dk[0, 1:].abs().max()) == 0.0 and float(r.dv[1, 5:].abs().max()) == 0.0      # masked keys
    # delta: from the stored o at full length, the exact one for samples with masked keys
    exact = (_heads(do, H) * O.detach()).sum(-1)
    assert float((r.delta[:2] - exact[:2]).abs().max()) < 1e-12
    assert float((r.delta[2] - (_heads(do, H) * _heads(r.o_st, H)).sum(-1)[2]).abs().max()) < 1e-12
    assert all(bool((getattr(r, n + "_mag") >= 0).all()) and bool((getattr(r, n + "_extra") >= 0).all()) for n in R.OUTPUTS)


# ---------------------------------------------------------------------------------------- (a) accepts a correct result
def test_bound_accepts_torch_restatement(case):
    cs, runs = case
    for varlen, route, ops, ref, p, seed in runs:
        R.check_all(torch_restatement(ops, cs[1], route[0], ref, p), ref, K.DTYPES[cs[1]], f"{cs[0]} varlen={varlen} torch", c=R.C_TORCH)
    for (dname, name), c in sorted(_measure(cs, runs).items()):
        _report(f"torch_c {cs[0]} {dname} {name} {c:.4g}")


def test_bound_accepts_formula_model(case):
    """The unmutated model the defects below start from - the bf16 emulation on the bf16 MFMA family - is within the bounds at
    C_ATTN."""
    cs, runs = case
    for varlen, route, ops, ref, p, seed in runs:
        ratios = R.check_all(formula_model(ops, cs, route[0], ref, p, seed, route), ref, K.DTYPES[cs[1]], f"{cs[0]} varlen={varlen} model")
        _report(f"model {cs[0]} {cs[1]} family{route[0]} " + " ".join(f"{n}={v:.3g}" for n, v in ratios.items()))


def test_c_attn_is_four_times_torchs_own_error():
    """C_ATTN = 4 C_TORCH, and C_TORCH is what torch's fp32 restatement needs on this host.  It is a constant in attn_ref.py,
    not computed at import, so that the GPU tests hold the kernels to one bound everywhere; torch's CPU kernels sum in an order
    that depends on the host's vector width and thread count, so the measurement may fall up to 20 % short of the constant and
    must not exceed it (the rule of tests/test_gn_ref_cpu.py)."""
    worst = {}
    for cs in K.CASES:
        for key, c in _measure(cs).items():
            worst[key] = max(worst.get(key, 0.0), c)
    top = max(worst.values())
    for key, c in sorted(worst.items()):
        _report(f"torch_c_max {key[0]} {key[1]} {c:.4g}")
    assert R.C_ATTN == 4.0 * R.C_TORCH
    assert 0.8 * R.C_TORCH <= top <= R.C_TORCH, f"largest smallest-passing c of torch's restatement: {top:.4g}, C_TORCH {R.C_TORCH}"


def test_report_states_the_constant():
    txt = open(os.path.join(GOLDEN, "REPORT_attention_routes.txt")).read()
    assert f"C_TORCH = {R.C_TORCH:g}, C_ATTN = 4 x C_TORCH = {R.C_ATTN:g}" in txt
    for mut in MUTATIONS:
        assert mut in txt
    assert "loosest check" in txt


# ------------------------------------------------------------------------------------------ (b) rejects subtle defects
MUTATION_CASES = 3       # per defect and dtype: the first cases of the table on which it applies


def _mutation_runs():
    picked = []
    for mut in MUTATIONS:
        for dname in K.DTYPES:
            n = 0
            for cs in K.CASES[::-1]:                   # (the named cases first)
                if cs[1] != dname or n >= MUTATION_CASES:
                    continue
                var = K.variations(cs)
                p = K.DROP_P if var["drop"] else 0.0
                for varlen, pb in ((False, K.BWD), (True, K.BWD_VARLEN)):
                    ends = R.key_ends(var["kv_len"] if varlen else None, var["B"], cs[4])
                    fake = type("E", (), {"ends": ends})
                    if n < MUTATION_CASES and mutation_applies(mut, cs, varlen, fake, p, K.expected_route(cs, pb)):
                        picked.append((mut, cs, varlen))
                        n += 1
    return picked


@pytest.mark.parametrize("mut,cs,varlen", _mutation_runs(), ids=lambda v: v if isinstance(v, str) else (v[0] if isinstance(v, tuple) else str(int(v))))
def test_bound_rejects_defect(mut, cs, varlen):
    """The defect puts at least one output out of its bound (an output the defect leaves untouched is not counted)."""
    varlen_, route, ops, ref, p, seed = [r for r in _runs(cs) if r[0] == varlen][0]
    clean = formula_model(ops, cs, route[0], ref, p, seed, route)
    got = formula_model(ops, cs, route[0], ref, p, seed, route, mut)
    caught = []
    for name in R.OUTPUTS:
        if torch.equal(got[name], clean[name]):
            continue
        try:
            R.check_all(got, ref, K.DTYPES[cs[1]], "mutated", names=[name])
        except AssertionError:
            caught.append(name)
    _report(f"mutation {mut} {cs[0]} {cs[1]} varlen={int(varlen)} caught_by {','.join(caught) or 'NONE'}")
    assert caught, f"{mut} on {cs[0]} varlen={varlen} leaves every output within its bound"


def test_every_mutation_applies_in_both_dtypes():
    runs = _mutation_runs()
    for mut in MUTATIONS:
        for dname in K.DTYPES:
            if mut == "dk_partial_missing" and dname == "f32":
                continue                               # (only the bf16 MFMA dK/dV kernel splits a key tile's queries over waves)
            assert any(m == mut and cs[1] == dname for m, cs, _ in runs), (mut, dname)


# --------------------------------------------------------------------------------------------------------------- (c) mask
def test_mask_restatement_known_answers():
    """mix32 is murmur3's 32-bit finaliser (known answers from its reference implementation); the pair hashes and keep bits of
    tests/golden/attn_mask_known.json were computed once with a C program in uint32_t / uint64_t arithmetic."""
    assert [int(v) for v in R.mix32(np.array([0, 1, 0xFFFFFFFF, 0x12345678], dtype=np.uint64))] == [0, 0x514E28B7, 0x81F16F39, 0xE37CD1BC]
    known = json.load(open(os.path.join(GOLDEN, "attn_mask_known.json")))
    for seed, pair, want in known["drop_hash_pair"]:
        assert int(R.drop_hash_pair(int(seed), np.array([int(pair)], dtype=np.uint64))[0]) == want, (seed, pair)
    assert R.drop_thresh(0.3) == known["drop_thresh_0.3"]
    for row in known["keep"]:
        m = R.keep_mask(int(row["seed"]), row["BH"], row["L"], row["S"], row["p"])
        bits = "".join("1" if b else "0" for b in m[row["bh"], row["l"]])
        assert bits == row["bits"], row


def test_mask_keep_rate():
    for S in (49, 64):
        m = R.keep_mask(0xC0FFEE, 6, 40, S, 0.3)
        assert abs(float(m.mean()) - 0.7) < 0.03
        assert abs(float(m[:, :, ::2].mean()) - 0.7) < 0.03 and abs(float(m[:, :, 1::2].mean()) - 0.7) < 0.03
    assert bool(R.keep_mask(1, 2, 3, 5, 0.0).all())


# ------------------------------------------------------------------------------------------------- (d) route coverage
def test_route_query_rejects_what_the_launches_reject(lib):
    """The error codes of attn_check and the LDS check, which the launch entries run too (nothing is launched)."""
    out = (C.c_int32 * len(K.ROUTE_FIELDS))()
    o = C.cast(out, C.c_void_p)

    def rc(p=0, dt=0, B=2, H=3, L=8, S=8, d=16, ldq=48, ldk=48, ldv=48, ldo=48, ldg=48, al=1, o_=o):
        return lib.psg_attn_route(p, dt, B, H, L, S, d, ldq, ldk, ldv, ldo, ldg, al, o_)

    assert rc() == 0
    assert rc(dt=7) == -2                                                          # PSG_ERR_DTYPE
    for kw in (dict(d=6), dict(d=324), dict(B=0), dict(S=0), dict(ldq=44), dict(S=4097), dict(B=30000), dict(p=2, ldg=44), dict(S=2400, d=320)):
        assert rc(**kw) == -1, kw                                                  # PSG_ERR_SHAPE
    assert rc(ldk=50) == -3                                                        # PSG_ERR_ALIGN
    assert rc(p=2, ldg=50) == -1                                                   # (the launch's gradient-stride check)
    assert rc(p=5) == -6 and rc(o_=None) == -6                                     # PSG_ERR_ARG
    # the launch entries answer alike (no GPU is needed: the checks come first)
    assert lib.psg_attn_fwd(0x10, 44, 0x10, 48, 0x10, 48, 0x10, 48, 0x10, 2, 3, 8, 8, 16, 1.0, 0.0, 0, 0, None) == -1
    assert lib.psg_attn_fwd(0x10, 48, 0x10, 50, 0x10, 48, 0x10, 48, 0x10, 2, 3, 8, 8, 16, 1.0, 0.0, 0, 0, None) == -3


def test_route_query_honours_set_paths_and_counts_nothing(lib):
    before = [C.c_int64() for _ in range(3)]
    lib.psg_attn_path_counts(*[C.byref(b) for b in before])
    try:
        for mask, want_b, want_f in ((3, 0, 2), (2, 1, 2), (1, 0, 1), (0, 1, 1)):
            lib.psg_attn_set_paths(mask)
            assert K.query_route(lib, 0, "bf16", 2, 3, 40, 40, 64, 192, 192, 192, 192, 192, 1)[1][0] == want_b
            assert K.query_route(lib, 0, "f32", 2, 3, 40, 40, 64, 192, 192, 192, 192, 192, 1)[1][0] == want_f
    finally:
        lib.psg_attn_set_paths(3)
    after = [C.c_int64() for _ in range(3)]
    lib.psg_attn_path_counts(*[C.byref(b) for b in after])
    assert [b.value for b in before] == [a.value for a in after]


def test_table_routes_are_the_librarys(lib):
    assert set(K.ROUTES) == set(K.IDS)
    for cs in K.CASES:
        for p in range(len(K.PASSES)):
            rc, got = K.query_route(lib, p, cs[1], *K.route_args(cs, p))
            assert rc == 0
            want = K.expected_route(cs, p)
            assert got == want, f"{cs[0]} {K.PASSES[p]}: library {dict(zip(K.ROUTE_FIELDS, got))}, table {dict(zip(K.ROUTE_FIELDS, want))}"


def _table_keys():
    return {K.route_key(cs[1], p, K.expected_route(cs, p)) for cs in K.CASES for p in range(len(K.PASSES))}


def _routes_of(name):
    return [dict(zip(K.ROUTE_FIELDS, K.ROUTES[name][p])) for p in range(len(K.PASSES))]


def test_table_holds_the_named_variants():
    """What each named case is in the table for."""
    fam = lambda name: [r["family"] for r in _routes_of(name)]                     # fwd, fwd_varlen, bwd, fwd_varlen_train, bwd_varlen
    assert fam("b320-S96") == [0] * 5 and fam("b320-S97") == [1] * 5
    assert fam("b320-L64") == [0] * 5 and fam("b320-L65") == [1, 0, 1, 1, 1]
    assert fam("b160-L196") == [1, 0, 1, 1, 1]
    assert fam("f160-96") == [2] * 5 and fam("f160-S97") == [1] * 5 and fam("f160-L97") == [1, 2, 1, 1, 1]
    assert fam("b64-ld8") == [0] * 5 and fam("b64-ld4") == [1] * 5 and fam("b64-ptr4") == [1] * 5
    r = _routes_of("b16-qwcut")[K.BWD]
    assert (r["KW"], r["QW"], r["qw_cut"]) == (1, 2, 1)
    r = _routes_of("b160-wcut")[K.BWD]
    assert r["w_cut"] == 1 and r["KV_REG"] == 0 and r["dkv_waves"] < 3
    r = _routes_of("b320-S81")[K.BWD]
    assert (r["family"], r["NH"], r["dkv_waves"]) == (0, 2, 1)                     # three key tiles on one wave
    keys = _table_keys()
    assert {k[3] for k in keys if k[2] == 0} == {1, 2, 4, 5, 10, 20} and {k[3] for k in keys if k[2] == 2} == {1, 2, 4, 5, 10}
    for family in (0, 2):
        assert {k[4] for k in keys if k[2] == family} == {1, 2, 3, 4}
    assert {(k[5], k[6]) for k in keys if k[2] == 0 and k[1] == "bwd"} >= {(1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (2, 2), (3, 1), (4, 1)}
    for dname in K.DTYPES:                                                         # every stride mode, dropout and lse = NULL on each family
        for family in ((0, 1) if dname == "bf16" else (2, 1)):
            mine = [cs for cs in K.CASES if cs[1] == dname and K.expected_route(cs, K.BWD)[0] == family]
            assert {K.variations(cs)["mode"] for cs in mine} >= set(K.MODES)
            assert any(K.variations(cs)["drop"] and cs[4] % 2 for cs in mine) and any(K.variations(cs)["lse_null"] for cs in mine)
            assert any(K.variations(cs)["kv_len"] == [0, 1, 7, 32, 33, cs[4] - 1, cs[4], cs[4] + 5] for cs in mine)      # every key length at once
    assert any(cs[1] == "f32" and cs[2] == 320 for cs in K.CASES) and {4, 8, 20, 40} <= {cs[2] for cs in K.CASES if cs[1] == "bf16"}


def test_sweep_reaches_nothing_the_table_does_not(lib):
    """Every accepted head_dim, both dtypes, all five passes, L and S = 1 ... 260 on the head dims a matrix-core family takes
    (there the launch depends on L and S); on the others the call runs on the VALU kernels whatever L and S are - asserted on
    a coarse grid - and the launch variant depends on head_dim alone.  Every variant reached is one the table launches."""
    table = _table_keys()
    out = (C.c_int32 * len(K.ROUTE_FIELDS))()
    o = C.cast(out, C.c_void_p)
    fn = lib.psg_attn_route
    seen = set()
    coarse = (1, 17, 64, 65, 96, 97, 129, 260)
    for dt, dname in ((0, "f32"), (1, "bf16")):
        for d in range(4, 321, 4):
            mfma = d in (16, 32, 64, 80, 160, 320)
            HD = 3 * d
            for p in range(5):
                dirn = "bwd" if p in (K.BWD, K.BWD_VARLEN) else "fwd"
                for L in (range(1, 261) if mfma else coarse):
                    for S in (range(1, 261) if mfma else coarse):
                        assert fn(p, dt, 2, 3, L, S, d, HD, HD, HD, HD, HD, 1, o) == 0
                        assert mfma or out[0] == 1
                        seen.add((dname, dirn, out[0], out[1], out[2], out[3], out[4], out[6], out[7], out[8], out[19]))
    assert not seen - table, f"reached by a shape of the sweep but by no case of the table: {sorted(seen - table)}"
