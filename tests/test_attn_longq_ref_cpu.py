"""CPU checks of tests/attn_longq_cases.py: the table reaches what its docstring claims (every head_dim x dtype on each of the
four (nkt, tps) paths, the edges of L and S, every layout) with the slab arithmetic checked against the library's workspace
query; the bounds of tests/attn_ref.py at C_LONGQ accept a correct fp32 / bf16 result on these shapes - torch's own matmul /
softmax / autograd, which also measures C_TORCH_LONGQ, and a formula model of the kernel pair - and reject eight defects this
kernel could have."""
import os

import pytest
import torch

from tests import attn_longq_cases as K
from tests import attn_ref as R
from tests.test_attn_ref_cpu import _heads, _rows, _store, torch_restatement

REPORT = os.environ.get("PSG_ATTN_LONGQ_REPORT")      # optional: append the measured figures to this file
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


_last = {}       # the reference of the case used last (the large cases are too large to keep them all)


def _run(case):
    """(operands, fp64 reference) of a case: family VALU, no dropout, no key lengths."""
    if _last.get("name") != case.name:
        ops = K.operands(case)
        ref = R.reference(ops["q"], ops["k"], ops["v"], case.heads, ops["scale"], R.VALU, case.dname == "bf16", dout=ops["dout"])
        _last.update(name=case.name, run=(ops, ref))
    return _last["run"]


# ------------------------------------------------------------------------------------------------------------ the table
def test_table_paths_are_the_librarys(lib):
    """The restated lq_tps / lq_nslab give every case the path it is named for, and the slab count is the one the library's
    workspace query implies."""
    for cs in K.CASES:
        assert K.path_of(cs) == cs.path, cs.name
        need = lib.psg_attn_bwd_longq_workspace_bytes(cs.B, cs.heads, cs.L, cs.S, cs.d)
        per_slab = cs.B * cs.heads * 2 * cs.S * cs.d * 4
        assert need > 0 and need % per_slab == 0 and need // per_slab == K.lq_nslab(cs.B, cs.heads, cs.L), cs.name
    # the decoder's maps at the stage-3 batch, for the record of what the product launches: tps > 1 only with nkt == 1
    assert [K.lq_tps(2, 8, L) for L in (729, 2916, 11664, 46225)] == [1, 1, 2, 11]


def test_table_reaches_every_variant_on_every_path():
    reached = {(cs.d, cs.dname, K.path_of(cs)) for cs in K.CASES}
    assert reached == {(d, dn, p) for d in K.HEAD_DIMS for dn in K.DTYPES for p in K.PATHS}
    assert len(reached) == 5 * 2 * 4
    assert any(K.lq_tps(cs.B, cs.heads, cs.L) >= 3 and K.lq_nkt(cs.S) > 1 for cs in K.CASES)          # a partial added into twice
    tiles = lambda cs: (cs.L + 63) // 64
    # a slab of a single tile behind slabs of several, and a ragged last tile, where partials are added
    assert any(cs.path == "kNtN" and tiles(cs) % K.lq_tps(cs.B, cs.heads, cs.L) == 1 and cs.L % 64 for cs in K.CASES)
    assert any(cs.path in ("k1t1", "kNt1") and K.lq_nslab(cs.B, cs.heads, cs.L) > 1 for cs in K.CASES)


def test_table_holds_the_edges():
    Ls, Ss = {cs.L for cs in K.CASES}, {cs.S for cs in K.CASES}
    assert {1, 63, 64, 65} <= Ls and any(L > 64 and L % 64 == 1 for L in Ls)
    assert {1, 31, 32, 33, 256} <= Ss and any(S > 32 and S % 32 == 1 for S in Ss)
    for path in K.PATHS:
        mine = [cs for cs in K.CASES if cs.path == path]
        assert any(cs.S * cs.d < 256 for cs in mine) and any(cs.S * cs.d > 256 for cs in mine), path
    for cs in K.CASES:
        assert cs.B >= 2 and cs.heads >= 3 and cs.S <= K.LQ_MAX_S and cs.B * cs.heads * cs.L * cs.S <= 1.1e7, cs.name


def test_table_holds_every_layout():
    for dname, modes in K.MODES.items():
        for path in K.PATHS:
            assert {K.mode_of(cs) for cs in K.CASES if cs.dname == dname and cs.path == path} == set(modes), (dname, path)
    for cs in K.CASES:
        mode, lay = K.layout(cs)
        HD = cs.heads * cs.d
        for n, (ld, off) in lay.items():
            assert ld % 4 == 0 and ld >= HD, (cs.name, n)
            if mode == "kv" and n in ("k", "v", "dk", "dv"):
                assert ld == 2 * HD and off == (HD if n in ("v", "dv") else 0)
            else:
                assert off + HD <= ld, (cs.name, n)
            if n not in ("dk", "dv"):
                assert off % 4 == 0, (cs.name, n)                       # the contract's 4-element boundary
        if mode == "ptr4":
            assert cs.dname == "bf16" and all(lay[n][1] * 2 % 16 == 8 for n in ("q", "k", "v", "o", "dout", "dq"))
        if mode == "odd":
            assert lay["dk"][1] % 2 == 1 and lay["dv"][1] % 2 == 1


# ------------------------------------------------------------------------------------------ the kernel pair as formulas
MUTATIONS = ("slab_partial_missing", "later_tile_overwrites", "pad_key_zero", "dq_no_scale", "delta_neighbour", "last_qtile_unwritten",
             "head_stride", "ng_group_missing")


def mutation_applies(mut, cs):
    tps, nslab, nkt = K.lq_tps(cs.B, cs.heads, cs.L), K.lq_nslab(cs.B, cs.heads, cs.L), K.lq_nkt(cs.S)
    if mut == "slab_partial_missing":
        return nslab > 1
    if mut == "later_tile_overwrites":
        return tps > 1 and nkt > 1
    if mut == "pad_key_zero":
        return cs.S % 32 != 0
    if mut == "delta_neighbour":
        return cs.L > 1
    if mut == "last_qtile_unwritten":
        return cs.L % 64 != 0
    if mut == "ng_group_missing":
        return cs.d < 32
    if mut in ("dq_no_scale", "head_stride"):
        return cs.S > 1                      # (one key: P = 1 and dS = 0 whatever k and scale are)
    return True


def longq_model(ops, cs, ref, mut=None):
    """psg_attn_bwd_longq written out in fp32 torch operations the way the kernels compute it - P from the stored lse, delta
    from the stored o, q pre-scaled, dk / dv summed over the query tiles - a correct implementation when mut is None, and
    with `mut` one of MUTATIONS that defect:

      slab_partial_missing    the reduce kernel skips the last slab's partial
      later_tile_overwrites   flush()'s later visits of a key tile store instead of adding: dk / dv of keys >= 32 hold only the
                              last tile of each slab
      pad_key_zero            a key at index >= S of the last key tile is a zero key rather than a masked one.  Such a key adds
                              nothing to dq (k = 0) and its dk / dv rows are not stored, so in a backward that is handed lse the
                              defect shows only with the forward's half of it: the zero key takes part in the normalisation
                              (lse -> log(exp(lse) + 1)), the form tests/test_attn_ref_cpu.py gives the same defect
      dq_no_scale             dq stored without `scale`
      delta_neighbour         delta of row l taken from row l - 1
      last_qtile_unwritten    the rows of a ragged last query tile never stored (dq, delta left at 0)
      head_stride             head h of k read h elements early (a head stride of d - 1)
      ng_group_missing        the LDS sum over the NG query groups of head_dim < 32 leaves out the last group"""
    H, B, L, S, d = cs.heads, cs.B, cs.L, cs.S, cs.d
    scale = R.stored(torch.tensor(ops["scale"]), False).float()
    k = ops["k"]
    if mut == "head_stride":
        k = torch.cat([k[:, :, h * (d - 1):h * (d - 1) + d] for h in range(H)], -1)
    Q, Kk, V, G = _heads(ops["q"], H) * scale, _heads(k, H), _heads(ops["v"], H), _heads(ops["dout"], H)
    lse = ref.lse_st.float().unsqueeze(-1)
    if mut == "pad_key_zero":
        lse = torch.logaddexp(lse, torch.zeros(()))
    P = torch.exp(Q @ Kk.transpose(2, 3) - lse)
    delta = (G * _heads(ref.o_st.float(), H)).sum(-1, keepdim=True)
    if mut == "delta_neighbour":
        delta = torch.roll(delta, 1, 2)
    dS = P * (G @ V.transpose(2, 3) - delta)
    dQ = (dS @ Kk) * (1.0 if mut == "dq_no_scale" else scale)
    tps = K.lq_tps(B, H, L)
    tile = torch.arange(L) // 64
    w = torch.ones(L, S)                                  # which (query, key) products reach dk / dv
    if mut == "slab_partial_missing":
        w[tile // tps == K.lq_nslab(B, H, L) - 1] = 0.0
    if mut == "later_tile_overwrites":
        last_of_slab = torch.minimum((tile // tps + 1) * tps, torch.tensor((L + 63) // 64)) - 1
        w[tile != last_of_slab, 32:] = 0.0
    if mut == "ng_group_missing":
        NG = 8 // (d // 4)
        w[(torch.arange(L) % 64) % NG == NG - 1] = 0.0
    dK = (dS * w).transpose(2, 3) @ Q
    dV = (P * w).transpose(2, 3) @ G
    if mut == "last_qtile_unwritten":
        dQ, delta = dQ.clone(), delta.clone()
        dQ[:, :, L - L % 64:] = 0.0
        delta[:, :, L - L % 64:] = 0.0
    out = dict(delta=delta.squeeze(-1), dq=_rows(dQ), dk=_rows(dK), dv=_rows(dV))
    return {n: _store(t, n, cs.dname) for n, t in out.items()}


# ---------------------------------------------------------------------------------------- (a) accepts a correct result
_measured = {}       # case name -> {output: smallest c of torch's restatement}


def _measure(cs):
    if cs.name not in _measured:
        ops, ref = _run(cs)
        got = torch_restatement(ops, cs.dname, R.VALU, ref, 0.0)
        _measured[cs.name] = {name: R.smallest_c(got[name], getattr(ref, name), getattr(ref, name + "_mag"), R.out_dtype(name, K.DTYPES[cs.dname]),
                                                 extra=getattr(ref, name + "_extra")) for name in R.OUTPUTS}
    return _measured[cs.name]


@pytest.mark.parametrize("cs", K.CASES, ids=K.IDS)
def test_bounds_accept_correct_results(cs):
    """torch's restatement is within every bound at the larger of the two measured constants - its own error on either table -
    and the formula model the defects start from is within them at C_LONGQ."""
    ops, ref = _run(cs)
    for name, c in _measure(cs).items():
        _report(f"torch_c {cs.name} {cs.dname} {name} {c:.4g}")
        assert c <= max(R.C_TORCH, K.C_TORCH_LONGQ), (name, c)
    ratios = R.check_all(longq_model(ops, cs, ref), ref, K.DTYPES[cs.dname], f"{cs.name} model", c=K.C_LONGQ)
    _report(f"model {cs.name} {cs.dname} " + " ".join(f"{n}={v:.3g}" for n, v in ratios.items()))


def test_c_torch_longq_is_what_torch_needs_here():
    """C_TORCH_LONGQ is the largest smallest-passing c of torch's fp32 restatement over this table - measured against torch,
    never against the kernel.  It is a constant, so that every host holds the kernel to one bound; torch's CPU kernels sum in
    an order that depends on the host, so the measurement may fall up to 20 % short of the constant and must not exceed it
    (the rule of test_attn_ref_cpu.test_c_attn_is_four_times_torchs_own_error)."""
    worst = {}
    for cs in K.CASES:
        for name, c in _measure(cs).items():
            key = (cs.dname, name)
            if c > worst.get(key, (-1.0, ""))[0]:
                worst[key] = (c, cs.name)
    for (dname, name), (c, where) in sorted(worst.items()):
        _report(f"torch_c_max {dname} {name} {c:.4g} {where}")
    top = max(c for c, _ in worst.values())
    assert K.C_LONGQ == 4.0 * max(R.C_TORCH, K.C_TORCH_LONGQ)
    assert 0.8 * K.C_TORCH_LONGQ <= top <= K.C_TORCH_LONGQ, f"largest smallest-passing c of torch's restatement: {top:.4g}, C_TORCH_LONGQ {K.C_TORCH_LONGQ}"


def test_report_states_the_constants():
    txt = open(os.path.join(GOLDEN, "REPORT_attn_longq.txt")).read()
    assert f"C_TORCH_LONGQ = {K.C_TORCH_LONGQ:g}, C_LONGQ = 4 x max(C_TORCH, C_TORCH_LONGQ) = {K.C_LONGQ:g}" in txt
    for cs in K.CASES:
        assert f"gpu {cs.name} " in txt, cs.name
    for mut in MUTATIONS:
        assert mut in txt


# ------------------------------------------------------------------------------------------ (b) rejects subtle defects
MUTATION_CASES = 2       # per defect and dtype: the smallest cases of the table on which it applies


def _mutation_runs():
    picked = []
    by_size = sorted(K.CASES, key=lambda cs: cs.B * cs.heads * cs.L * (cs.S + cs.d))
    for mut in MUTATIONS:
        for dname in K.DTYPES:
            picked += [(mut, cs) for cs in [c for c in by_size if c.dname == dname and c.L > 1 and mutation_applies(mut, c)][:MUTATION_CASES]]
    return sorted(picked, key=lambda mc: mc[1].i)       # (cases together: one reference each)


@pytest.mark.parametrize("mut,cs", _mutation_runs(), ids=lambda v: v if isinstance(v, str) else v.name)
def test_bound_rejects_defect(mut, cs):
    """The defect puts at least one output out of its bound at C_LONGQ (an output the defect leaves untouched is not counted)."""
    ops, ref = _run(cs)
    clean = longq_model(ops, cs, ref)
    got = longq_model(ops, cs, ref, mut)
    caught = []
    for name in R.BWD_OUTPUTS:
        if torch.equal(got[name], clean[name]):
            continue
        try:
            R.check_all(got, ref, K.DTYPES[cs.dname], "mutated", names=[name], c=K.C_LONGQ)
        except AssertionError:
            caught.append(name)
    _report(f"mutation {mut} {cs.name} caught_by {','.join(caught) or 'NONE'}")
    assert caught, f"{mut} on {cs.name} leaves every output within its bound"


def test_every_mutation_applies_in_both_dtypes():
    runs = _mutation_runs()
    for mut in MUTATIONS:
        for dname in K.DTYPES:
            assert any(m == mut and cs.dname == dname for m, cs in runs), (mut, dname)
