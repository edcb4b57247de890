"""CPU checks of tests/gn_ref.py and tests/gn_cases.py: the fp64 GroupNorm reference equals torch's, its per-element bounds
accept a correct fp32 / bf16 result (torch's own kernels, and an fp32 emulation of the split kernels' summation order) on
every case of the table and reject nine subtle kernel defects wherever they apply; the constant of the bounds is what torch's
own error measures; and, through psg_groupnorm_route, the table takes the routes it stores and reaches every kernel variant
that any legal shape reaches."""
import ctypes as C
import math
import os

import pytest
import torch
import torch.nn.functional as F

from tests import gn_cases as K
from tests import gn_ref as R

REPORT = os.environ.get("PSG_GN_REPORT")      # optional: append the measured figures to this file


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


def _round(t, name, dname):
    """Store an fp32 result the way the launch stores it: y and dx in the launch's dtype."""
    return t.to(K.DTYPES[dname]) if name in ("y", "dx") else t


# ------------------------------------------------------------------------------------------------- correct implementations
def torch_restatement(ops, shape, var, dname):
    """torch's own fp32 GroupNorm (+SiLU) and its autograd backward on the operands, outputs stored like the launch's."""
    B, HW, Cc, G = shape
    x = ops["x"].permute(0, 2, 1).contiguous().requires_grad_(True)          # [B, C, HW]
    gamma, beta = ops["gamma"].clone().requires_grad_(True), ops["beta"].clone().requires_grad_(True)
    eps = R.f32(var["eps"])
    y = F.group_norm(x, G, gamma, beta, eps)
    if var["silu"]:
        y = F.silu(y)
    y.backward(ops["dy"].permute(0, 2, 1))
    _, mean, rstd = torch.native_group_norm(x.detach(), gamma.detach(), beta.detach(), B, Cc, HW, G, eps)
    dx = x.grad.permute(0, 2, 1)
    if var["dres"]:
        dx = dx + ops["dres"]
    dg, db = gamma.grad, beta.grad
    if var["accumulate"]:
        dg, db = dg + ops["prefill"][0], db + ops["prefill"][1]
    out = dict(y=y.detach().permute(0, 2, 1), mean=mean, rstd=rstd, dx=dx, dgamma=dg, dbeta=db)
    return {n: _round(t, n, dname) for n, t in out.items()}


def split_forward_emulation(ops, shape, var, dname, route):
    """The split forward in fp32 in the kernels' own order (gn_stats_kernel / gn_apply_kernel): a lane sums its pixels of a
    pixel split in steps of PP, one lane per group then adds the PP x Cg lane sums in order (in double), the splits are combined in
    double as E[x^2] - mean^2, and y = x sc + sh with sc = rstd gamma, sh = beta - mean sc."""
    B, HW, Cc, G = shape
    Cg = Cc // G
    rt = dict(zip(K.ROUTE_FIELDS, route))
    PP, NS, pps = rt["PP"], rt["NS"], rt["pps"]
    x = ops["x"]
    a0 = torch.zeros(B, G, dtype=torch.float64)
    a1 = torch.zeros(B, G, dtype=torch.float64)
    for sp in range(NS):
        xs = x[:, sp * pps:min(HW, (sp + 1) * pps)]
        trips = -(-xs.shape[1] // PP)
        xs = F.pad(xs, (0, 0, 0, trips * PP - xs.shape[1])).reshape(B, trips, PP, Cc)
        s = torch.zeros(B, PP, Cc)
        q = torch.zeros(B, PP, Cc)
        for t in range(trips):                     # (absent pixels add zeros: w = 0 in the kernel)
            s = s + xs[:, t]
            q = q + xs[:, t] * xs[:, t]
        s, q = s.reshape(B, PP, G, Cg), q.reshape(B, PP, G, Cg)
        p0 = torch.zeros(B, G, dtype=torch.float64)          # (the lane sums are added in double, stored as fp32 partials)
        p1 = torch.zeros(B, G, dtype=torch.float64)
        for l in range(PP):
            for j in range(Cg):
                p0 = p0 + s[:, l, :, j].double()
                p1 = p1 + q[:, l, :, j].double()
        a0 += p0.float().double()
        a1 += p1.float().double()
    n = float(HW * Cg)
    mean = a0 / n
    v = (a1 / n - mean * mean).clamp_min(0.0)
    rstd = (1.0 / torch.sqrt(v + R.f32(var["eps"]))).float()
    mean = mean.float()
    sc = rstd.repeat_interleave(Cg, 1) * ops["gamma"]
    sh = ops["beta"] - mean.repeat_interleave(Cg, 1) * sc
    y = x * sc[:, None, :] + sh[:, None, :]
    if var["silu"]:
        y = y * torch.sigmoid(y)
    return dict(y=_round(y, "y", dname), mean=mean, rstd=rstd)


MUTATIONS = ("stat_last_pixel", "count_padded", "straddle", "dres_column", "last_split", "sample32", "silu_no_beta",
             "no_accumulate", "no_gamma_in_sums")


def mutation_applies(mut, shape, var, dname):
    B, HW, Cc, G = shape
    Cg = Cc // G
    fwd = dict(zip(K.ROUTE_FIELDS, K.expected_route(shape, dname, False, False)))
    bwd = dict(zip(K.ROUTE_FIELDS, K.expected_route(shape, dname, True, var["dres"])))
    if mut == "count_padded":
        return bool(fwd["fused"]) and HW % fwd["PP"] != 0
    if mut == "straddle":
        return bool((fwd["fused"] and Cg % fwd["N"]) or (bwd["fused"] and Cg % bwd["N"]))
    if mut == "dres_column":
        return var["dres"]
    if mut == "last_split":
        return not bwd["fused"] and bwd["NS"] > 1
    if mut == "sample32":
        return B > 32
    if mut == "silu_no_beta":
        return var["silu"]
    if mut == "no_accumulate":
        return var["accumulate"]
    return True


def _gsum(t):
    """[B, HW, G, Cg] -> [B, G] sums over contiguous rows (torch's cascade summation: the accuracy of a reduction tree)."""
    return t.permute(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], -1).sum(-1)


def formula_model(ops, shape, var, dname, mut=None):
    """GroupNorm forward and backward written out in fp32 torch operations - a correct implementation when mut is None, and
    with `mut` one of MUTATIONS the defect of that name, as a kernel of this shape's route would have it."""
    B, HW, Cc, G = shape
    Cg = Cc // G
    fwd = dict(zip(K.ROUTE_FIELDS, K.expected_route(shape, dname, False, False)))
    bwd = dict(zip(K.ROUTE_FIELDS, K.expected_route(shape, dname, True, var["dres"])))
    x, dy, gamma, beta = ops["x"], ops["dy"], ops["gamma"], ops["beta"]
    eps = R.f32(var["eps"])

    def stats(mutated):
        X = x.reshape(B, HW, G, Cg)
        n = float(HW * Cg)
        Xs = X
        if mutated and mut == "stat_last_pixel":
            Xs = X[:, :HW - 1]
        if mutated and mut == "count_padded":
            n = float(fwd["PP"] * (-(-HW // fwd["PP"])) * Cg)
        mean = _gsum(Xs) / n
        v = _gsum((Xs - mean[:, None, :, None]) ** 2) / n
        return mean, 1.0 / torch.sqrt(v + eps)

    def per_channel(t, rt):
        """[B, G] statistics -> [B, 1, C]; the straddle defect: the whole chunk takes the group of its first channel."""
        grp = torch.arange(Cc) // Cg
        if mut == "straddle" and rt["fused"] and Cg % rt["N"]:
            grp = ((torch.arange(Cc) // rt["N"]) * rt["N"]) // Cg
        return t[:, grp][:, None, :]

    mean_o, rstd_o = stats(True)
    mu, rs = per_channel(mean_o, fwd), per_channel(rstd_o, fwd)
    z = (x - mu) * rs * gamma + beta
    y = z * torch.sigmoid(z) if var["silu"] else z
    # backward: the launch reads mean / rstd as inputs - the correct ones
    mean_c, rstd_c = stats(False)
    mu, rs = per_channel(mean_c, bwd), per_channel(rstd_c, bwd)
    xh = (x - mu) * rs
    dz = dy
    if var["silu"]:
        zb = xh * gamma + (0.0 if mut == "silu_no_beta" else beta)
        s = torch.sigmoid(zb)
        dz = dy * (s * (1.0 + zb * (1.0 - s)))
    t = dz if mut == "no_gamma_in_sums" else dz * gamma
    s1 = _gsum(t.reshape(B, HW, G, Cg)) / float(HW * Cg)
    s2 = _gsum((t * xh).reshape(B, HW, G, Cg)) / float(HW * Cg)
    grp = torch.arange(Cc) // Cg
    dx = rs * (dz * gamma - s1[:, grp][:, None, :] - xh * s2[:, grp][:, None, :])
    if var["dres"]:
        dr = ops["dres"]
        if mut == "dres_column":
            k = (Cc // 8) // 2
            dr = dr.clone()
            dr[:, :, 8 * k:8 * k + 8] = 0.0
        dx = dx + dr
    dzs, xhs = dz, xh
    if mut == "last_split":
        dzs, xhs = dz[:, :(bwd["NS"] - 1) * bwd["pps"]], xh[:, :(bwd["NS"] - 1) * bwd["pps"]]
    if mut == "sample32":
        dzs, xhs = dzs[:32], xhs[:32]
    dg, db = (dzs * xhs).sum((0, 1)), dzs.sum((0, 1))
    if var["accumulate"] and mut != "no_accumulate":
        dg, db = dg + ops["prefill"][0], db + ops["prefill"][1]
    out = dict(y=y, mean=mean_o, rstd=rstd_o, dx=dx, dgamma=dg, dbeta=db)
    return {n: _round(v, n, dname) for n, v in out.items()}


# ------------------------------------------------------------------------------------------------------ per-case fixture
def _runs(shape):
    """Every (dtype, variant) launch of a case with its operands and fp64 reference."""
    out = []
    for dname in K.DTYPES:
        ops = K.operands(shape, dname)
        for vi, var in enumerate(K.variants(shape)):
            ref = R.reference(ops["x"], ops["gamma"], ops["beta"], shape[3], var["eps"], var["silu"], dy=ops["dy"],
                              dres=ops["dres"] if var["dres"] else None, prefill=ops["prefill"] if var["accumulate"] else None,
                              bf16=dname == "bf16")
            out.append((dname, vi, var, ops, ref))
    return out


@pytest.fixture(scope="module", params=[s for _, s in K.case_ids()], ids=[i for i, _ in K.case_ids()])
def case(request):
    return request.param, _runs(request.param)


_measured = {}       # shape -> {(dname, output): smallest c of torch's restatement}


def _measure(shape, runs):
    if shape not in _measured:
        m = {}
        for dname, vi, var, ops, ref in runs:
            got = torch_restatement(ops, shape, var, dname)
            for name in R.OUTPUTS:
                c = R.smallest_c(got[name], getattr(ref, name), getattr(ref, name + "_mag"), R.out_dtype(name, K.DTYPES[dname]),
                                 extra=getattr(ref, name + "_extra"))
                m[(dname, name)] = max(m.get((dname, name), 0.0), c)
        _measured[shape] = m
    return _measured[shape]


# ------------------------------------------------------------------------------------------------------ reference == torch
def test_reference_matches_torch_fp64():
    g = torch.Generator().manual_seed(5)
    B, HW, Cc, G = 3, 11, 24, 4
    xb = torch.randn(B, HW, Cc + 8, dtype=torch.float64, generator=g)
    x = xb[..., 4:4 + Cc]                                                         # a strided view
    gamma, beta = torch.randn(Cc, dtype=torch.float64, generator=g), torch.randn(Cc, dtype=torch.float64, generator=g)
    dy, dres = torch.randn(B, HW, Cc, dtype=torch.float64, generator=g), torch.randn(B, HW, Cc, dtype=torch.float64, generator=g)
    pg, pb = torch.randn(Cc, dtype=torch.float64, generator=g), torch.randn(Cc, dtype=torch.float64, generator=g)
    for silu in (False, True):
        xn = x.permute(0, 2, 1).contiguous().requires_grad_(True)
        gn, bn = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        y = F.group_norm(xn, G, gn, bn, 1e-5)
        y = F.silu(y) if silu else y
        y.backward(dy.permute(0, 2, 1))
        r = R.reference(x, gamma, beta, G, 1e-5, silu, dy=dy, dres=dres, prefill=(pg, pb))
        for a, b, what in ((r.y, y.detach().permute(0, 2, 1), "y"), (r.dx, xn.grad.permute(0, 2, 1) + dres, "dx"),
                           (r.dgamma, gn.grad + pg, "dgamma"), (r.dbeta, bn.grad + pb, "dbeta")):
            err = float((a - b).abs().max() / b.abs().max())
            assert err < 1e-9, f"{what} silu={silu}: {err:.3g}"        # (eps is rounded to fp32 in the reference)
        assert all(bool((getattr(r, n + "_mag") >= 0).all()) for n in R.OUTPUTS)


# ---------------------------------------------------------------------------------------- (a) accepts a correct result
def test_bound_accepts_torch_restatement(case):
    shape, runs = case
    for dname, vi, var, ops, ref in runs:
        R.check_all(torch_restatement(ops, shape, var, dname), ref, K.DTYPES[dname], f"{shape} {dname} v{vi} torch")
    for (dname, name), c in sorted(_measure(shape, runs).items()):
        _report(f"torch_c {'x'.join(map(str, shape))} {dname} {name} {c:.4g}")


def test_bound_accepts_formula_model(case):
    """The unmutated model the mutations below start from is itself within the bounds."""
    shape, runs = case
    for dname, vi, var, ops, ref in runs:
        R.check_all(formula_model(ops, shape, var, dname), ref, K.DTYPES[dname], f"{shape} {dname} v{vi} model")


def test_bound_accepts_split_order_emulation(case):
    """... on every launch of the case whose forward is split, and on its extra constant-sample forward launch.  Only the
    forward is emulated: the split backward's order (gn_bwd_reduce_kernel, gn_bwd_apply_kernel, gn_param_reduce_kernel) has no
    emulation here, so for dx, dgamma and dbeta part (a) rests on torch's restatement and the formula model alone."""
    shape, runs = case
    todo = [(dname, f"v{vi}", var, ops, ref) for dname, vi, var, ops, ref in runs]
    for extra in K.extra_forwards(shape):
        for dname in K.DTYPES:
            ops, var = K.operands(shape, dname, extra), K.variants(shape)[0]
            ref = R.reference(ops["x"], ops["gamma"], ops["beta"], shape[3], var["eps"], var["silu"], bf16=dname == "bf16")
            todo.append((dname, extra, var, ops, ref))
    for dname, tag, var, ops, ref in todo:
        route = K.expected_route(shape, dname, False, False)
        if route[0]:
            continue
        got = split_forward_emulation(ops, shape, var, dname, route)
        ratios = R.check_all(got, ref, K.DTYPES[dname], f"{shape} {dname} {tag} split emulation")
        _report(f"split_emulation {'x'.join(map(str, shape))} {dname} {tag} " + " ".join(f"{n}={v:.3g}" for n, v in ratios.items()))


def test_c_gn_is_four_times_torchs_own_error():
    """C_GN = 4 C_TORCH, and C_TORCH is what torch's fp32 restatement needs on this host.  It is a constant in gn_ref.py, not
    computed at import, so that the GPU tests hold the kernels to one bound everywhere; torch's CPU kernels sum in an order
    that depends on the host's vector width and thread count, so the measurement may fall up to 20 % short of the constant
    (the margin is then 4x to 5x of this host's figure) and must not exceed it.  A host whose torch sums more than 20 % more
    accurately fails here although no kernel is involved: then re-measure and lower C_TORCH."""
    worst = {}
    for _, shape in K.case_ids():
        for key, c in _measure(shape, _runs(shape) if shape not in _measured else None).items():
            worst[key] = max(worst.get(key, 0.0), c)
    top = max(worst.values())
    for key, c in sorted(worst.items()):
        _report(f"torch_c_max {key[0]} {key[1]} {c:.4g}")
    assert R.C_GN == 4.0 * R.C_TORCH
    assert 0.8 * R.C_TORCH <= top <= R.C_TORCH, f"largest smallest-passing c of torch's restatement: {top:.4g}, C_TORCH {R.C_TORCH}"


def test_report_states_the_constant():
    """tests/golden/REPORT_groupnorm_routes.txt (tools/gn_routes_report.py writes it from the figures these tests append to
    the file PSG_GN_REPORT names) is about the constant the bounds use."""
    txt = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "REPORT_groupnorm_routes.txt")).read()
    assert f"C_TORCH = {R.C_TORCH:g}, C_GN = 4 x C_TORCH = {R.C_GN:g}" in txt
    for mut in MUTATIONS:
        assert mut in txt


# ------------------------------------------------------------------------------------------ (b) rejects subtle defects
def test_bound_rejects_every_defect(case):
    """Each defect of MUTATIONS, on every launch of the case it applies to, puts at least one output out of its bound."""
    shape, runs = case
    missed = []
    for dname, vi, var, ops, ref in runs:
        clean = formula_model(ops, shape, var, dname)
        for mut in MUTATIONS:
            if not mutation_applies(mut, shape, var, dname):
                continue
            got = formula_model(ops, shape, var, dname, mut)
            caught = []
            for name in R.OUTPUTS:
                if torch.equal(got[name], clean[name]):
                    continue                                   # untouched by this defect: within its bound like the clean model
                try:
                    R.check_all(got, ref, K.DTYPES[dname], "mutated", names=[name])
                except AssertionError:
                    caught.append(name)
            _report(f"mutation {mut} {'x'.join(map(str, shape))} {dname} v{vi} caught_by {','.join(caught) or 'NONE'}")
            if not caught:
                missed.append((mut, dname, vi))
    assert not missed, f"{shape}: defects that leave every output within its bound (defect, dtype, variant): {missed}"


def test_every_mutation_applies_somewhere():
    for mut in MUTATIONS:
        for dname in K.DTYPES:
            assert any(mutation_applies(mut, s, v, dname) for _, s in K.case_ids() for v in K.variants(s)), (mut, dname)


# ------------------------------------------------------------------------------------------------- (c) route coverage
def _key(backward, dname, route, silu, dres):
    fused, N, Rr = route[0], route[1], route[2]
    return ("bwd" if backward else "fwd", dname, fused, N if fused else 0, Rr if fused else 0, bool(silu), bool(dres and backward))


def _table_keys():
    keys = set()
    for _, shape in K.case_ids():
        for dname in K.DTYPES:
            for var in K.variants(shape):
                keys.add(_key(False, dname, K.expected_route(shape, dname, False, False), var["silu"], False))
                keys.add(_key(True, dname, K.expected_route(shape, dname, True, var["dres"]), var["silu"], var["dres"]))
    return keys


def test_route_query_rejects_what_the_launches_reject(lib):
    """The error codes of gn_check_shape, which the launches run too (nothing is launched here: no pointer is invented)."""
    out = (C.c_int32 * 12)()
    o = C.cast(out, C.c_void_p)
    for dt, B, HW, Cc, G in ((1, 2, 9, 12, 4), (0, 2, 9, 6, 2), (0, 2, 9, 260, 65), (0, 0, 9, 32, 8), (1, 2, 9, 64, 24), (0, 2, 9, 8192, 32)):
        assert lib.psg_groupnorm_route(0, dt, B, HW, Cc, G, 0, o) == -1                # PSG_ERR_SHAPE
        assert lib.psg_groupnorm_route(1, dt, B, HW, Cc, G, 1, o) == -1
    assert lib.psg_groupnorm_route(0, 7, 2, 9, 32, 8, 0, o) == -2                       # PSG_ERR_DTYPE
    assert lib.psg_groupnorm_route(0, 0, 2, 9, 32, 8, 0, None) == -6                    # PSG_ERR_ARG


def test_table_routes_are_the_librarys(lib):
    for _, shape in K.case_ids():
        for dname in K.DTYPES:
            for backward, dres in ((0, 0), (1, 0), (1, 1)):
                rc, got = K.query_route(lib, backward, dname, *shape, dres)
                assert rc == 0
                want = K.expected_route(shape, dname, backward, dres)
                assert got == want, f"{shape} {dname} backward={backward} dres={dres}: library " \
                                    f"{dict(zip(K.ROUTE_FIELDS, got))}, table {dict(zip(K.ROUTE_FIELDS, want))}"


def _required_keys():
    req = set()
    for silu in (False, True):
        for dname, N in (("f32", 4), ("bf16", 8)):
            for Rr in (4, 8, 16):
                req.add(("fwd", dname, 1, N, Rr, silu, False))                     # 12 fused forward
            req.add(("fwd", dname, 0, 0, 0, silu, False))                          # split forward
        for res in (False, True):
            for Rr in (4, 8):
                req.add(("bwd", "f32", 1, 2, Rr, silu, res))                       # 8 fp32 fused backward
                req.add(("bwd", "bf16", 1, 4, Rr, silu, res))                      # 8 bf16 N = 4
            for dname in K.DTYPES:
                req.add(("bwd", dname, 0, 0, 0, silu, res))                        # split backward, with and without dres
        for Rr in (4, 8):
            req.add(("bwd", "bf16", 1, 8, Rr, silu, True))                         # the 4 bf16 N = 8 with RES
    return req


def test_table_reaches_every_required_variant():
    missing = _required_keys() - _table_keys()
    assert not missing, f"kernel variants no case of the table launches: {sorted(missing)}"


def test_sweep_reaches_nothing_the_table_does_not(lib):
    """Every legal shape of G x Cg x H^2: the (direction, dtype, fused, N, R, res) it routes to is one the table launches (with
    both SiLU values), the four bf16 backward N = 8 instantiations without dres are reached by none, and neither is the
    fall-back of a slab plan whose LDS exceeds 64 KiB.  A routing change that makes one of them live fails here until a case
    is added."""
    table = _table_keys()
    out = (C.c_int32 * 12)()
    o = C.cast(out, C.c_void_p)
    seen = set()
    for G in (1, 2, 4, 8, 16, 32, 64):
        for Cg in (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 40, 80):
            for dt, dname in ((0, "f32"), (1, "bf16")):
                for backward, dres in ((0, 0), (1, 0), (1, 1)):
                    if lib.psg_groupnorm_route(backward, dt, 2, 1, G * Cg, G, dres, o) != 0:
                        continue                                                   # not a legal shape in this dtype
                    for H in range(1, 216):
                        assert lib.psg_groupnorm_route(backward, dt, 2, H * H, G * Cg, G, dres, o) == 0
                        fused, N, Rr = out[0], out[1], out[2]
                        assert fused or not Rr, f"LDS fall-back reached: G={G} Cg={Cg} H={H} {dname} backward={backward} dres={dres}"
                        assert out[5] <= 64 * 1024 and out[6] <= 64 * 1024 and 1 <= out[4] <= 1024
                        seen.add(_key(backward, dname, (fused, N, Rr), True, dres))
    unreachable = {k for k in seen if k[:4] == ("bwd", "bf16", 1, 8) and not k[6]}
    assert not unreachable, f"bf16 backward N = 8 without dres is now reachable: {sorted(unreachable)}"
    assert not seen - table, f"reached by a legal shape but by no case of the table: {sorted(seen - table)}"
    assert {k for k in _required_keys() if k[5]} <= seen
