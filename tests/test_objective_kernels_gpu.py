"""-m gpu: psg_diffusion_loss_f32, psg_guided_update_pred_f32 and psg_pred_to_eps_f32 through the C ABI against
tests/objective_ref.py: the target and the two sampler entries on the bits of the float32 restatements, the weighted loss and
its gradient element by element within the bounds derived there.  Every device buffer sits between guard words that must keep
their bits; outputs start as NaN; inputs must keep their bits; every comparison prints `RATIO <what> <err / bound>` before it
asserts (0 = a bit comparison).

Loss shapes (B, chw): (1, 1), (3, 7) (scalar path, a ragged block), (5, 1001) (odd row: scalar path, several blocks),
(2, 5832) (one latent batch pair: float4 path, rows of 1458 float4s) and (91, 5832) = 530 712 elements, past 2 RED_CAP + 333
(three trips of the scalar grid, more than one of the float4 grid's blocks per lane).  t holds 0, 260, 261 (either side of the
gamma = 5 truncation), 999 and repeats."""
import itertools

import numpy as np
import pytest
import torch

from tests import guided_ref as G
from tests import objective_ref as O
from tests import step_ref as R
from tests.test_guided_kernels_gpu import CLIPS, JS, K_STEPS, NS as GUIDED_NS, WS, _combos, _inputs
from tests.test_step_kernels_gpu import Dev, _all_ok, _bitcheck, _check, _i32, _note, _run, _stream, _ws

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (3, 7), (5, 1001), (2, 5832), (91, 5832)]
BETA, SCALE, GAMMA, NUM_T = 0.1, 0.37, 5.0, 1000
T_PATTERN = [0, 260, 261, 999, 999, 500, 0, 261, 260, 17]
NS = [1, 3, 4, 7, 5832, 2 * 5832 + 1, R.GRID_CAP * 4 + 5]
assert NS == GUIDED_NS and SHAPES[-1][0] * SHAPES[-1][1] > 2 * R.RED_CAP + 333


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    return _lib.init(0)


@pytest.fixture(scope="module")
def sched():
    """(abar, tabA, tabB, {prediction: wtab}) fp32 numpy of stage 2's schedule; the weights from the restatement
    (test_objective_ref_cpu holds the package's to it on the bits)."""
    import pokemon_sprite_generator_amd as psg
    s = psg.NoiseScheduler()
    abar, tabA, tabB = (getattr(s, n).cpu().numpy().astype(np.float32) for n in ("alphas_cumprod", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"))
    return abar, tabA, tabB, {p: O.min_snr_weights(abar, GAMMA, p) for p in (O.PRED_EPS, O.PRED_V)}


_CASES = {}


def _case(B, chw, sched):
    """x0 ~ N(0, 2^2), noise ~ N(0, 1), t from T_PATTERN, and per prediction pred = target(do_clamp = 1) + N(0, 0.1^2).  Shared
    among the tests and never written."""
    if (B, chw) not in _CASES:
        _, tabA, tabB, _ = sched
        rng = np.random.default_rng(B * 100003 + chw)
        x0 = (2.0 * rng.standard_normal((B, chw))).astype(np.float32)
        noise = rng.standard_normal((B, chw)).astype(np.float32)
        t = np.array((T_PATTERN * (B // len(T_PATTERN) + 1))[:B], dtype=np.int64)
        res = (0.1 * rng.standard_normal((B, chw))).astype(np.float32)
        pred = {p: (O.target(p, x0, noise, t, tabA, tabB, 1) + res).astype(np.float32) for p in (O.PRED_EPS, O.PRED_V)}
        _CASES[(B, chw)] = (x0, noise, t, pred)
    return _CASES[(B, chw)]


def _launch_loss(lib, b, prediction, has_w, do_clamp, with_grad, with_tgt, B, chw, what, n_out, off=0, flag_init=0, with_flag=True, num_t=NUM_T):
    grad, tgt, loss, flag = Dev(n=n_out, off=off), Dev(n=n_out, off=off), Dev(n=1), _i32(flag_init)
    ws = _ws(lib, lib.psg_reduce_workspace_bytes())
    _run(lib.psg_diffusion_loss_f32(b["pred"].ptr(), b["x0"].ptr() if "x0" in b else None, b["noise"].ptr(), b["t"].ptr(),
                                    b["tabA"].ptr() if "tabA" in b else None, b["tabB"].ptr() if "tabB" in b else None,
                                    b["wtab"].ptr() if has_w else None, prediction, grad.ptr() if with_grad else None,
                                    tgt.ptr() if with_tgt else None, loss.ptr(), flag.ptr() if with_flag else None, BETA, SCALE, B, chw, num_t,
                                    do_clamp, ws.ptr(), _stream()), what)
    _all_ok(b, what)
    assert grad.intact() and tgt.intact() and loss.intact() and flag.intact() and ws.intact(), f"{what}: a store outside an output or behind the workspace"
    if not with_grad:
        assert bool(torch.isnan(grad.v).all()), f"{what}: grad = NULL was written"
    if not with_tgt:
        assert bool(torch.isnan(tgt.v).all()), f"{what}: target_out = NULL was written"
    return loss.cpu().clone(), grad.cpu().clone(), tgt.cpu().clone(), int(flag.cpu()[0])


def _loss_cross(lib, sched, B, chw, prediction, off=0):
    _, tabA, tabB, wtabs = sched
    x0, noise, t, preds = _case(B, chw, sched)
    pred = preds[prediction]
    n = B * chw
    vec = O.loss_is_vec(chw, aligned=off == 0)
    b = dict(pred=Dev(pred, off=off), x0=Dev(x0, off=off), noise=Dev(noise, off=off), t=Dev(t), tabA=Dev(tabA), tabB=Dev(tabB),
             wtab=Dev(wtabs[prediction]))
    for has_w, do_clamp in itertools.product([False, True], [0, 1]):
        tag = f"diffusion_loss {B}x{chw} pred={prediction} w={has_w} clamp={do_clamp} off={off}"
        ref = O.diffusion_loss(pred, x0, noise, t, tabA, tabB, wtabs[prediction] if has_w else None, prediction, BETA, SCALE, do_clamp, vec)
        want_tg = O.target(prediction, x0, noise, t, tabA, tabB, do_clamp)
        if n >= 1000:                                   # on the reference alone: the case exercises both branches and the clamp
            d = np.abs(pred.astype(np.float64) - want_tg)
            quad, clamped = float((d < R.f32(BETA)).mean()), float((np.abs(x0) > 3).mean())
            print(f"SHARES {tag}: quadratic {quad:.3f}, linear {1 - quad:.3f}, clamped {clamped:.3f}")
            assert quad >= 0.2 and 1 - quad >= 0.2 and 0.05 <= clamped <= 0.25
        runs = {}
        for with_grad, with_tgt in itertools.product([True, False], repeat=2):
            what = f"{tag} grad={with_grad} target_out={with_tgt}"
            loss, grad, tg, flag = _launch_loss(lib, b, prediction, has_w, do_clamp, with_grad, with_tgt, B, chw, what, n, off)
            assert flag == 0, f"{what}: flag word {flag}"
            runs[(with_grad, with_tgt)] = (loss, grad, tg)
        again = _launch_loss(lib, b, prediction, has_w, do_clamp, True, True, B, chw, tag + " again", n, off)
        first = runs[(True, True)]
        assert all(R.same_bits(again[i], first[i]) for i in range(3)), f"{tag}: a second identical launch gives other bits"
        for key, (loss, grad, tg) in runs.items():
            assert R.same_bits(loss, first[0]), f"{tag}: grad / target_out = NULL ({key}) changes the loss"
            if key[0]:
                assert R.same_bits(grad, first[1]), f"{tag}: target_out = NULL changes the gradient"
            if key[1]:
                assert R.same_bits(tg, first[2])
        _bitcheck("diffusion_loss target", tag + " target", first[2].numpy().reshape(B, chw), want_tg)
        r = torch.as_tensor(ref["loss"], dtype=torch.float64).reshape(1)
        _check("diffusion_loss loss", tag + " loss", first[0].reshape(1), r, r.abs(), ref["depth_loss"], extra=ref["extra_loss"])
        _check("diffusion_loss grad", tag + " grad", first[1], ref["grad"], ref["S_grad"], ref["depth_grad"], extra=ref["extra_grad"].reshape(-1))


@pytest.mark.parametrize("prediction", [O.PRED_EPS, O.PRED_V], ids=["eps", "v"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_diffusion_loss(lib, sched, shape, prediction):
    _loss_cross(lib, sched, shape[0], shape[1], prediction)


@pytest.mark.parametrize("prediction", [O.PRED_EPS, O.PRED_V], ids=["eps", "v"])
def test_diffusion_loss_every_pointer_off_the_boundary(lib, sched, prediction):
    """chw % 4 == 0 with pred, x0, noise, grad and target_out one float off the 16-byte boundary: the element-by-element path."""
    _loss_cross(lib, sched, 2, 5832, prediction, off=1)


def test_diffusion_loss_eps_needs_no_x0_and_no_tables(lib, sched):
    _, tabA, tabB, wtabs = sched
    B, chw = 3, 7
    x0, noise, t, preds = _case(B, chw, sched)
    b = dict(pred=Dev(preds[O.PRED_EPS]), noise=Dev(noise), t=Dev(t), wtab=Dev(wtabs[O.PRED_EPS]))
    loss, grad, tg, flag = _launch_loss(lib, b, O.PRED_EPS, True, 1, True, True, B, chw, "diffusion_loss eps without x0", B * chw)
    full = dict(b, x0=Dev(x0), tabA=Dev(tabA), tabB=Dev(tabB))
    want = _launch_loss(lib, full, O.PRED_EPS, True, 1, True, True, B, chw, "diffusion_loss eps with x0", B * chw)
    assert flag == 0 and R.same_bits(loss, want[0]) and R.same_bits(grad, want[1]) and R.same_bits(tg, torch.from_numpy(noise).reshape(-1))
    _note("diffusion_loss target", "diffusion_loss eps without x0", 0.0)


@pytest.mark.parametrize("case", ["nan-pred", "inf-pred", "inf-x0-v", "inf-x0-v-clamped", "t-minus-1", "t-num_t", "nan-pred-no-flag"])
def test_diffusion_loss_flags(lib, sched, case):
    """PRED_BAD for a non-finite pred, LOSS_BAD for a non-finite loss (an infinite x0 under v makes the target infinite - unless
    the clamp, add_noise's own, brings it to 3), T_RANGE for a t outside the table, which reads the nearest entry.  The word is
    OR-ed, never cleared; nan_flag = NULL is legal."""
    _, tabA, tabB, wtabs = sched
    B, chw = 5, 1001
    x0, noise, t, preds = _case(B, chw, sched)
    x0, t, pred = x0.copy(), t.copy(), preds[O.PRED_V].copy()
    do_clamp = 1
    if case.endswith("pred") or case.endswith("no-flag"):
        pred[2, chw // 2] = np.inf if case == "inf-pred" else np.nan
    elif case.startswith("inf-x0"):
        x0[1, 5] = np.inf
        do_clamp = 1 if case.endswith("clamped") else 0
    else:
        t[3] = -1 if case == "t-minus-1" else NUM_T
    want_tg = O.target(O.PRED_V, x0, noise, t, tabA, tabB, do_clamp)
    want = O.loss_flags(pred, want_tg, t, NUM_T)
    assert want == {"nan-pred": 12, "inf-pred": 12, "inf-x0-v": 8, "inf-x0-v-clamped": 0, "t-minus-1": 2, "t-num_t": 2, "nan-pred-no-flag": 12}[case]
    b = dict(pred=Dev(pred), x0=Dev(x0), noise=Dev(noise), t=Dev(t), tabA=Dev(tabA), tabB=Dev(tabB), wtab=Dev(wtabs[O.PRED_V]))
    # (Dev.kept compares bits: the planted NaN / infinity included)
    loss, grad, tg, flag = _launch_loss(lib, b, O.PRED_V, True, do_clamp, True, True, B, chw, f"diffusion_loss {case}", B * chw,
                                        flag_init=R.FLAG_FALLBACK, with_flag=not case.endswith("no-flag"))
    assert flag == (R.FLAG_FALLBACK if case.endswith("no-flag") else R.FLAG_FALLBACK | want), f"{case}: flag word {flag}"
    assert R.same_bits(tg.numpy().reshape(B, chw), want_tg)
    assert bool(torch.isfinite(loss).all()) == (not want & R.FLAG_LOSS_BAD)
    if case.startswith("t-"):                                       # the nearest entry was read: the loss is the clipped t's
        ref = O.diffusion_loss(pred, x0, noise, t, tabA, tabB, wtabs[O.PRED_V], O.PRED_V, BETA, SCALE, do_clamp, False)
        r = torch.as_tensor(ref["loss"], dtype=torch.float64).reshape(1)
        _check("diffusion_loss loss", f"diffusion_loss {case} loss", loss.reshape(1), r, r.abs(), ref["depth_loss"], extra=ref["extra_loss"])
    _note("diffusion_loss flags", f"diffusion_loss {case}", 0.0)


# ------------------------------------------------------------------------------------------------ guided_update_pred
@pytest.fixture(scope="module")
def tab(sched):
    return G.ddim_tables(sched[0], G.ddim_timesteps(NUM_T, K_STEPS), 0.7)


def _v_inputs(n, tab, j):
    """x = S0 x0 + S1 e_c of test_guided_kernels_gpu's inputs (x0 by index % 3: clamped at clip 0.25 only / never / always) and
    the v that belong to (x0, e_c) and (x0, e_u)."""
    x0, ec, eu, z = _inputs(n)
    jc = min(max(j, 0), K_STEPS - 1)
    s0, s1 = tab[0, jc], tab[1, jc]
    x = (s0 * x0 + s1 * ec).astype(np.float32)
    return x, (s0 * ec - s1 * x0).astype(np.float32), (s0 * eu - s1 * x0).astype(np.float32), z


@pytest.mark.parametrize("copy", ["none", "adjacent", "separate"])
@pytest.mark.parametrize("n", NS)
def test_guided_update_pred_v(lib, tab, n, copy):
    clamped = total = 0
    for has_u, has_z, j, w, clip in _combos(n):
        what = f"guided_update_pred v n={n} copy={copy} u={has_u} z={has_z} j={j} w={w} clip={clip}"
        x, vc, vu, z = _v_inputs(n, tab, j)
        want = O.guided_update_pred(x, vc, vu if has_u else None, z if has_z else None, tab, j, w, clip, O.PRED_V)
        if clip > 0:
            jc = min(max(j, 0), K_STEPS - 1)
            p = G.cfg_combine(vc, vu, w) if has_u else vc
            x0 = ((tab[0, jc] * x).astype(np.float32) - (tab[1, jc] * p).astype(np.float32)).astype(np.float32)
            clamped, total = clamped + int((np.abs(x0) > clip).sum()), total + n
        tb, cb_, ub, zb = Dev(tab), Dev(vc), Dev(vu), Dev(z)
        if copy == "adjacent":                                   # the 2n input buffer: x_copy = x + n, unaligned for odd n
            xb = Dev(np.concatenate([x, np.full(n, 77.0, dtype=np.float32)]))
            xp, cp = xb.ptr(), xb.ptr() + 4 * n
        else:
            xb = Dev(x)
            cb = Dev(np.full(n, 77.0, dtype=np.float32)) if copy == "separate" else None
            xp, cp = xb.ptr(), (cb.ptr() if cb is not None else None)
        sb = _i32(j)
        _run(lib.psg_guided_update_pred_f32(xp, cp, cb_.ptr(), ub.ptr() if has_u else None, zb.ptr() if has_z else None, tb.ptr(), K_STEPS,
                                            sb.ptr(), w, clip, n, O.PRED_V, _stream()), what)
        _all_ok(dict(tab=tb, pred_c=cb_, pred_u=ub, z=zb, step=sb), what)
        assert xb.intact(), what
        got = xb.np()
        _bitcheck("guided_update_pred", what, got[:n], want)
        if copy == "adjacent":
            assert R.same_bits(got[n:], want), f"{what}: x_copy"
        elif copy == "separate":
            assert cb.intact() and R.same_bits(cb.np(), want), f"{what}: x_copy"
    share = clamped / total
    print(f"CLAMPED SHARE guided_update_pred n={n} copy={copy}: {share:.3f} of {total} elements over the launches with clip > 0")
    assert 0.0 < share < 1.0


@pytest.mark.parametrize("n", [7, 5832, 2 * 5832 + 1])
def test_guided_update_pred_eps_is_guided_update_on_the_bits(lib, tab, n):
    x0, ec, eu, z = _inputs(n)
    for has_u, has_z, j, w, clip in _combos(7):
        if j not in (0, K_STEPS - 1, K_STEPS) or w not in (7.5, -1.0):
            continue
        what = f"guided_update_pred eps n={n} u={has_u} z={has_z} j={j} w={w} clip={clip}"
        jc = min(max(j, 0), K_STEPS - 1)
        x = (tab[0, jc] * x0 + tab[1, jc] * ec).astype(np.float32)
        outs = []
        for entry in ("pred", "plain"):
            xb, sb = Dev(np.concatenate([x, np.full(n, 77.0, dtype=np.float32)])), _i32(j)
            b = dict(tab=Dev(tab), eps_c=Dev(ec), eps_u=Dev(eu), z=Dev(z), step=sb)
            a = (xb.ptr(), xb.ptr() + 4 * n, b["eps_c"].ptr(), b["eps_u"].ptr() if has_u else None, b["z"].ptr() if has_z else None, b["tab"].ptr(),
                 K_STEPS, sb.ptr(), w, clip, n)
            rc = lib.psg_guided_update_pred_f32(*a, O.PRED_EPS, _stream()) if entry == "pred" else lib.psg_guided_update_f32(*a, _stream())
            _run(rc, what)
            _all_ok(b, what)
            assert xb.intact()
            outs.append(xb.np())
        want = G.guided_update(x, ec, eu if has_u else None, z if has_z else None, tab, j, w, clip)
        _bitcheck("guided_update_pred", what, outs[0], np.concatenate([want, want]))
        assert R.same_bits(outs[0], outs[1]), f"{what}: not psg_guided_update_f32's bits"


@pytest.mark.parametrize("n", [7, 5832])
def test_guided_update_pred_nan_stays_where_it_is(lib, tab, n):
    x, vc, vu, z = _v_inputs(n, tab, 3)
    vc = vc.copy()
    at = n // 2
    vc[at] = np.nan
    for clip in (0.0, 3.0):
        for has_u in (False, True):
            xb, sb = Dev(np.concatenate([x, x])), _i32(3)
            b = dict(tab=Dev(tab), pred_c=Dev(vc), pred_u=Dev(vu), z=Dev(z), step=sb)
            _run(lib.psg_guided_update_pred_f32(xb.ptr(), xb.ptr() + 4 * n, b["pred_c"].ptr(), b["pred_u"].ptr() if has_u else None, b["z"].ptr(),
                                                b["tab"].ptr(), K_STEPS, sb.ptr(), 2.0, clip, n, O.PRED_V, _stream()), f"guided_update_pred NaN n={n}")
            got = xb.np()
            want = O.guided_update_pred(x, vc, vu if has_u else None, z, tab, 3, 2.0, clip, O.PRED_V)
            nan = np.isnan(got[:n])
            assert nan[at] and int(nan.sum()) == 1 and R.same_bits(got[:n], want) and R.same_bits(got[n:], want)
            assert xb.intact() and all(v.intact() for v in b.values()) and b["pred_u"].kept() and b["z"].kept() and b["tab"].kept()
    _note("guided_update_pred", f"guided_update_pred NaN n={n}", 0.0)


# -------------------------------------------------------------------------------------------------------- pred_to_eps
@pytest.mark.parametrize("alias", [False, True], ids=["out", "in-place"])
@pytest.mark.parametrize("prediction", [O.PRED_EPS, O.PRED_V], ids=["eps", "v"])
@pytest.mark.parametrize("n", NS)
def test_pred_to_eps(lib, sched, n, prediction, alias):
    _, tabA, tabB, _ = sched
    x, pc, pu, _ = _inputs(n)
    ts = [0, 260, 999, -1, NUM_T] if n < 100000 else [261, NUM_T + 5]
    xb, ub, ab, bb = Dev(x), Dev(pu), Dev(tabA), Dev(tabB)
    for i, t in enumerate(ts):
        for has_u in (False, True):
            w = WS[(i + has_u) % len(WS)]
            what = f"pred_to_eps n={n} pred={prediction} alias={alias} u={has_u} t={t} w={w}"
            cb, tb = Dev(pc), _i32(t)
            ob = cb if alias else Dev(n=n)
            _run(lib.psg_pred_to_eps_f32(xb.ptr(), cb.ptr(), ub.ptr() if has_u else None, w, ab.ptr(), bb.ptr(), NUM_T, tb.ptr(), prediction,
                                         ob.ptr(), n, _stream()), what)
            assert xb.kept() and ub.kept() and ab.kept() and bb.kept() and tb.kept() and ob.intact() and (alias or cb.kept()), what
            _bitcheck("pred_to_eps", what, ob.np(), O.pred_to_eps(x, pc, pu if has_u else None, w, tabA, tabB, t, prediction))
    if n >= 4:                                                     # bases off the 16-byte boundary: the element-by-element path
        x1, cb, u1, ob, tb = Dev(x, off=3), Dev(pc, off=1), Dev(pu, off=2), Dev(n=n, off=3), _i32(500)
        _run(lib.psg_pred_to_eps_f32(x1.ptr(), cb.ptr(), u1.ptr(), 7.5, ab.ptr(), bb.ptr(), NUM_T, tb.ptr(), prediction, ob.ptr(), n, _stream()),
             "pred_to_eps unaligned")
        assert x1.kept() and cb.kept() and u1.kept() and ob.intact()
        _bitcheck("pred_to_eps", f"pred_to_eps unaligned n={n} pred={prediction}", ob.np(), O.pred_to_eps(x, pc, pu, 7.5, tabA, tabB, 500, prediction))


def test_pred_to_eps_eps_mode_reads_no_x_and_no_table(lib):
    n = 5832
    _, pc, pu, _ = _inputs(n)
    cb, ub, ob, tb = Dev(pc), Dev(pu), Dev(n=n), _i32(3)
    _run(lib.psg_pred_to_eps_f32(None, cb.ptr(), ub.ptr(), 2.5, None, None, NUM_T, tb.ptr(), O.PRED_EPS, ob.ptr(), n, _stream()), "pred_to_eps eps bare")
    assert cb.kept() and ub.kept() and ob.intact()
    _bitcheck("pred_to_eps", "pred_to_eps eps without x and tables", ob.np(), G.cfg_combine(pc, pu, 2.5))
    c2 = Dev(pc)                                                   # unguided and in place: eps already - nothing is launched or written
    _run(lib.psg_pred_to_eps_f32(None, c2.ptr(), None, 2.5, None, None, NUM_T, tb.ptr(), O.PRED_EPS, c2.ptr(), n, _stream()), "pred_to_eps eps no-op")
    assert c2.kept()
