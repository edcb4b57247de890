"""CPU suite for the step-kernel tests: the references of tests/step_ref.py agree with torch's own fp64 operations and with
the restatements of oracle/; every bound admits the kernel's arithmetic restated in fp32 and rejects a planted mistake at the
shapes of tests/step_cases.py; the fp32 restatement of every reduction uses at most half of its bound; and the host-only
refusals of the launchers, with their codes and messages - nothing here launches a kernel."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import step_cases as K
from tests import step_ref as R

FAKE = 0x7F0000000000          # a 16-byte aligned address nothing dereferences: every call below returns before a launch
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def _close(a, b, rtol=1e-12):
    return torch.allclose(torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64), rtol=rtol, atol=1e-300)


# ------------------------------------------------------------------------------------- references against torch's own fp64
def test_smooth_l1_reference_is_torchs():
    pred, target = K.smooth_l1_inputs(K.N_SMALL)
    p = pred.double().requires_grad_(True)
    loss = F.smooth_l1_loss(p, target.double(), beta=R.f32(K.SL1_BETA))
    loss.backward()
    ref, _, g, _, _ = R.smooth_l1(pred, target, K.SL1_BETA, K.SL1_SCALE)
    assert _close(ref, loss.detach()) and _close(g, p.grad * R.f32(K.SL1_SCALE))
    from oracle import unet_oracle as O
    assert _close(ref, O.smooth_l1(pred.double(), target.double(), R.f32(K.SL1_BETA)))


@pytest.mark.parametrize("w", K.RECON_W, ids=str)
def test_recon_loss_reference_is_torchs(w):
    pred, target = K.recon_inputs(K.N_SMALL)
    w1, w2 = R.f32(w[0]), R.f32(w[1])
    p = pred.double().requires_grad_(True)
    l1, mse = F.l1_loss(p, target.double()), F.mse_loss(p, target.double())
    (w1 * l1 + w2 * mse).backward()
    out3, _, g, S, _ = R.recon_loss(pred, target, *w)
    assert _close(out3, torch.stack([w1 * l1 + w2 * mse, l1, mse]).detach()) and _close(g, p.grad)
    assert bool((g[torch.arange(8) * (K.N_SMALL // 8)] == 0).all())                # sign(0) = 0, as autograd's
    assert bool((S >= g.abs() * (1 - 1e-12)).all())


def test_reparam_references_are_autograds():
    mu, lv, ep = K.reparam_inputs(K.N_SMALL)
    m, l = mu.double().requires_grad_(True), lv.double().requires_grad_(True)
    out = m + ep.double() * torch.exp(0.5 * l)
    d = K.h((K.N_SMALL,), "step.rp.d", 1.0)
    out.backward(d.double())
    assert _close(R.reparam(mu, lv, ep)[0], out.detach())
    (dm, _, depth), (dl, _, _, _) = R.reparam_bwd(d, lv, ep)
    assert _close(dm, m.grad) and _close(dl, l.grad) and depth == 0
    pm, pl = K.h((K.N_SMALL,), "step.rp.pm", 1.0), K.h((K.N_SMALL,), "step.rp.pl", 1.0)
    (dm, _, _), (dl, _, _, _) = R.reparam_bwd(d, lv, ep, pm, pl)
    assert _close(dm, pm.double() + m.grad) and _close(dl, pl.double() + l.grad)


@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("norm", [None, K.NORM_ABOVE, K.NORM_BELOW], ids=["no-clip", "clip", "clip-idle"])
def test_adamw_reference_is_torch_optim_adamw(step, norm):
    """torch.optim.AdamW on fp64 parameters after clip_grad_norm_, from the state of `step - 1` steps.  clip_grad_norm_ takes
    the norm of the gradient it is given, so the gradient is scaled to the squared norm the case stores (to fp64 rounding;
    the reference reads that norm as an fp32 scalar, hence 1e-6)."""
    kw = K.adam_kw({})
    p, g, m, v = K.adam_inputs(1000)
    lr, b1, b2, eps, wd = (R.f32(kw[k]) for k in ("lr", "beta1", "beta2", "eps", "wd"))
    gd = g.double()
    if norm is not None:
        gd = gd * math.sqrt(R.f32(norm[0]) / float(gd.pow(2).sum()))
    q = torch.nn.Parameter(p.double())
    opt = torch.optim.AdamW([q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.double().clone(), "exp_avg_sq": v.double().clone()}
    q.grad = gd.clone()
    if norm is not None:
        torch.nn.utils.clip_grad_norm_([q], R.f32(norm[1]))
    opt.step()
    ref = R.adamw(p.double(), gd, m, v, step, **_akw(kw), normsq=None if norm is None else norm[0], max_norm=0.0 if norm is None else norm[1])
    rtol = 1e-12 if norm is None else 1e-6
    assert _close(ref["p"][0], q.detach(), rtol) and _close(ref["m"][0], opt.state[q]["exp_avg"], rtol)
    assert _close(ref["v"][0], opt.state[q]["exp_avg_sq"], rtol)
    if norm is None:
        from oracle import unet_oracle as O
        po, mo, vo = O.adamw_update(p.double(), gd, m.double(), v.double(), step, lr, b1, b2, eps, wd)
        assert _close(ref["p"][0], po) and _close(ref["m"][0], mo) and _close(ref["v"][0], vo)
    else:
        from oracle import unet_oracle as O
        assert math.isclose(R.clip_coef(*norm), O.clip_coef(math.sqrt(R.f32(norm[0])), R.f32(norm[1])), rel_tol=1e-6)


def _akw(kw):
    return dict(lr=kw["lr"], beta1=kw["beta1"], beta2=kw["beta2"], eps=kw["eps"], wd=kw["wd"])


def test_clip_scale_reference_is_clip_grad_norm():
    g = K.h((K.N_SMALL,), "step.clip.g", 1.0).double()
    for name, (nsq, mx) in K.CLIP.items():
        gd = g * math.sqrt(R.f32(nsq) / float(g.pow(2).sum()))
        q = torch.nn.Parameter(torch.zeros_like(gd))
        q.grad = gd.clone()
        torch.nn.utils.clip_grad_norm_([q], R.f32(mx))
        assert _close(R.clip_scale(gd, nsq, mx)[0], q.grad, 1e-6), name
    assert R.clip_coef(*K.CLIP["below"]) == 1.0 and R.clip_coef(*K.CLIP["above"]) < 0.6 and 0.999 < R.clip_coef(*K.CLIP["at"]) < 1.0


def test_bit_exact_restatements_agree_with_torch_and_the_oracle():
    """numpy float32, one operation at a time, against the same expressions in torch fp32 on the CPU and oracle/'s own."""
    from oracle import unet_oracle as O
    B, chw = K.NOISE_SHAPES[0]
    tabA, tabB = K.noise_tables()
    x0, noise, t = K.noise_inputs(B, chw, False)
    x0[0, 5] = 0.5                                             # no NaN: the oracle would take its fallback
    out, flag = R.noise_add(x0, noise, t, tabA, tabB, 0)
    want = O.add_noise(torch.from_numpy(x0).view(B, chw, 1, 1), torch.from_numpy(noise).view(B, chw, 1, 1), torch.from_numpy(t), O.cosine_clipped_tables(K.NUM_T))
    assert flag == 0 and R.same_bits(out, want.view(B, chw).numpy())
    outc, _ = R.noise_add(x0, noise, t, tabA, tabB, 1)
    a, c = torch.from_numpy(tabA)[t].view(-1, 1), torch.from_numpy(tabB)[t].view(-1, 1)
    assert R.same_bits(outc, (a * torch.from_numpy(x0).clamp(-3, 3) + c * torch.from_numpy(noise)).numpy())
    assert R.noise_add(x0, noise, np.where(np.arange(B) == 1, -1, t), tabA, tabB, 0)[1] == R.FLAG_T_RANGE
    x, e, z = (torch.from_numpy(v) for v in K.xez(K.N_SMALL, "cpu"))
    fb, bad = R.noise_fallback(x.numpy(), z.numpy(), 0)
    assert bad == 0 and R.same_bits(fb, (x + 0.1 * z).numpy())
    c1, c2, sg = (torch.from_numpy(v) for v in K.ddpm_tables())
    assert R.same_bits(R.ddpm_update(x.numpy(), e.numpy(), z.numpy(), c1.numpy(), c2.numpy(), sg.numpy(), 5), (c1[5] * (x - c2[5] * e) + sg[5] * z).numpy())
    assert R.same_bits(R.ddpm_update(x.numpy(), e.numpy(), z.numpy(), c1.numpy(), c2.numpy(), sg.numpy(), 0), (c1[0] * (x - c2[0] * e)).numpy())
    # mode 1 is oracle/'s sample_previous_timestep with its own tables; mode 3 the demo sampler's two lines; mode 2 x - eps
    tb, ts = O.final_linear_tables(), 500
    c = (tb["sqrt_recip_alphas"][ts], tb["betas"][ts], tb["sqrt_one_minus_alphas_cumprod"][ts], torch.sqrt(tb["posterior_variance"][ts]))
    got = R.sampler_update(x.numpy(), e.numpy(), z.numpy(), 1, *(float(v) for v in c))
    assert R.same_bits(got, O.sample_previous_timestep(x, e, ts, tb, z).numpy())
    c0, c1_, c2_, c3 = (torch.tensor(v, dtype=F32) for v in K.SAMPLER_C)
    assert R.same_bits(R.sampler_update(x.numpy(), e.numpy(), z.numpy(), 3, *K.SAMPLER_C), (c2_ * ((x - c0 * e) / c1_) + c3 * z).numpy())
    assert R.same_bits(R.sampler_update(x.numpy(), e.numpy(), None, 3, *K.SAMPLER_C), ((x - c0 * e) / c1_).numpy())
    assert R.same_bits(R.sampler_update(x.numpy(), e.numpy(), None, 2, *K.SAMPLER_C), (x - e).numpy())


@pytest.mark.parametrize("n", K.STREAM_N)
def test_sampler_division_order_is_visible_in_the_bits(n):
    """Mode 1 with the division before the multiplication differs by an ulp in places: the bit comparison sees it."""
    x, e, z = K.xez(n, "samp")
    good = R.sampler_update(x, e, z, 1, *K.SAMPLER_C)
    bad = R.sampler_update(x, e, z, 1, *K.SAMPLER_C, mistake="div_first")
    assert R.same_bits(good, good.copy()) and not R.same_bits(bad, good)
    assert float(np.abs(bad.astype(np.float64) - good).max()) <= 2.0 ** -22 * float(np.abs(good).max())      # and it is an ulp, no more


def test_same_bits_treats_nan_by_position():
    a = torch.tensor([1.0, float("nan"), -0.0])
    assert R.same_bits(a, a.clone()) and not R.same_bits(a, torch.tensor([1.0, float("nan"), 0.0]))
    assert not R.same_bits(torch.tensor([1.0, 2.0, -0.0]), a) and not R.same_bits(a, torch.tensor([float("nan"), float("nan"), -0.0]))


# -------------------------------------------------------------------------------------------------- planted mistakes
def _chk(got, ref, S, depth, what, extra=None):
    return R.check(got, ref, S, F32, what, depth, extra=extra)


@pytest.mark.parametrize("n", K.STREAM_N)
def test_reparam_bounds_notice_exp_of_logvar(n):
    mu, lv, ep = K.reparam_inputs(n)
    d = K.h((n,), f"step.rp.d.{n}", 1.0)
    ref, S, depth, extra = R.reparam(mu, lv, ep)
    _chk(R.reparam(mu, lv, ep, dtype=F32)[0], ref, S, depth, "reparam fp32", extra)
    assert _fails(lambda: _chk(R.reparam(mu, lv, ep, dtype=F32, mistake="exp_logvar")[0], ref, S, depth, "reparam", extra))
    pm, pl = K.h((n,), f"step.rp.pm.{n}", 0.77), K.h((n,), f"step.rp.pl.{n}", 0.77)
    for prev in ((None, None), (pm, pl)):
        (rm, Sm, dm), (rl, Sl, dl, xl) = R.reparam_bwd(d, lv, ep, *prev)
        (gm, _, _), (gl, _, _, _) = R.reparam_bwd(d, lv, ep, *prev, dtype=F32)
        _chk(gm, rm, Sm, dm, "reparam_bwd dmu fp32")
        _chk(gl, rl, Sl, dl, "reparam_bwd dlogvar fp32", xl)
        bad = R.reparam_bwd(d, lv, ep, *prev, dtype=F32, mistake="exp_logvar")[1][0]
        assert _fails(lambda: _chk(bad, rl, Sl, dl, "reparam_bwd", xl))
        if prev[0] is not None:
            assert _fails(lambda: _chk(d, rm, Sm, dm, "reparam_bwd dmu overwritten"))


@pytest.mark.parametrize("n", K.RED_N)
def test_smooth_l1_bounds_notice_planted_mistakes(n):
    pred, target = K.smooth_l1_inputs(n)
    loss, dl, g, S, dg = R.smooth_l1(pred, target, K.SL1_BETA, K.SL1_SCALE)
    l32, _, g32, _, _ = R.smooth_l1(pred, target, K.SL1_BETA, K.SL1_SCALE, dtype=F32)
    assert R.check_scalar(l32, loss, dl, "smooth_l1 loss fp32") <= 0.5          # the condition: half of the bound at most
    _chk(g32, g, S, dg, "smooth_l1 grad fp32")
    nq = int(((pred.double() - target.double()).abs() < R.f32(K.SL1_BETA)).sum())
    assert 0.05 * n < nq < 0.95 * n                                             # both branches, in numbers
    for mistake in ("no_div_beta", "n_minus_1") + (("drop_trip",) if n > R.RED_CAP else ()):
        lb, _, gb, _, _ = R.smooth_l1(pred, target, K.SL1_BETA, K.SL1_SCALE, dtype=F32, mistake=mistake)
        seen_loss = _fails(lambda: R.check_scalar(lb, loss, dl, mistake))
        seen_grad = _fails(lambda: _chk(gb, g, S, dg, mistake))
        if mistake == "drop_trip":
            assert seen_loss
        elif mistake == "n_minus_1" and n > R.RED_CAP:
            # 1 / (n - 1) is 1 / n (1 + 2^-19) here, 32 x 2^-24: inside the 37 x 2^-24 a sum of three trips and its tree may
            # lose, so the scalar cannot see it at this size - the gradient (9 x 2^-24) does
            assert seen_grad
        else:
            assert seen_loss and seen_grad, mistake
    # |d| 8 ulps below beta sits in the quadratic branch: the linear branch's +-1 there is outside the bound
    k = 2 + 4 * K.SL1_ULPS.index(8) + 2
    d = pred[k].double() - target[k].double()
    assert 0 < float(d) < R.f32(K.SL1_BETA)
    flipped = g32.clone(); flipped[k] = float(torch.sign(d)) * R.f32(K.SL1_SCALE) / n
    assert _fails(lambda: _chk(flipped, g, S, dg, "branch"))


@pytest.mark.parametrize("n", K.RED_N)
@pytest.mark.parametrize("w", K.RECON_W, ids=str)
def test_recon_loss_bounds_notice_planted_mistakes(n, w):
    pred, target = K.recon_inputs(n)
    out3, d3, g, S, dg = R.recon_loss(pred, target, *w)
    o32, _, g32, _, _ = R.recon_loss(pred, target, *w, dtype=F32)
    for i in range(3):
        assert R.check_scalar(o32[i], out3[i], d3[i], f"recon out3[{i}] fp32") <= 0.5
    _chk(g32, g, S, dg, "recon grad fp32")
    mistakes = ["n_minus_1"] + (["sign0_is_1"] if w[0] else []) + (["mse_no_2"] if w[1] else []) + (["drop_trip"] if n > R.RED_CAP else [])
    for mistake in mistakes:
        ob, _, gb, _, _ = R.recon_loss(pred, target, *w, dtype=F32, mistake=mistake)
        if mistake == "drop_trip":
            assert all(_fails(lambda: R.check_scalar(ob[i], out3[i], d3[i], mistake)) for i in (1, 2))
        else:
            assert _fails(lambda: _chk(gb, g, S, dg, mistake)), mistake
        if mistake == "n_minus_1" and n <= R.RED_CAP:
            assert _fails(lambda: R.check_scalar(ob[1], out3[1], d3[1], mistake))


@pytest.mark.parametrize("prev", [None, K.SUMSQ_PREV])
@pytest.mark.parametrize("n", K.SUMSQ_N)
def test_sumsq_bound_notices_planted_mistakes(n, prev):
    g = K.h((n,), f"step.sumsq.{n}", 1.0)
    ref, depth = R.sumsq(g, prev)
    s32 = R.sumsq(g, prev, dtype=F32)[0]
    assert R.check_scalar(s32, ref, depth, "sumsq fp32") <= 0.5
    assert _close(ref, g.double().pow(2).sum() + (prev or 0.0))
    # (one element among two million is below any bound of a sum: the tail handled twice is planted at the small sizes)
    mistakes = (["tail_twice"] if n % 4 and n < R.SUMSQ_CAP else []) + (["drop_trip"] if n > R.SUMSQ_CAP else [])
    for mistake in mistakes:
        assert _fails(lambda: R.check_scalar(R.sumsq(g, prev, dtype=F32, mistake=mistake)[0], ref, depth, mistake)), mistake
    if prev is not None:
        assert _fails(lambda: R.check_scalar(R.sumsq(g, None, dtype=F32)[0], ref, depth, "accumulate ignored"))


def test_reduction_depths_are_the_counted_ones():
    assert R.red_tree(1024) == 10 + 4 + 10 + 2 and R.red_tree(4) == 10 + 1 + 10 + 2
    assert R.red_trips(K.N_RED) == 3 and R.red_trips(K.N_SMALL) == 1 and R.red_blocks(K.N_SMALL) == 4 and R.red_blocks(K.N_RED) == 1024
    assert R.red_depth(K.N_RED, 4) == 3 + 26 + 4
    assert R.sumsq(torch.zeros(K.N_SUMSQ))[1] == 3 + 26 + 4 + 1 and R.sumsq(torch.zeros(1003), 1.0)[1] == 1 + (10 + 1 + 10 + 2) + 4 + 1 + 1


@pytest.mark.parametrize("n", K.CLIP_N)
def test_clip_scale_bound_notices_a_missing_epsilon(n):
    g = K.h((n,), f"step.clip.g.{n}", 1.0)
    for name, (nsq, mx) in K.CLIP.items():
        ref, S, depth = R.clip_scale(g, nsq, mx)
        _chk(R.clip_scale(g, nsq, mx, dtype=F32)[0], ref, S, depth, f"clip_scale {name} fp32")
        if name == "below":
            assert torch.equal(ref, g.double())
    ref, S, depth = R.clip_scale(g, *K.CLIP["above"])
    assert _fails(lambda: _chk(R.clip_scale(g, *K.CLIP["above"], dtype=F32, mistake="clip_no_eps")[0], ref, S, depth, "clip_no_eps"))
    ref, S, depth = R.clip_scale(g, *K.CLIP["at"])
    assert _fails(lambda: _chk(g, ref, S, depth, "not scaled at the norm itself"))


def _adam_case(cid, dtype=F64, mistake=None):
    n, step, norm, over = K.ADAM_CASES[cid]
    p, g, m, v = K.adam_inputs(n)
    nsq, mx = norm if norm is not None else (None, 0.0)
    return R.adamw(p, g, m, v, step, **_akw(K.adam_kw(over)), normsq=nsq, max_norm=mx, dtype=dtype, mistake=mistake)


@pytest.mark.parametrize("cid", list(K.ADAM_CASES))
def test_adamw_bounds_notice_planted_mistakes(cid):
    n, step, norm, over = K.ADAM_CASES[cid]
    ref = _adam_case(cid)
    got = _adam_case(cid, F32)
    ratios = R.check_adamw({k: got[k][0] for k in "pmv"}, ref, cid + " fp32")
    assert max(ratios.values()) <= 1.0
    mistakes = ["bc_step_minus_1", "eps_in_sqrt"]
    if K.adam_kw(over)["wd"] != 0:
        mistakes.append("wd_on_grad")
    if norm is not None and R.clip_coef(*norm) < 1:
        mistakes.append("clip_no_eps")
    for mistake in mistakes:
        bad = _adam_case(cid, F32, mistake)
        assert _fails(lambda: R.check_adamw({k: bad[k][0] for k in "pmv"}, ref, mistake)), (cid, mistake)
    # a 1 % error in the update alone (m and v right) is far outside p's bound
    off = ref["p"][0] + 0.01 * (ref["p"][0] - K.adam_inputs(n)[0].double() * (1 - R.f32(K.adam_kw(over)["lr"]) * R.f32(K.adam_kw(over)["wd"])))
    assert _fails(lambda: R.check(off.float(), ref["p"][0], ref["p"][1], F32, "1 % of the update", 1))


def test_adamw_schedule_tables_feed_the_moment_and_the_correction():
    """beta1 from the table in the moment only, or in the bias correction only, is outside the bound (step 2, entry 1)."""
    p, g, m, v = K.adam_inputs(1000)
    kw = _akw(K.adam_kw({}))
    ref = R.adamw(p, g, m, v, 2, **dict(kw, lr=K.SCHED_LR[1], beta1=K.SCHED_B1[1] - 0.05))
    wrong_moment = R.adamw(p, g, m, v, 2, **dict(kw, lr=K.SCHED_LR[1], beta1=K.SCHED_B1[1]), dtype=F32)
    assert _fails(lambda: R.check_adamw({k: wrong_moment[k][0] for k in "pmv"}, ref, "beta1"))
    ok = R.adamw(p, g, m, v, 2, **dict(kw, lr=K.SCHED_LR[1], beta1=K.SCHED_B1[1] - 0.05), dtype=F32)
    R.check_adamw({k: ok[k][0] for k in "pmv"}, ref, "beta1 fp32")
    mixed = dict(ok)
    other = R.adamw(p, g, ok["m"][0], ok["v"][0], 2, **dict(kw, lr=K.SCHED_LR[1], beta1=K.SCHED_B1[1]), dtype=F32)
    mixed["p"] = (ok["p"][0] + (other["p"][0] - ok["p"][0]) * 0.5, None)
    assert _fails(lambda: R.check_adamw({k: mixed[k][0] for k in "pmv"}, ref, "correction from another beta1"))


def test_text_pool_and_sinusoid_references():
    text = K.h((K.TEXT_B, 32, 300), "step.pool.text", 1.5)
    ref, S, depth = R.text_pool(text)
    assert depth == 32 and _close(ref, text.double().mean(1))
    R.check(R.text_pool(text, dtype=F32)[0], ref, S, F32, "text_pool fp32", depth)
    R.check(R.text_pool(text, dtype=F32)[0].bfloat16(), ref, S, torch.bfloat16, "text_pool bf16", depth)
    assert _fails(lambda: R.check((text.double().sum(1) / 31).float(), ref, S, F32, "text_pool / (S - 1)", depth))
    assert _fails(lambda: R.check(text[:, :31].double().mean(1).float() * 31 / 32, ref, S, F32, "text_pool last token dropped", depth))
    for half in K.SIN_HALF:
        coeff, t = R.sinusoid_coeff(half), torch.tensor(K.SIN_T)
        ref = R.sinusoid(t, coeff)
        e = t.float().unsqueeze(-1) * coeff.unsqueeze(0)
        assert float((torch.cat([torch.sin(e), torch.cos(e)], -1).double() - ref).abs().max()) < R.SIN_BAR[F32] / 2
        assert float(coeff[0]) == 1.0 and math.isclose(float(coeff[-1]), 1e-4, rel_tol=1e-5)


def test_layout_references_are_permutes():
    B, C, HW = K.LAYOUT_SHAPES[0]
    src = K.h((B, C, HW), "step.lay.cpu", 2.0)
    for dt in K.DTYPES.values():
        rows = R.nchw_to_nhwc(src, dt)
        assert rows.shape == (B * HW, C) and rows.dtype == dt and rows[HW + 3, 2] == src[1, 2, 3].to(dt)
        assert torch.equal(R.nhwc_to_nchw(rows, B, C, HW), src.to(dt).float())


# ----------------------------------------------------------------------------------------------------- host-side refusals
def _err(lib):
    return lib.psg_last_error().decode()


def test_null_pointers_are_refused(lib):
    from pokemon_sprite_generator_amd import _lib
    P = FAKE
    calls = {
        "noise_add": lambda a: lib.psg_noise_add_f32(a[0], a[1], a[2], a[3], a[4], a[5], a[6], 2, 8, 10, 0, None),
        "noise_fallback": lambda a: lib.psg_noise_fallback_f32(a[0], a[1], a[2], a[3], 8, 0, None),
        "ddpm_update": lambda a: lib.psg_ddpm_update_f32(a[0], a[1], a[2], a[3], a[4], a[5], a[6], 8, None),
        "sampler_update": lambda a: lib.psg_sampler_update_f32(a[0], a[1], P, 1, 1.0, 1.0, 1.0, 1.0, 8, None),
        "reparam": lambda a: lib.psg_reparam_f32(a[0], a[1], a[2], a[3], 8, None),
        "smooth_l1": lambda a: lib.psg_smooth_l1_f32(a[0], a[1], P, a[2], P, 0.1, 1.0, 8, a[3], None),
        "recon_loss": lambda a: lib.psg_recon_loss_f32(a[0], a[1], P, a[2], 8, 1.0, 0.1, a[3], None),
        "sumsq": lambda a: lib.psg_sumsq_f32(a[0], 8, a[1], 0, a[2], None),
        "adamw": lambda a: lib.psg_adamw_f32(a[0], a[1], a[2], a[3], 8, 0.1, 0.9, 0.999, 1e-6, 0.0, 1, None, 0.0, None, None, None),
        "adamw_dev": lambda a: lib.psg_adamw_dev_f32(a[0], a[1], a[2], a[3], 8, a[4], P, 1, 0.9, 0.999, 1e-6, 0.0, a[5], None, 0.0, None, None, None),
        "clip_scale": lambda a: lib.psg_clip_scale_f32(a[0], 8, a[1], 1.0, None),
        "nchw_to_nhwc": lambda a: lib.psg_nchw_to_nhwc(a[0], a[1], 8, 1, 8, 4, 0, None),
        "nhwc_to_nchw": lambda a: lib.psg_nhwc_to_nchw(a[0], 8, a[1], 1, 8, 4, 0, None),
        "text_pool": lambda a: lib.psg_text_pool(a[0], a[1], 8, None, 1, 2, 8, 0, None),
        "sinusoid": lambda a: lib.psg_timestep_sinusoid(a[0], a[1], a[2], 8, 1, 4, 0, None),
    }
    nargs = {"noise_add": 7, "noise_fallback": 4, "ddpm_update": 7, "sampler_update": 2, "reparam": 4, "smooth_l1": 4, "recon_loss": 4,
             "sumsq": 3, "adamw": 4, "adamw_dev": 6, "clip_scale": 2, "nchw_to_nhwc": 2, "nhwc_to_nchw": 2, "text_pool": 2, "sinusoid": 3}
    for name, call in calls.items():
        for k in range(nargs[name]):
            a = [P] * nargs[name]
            a[k] = None
            assert call(a) == _lib.ERR_ARG and _err(lib) == f"{name}: null pointer", (name, k, _err(lib))
    # psg_reparam_bwd_f32: dlatent, at least one output, and logvar / eps when dlogvar is asked for
    for a in ((None, P, P, P, P), (P, P, P, None, None), (P, None, P, None, P), (P, P, None, P, P)):
        assert lib.psg_reparam_bwd_f32(a[0], a[1], a[2], a[3], a[4], 0, 8, None) == _lib.ERR_ARG and _err(lib) == "reparam_bwd: null pointer"


def test_sizes_and_scalars_are_refused_or_ignored(lib):
    from pokemon_sprite_generator_amd import _lib
    P, OK, SHAPE, ARG, ALIGN = FAKE, _lib.OK, _lib.ERR_SHAPE, _lib.ERR_ARG, _lib.ERR_ALIGN
    # n <= 0 is an error where a mean or a norm has no value ...
    for n in (0, -3):
        assert lib.psg_smooth_l1_f32(P, P, P, P, P, 0.1, 1.0, n, P, None) == SHAPE and _err(lib).startswith(f"smooth_l1: n={n} ")
        assert lib.psg_recon_loss_f32(P, P, P, P, n, 1.0, 0.1, P, None) == SHAPE and _err(lib) == f"recon_loss: n={n}"
        assert lib.psg_sumsq_f32(P, n, P, 0, P, None) == SHAPE and _err(lib) == f"sumsq: n={n}"
        assert lib.psg_adamw_f32(P, P, P, P, n, 0.1, 0.9, 0.999, 1e-6, 0.0, 1, None, 0.0, None, None, None) == SHAPE and _err(lib) == f"adamw: n={n} step=1"
        assert lib.psg_adamw_dev_f32(P, P, P, P, n, P, None, 1, 0.9, 0.999, 1e-6, 0.0, P, None, 0.0, None, None, None) == SHAPE
        assert _err(lib) == f"adamw_dev: n={n} sched_len=1"
        # ... and a silent success, with nothing launched, for the streaming updates
        assert lib.psg_noise_fallback_f32(P, P, P, P, n, 0, None) == OK
        assert lib.psg_ddpm_update_f32(P, P, P, P, P, P, P, n, None) == OK
        assert lib.psg_sampler_update_f32(P, P, None, 2, 0.0, 0.0, 0.0, 0.0, n, None) == OK
        assert lib.psg_reparam_f32(P, P, P, P, n, None) == OK
        assert lib.psg_reparam_bwd_f32(P, P, P, P, P, 1, n, None) == OK
        assert lib.psg_clip_scale_f32(P, n, P, 1.0, None) == OK
    assert lib.psg_noise_add_f32(P, P, P, P, P, P, P, 0, 8, 10, 0, None) == OK                    # an empty batch
    for B, chw, num_t in ((-1, 8, 10), (2, 0, 10), (2, 8, 0)):
        assert lib.psg_noise_add_f32(P, P, P, P, P, P, P, B, chw, num_t, 0, None) == SHAPE and _err(lib) == f"noise_add: bad shape B={B} chw={chw}"
    assert lib.psg_adamw_f32(P, P, P, P, 8, 0.1, 0.9, 0.999, 1e-6, 0.0, 0, None, 0.0, None, None, None) == SHAPE and _err(lib) == "adamw: n=8 step=0"
    assert lib.psg_adamw_dev_f32(P, P, P, P, 8, P, None, 0, 0.9, 0.999, 1e-6, 0.0, P, None, 0.0, None, None, None) == SHAPE
    assert _err(lib) == "adamw_dev: n=8 sched_len=0"
    for beta in (0.0, -0.1):
        assert lib.psg_smooth_l1_f32(P, P, P, P, P, beta, 1.0, 8, P, None) == SHAPE and _err(lib).startswith("smooth_l1: n=8 beta=")
    for mode in (0, 4, -1):
        assert lib.psg_sampler_update_f32(P, P, None, mode, 0.0, 0.0, 0.0, 0.0, 8, None) == ARG and _err(lib) == f"sampler_update: mode {mode}"
    assert lib.psg_nchw_to_nhwc(P, P, 7, 1, 8, 4, 0, None) == SHAPE and _err(lib) == "nchw_to_nhwc: bad shape"
    assert lib.psg_nhwc_to_nchw(P, 7, P, 1, 8, 4, 0, None) == SHAPE and _err(lib) == "nhwc_to_nchw: bad shape"
    assert lib.psg_text_pool(P, P, 7, None, 1, 2, 8, 0, None) == SHAPE and _err(lib) == "text_pool: bad shape"
    assert lib.psg_timestep_sinusoid(P, P, P, 7, 1, 4, 0, None) == SHAPE and _err(lib) == "sinusoid: bad shape"
    for off in (4, 8, 12):
        assert lib.psg_sumsq_f32(P + off, 8, P, 0, P, None) == ALIGN and _err(lib) == "sumsq: g must be 16-byte aligned"
    # the bf16 shadow exists on the float4 path only: n % 4 != 0, or any of p, g, m, v off a 16-byte boundary
    for n, a in ((9, (P, P, P, P)), (8, (P + 4, P, P, P)), (8, (P, P + 4, P, P)), (8, (P, P, P + 4, P)), (8, (P, P, P, P + 4))):
        assert lib.psg_adamw_f32(a[0], a[1], a[2], a[3], n, 0.1, 0.9, 0.999, 1e-6, 0.0, 1, None, 0.0, None, P, None) == ALIGN
        assert _err(lib).startswith("adamw: the bf16 shadow needs")
        assert lib.psg_adamw_dev_f32(a[0], a[1], a[2], a[3], n, P, None, 1, 0.9, 0.999, 1e-6, 0.0, P, None, 0.0, None, P, None) == ALIGN
    assert lib.psg_adamw_f32(P, P, P, P, 8, 0.1, 0.9, 0.999, 1e-6, 0.0, 1, None, 0.0, None, P + 4, None) == ALIGN     # the shadow itself: 8 bytes
