"""-m gpu: the grouped optimizer - psg_sumsq_groups_f32 / psg_adamw_groups_f32 through the C ABI, and optim.GroupedAdamW
(stage 1's two param groups under one launch, vae_trainer.py:164-187,341-342).

  * G = 1 is psg_adamw_dev_f32 bit for bit (p, m, v after 3 steps) at n = 8, 1032, 3*256*8+8, and at an arena large enough for
    the grid cap of both kernels (more than 262144 workgroups of float4s: the second float4 of the two-per-trip loop, whole for
    some lanes and absent for others); the group norms against fp64 at psg_sumsq_f32's bar (relative 1e-5).
  * Three groups and an empty one, per-group lr / weight decay / max norm, clipping active in some groups and inactive in the
    others and swapped on the next step, against torch.optim.AdamW + one clip_grad_norm_ per group on the CPU at
    test_flat_arena_adamw_matches_torch's bar (max-rel < 2e-6 per parameter); arena padding stays exactly zero.
  * determinism, the skip flag, a learning rate changed between steps, state dicts exchanged with torch.optim.AdamW both ways.
"""
import ctypes as C

import pytest
import torch

from tests.util import maxrel

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 2e-6                                     # test_flat_arena_adamw_matches_torch's
NORM_BAR = 1e-5                                # test_sumsq_adamw_clip's
KW = dict(betas=(0.9, 0.999), eps=1e-6)
# the shapes of test_flat_arena_adamw_matches_torch in three groups of 8, 77*13 -> 1008 and 64*32*3*3 floats + the rest, and an
# empty group between two of them
GROUPS = [[(5,)], [(77, 13), (130,)], [], [(64, 32, 3, 3), (96, 64, 1, 1)]]
LRS, WDS, MAX_NORMS = [3e-4, 1e-3, 5e-5, 2e-4], [0.01, 0.0, 0.3, 0.1], [1.0, 0.5, 7.0, 2.0]
# scale 3.0: every group's norm is above its max norm (the smallest group's, 5 values, is about 6.7); 0.01: below
# (0.01 * sqrt(24576) = 1.6 < 2.0, 0.01 * sqrt(1131) = 0.34 < 0.5) - Rig.step asserts both
SCALES = (3.0, 0.01)


@pytest.fixture(scope="module")
def psg():
    import pokemon_sprite_generator_amd as m
    from pokemon_sprite_generator_amd import _lib
    _lib.init(0)
    yield m
    m.ops.GradSink.unregister_all()
    m.ops.WeightCache.clear()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _i64(vals):
    return (C.c_int64 * len(vals))(*vals)


def _f32(vals):
    return (C.c_float * len(vals))(*vals)


def _sumsq_groups(lib, g, bounds):
    from pokemon_sprite_generator_amd import _lib
    G = len(bounds) - 1
    out = torch.full((G,), float("nan"), device=DEV)
    ws = _lib.workspace(lib.psg_reduce_workspace_bytes(), g.device)
    _lib.check(lib.psg_sumsq_groups_f32(_ptr(g), g.numel(), _i64(bounds), G, _ptr(out), _ptr(ws), _lib.stream_ptr()), "sumsq_groups")
    return out


DEV_KW = dict(lr=3e-4, wd=0.01, max_norm=1.0, beta1=0.9, beta2=0.999, eps=1e-6)


def _dev_vs_groups(lib, n, steps, seed, slices=None):
    """The same buffers through psg_adamw_dev_f32 and psg_adamw_groups_f32 (G = 1): (p, m, v) of both.  slices: also return what
    the last step started from on those slices - {"p", "g", "m", "v": one tensor per slice, "nsq": the squared norm it read}."""
    from pokemon_sprite_generator_amd import _lib
    gen = torch.Generator(device=DEV).manual_seed(seed)
    p0 = torch.randn(n, device=DEV, generator=gen)
    a, b = [p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)], [p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)]
    del p0
    step_a, step_b = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    lr, wd, max_norm = DEV_KW["lr"], DEV_KW["wd"], DEV_KW["max_norm"]
    table = torch.full((1,), lr, device=DEV)
    kept = None
    g = torch.empty(n, device=DEV)
    for step in range(steps):
        g.normal_(generator=gen).mul_(SCALES[step % 2])
        nsq = _sumsq_groups(lib, g, [0, n])
        ref = float(g.double().pow(2).sum())
        assert abs(float(nsq[0]) - ref) / ref < NORM_BAR, (n, step, float(nsq[0]), ref)
        if slices is not None and step == steps - 1:
            kept = {k: [t[s].clone() for s in slices] for k, t in (("p", a[0]), ("g", g), ("m", a[1]), ("v", a[2]))}
            kept["nsq"] = float(nsq[0])
        _lib.check(lib.psg_adamw_dev_f32(_ptr(a[0]), _ptr(g), _ptr(a[1]), _ptr(a[2]), n, _ptr(table), None, 1, 0.9, 0.999, 1e-6, wd,
                                         _ptr(step_a), _ptr(nsq), max_norm, None, None, _lib.stream_ptr()), "adamw_dev")
        _lib.check(lib.psg_adamw_groups_f32(_ptr(b[0]), _ptr(g), _ptr(b[1]), _ptr(b[2]), n, _i64([0, n]), 1, _f32([lr]), _f32([wd]),
                                            _f32([max_norm]), 0.9, 0.999, 1e-6, _ptr(step_b), _ptr(nsq), None, _lib.stream_ptr()),
                   "adamw_groups")
    assert int(step_a) == int(step_b) == steps
    return (a, b) if slices is None else (a, b, kept)


@pytest.mark.parametrize("n", [8, 1032, 3 * 256 * 8 + 8])
def test_one_group_is_adamw_dev_bitwise(psg, n):
    from pokemon_sprite_generator_amd import _lib
    a, b = _dev_vs_groups(_lib.load(), n, 3, 11)
    for x, y, name in zip(a, b, "pmv"):
        assert torch.equal(x, y), (n, name)
    assert not torch.equal(a[0], torch.zeros_like(a[0])) and float(a[2].abs().max()) > 0


def test_one_group_past_the_grid_cap_is_adamw_dev_bitwise(psg):
    """262144 * 256 float4s fill the capped grid once: 778 more make the second float4 of a trip exist for some lanes only.  The
    norm reduction runs its 1024 workgroups over ~1000 trips each.

    Both kernels share one loop body, so equal bits alone would let a mispaired second float4 pass: three slices of p, m and v
    are also held to the fp64 restatement and bound of tests/step_ref.py (computed on the device) - the first 4096 float4s,
    the float4s from index 262144 * 256 on (the first elements reached as the second float4 of a trip; 778 exist), and the
    last 4096 float4s (the tail of the first trip, lanes whose second float4 does not exist, and those 778 again)."""
    from pokemon_sprite_generator_amd import _lib
    from tests import step_ref
    cap4, steps = 262144 * 256, 1
    n4 = cap4 + 778
    n = n4 * 4
    slices = [slice(0, 4 * 4096), slice(4 * cap4, 4 * min(cap4 + 4096, n4)), slice(4 * (n4 - 4096), n)]
    a, b, start = _dev_vs_groups(_lib.load(), n, steps, 12, slices)
    for x, y, name in zip(a, b, "pmv"):
        assert torch.equal(x, y), name
    for i, s in enumerate(slices):
        ref = step_ref.adamw(start["p"][i], start["g"][i], start["m"][i], start["v"][i], steps, lr=DEV_KW["lr"], beta1=DEV_KW["beta1"],
                             beta2=DEV_KW["beta2"], eps=DEV_KW["eps"], wd=DEV_KW["wd"], normsq=start["nsq"], max_norm=DEV_KW["max_norm"])
        assert ref["p"][0].is_cuda and ref["p"][0].numel() == s.stop - s.start > 0
        ratios = step_ref.check_adamw({"p": a[0][s], "m": a[1][s], "v": a[2][s]}, ref, f"past the cap, slice {i}")
        print(f"RATIO adamw_dev past the cap, slice {i}: p {ratios['p']:.3g} m {ratios['m']:.3g} v {ratios['v']:.3g}")
        assert not torch.equal(a[0][s], start["p"][i])
    del a, b, start
    torch.cuda.empty_cache()


class Rig:
    """GroupedAdamW over GROUPS on the device and torch.optim.AdamW over CPU twins of the same parameters."""

    def __init__(self, psg, seed=2, groups=GROUPS):
        gen = torch.Generator().manual_seed(seed)
        self.shapes = groups
        self.ref_groups = [[torch.nn.Parameter(torch.randn(s, generator=gen)) for s in grp] for grp in groups]
        self.own_groups = [[torch.nn.Parameter(p.detach().clone().to(DEV)) for p in grp] for grp in self.ref_groups]
        self.ps_ref = [p for grp in self.ref_groups for p in grp]
        self.ps = [p for grp in self.own_groups for p in grp]
        self.pa, self.ga = psg.ParamArena(self.ps), psg.GradArena(self.ps)
        self.opt = self.new_own(psg)
        self.ref = self.new_ref()

    def _dicts(self, groups):
        return [{"params": list(grp), "lr": lr, "weight_decay": wd, "name": f"g{i}"} for i, (grp, lr, wd) in enumerate(zip(groups, LRS, WDS))]

    def new_own(self, psg):
        return psg.GroupedAdamW(self._dicts(self.own_groups), self.pa, self.ga, **KW)

    def new_ref(self):
        return torch.optim.AdamW(self._dicts(self.ref_groups), **KW)

    def grads(self, step):
        """Clipping active in the even groups and inactive in the odd ones, swapped on the next step."""
        gen = torch.Generator().manual_seed(100 + step)
        self.ga.zero()
        for gi, (own, ref) in enumerate(zip(self.own_groups, self.ref_groups)):
            scale = SCALES[(step + gi) % 2]
            for p, pr in zip(own, ref):
                g = torch.randn(pr.shape, generator=gen) * scale
                pr.grad = g.clone()
                p.grad.copy_(g.to(DEV))

    def step(self, step, opt=None, ref=None, skip_flag=None):
        opt, ref = opt or self.opt, ref or self.ref
        self.grads(step)
        norms = [torch.nn.utils.clip_grad_norm_(grp, max_norm=mx) if grp else None for grp, mx in zip(self.ref_groups, MAX_NORMS)]
        nsq = opt.group_norm_sq()
        for gi, nr in enumerate(norms):
            if nr is None:
                assert float(nsq[gi]) == 0.0                                   # the empty group
                continue
            active = SCALES[(step + gi) % 2] == 3.0
            assert (float(nr) > MAX_NORMS[gi]) == active, (step, gi, float(nr))
            assert abs(float(nsq[gi].sqrt()) - float(nr)) / float(nr) < NORM_BAR, (step, gi)
        ref.step()
        opt.step(normsq=nsq, max_norms=MAX_NORMS, skip_flag=skip_flag)
        return nsq.clone()

    def check(self, what):
        for i, (p, pr) in enumerate(zip(self.ps, self.ps_ref)):
            e = maxrel(p, pr)
            assert e < BAR, (what, i, tuple(pr.shape), e)

    def padding_mask(self):
        mask = torch.ones(self.pa.numel, dtype=torch.bool, device=DEV)
        for p, o in zip(self.pa.params, self.pa.offsets):
            mask[o:o + p.numel()] = False
        return mask

    def release(self):
        self.ga.release()
        self.pa.release()


def test_three_groups_swapped_clipping_against_torch(psg):
    rig = Rig(psg)
    assert rig.opt.bounds == [0, 8, 8 + 1008 + 136, 1152, 1152 + 18432 + 6144] and len(rig.opt.param_groups) == 4
    pad = rig.padding_mask()
    assert int(pad.sum()) == 3 + 7 + 6
    for step in range(4):
        rig.step(step)
        rig.check(f"step {step}")
        for buf in (rig.pa.flat, rig.opt._m, rig.opt._v, rig.ga.flat):
            assert not bool(buf[pad].any()), step                              # arena padding stays exactly zero
    assert rig.opt.steps_done() == 4
    rig.release()


def test_two_runs_are_bitwise_equal(psg):
    runs = []
    for _ in range(2):
        rig = Rig(psg)
        norms = [rig.step(step) for step in range(2)]
        runs.append((norms, rig.pa.flat.clone(), rig.opt._m.clone(), rig.opt._v.clone()))
        rig.release()
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert torch.equal(a, b)


def test_skip_flag_moves_nothing(psg):
    from pokemon_sprite_generator_amd import _lib
    rig = Rig(psg)
    rig.step(0)
    before = [t.clone() for t in (rig.pa.flat, rig.opt._m, rig.opt._v, rig.opt.step_dev)]
    flag = torch.tensor([_lib.FLAG_LOSS_BAD], dtype=torch.int32, device=DEV)
    rig.step(1, skip_flag=flag)
    for a, b in zip(before, (rig.pa.flat, rig.opt._m, rig.opt._v, rig.opt.step_dev)):
        assert torch.equal(a, b)
    assert rig.opt.steps_done() == 1
    flag.zero_()                                                               # a clear flag lets the step through
    rig.grads(1)
    rig.opt.step(normsq=rig.opt.group_norm_sq(), max_norms=MAX_NORMS, skip_flag=flag)
    assert rig.opt.steps_done() == 2 and not torch.equal(before[0], rig.pa.flat)
    rig.release()


def test_learning_rate_is_live(psg):
    same = Rig(psg)
    same.step(0)
    same.step(1)
    kept = same.pa.flat.clone()
    same.release()
    rig = Rig(psg)
    rig.step(0)
    for opt in (rig.opt, rig.ref):
        opt.param_groups[1]["lr"] = LRS[1] * 10
    rig.step(1)
    rig.check("after the change")
    b = rig.opt.bounds
    assert torch.equal(rig.pa.flat[:b[1]], kept[:b[1]]) and torch.equal(rig.pa.flat[b[2]:], kept[b[2]:])      # the other groups
    assert not torch.equal(rig.pa.flat[b[1]:b[2]], kept[b[1]:b[2]])
    rig.release()


def test_state_dict_round_trip_with_torch(psg):
    rig = Rig(psg)
    for step in range(2):
        rig.step(step)
    own_sd, ref_sd = rig.opt.state_dict(), rig.ref.state_dict()
    assert len(own_sd["param_groups"]) == 4 and [g["params"] for g in own_sd["param_groups"]] == [[0], [1, 2], [], [3, 4]]
    assert set(own_sd["state"][3]) == {"step", "exp_avg", "exp_avg_sq"} and float(own_sd["state"][3]["step"]) == 2.0
    assert own_sd["state"][3]["exp_avg"].shape == (64, 32, 3, 3) and own_sd["param_groups"][1]["name"] == "g1"

    def clone(sd):
        return {"state": {k: {kk: (vv.clone() if torch.is_tensor(vv) else vv) for kk, vv in v.items()} for k, v in sd["state"].items()},
                "param_groups": [dict(g) for g in sd["param_groups"]]}

    ref2 = rig.new_ref()
    ref2.load_state_dict(clone(own_sd))                    # ours -> torch.optim.AdamW
    own2 = rig.new_own(psg)
    own2.load_state_dict(clone(ref_sd))                    # torch.optim.AdamW -> ours
    assert own2.steps_done() == 2
    for step in range(2, 4):
        rig.step(step, opt=own2, ref=ref2)
        rig.check(f"resumed step {step}")
    assert own2.steps_done() == 4
    rig.release()
