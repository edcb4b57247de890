"""-m gpu: clip sets in the grouped optimizer - psg_adamw_groups_sets_f32 and optim.GroupedAdamW.step(..., clip_sets=): groups
that keep their own learning rate and weight decay and share ONE clip norm (stage 3's joint phase, final_trainer.py:480-483).

  * NULL and the identity map give psg_adamw_groups_f32's bits (p, m, v after 3 steps) on tests/test_opt_groups_gpu.py's four
    groups, the empty one included.
  * Sets [0, 1, 1, 0] against torch.optim.AdamW + one clip_grad_norm_ per SET on the CPU, at that file's bar (max-rel < 2e-6
    per parameter); clipping active in one set and inactive in the other, swapped on the next step; arena padding stays zero.
  * determinism and the skip flag.
"""
import ctypes as C

import pytest
import torch

from tests.util import maxrel
from tests.test_opt_groups_gpu import DEV, GROUPS, LRS, NORM_BAR, WDS, Rig

pytestmark = pytest.mark.gpu
SETS = [0, 1, 1, 0]
SET_MAX = {0: 1.0, 1: 0.5}
MAX_NORMS = [SET_MAX[s] for s in SETS]
IDENTITY_MAX = [1.0, 0.5, 7.0, 2.0]
# set 0 = groups 0 and 3 (5 + 24576 values), set 1 = groups 1 and 2 (1131 values and the empty group).  Scale 3.0: the set's
# norm is far above its max norm (3 * sqrt(1131) = 101 > 0.5); 0.002: below (0.002 * sqrt(24581) = 0.31 < 1.0,
# 0.002 * sqrt(1131) = 0.07 < 0.5) - SetRig.step asserts both
SCALES = (3.0, 0.002)


@pytest.fixture(scope="module")
def psg():
    import pokemon_sprite_generator_amd as m
    from pokemon_sprite_generator_amd import _lib
    _lib.init(0)
    yield m
    m.ops.GradSink.unregister_all()
    m.ops.WeightCache.clear()


class SetRig(Rig):
    """test_opt_groups_gpu.Rig with the gradient scale chosen per SET and one clip_grad_norm_ per set on the CPU."""

    def grads(self, step):
        gen = torch.Generator().manual_seed(100 + step)
        self.ga.zero()
        for gi, (own, ref) in enumerate(zip(self.own_groups, self.ref_groups)):
            scale = SCALES[(step + SETS[gi]) % 2]
            for p, pr in zip(own, ref):
                g = torch.randn(pr.shape, generator=gen) * scale
                pr.grad = g.clone()
                p.grad.copy_(g.to(DEV))

    def step(self, step, skip_flag=None, clip_sets=SETS, max_norms=MAX_NORMS):
        self.grads(step)
        nsq = self.opt.group_norm_sq()
        reported = self.opt.set_norms(clip_sets, nsq)
        assert reported.is_cuda and reported.shape == (len(set(clip_sets)),)
        for k, s in enumerate(sorted(set(clip_sets))):
            members = [p for gi, grp in enumerate(self.ref_groups) if clip_sets[gi] == s for p in grp]
            nr = torch.nn.utils.clip_grad_norm_(members, max_norm=SET_MAX[s])
            active = SCALES[(step + s) % 2] == 3.0
            assert (float(nr) > SET_MAX[s]) == active, (step, s, float(nr))            # active in one set, inactive in the other
            assert abs(float(reported[k]) - float(nr)) / float(nr) < NORM_BAR, (step, s)
        self.ref.step()
        self.opt.step(normsq=nsq, max_norms=max_norms, skip_flag=skip_flag, clip_sets=clip_sets)
        return nsq.clone()


def test_identity_and_null_are_the_existing_entry_bitwise(psg):
    """Three rigs over the same parameters and gradients: step(), step(clip_sets=None) through the existing entry, and
    step(clip_sets=[0, 1, 2, 3]) through the new one, with clipping active in some groups and swapped on the next step."""
    rigs = [Rig(psg) for _ in range(3)]
    for step in range(3):
        for rig, sets in zip(rigs, ("old", None, list(range(len(GROUPS))))):
            rig.grads(step)
            nsq = rig.opt.group_norm_sq()
            if sets == "old":
                rig.opt.step(normsq=nsq, max_norms=IDENTITY_MAX)
            else:
                rig.opt.step(normsq=nsq, max_norms=IDENTITY_MAX, clip_sets=sets)
    a = rigs[0]
    assert a.opt.steps_done() == 3 and float(a.opt._v.abs().max()) > 0
    for b in rigs[1:]:
        for x, y, name in ((a.pa.flat, b.pa.flat, "p"), (a.opt._m, b.opt._m, "m"), (a.opt._v, b.opt._v, "v")):
            assert torch.equal(x, y), name
    # the same through the C ABI with a NULL clip set
    from pokemon_sprite_generator_amd import _lib
    lib = _lib.load()
    c, G = Rig(psg), len(GROUPS)
    F = C.c_float * G
    for step in range(3):
        c.grads(step)
        nsq = c.opt.group_norm_sq()
        _lib.check(lib.psg_adamw_groups_sets_f32(_lib.ptr(c.pa.flat), _lib.ptr(c.ga.flat), _lib.ptr(c.opt._m), _lib.ptr(c.opt._v), c.pa.numel,
                                                 c.opt._bounds_c, G, F(*LRS), F(*WDS), F(*IDENTITY_MAX), None, 0.9, 0.999, 1e-6,
                                                 _lib.ptr(c.opt.step_dev), _lib.ptr(nsq), None, _lib.stream_ptr()), "adamw_groups_sets")
    for x, y, name in ((a.pa.flat, c.pa.flat, "p"), (a.opt._m, c.opt._m, "m"), (a.opt._v, c.opt._v, "v")):
        assert torch.equal(x, y), name
    for rig in rigs + [c]:
        rig.release()


def test_two_sets_swapped_clipping_against_torch(psg):
    rig = SetRig(psg)
    pad = rig.padding_mask()
    assert int(pad.sum()) == 3 + 7 + 6
    for step in range(4):
        rig.step(step)
        rig.check(f"step {step}")
        for buf in (rig.pa.flat, rig.opt._m, rig.opt._v, rig.ga.flat):
            assert not bool(buf[pad].any()), step                              # arena padding stays exactly zero
    assert rig.opt.steps_done() == 4
    # The sets are really shared.  Group 0 (5 values, norm about 6.7 at scale 3.0) shares set 0 with group 3 (24576 values, norm
    # about 470): its first moment after step 1 is 0.1 * g * coef with the SET's coefficient, 70 x smaller than its own.  (Adam's
    # first update itself is nearly blind to the scale of g, so the moment is compared, at 10 x the norm's bar.)
    own, per_group = SetRig(psg), SetRig(psg)
    own.step(0)
    per_group.grads(0)
    per_group.opt.step(normsq=per_group.opt.group_norm_sq(), max_norms=MAX_NORMS)
    p0, p0_ref = own.ps[0], own.ps_ref[0]
    m_own, m_ref = own.opt.state[p0]["exp_avg"], own.ref.state[p0_ref]["exp_avg"]
    assert maxrel(m_own, m_ref) < 10 * NORM_BAR
    ratio = float(per_group.opt.state[per_group.ps[0]]["exp_avg"].abs().max() / m_own.abs().max())
    assert 20 < ratio < 200, ratio
    for r in (rig, own, per_group):
        r.release()
    # python-side refusals
    r = SetRig(psg)
    r.grads(0)
    nsq = r.opt.group_norm_sq()
    with pytest.raises(ValueError):
        r.opt.step(normsq=nsq, max_norms=MAX_NORMS, clip_sets=[0, 1, 1])
    with pytest.raises(ValueError):
        r.opt.step(normsq=nsq, max_norms=MAX_NORMS, clip_sets=[0, 1, 4, 0])
    with pytest.raises(ValueError):
        r.opt.step(clip_sets=SETS)
    with pytest.raises(psg.PsgError):
        r.opt.step(normsq=nsq, max_norms=IDENTITY_MAX, clip_sets=SETS)              # one set, two max norms: PSG_ERR_SHAPE
    assert r.opt.steps_done() == 0
    r.release()


def test_two_runs_are_bitwise_equal(psg):
    runs = []
    for _ in range(2):
        rig = SetRig(psg)
        norms = [rig.step(step) for step in range(2)]
        runs.append((norms, rig.pa.flat.clone(), rig.opt._m.clone(), rig.opt._v.clone()))
        rig.release()
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert torch.equal(a, b)


def test_skip_flag_moves_nothing(psg):
    from pokemon_sprite_generator_amd import _lib
    rig = SetRig(psg)
    rig.step(0)
    before = [t.clone() for t in (rig.pa.flat, rig.opt._m, rig.opt._v, rig.opt.step_dev)]
    flag = torch.tensor([_lib.FLAG_LOSS_BAD], dtype=torch.int32, device=DEV)
    rig.step(1, skip_flag=flag)
    for a, b in zip(before, (rig.pa.flat, rig.opt._m, rig.opt._v, rig.opt.step_dev)):
        assert torch.equal(a, b)
    assert rig.opt.steps_done() == 1
    flag.zero_()                                                               # a clear flag lets the step through
    rig.grads(1)
    rig.opt.step(normsq=rig.opt.group_norm_sq(), max_norms=MAX_NORMS, skip_flag=flag, clip_sets=SETS)
    assert rig.opt.steps_done() == 2 and not torch.equal(before[0], rig.pa.flat)
    rig.release()
