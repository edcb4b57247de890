"""-m "not gpu": the clip-set entry of the grouped optimizer (psg_adamw_groups_sets_f32: declared, exported, bound, validated on
the host before anything touches the GPU) and the host side of stage 3's joint phase (final_trainer.py:590-642): FinalStepper's
keywords and config dict, the param groups of both phases and their per-epoch learning rates against torch.optim.lr_scheduler
on a dummy optimizer, and the refusal of a generator whose decoder was built frozen."""
import ctypes as C
import os
import warnings

import pytest
import torch

from tests import text_cases as TC


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


NAMES = ["p", "g", "m", "v", "n", "bounds", "G", "lr", "weight_decay", "max_norm", "clip_set", "beta1", "beta2", "eps", "step_dev",
         "normsq", "skip_flag", "stream"]


def test_header_declares_library_exports_binding_binds(lib):
    from pokemon_sprite_generator_amd import _lib
    res, params = _lib.ABI.functions["psg_adamw_groups_sets_f32"]
    assert res is C.c_int and [p[2] for p in params] == NAMES
    assert params[NAMES.index("clip_set")][1] == "const int32_t*"
    # the existing entry's parameters with `clip_set` put in after `max_norm`
    old = [p[1:] for p in _lib.ABI.functions["psg_adamw_groups_f32"][1]]
    assert [p[1:] for p in params if p[2] != "clip_set"] == old
    assert hasattr(lib, "psg_adamw_groups_sets_f32")
    fn = lib.psg_adamw_groups_sets_f32
    assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SIGNATURES["psg_adamw_groups_sets_f32"][1] and len(fn.argtypes) == 18


A, ODD = C.c_void_p(0x10000), C.c_void_p(0x10004)        # never dereferenced: every call below fails its host-side checks


def _i64(*b):
    return (C.c_int64 * len(b))(*b)


def _call(lib, sets="none", old=False, p=A, g=A, n=64, bounds=(0, 24, 40, 64), G=3, max_norm=(1.0, 1.0, 1.0), normsq=A, lr=True):
    """The new entry with a clip set (a tuple), NULL (None), or - `old` - the existing entry with the same arguments."""
    F = (C.c_float * 8)(*([0.1] * 8))
    mx = (C.c_float * len(max_norm))(*max_norm) if max_norm is not None else None
    head = (p, g, A, A, n, _i64(*bounds) if bounds is not None else None, G, F if lr else None, F, mx)
    tail = (0.9, 0.999, 1e-8, A, normsq, None, None)
    if old:
        return lib.psg_adamw_groups_f32(*head, *tail)
    return lib.psg_adamw_groups_sets_f32(*head, (C.c_int32 * len(sets))(*sets) if sets is not None else None, *tail)


def test_clip_set_refusals_on_the_host(lib):
    from pokemon_sprite_generator_amd import _lib
    ARG, SHAPE = _lib.ERR_ARG, _lib.ERR_SHAPE
    # a set index outside 0..G-1
    assert _call(lib, sets=(0, 3, 0)) == SHAPE and b"clip_set" in lib.psg_last_error()
    assert _call(lib, sets=(-1, 0, 0)) == SHAPE
    assert _call(lib, sets=(0, 0, 7)) == SHAPE
    # two groups of one set with different max norms: one clip_grad_norm_ call has one
    assert _call(lib, sets=(0, 1, 0), max_norm=(1.0, 1.0, 0.5)) == SHAPE and b"max_norm" in lib.psg_last_error()
    assert _call(lib, sets=(2, 2, 1), max_norm=(1.0, 0.5, 0.5)) == SHAPE
    # a clip set without normsq or without max_norm
    assert _call(lib, sets=(0, 0, 1), normsq=None) == ARG
    assert _call(lib, sets=(0, 0, 1), max_norm=None) == ARG
    assert _call(lib, sets=(0, 0, 1), max_norm=None, normsq=None) == ARG


def test_null_clip_set_is_the_existing_entry_on_bad_arguments(lib):
    from pokemon_sprite_generator_amd import _lib
    nine = tuple(range(0, 80, 8))
    cases = [dict(g=None), dict(bounds=None), dict(lr=False), dict(max_norm=None), dict(G=0, bounds=(0,), n=8),
             dict(G=9, bounds=nine, n=72, max_norm=(1.0,) * 9), dict(bounds=(0, 72, 40, 64)), dict(bounds=(8, 24, 40, 64)),
             dict(bounds=(0, 24, 40, 56)), dict(n=0, bounds=(0, 0, 0, 0)), dict(bounds=(0, 28, 40, 64)), dict(p=ODD), dict(g=ODD)]
    seen = set()
    for kw in cases:
        want = _call(lib, old=True, **kw)
        assert want != _lib.OK, kw
        assert _call(lib, sets=None, **kw) == want, kw
        if kw.get("G", 3) == 3:                            # (a valid identity map changes nothing about the refusal either)
            assert _call(lib, sets=(0, 1, 2), **kw) == want or kw == dict(max_norm=None), kw
        seen.add(want)
    assert seen == {_lib.ERR_ARG, _lib.ERR_SHAPE, _lib.ERR_ALIGN}


# ---- FinalStepper, host side -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def psg():
    import pokemon_sprite_generator_amd as m
    yield m
    m.ops.GradSink.unregister_all()
    m.ops.WeightCache.clear()


def _generator(psg, trainable=True, unet=None):
    te = psg.TextEncoder(bert_config=TC.bert_config(2), hidden_dim=256, trainable=True, finetune_strategy="minimal")
    return psg.FinalPokemonGenerator(psg.VAEEncoder(3, 8), psg.VAEDecoder(8, 256, trainable=trainable), unet, te)


def _release(st):
    if st.arena is not None:
        st.arena.release()
        st.param_arena.release()


def test_default_decoder_still_refuses_the_joint_phase(psg):
    gen = _generator(psg, trainable=False)
    with pytest.raises(psg.PsgError, match="joint phase not built") as e:
        gen.unfreeze_vae_decoder()
    assert "trainable=True" in str(e.value) and "built frozen" in str(e.value)          # why, and how to build it trainable
    with pytest.raises(psg.PsgError, match="joint phase not built"):
        gen.unfreeze_unet()
    st = psg.FinalStepper(gen)
    with pytest.raises(psg.PsgError, match="joint phase not built"):
        st.switch_to_joint_training()
    assert st.training_phase == "text_encoder" and not any(p.requires_grad for p in gen.vae_decoder.parameters())


def test_trainable_decoder_starts_frozen_and_switches_both_ways(psg):
    unet = torch.nn.Linear(3, 3)
    gen = _generator(psg, unet=unet)
    dec = gen.vae_decoder
    assert dec.trainable and not dec.live_weights() and not any(p.requires_grad for p in dec.parameters())
    assert not any(p.requires_grad for p in unet.parameters())
    epoch = psg.ops.WeightCache.epoch
    gen.unfreeze_vae_decoder()
    assert dec.live_weights() and all(p.requires_grad for p in dec.parameters()) and psg.ops.WeightCache.epoch > epoch
    gen.unfreeze_unet()
    assert all(p.requires_grad for p in unet.parameters())
    epoch = psg.ops.WeightCache.epoch
    gen.freeze_vae_decoder()
    assert not dec.live_weights() and not any(p.requires_grad for p in dec.parameters()) and psg.ops.WeightCache.epoch > epoch
    gen.freeze_unet()
    assert not any(p.requires_grad for p in unet.parameters())
    _generator(psg).unfreeze_unet()                                                     # no U-Net: a no-op
    assert not any(p.requires_grad for p in gen.vae_encoder.parameters())


def test_keywords_config_and_groups(psg):
    gen = _generator(psg)
    te, dec = gen.text_encoder, gen.vae_decoder
    st = psg.FinalStepper(gen, lr=4e-4)
    assert st.update == "torch" and type(st.optimizer) is torch.optim.AdamW and st.training_phase == "text_encoder"
    assert st.learning_rates() == (4e-4,) and st.config["vae_decoder_lr"] == 4e-4 * 0.1           # :609
    assert [g["name"] for g in st.optimizer.param_groups] == ["text_encoder"] and st.optimizer.param_groups[0]["weight_decay"] == 0.01
    assert sorted(id(p) for p in st.params) == sorted(id(p) for p in te.parameters() if p.requires_grad)
    names = {id(p): n for n, p in te.named_parameters()}
    stepped = sorted(names[id(p)] for p in st.optimizer.param_groups[0]["params"])
    assert stepped == sorted(n for n, p in te.named_parameters() if p.requires_grad and not n.startswith("bert.pooler."))
    assert "projection.weight" in stepped and any(n.startswith("bert.pooler.") for n, p in te.named_parameters() if p.requires_grad)
    st.switch_to_joint_training()
    assert st.training_phase == "joint" and st.learning_rates() == (4e-4, 4e-4 * 0.1)
    assert [g["name"] for g in st.optimizer.param_groups] == ["text_encoder", "vae_decoder"]
    g_dec = st.optimizer.param_groups[1]["params"]
    assert len(g_dec) == 144 and all(a is b for a, b in zip(g_dec, dec.parameters())) and all(p.requires_grad for p in g_dec)
    assert sorted(names[id(p)] for p in st.optimizer.param_groups[0]["params"]) == stepped
    st.switch_to_joint_training()                                                       # a second call changes nothing
    assert len(st.optimizer.param_groups) == 2

    # the reference's config dict; keywords override it
    cfg = {"optimization": {"text_encoder_lr": 3e-5, "vae_decoder_lr": 7e-6, "optimizer": "adamw", "weight_decay": 0.05,
                            "scheduler": "step", "step_size": 2, "gamma": 0.5, "beta1": 0.5, "beta2": 0.9},
           "training": {"final_epochs": 7}}
    st = psg.FinalStepper(_generator(psg), config=cfg)
    assert st.learning_rates() == (3e-5,) and st.config["final_epochs"] == 7 and st.optimizer.param_groups[0]["weight_decay"] == 0.05
    assert tuple(st.optimizer.param_groups[0]["betas"]) == (0.9, 0.999)                # beta1 / beta2 are Adam's only
    st.switch_to_joint_training()
    assert st.learning_rates() == (3e-5, 7e-6)
    st = psg.FinalStepper(_generator(psg), lr=1e-3, config=cfg, vae_decoder_lr=2e-4, update="grouped")
    assert isinstance(st.optimizer, psg.GroupedAdamW) and st.learning_rates() == (1e-3,) and len(st.optimizer.bounds) == 2
    first = st.arena
    st.switch_to_joint_training()
    assert st.learning_rates() == (1e-3, 2e-4) and isinstance(st.optimizer, psg.GroupedAdamW) and st.arena is not first
    n_text = len(st.text_params)
    assert len(st.arena.params) == n_text + 144 and st.optimizer.bounds[1] == st.arena.offsets[n_text]        # text encoder first
    assert st.optimizer.steps_done() == 0 and not bool(st.optimizer._m.any()) and not bool(st.optimizer._v.any())
    with pytest.raises(psg.PsgError):
        first.check_alive()                                                             # the text-phase arena was released
    _release(st)
    adam = psg.FinalStepper(_generator(psg), config=dict(cfg, optimization=dict(cfg["optimization"], optimizer="adam")), update="grouped")
    assert all(g["weight_decay"] == 0.0 and tuple(g["betas"]) == (0.5, 0.9) for g in adam.optimizer.param_groups)
    _release(adam)
    twin = psg.FinalStepper(_generator(psg), optimizer="adam", beta1=0.8)
    assert type(twin.optimizer) is torch.optim.Adam and tuple(twin.optimizer.param_groups[0]["betas"]) == (0.8, 0.999)
    assert twin.optimizer.param_groups[0]["weight_decay"] == 0.01                       # without a config: as this class always did
    with pytest.raises(ValueError, match="Unknown optimizer"):
        psg.FinalStepper(gen, optimizer="sgd")
    with pytest.raises(ValueError, match="Unknown scheduler"):
        psg.FinalStepper(gen, scheduler="linear")
    with pytest.raises(ValueError, match="Unknown update"):
        psg.FinalStepper(gen, update="fused")
    with pytest.raises(ValueError, match="weight_decay=0"):
        psg.FinalStepper(gen, optimizer="adam", update="grouped")
    with pytest.raises(TypeError):
        psg.FinalStepper(gen, vae_decoder_lrr=1.0)


@pytest.mark.parametrize("update", ["grouped", "torch"])
@pytest.mark.parametrize("kind", ["cosine", "step", "constant"])
def test_learning_rates_follow_torch_schedulers_in_both_phases(psg, kind, update):
    lr, dlr = 2e-4, 5e-5
    st = psg.FinalStepper(_generator(psg), lr=lr, vae_decoder_lr=dlr, scheduler=kind, final_epochs=5, step_size=2, gamma=0.5, update=update)
    S = torch.optim.lr_scheduler

    def dummy(lrs):
        opt = torch.optim.AdamW([{"params": [torch.nn.Parameter(torch.zeros(1))], "lr": x} for x in lrs])
        return opt, {"cosine": lambda: S.CosineAnnealingLR(opt, T_max=5), "step": lambda: S.StepLR(opt, step_size=2, gamma=0.5),
                     "constant": lambda: S.LambdaLR(opt, lr_lambda=lambda e: 1.0)}[kind]()

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                    # (no optimizer.step() between the scheduler steps here)
        opt, sched = dummy([lr])
        for epoch in range(3):
            assert st.epoch == epoch and st.learning_rates() == tuple(g["lr"] for g in opt.param_groups), (kind, epoch)
            st.end_epoch()
            sched.step()
        if kind != "constant":
            assert st.learning_rates()[0] < lr
        st.switch_to_joint_training()                      # the scheduler is rebuilt: back at the base learning rates
        assert st.learning_rates() == (lr, dlr) and st.epoch == 3
        opt, sched = dummy([lr, dlr])
        for epoch in range(5):
            assert st.learning_rates() == tuple(g["lr"] for g in opt.param_groups), (kind, epoch)
            st.end_epoch()
            sched.step()
        if kind != "constant":
            assert st.learning_rates()[1] < dlr
    _release(st)


def test_checkpoint_keys_and_phase_switch_on_load(psg):
    a = psg.FinalStepper(_generator(psg), lr=1e-4, scheduler="cosine", final_epochs=4)
    a.end_epoch()
    a.switch_to_joint_training()
    a.end_epoch()
    a.best_val_loss, a.global_step = 0.25, 9
    ck = a.state_dict()
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "global_step", "best_val_loss",
                       "training_phase"}
    assert ck["training_phase"] == "joint" and ck["epoch"] == 2
    assert {k.split(".")[0] for k in ck["model_state_dict"]} == {"vae_encoder", "vae_decoder", "text_encoder"}
    b = psg.FinalStepper(_generator(psg), lr=1e-4, scheduler="cosine", final_epochs=4)
    b.load_state_dict(ck)
    assert b.training_phase == "joint" and b.learning_rates() == a.learning_rates() and len(b.learning_rates()) == 2
    assert (b.epoch, b.global_step, b.best_val_loss) == (2, 9, 0.25) and b.generator.vae_decoder.live_weights()
    text = psg.FinalStepper(_generator(psg), lr=1e-4).state_dict()
    assert text["training_phase"] == "text_encoder"
    with pytest.raises(psg.PsgError, match="text_encoder"):
        b.load_state_dict(text)
