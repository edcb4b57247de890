"""-m gpu: the EMA of the U-Net weights through the optimizer, the stepper, the trainer and the checkpoint consumers, on the
full-width bf16 U-Net at batch 2 (built as tests/test_trainer_gpu.py builds it; its stubs and config are imported).

Everything is compared on the bits: a stepper with an EMA trains exactly as one without; the EMA buffer is the fp32 restatement
of tests/ema_ref.py folded over the recorded masters; a skipped step moves nothing; inside `ema_weights()` the model IS the
averaged model and afterwards training continues as if the scope had never been entered; a captured graph carries the EMA
along; checkpoints round-trip it and the consumers load it."""
import pytest
import torch

from tests import ema_ref as E
from tests.test_trainer_gpu import _TextStub, _VAEStub, _config, _loaders

pytestmark = pytest.mark.gpu
DEV = "cuda"
DECAY = 0.999


@pytest.fixture(scope="module")
def psg():
    import pokemon_sprite_generator_amd as m
    from pokemon_sprite_generator_amd import _lib
    _lib.init(0)
    return m


@pytest.fixture(scope="module")
def no_dropout():
    """Dropout seeds are drawn per call: off, so that twin steppers see the same masks (none)."""
    import pokemon_sprite_generator_amd.unet as U
    old, U.ATTN_DROPOUT = U.ATTN_DROPOUT, 0.0
    yield
    U.ATTN_DROPOUT = old


def _batches(n, B=2, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = []
    for _ in range(n):
        out.append((torch.randn(B, 8, 27, 27, device=DEV, generator=g), torch.randn(B, 32, 256, device=DEV, generator=g),
                    torch.randint(0, 1000, (B,), device=DEV, generator=g), torch.randn(B, 8, 27, 27, device=DEV, generator=g)))
    return out


def _unet(psg, *a, **kw):
    """A UNet initialised on the GPU (torch.device context): the 640 M parameters take seconds to draw on the CPU."""
    with torch.device(DEV):
        return psg.UNet(*a, **kw)


def _stepper(psg, **kw):
    torch.manual_seed(0)
    return psg.DiffusionStepper(_unet(psg, compute_dtype=torch.bfloat16), psg.NoiseScheduler(), lr=3e-4, distributed=False, **kw)


def _same(a, b):
    """Bitwise equality of two tensors of one dtype (NaN-proof: compared as integers)."""
    iv = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(iv), b.contiguous().view(iv)))


@pytest.fixture(scope="module")
def twins(psg, no_dropout):
    """Two steppers from the same weights on the same three batches, noise and t; one keeps an EMA.  The EMA twin's masters are
    recorded before the first and after every step."""
    plain, ema = _stepper(psg), _stepper(psg, ema_decay=DECAY)
    assert _same(plain.params.flat, ema.params.flat) and not plain.ema_enabled and ema.ema_enabled
    rec = {"ema0": ema.optimizer._ema.clone(), "masters": []}
    assert _same(rec["ema0"], ema.params.flat)                        # the average starts as a copy of the masters
    for lat, txt, t, nz in _batches(3):
        op, oe = plain.train_step(lat, txt, t, noise=nz), ema.train_step(lat, txt, t, noise=nz)
        assert int(op["nan_flag"].item()) == 0 and int(oe["nan_flag"].item()) == 0
        assert float(op["loss"].item()) == float(oe["loss"].item())
        rec["masters"].append(ema.params.flat.clone())
    rec["ema3"] = ema.optimizer._ema.clone()
    rec["plain3"] = {k: v.clone() for k, v in (("p", plain.params.flat), ("m", plain.optimizer._m), ("v", plain.optimizer._v), ("shadow", plain.params.shadow))}
    rec["ema_side3"] = {k: v.clone() for k, v in (("p", ema.params.flat), ("m", ema.optimizer._m), ("v", ema.optimizer._v), ("shadow", ema.params.shadow))}
    rec["steps3"] = (plain.steps_done(), ema.steps_done())
    yield plain, ema, rec
    plain.close()
    ema.close()


def test_ema_changes_nothing_else(twins):
    _, _, rec = twins
    assert rec["steps3"] == (3, 3)
    for k, v in rec["plain3"].items():
        assert _same(rec["ema_side3"][k], v), f"after 3 steps {k} differs between the stepper with an EMA and the one without"
    assert not _same(rec["masters"][0], rec["ema0"]) and not _same(rec["masters"][2], rec["masters"][1])     # the steps moved the masters


def test_ema_values_are_the_restatement_folded_over_the_masters(twins):
    _, _, rec = twins
    want = E.fold(rec["ema0"], rec["masters"], DECAY, 1)              # steps k = 1, 2, 3 under the warm-up: d = 2/11, 3/12, 4/13
    assert _same(rec["ema3"], want)
    assert not _same(rec["ema3"], rec["masters"][2]) and not _same(rec["ema3"], rec["ema0"])
    off_by_one = E.fold(rec["ema0"], rec["masters"], DECAY, 1, k0=2)
    assert not _same(rec["ema3"], off_by_one)


def test_skipped_step_moves_nothing(twins):
    _, ema, _ = twins
    lat, txt, t, nz = _batches(1, seed=7)[0]
    p, e, n = ema.params.flat.clone(), ema.optimizer._ema.clone(), ema.steps_done()
    out = ema.train_step(lat, txt, t, noise=nz, pre_flag=torch.tensor([32], device=DEV))
    assert int(out["nan_flag"].item()) == 32
    assert _same(ema.params.flat, p) and _same(ema.optimizer._ema, e) and ema.steps_done() == n


def test_ema_weights_scope(psg, twins):
    """Inside the scope the model's parameters are the EMA (state_dict values) and its bf16 forward has the bits of a fresh UNet
    loaded with them - a fresh UNet under a stepper of its own, so that both forwards take the arena's launch route (bf16
    shadow slices as prepared weights, the projections grouped); afterwards masters and shadow have their old bits and the
    next step is the twin's that never entered a scope."""
    plain, ema, _ = twins
    lat, txt, t, nz = _batches(1, seed=11)[0]
    names = [n for n, p in ema.unet.named_parameters() if p.requires_grad]
    before = {n: v.clone() for n, v in zip(names, ema.ema_state())}
    ema_sd = ema.ema_state_dict()
    w = "enc_block1.0.res_block.conv1.weight"
    assert tuple(before[w].shape) == (640, 640, 3, 3) and list(ema_sd) == list(ema.unet.state_dict())
    masters, shadow, avg = ema.params.flat.clone(), ema.params.shadow.clone(), ema.optimizer._ema.clone()
    flat_ptr = ema.params.flat.data_ptr()
    with ema.ema_weights() as scope:
        assert scope is ema
        sd = ema.unet.state_dict()
        assert all(torch.equal(sd[n], before[n]) for n in names) and all(torch.equal(sd[k], v) for k, v in ema_sd.items())
        assert _same(ema.params.flat, avg) and _same(ema.optimizer._ema, masters) and ema.params.flat.data_ptr() == flat_ptr
        assert _same(ema.params.shadow, avg.to(torch.bfloat16))
        ema.unet.eval()
        with torch.no_grad():
            got = ema.unet(lat, t, txt).clone()
        with pytest.raises(psg.PsgError, match="ema_weights"):
            ema.train_step(lat, txt, t, noise=nz)
        with pytest.raises(psg.PsgError, match="ema_weights"):
            ema.capture_train_step(lat, txt, t)
        with pytest.raises(psg.PsgError, match="ema_weights"):
            ema.autotune_exchange(lat, txt, t)
        with pytest.raises(psg.PsgError, match="already inside"):
            with ema.ema_weights():
                pass
        assert _same(ema.params.flat, avg), "a refused call inside the scope moved the weights"
    assert _same(ema.params.flat, masters) and _same(ema.params.shadow, shadow) and _same(ema.optimizer._ema, avg)

    with pytest.raises(RuntimeError, match="boom"):                   # an exception inside the scope still swaps back
        with ema.ema_weights():
            assert _same(ema.params.flat, avg)
            raise RuntimeError("boom")
    assert _same(ema.params.flat, masters) and _same(ema.params.shadow, shadow) and _same(ema.optimizer._ema, avg) and not ema._ema_scope
    with pytest.raises(psg.PsgError, match="no EMA"):
        with plain.ema_weights():
            pass

    fresh = _unet(psg, compute_dtype=torch.bfloat16)
    fresh.load_state_dict(ema_sd)
    fs = psg.DiffusionStepper(fresh, psg.NoiseScheduler(), distributed=False)
    fresh.eval()
    with torch.no_grad():
        want = fresh(lat, t, txt).clone()
    fs.close()
    del fs, fresh
    assert bool(torch.isfinite(want).all()) and _same(got, want), "the forward inside ema_weights() is not the averaged model's"
    with torch.no_grad():
        raw = ema.unet(lat, t, txt)
    assert not _same(raw, got)                                        # (and outside the scope it is the raw model again)

    # the next step: the twin never entered a scope
    assert _same(plain.params.flat, ema.params.flat)
    op, oe = plain.train_step(lat, txt, t, noise=nz), ema.train_step(lat, txt, t, noise=nz)
    assert float(op["loss"].item()) == float(oe["loss"].item())
    assert _same(plain.params.flat, ema.params.flat) and _same(plain.params.shadow, ema.params.shadow) and plain.steps_done() == ema.steps_done()
    assert _same(ema.optimizer._ema, E.ema_f32(avg, ema.params.flat, DECAY, 1, ema.steps_done()))


def test_adam_branch_and_generic_optimizer_refuse_an_ema(psg):
    blk = torch.nn.Sequential(torch.nn.Conv2d(8, 16, 3, padding=1)).to(DEV)
    blk.compute_dtype = torch.float32
    with pytest.raises(psg.PsgError, match="ema_decay"):
        psg.DiffusionStepper(blk, psg.NoiseScheduler(), distributed=False, optimizer_type="adam", ema_decay=0.99)
    with pytest.raises(psg.PsgError, match="enable_ema"):
        psg.FusedAdamW(blk.parameters()).enable_ema(0.99)
    st = psg.DiffusionStepper(blk, psg.NoiseScheduler(), distributed=False, ema_decay=0)       # 0 and None: no EMA
    assert not st.ema_enabled and st.optimizer._ema is None
    with pytest.raises(ValueError):
        st.optimizer.enable_ema(1.0)
    with pytest.raises(psg.PsgError, match="no EMA"):
        st.optimizer.swap_ema()
    st.close()


def test_graphed_train_step_carries_the_ema(psg):
    """capture_train_step with an EMA: 2 warm-up steps and 3 replays against a twin's 5 eager steps under the same SeedSource
    mode - masters and EMA bit for bit; an ema_weights() scope between replays changes nothing that follows."""
    from pokemon_sprite_generator_amd import ops
    lat, txt, t, _ = _batches(1, B=4, seed=3)[0]
    try:
        word = ops.SeedSource.enable(torch.device(DEV, 0))
        word.zero_()
        a = _stepper(psg, ema_decay=DECAY)
        torch.manual_seed(5)
        for _ in range(5):
            a.train_step(lat, txt, t)
        torch.cuda.synchronize()
        pa, ea, wa = a.params.flat.clone(), a.optimizer._ema.clone(), int(word.item())
        a.close()
        del a
        word.zero_()
        b = _stepper(psg, ema_decay=DECAY)
        torch.manual_seed(5)
        gs = b.capture_train_step(lat, txt, t, warmup=2)
        gs.run(lat, txt, t)
        gs.run(lat, txt, t)
        with b.ema_weights():
            b.unet.eval()
            with torch.no_grad():
                assert bool(torch.isfinite(b.unet(lat, t, txt)).all())
            with pytest.raises(psg.PsgError, match="ema_weights"):
                gs.run(lat, txt, t)
        gs.run(lat, txt, t)
        torch.cuda.synchronize()
        assert b.steps_done() == 5 and int(word.item()) == wa
        assert _same(b.params.flat, pa), "graph replays (with an ema_weights() scope in between) must take the eager steps bit for bit"
        assert _same(b.optimizer._ema, ea), "the EMA after graph replays differs from the eager twin's"
        assert not _same(ea, pa)
        b.close()
    finally:
        ops.SeedSource.disable()


def _trainer(psg, tmp, name, ema=True):
    cfg = _config(tmp)
    if ema:
        cfg["training"]["ema_decay"] = DECAY
    comps = {"text_encoder": _TextStub(), "vae_encoder": _VAEStub(), "data_loaders": _loaders(nan_batch=-1)}
    return psg.ImprovedDiffusionTrainer(cfg, "unused.pth", name, components=comps, compute_dtype=torch.bfloat16)


TODAY_KEYS = {"epoch", "global_step", "unet_state_dict", "optimizer_state_dict", "scheduler_state_dict", "best_val_loss", "config"}


@pytest.fixture(scope="module")
def trained(psg, no_dropout, tmp_path_factory):
    """A trainer with `training.ema_decay` after two steps, and its checkpoint: the file, and the dict that was written.
    A full-width checkpoint is 10 GB of file traffic each way, so it goes through the file system once per direction that
    matters (saved here; loaded by a fresh trainer and by `SpriteGenerator.from_checkpoints` below); the checkpoint without
    the EMA section and the one of a trainer without `ema_decay` stay in memory.  Every UNet is initialised on the GPU."""
    from pokemon_sprite_generator_amd import generate, trainer as trainer_mod
    mp = pytest.MonkeyPatch()
    mp.setattr(trainer_mod, "UNet", lambda *a, **k: _unet(psg, *a, **k))
    mp.setattr(generate, "UNet", lambda *a, **k: _unet(psg, *a, **k))
    tmp = tmp_path_factory.mktemp("ema_trainer")
    batches = _batches(3, seed=21)
    torch.manual_seed(0)
    tr = _trainer(psg, tmp, "a")
    assert tr.stepper.ema_enabled and tr.optimizer.ema_decay == DECAY and tr.optimizer.ema_warmup is True
    for lat, txt, t, nz in batches[:2]:
        tr.train_step(lat, txt, t, noise=nz)
    saved, real_save = {}, torch.save
    with mp.context() as m:                                           # written for real; the dict is kept for the assertions
        m.setattr(torch, "save", lambda obj, path: (saved.update(obj), real_save(obj, path))[1])
        tr.save_checkpoint(0, is_best=True)
    path = tr.checkpoint_dir / "diffusion_best_model.pth"
    assert path.exists()
    yield {"tr": tr, "tmp": tmp, "batches": batches, "saved": saved, "path": path}
    tr.stepper.close()
    mp.undo()


def test_trainer_validates_and_samples_on_the_ema(psg, trained, monkeypatch):
    tr, batches = trained["tr"], trained["batches"]
    masters, avg = tr.stepper.params.flat.clone(), tr.optimizer._ema.clone()
    seen = []
    real_eval = tr.stepper.eval_loss
    monkeypatch.setattr(tr.stepper, "eval_loss", lambda *a, **k: (seen.append(_same(tr.stepper.params.flat, avg)), real_eval(*a, **k))[1])
    assert tr.validate_epoch(0)["val_loss"] > 0 and seen == [True]
    noise_fn = lambda i, shape: torch.zeros(shape) if i >= 0 else torch.ones(shape) * 0.5
    txt1 = batches[0][1][:1]
    s_ema, s_raw, s_default = tr.sample(txt1, 1, noise_fn=noise_fn, use_ema=True), tr.sample(txt1, 1, noise_fn=noise_fn, use_ema=False), tr.ddpm_sample(txt1, 1)
    assert bool(torch.isfinite(s_ema).all()) and not _same(s_ema, s_raw) and s_default.shape == s_ema.shape
    assert _same(tr.stepper.params.flat, masters) and _same(tr.optimizer._ema, avg) and not tr.stepper._ema_scope


def test_checkpoint_has_the_ema_section_next_to_todays_keys(trained):
    saved = trained["saved"]
    assert set(saved) == TODAY_KEYS | {"ema_unet_state_dict", "ema_decay"} and saved["ema_decay"] == DECAY
    usd, esd = saved["unet_state_dict"], saved["ema_unet_state_dict"]
    assert list(esd) == list(usd) and all(esd[k].shape == usd[k].shape and esd[k].dtype == usd[k].dtype for k in usd)
    assert any(not torch.equal(esd[k], usd[k]) for k in usd)
    assert set(saved["optimizer_state_dict"]["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}           # torch.optim.AdamW's layout


def test_checkpoint_resumes_to_the_bit(psg, trained, monkeypatch):
    """Last of the tests that read the trainer's state: it steps the trainer."""
    tr, saved, path = trained["tr"], trained["saved"], trained["path"]
    # a checkpoint without the section loads, and the EMA is the loaded weights; then the real file: the EMA is the saved one
    torch.manual_seed(1)
    tr2 = _trainer(psg, trained["tmp"], "b")
    bare = {k: v for k, v in saved.items() if k in TODAY_KEYS}
    with monkeypatch.context() as m:
        m.setattr(torch, "load", lambda *a, **k: bare)
        tr2.load_checkpoint("in-memory")
    assert _same(tr2.stepper.params.flat, tr.stepper.params.flat) and _same(tr2.optimizer._ema, tr2.stepper.params.flat)
    assert "no 'ema_unet_state_dict'" in (tr2.log_dir / "diffusion_training.log").read_text()
    tr2.load_checkpoint(str(path))
    assert _same(tr2.stepper.params.flat, tr.stepper.params.flat) and _same(tr2.optimizer._ema, tr.optimizer._ema)
    assert not _same(tr2.optimizer._ema, tr2.stepper.params.flat) and tr2.optimizer.steps_done() == tr.optimizer.steps_done() == 2
    lat, txt, t, nz = trained["batches"][2]
    o1, o2 = tr.train_step(lat, txt, t, noise=nz), tr2.train_step(lat, txt, t, noise=nz)
    assert float(o1["loss"].item()) == float(o2["loss"].item()) and tr2.optimizer.steps_done() == 3
    assert _same(tr2.stepper.params.flat, tr.stepper.params.flat), "the resumed trainer must take the identical step"
    assert _same(tr2.optimizer._ema, tr.optimizer._ema), "the resumed trainer's EMA differs from the uninterrupted one"
    tr2.stepper.close()


def test_trainer_without_ema_decay_writes_todays_keys(psg, trained, monkeypatch):
    torch.manual_seed(2)
    tr3 = _trainer(psg, trained["tmp"], "c", ema=False)
    assert not tr3.stepper.ema_enabled
    plain_ck = {}
    with monkeypatch.context() as m:
        m.setattr(torch, "save", lambda obj, path: plain_ck.update(obj))
        tr3.save_checkpoint(0, is_best=True)
    assert set(plain_ck) == TODAY_KEYS
    with pytest.raises(psg.PsgError, match="no EMA"):
        tr3.sample(trained["batches"][0][1][:1], 1, use_ema=True)
    tr3.stepper.close()


def test_sprite_generator_loads_the_ema_section(psg, trained, monkeypatch):
    """The real U-Net from the checkpoint file's EMA section (VAE and text encoder are stand-ins)."""
    from pokemon_sprite_generator_amd import generate
    from tests.test_generate_cpu import _StandIn
    tmp, path, esd = trained["tmp"], trained["path"], trained["saved"]["ema_unet_state_dict"]
    for name in ("PokemonVAE", "TextEncoder"):
        monkeypatch.setattr(generate, name, type(name, (_StandIn,), {}))
    torch.save({"vae_state_dict": {}}, tmp / "vae.pth")
    torch.save({"unet_state_dict": {}, "global_step": 2}, tmp / "no_ema.pth")
    model_cfg = dict(_config(tmp)["model"], num_heads=4)
    g = generate.SpriteGenerator.from_checkpoints(str(tmp / "vae.pth"), str(path), {"model": model_cfg}, compute_dtype=torch.bfloat16, use_ema=True)
    gsd = g.unet.state_dict()
    assert list(gsd) == list(esd) and all(torch.equal(gsd[k], esd[k]) for k in esd)
    w = "enc_block1.0.res_block.conv1.weight"
    assert not torch.equal(gsd[w], trained["saved"]["unet_state_dict"][w])        # (not the raw weights: the trainer's live masters)
    with pytest.raises(psg.PsgError, match="ema_unet_state_dict"):
        generate.SpriteGenerator.from_checkpoints(str(tmp / "vae.pth"), str(tmp / "no_ema.pth"), {"model": model_cfg}, use_ema=True)
