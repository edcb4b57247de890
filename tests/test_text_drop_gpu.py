"""-m gpu: classifier-free guidance training (DiffusionStepper(cond_drop_prob=), psg_text_cond_drop_f32 inside the step) and the
trainer / generator options around it, on the full-width bf16 U-Net at batch 8 (built as tests/test_ema_stepper_gpu.py builds
it; its helpers and the stubs of tests/test_trainer_gpu.py are imported).  Everything is compared on the bits."""
import numpy as np
import pytest
import torch

from tests import guided_ref as G
from tests.test_ema_stepper_gpu import TODAY_KEYS, _batches, _same, _stepper, _unet
from tests.test_trainer_gpu import _Recorder, _TextStub, _VAEStub, _config, _loaders

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, P, SEED = 8, 0.5, 1234


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


def _state(st):
    return {k: v.clone() for k, v in (("p", st.params.flat), ("m", st.optimizer._m), ("v", st.optimizer._v), ("shadow", st.params.shadow))}


@pytest.fixture(scope="module")
def stepped(psg, no_dropout):
    """Four steppers from the same weights, two steps each on the same latents, noise and t:
      drop   cond_drop_prob = 0.5, text_drop_seed = 1234, fed the text;
      plain  built without the argument, fed where(mask, null, text) with the restated mask;
      none / zero   cond_drop_prob = None / 0, fed what `plain` is fed."""
    import pokemon_sprite_generator_amd.unet as U
    batches = _batches(2, B=B, seed=11)
    null = torch.randn(32, 256, device=DEV, generator=torch.Generator(device=DEV).manual_seed(12))
    mask = G.text_drop_mask(SEED, B, P)
    m = torch.from_numpy(mask).to(DEV)
    rec = {"mask": mask}
    sts = {"drop": _stepper(psg, cond_drop_prob=P), "plain": _stepper(psg), "none": _stepper(psg, cond_drop_prob=None),
           "zero": _stepper(psg, cond_drop_prob=0)}
    for name, st in sts.items():
        outs, counts, dropped = [], [], []
        for lat, txt, t, nz in batches:
            c0 = U._SeedStream.counter
            if name == "drop":
                o = st.train_step(lat, txt, t, noise=nz, null_text=null, text_drop_seed=SEED)
                dropped.append(st.last_text_dropped.cpu().numpy().copy())
            else:
                o = st.train_step(lat, torch.where(m[:, None, None], null.unsqueeze(0), txt), t, noise=nz)
            counts.append(U._SeedStream.counter - c0)
            outs.append((o["loss"].clone(), o["grad_norm"].clone(), int(o["nan_flag"].item())))
        rec[name] = {"outs": outs, "counts": counts, "dropped": dropped, "state": _state(st), "last": st.last_text_dropped, "steps": st.steps_done()}
    yield rec, sts, null, batches
    for st in sts.values():
        st.close()


def test_drop_equals_substituted_text(stepped):
    rec = stepped[0]
    a, b = rec["drop"], rec["plain"]
    assert 0 < int(rec["mask"].sum()) < B and int(rec["mask"].sum()) == 3
    for d in a["dropped"]:
        assert d.dtype == np.int32 and np.array_equal(d.astype(bool), rec["mask"]), "last_text_dropped is not the restated mask"
    assert a["steps"] == b["steps"] == 2
    for (la, ga, fa), (lb, gb, fb) in zip(a["outs"], b["outs"]):
        assert fa == fb == 0 and _same(la, lb) and _same(ga, gb)
    for k, v in b["state"].items():
        assert _same(a["state"][k], v), f"after 2 steps {k} differs between the dropping stepper and the one fed the substituted text"
    assert a["counts"] == b["counts"], "a given text_drop_seed draws nothing from the seed stream"


def test_option_off_is_the_stepper_of_today(stepped):
    rec, sts = stepped[0], stepped[1]
    b = rec["plain"]
    for name in ("none", "zero"):
        c = rec[name]
        assert sts[name].cond_drop_prob is None and c["last"] is None
        for (lc, gc, fc), (lb, gb, fb) in zip(c["outs"], b["outs"]):
            assert fc == fb and _same(lc, lb) and _same(gc, gb)
        for k, v in b["state"].items():
            assert _same(c["state"][k], v), f"cond_drop_prob={name}: {k} differs from a stepper built without the argument"
        assert c["counts"] == b["counts"], "the seed stream moved"


def test_drop_needs_null_text_and_draws_one_seed(psg, stepped):
    import pokemon_sprite_generator_amd.unet as U
    rec, sts, null, batches = stepped
    lat, txt, t, nz = batches[0]
    st = sts["drop"]
    before = st.params.flat.clone()
    with pytest.raises(psg.PsgError, match="null_text"):
        st.train_step(lat, txt, t, noise=nz)
    assert _same(st.params.flat, before)
    with pytest.raises(ValueError):
        psg.DiffusionStepper(st.unet, psg.NoiseScheduler(), cond_drop_prob=1.0)
    # without text_drop_seed: one seed of the stream, before the forward; the mask is the restated one of that seed
    c0 = U._SeedStream.counter
    U._SeedStream.counter = c0
    want_seed = U._SeedStream.next()
    U._SeedStream.counter = c0
    st.train_step(lat, txt, t, noise=nz, null_text=null)
    assert U._SeedStream.counter - c0 == rec["plain"]["counts"][0] + 1
    assert np.array_equal(st.last_text_dropped.cpu().numpy().astype(bool), G.text_drop_mask(want_seed, B, P))
    # eval_loss stays conditional: it launches no drop
    l1, _ = st.eval_loss(lat, txt, t, noise=nz)
    kept = st.last_text_dropped.clone()
    l2, _ = st.eval_loss(lat, txt, t, noise=nz)
    assert _same(l1, l2) and torch.equal(kept, st.last_text_dropped)


def test_graphed_train_step_carries_the_text_drop(psg):
    """capture_train_step with the option: 2 warm-up steps and 2 replays against a twin's 4 eager steps under the same SeedSource
    mode, masters bit for bit; the seed is fixed in the graph and the device word moves, so the replays drop different samples,
    each the restated mask of (seed + word)."""
    from pokemon_sprite_generator_amd import ops
    import pokemon_sprite_generator_amd.unet as U
    lat, txt, t, _ = _batches(1, B=B, seed=3)[0]
    null = torch.randn(32, 256, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    try:
        word = ops.SeedSource.enable(torch.device(DEV, 0))
        word.zero_()
        a = _stepper(psg, cond_drop_prob=P)
        torch.manual_seed(5)
        U._SeedStream.counter = 0
        seed = U._SeedStream.next()                                # (under SeedSource every step restarts the counter: the first seed)
        masks_a = []
        for _ in range(4):
            w = int(word.item())
            a.train_step(lat, txt, t, null_text=null)
            masks_a.append(a.last_text_dropped.cpu().numpy().astype(bool))
            assert np.array_equal(masks_a[-1], G.text_drop_mask((seed + w) & 0xFFFFFFFFFFFFFFFF, B, P))
        torch.cuda.synchronize()
        pa, wa = a.params.flat.clone(), int(word.item())
        a.close()
        del a
        word.zero_()
        b = _stepper(psg, cond_drop_prob=P)
        torch.manual_seed(5)
        gs = b.capture_train_step(lat, txt, t, warmup=2, null_text=null)
        masks_b = []
        for _ in range(2):
            gs.run(lat, txt, t)
            masks_b.append(b.last_text_dropped.cpu().numpy().astype(bool))
        torch.cuda.synchronize()
        assert b.steps_done() == 4 and int(word.item()) == wa
        assert _same(b.params.flat, pa), "graph replays must take the eager steps bit for bit"
        assert np.array_equal(masks_b[0], masks_a[2]) and np.array_equal(masks_b[1], masks_a[3])
        assert not np.array_equal(masks_b[0], masks_b[1]), "the two replays dropped the same samples"
        b.close()
    finally:
        ops.SeedSource.disable()


# --------------------------------------------------------------------------------------------------- trainer, generator
def _decoder_stub(latent, text_emb):
    return latent[:, :3].clamp(-1.0, 1.0)


def _trainer(psg, tmp, name, **training):
    cfg = _config(tmp)
    cfg["training"].update(training)
    comps = {"text_encoder": _TextStub(), "vae_encoder": _VAEStub(), "vae_decoder": _decoder_stub, "data_loaders": _loaders(nan_batch=-1)}
    return psg.ImprovedDiffusionTrainer(cfg, "unused.pth", name, components=comps, compute_dtype=torch.bfloat16)


@pytest.fixture(scope="module")
def gpu_init(psg):
    from pokemon_sprite_generator_amd import trainer as trainer_mod
    mp = pytest.MonkeyPatch()
    mp.setattr(trainer_mod, "UNet", lambda *a, **k: _unet(psg, *a, **k))
    yield
    mp.undo()


def test_trainer_sampling_keys_and_checkpoint_without_the_option(psg, gpu_init, tmp_path, monkeypatch):
    torch.manual_seed(0)
    tr = _trainer(psg, tmp_path, "s", sampler="ddim", sample_steps=3, guidance_scale=2, ddim_eta=0.0)
    assert tr.cond_drop_prob is None and tr.stepper.cond_drop_prob is None
    seen = []
    real = tr.stepper.sample
    monkeypatch.setattr(tr.stepper, "sample", lambda *a, **k: (seen.append(k), real(*a, **k))[1])
    rec = _Recorder()
    tr.writer = rec
    tr.generate_samples(0)
    assert len(rec.images) == 4 and all(bool(torch.isfinite(img).all()) and img.shape == (3, 27, 27) for _, img, _ in rec.images)
    assert len({float(img.double().sum()) for _, img, _ in rec.images}) == 4
    assert len(seen) == 1 and seen[0]["sampler"] == "ddim" and seen[0]["num_steps"] == 3 and seen[0]["guidance_scale"] == 2.0 and seen[0]["eta"] == 0.0
    null = seen[0]["null_text"]
    assert tuple(null.shape) == (32, 256) and torch.equal(null, _TextStub()([""])[0].float()) and tr.null_text(32) is null     # cached per S
    # sample() / ddpm_sample() honour the keys: the chain by hand
    te = _TextStub()(["pokemon x", "pokemon y"]).float()
    nf = lambda i, shape: torch.full(shape, 0.25) if i < 0 else torch.zeros(shape)       # noqa: E731
    got = tr.sample(te, 2, noise_fn=nf)
    want = psg.ddim_sample(tr.unet, te, tr.noise_scheduler.alphas_cumprod, num_steps=3, guidance_scale=2.0, null_text=null, noise_fn=nf)
    assert _same(got, want) and tr.ddpm_sample(te, 2).shape == got.shape
    saved = {}
    monkeypatch.setattr(torch, "save", lambda obj, path: saved.update(obj))
    tr.save_checkpoint(0, is_best=True)
    assert set(saved) == TODAY_KEYS
    tr.stepper.close()


def test_trainer_cond_drop_trains_and_marks_the_checkpoint(psg, gpu_init, no_dropout, tmp_path, monkeypatch):
    torch.manual_seed(0)
    tr = _trainer(psg, tmp_path, "d", cond_drop_prob=0.25)
    assert tr.stepper.cond_drop_prob == 0.25
    lat, txt, t, nz = _batches(1, B=B, seed=31)[0]
    out = tr.train_step(lat, txt, t, noise=nz, text_drop_seed=SEED)
    assert int(out["nan_flag"].item()) == 0 and tr.optimizer.steps_done() == 1
    assert np.array_equal(tr.stepper.last_text_dropped.cpu().numpy().astype(bool), G.text_drop_mask(SEED, B, 0.25))
    m = tr.train_epoch(0)                                          # the loop supplies the null text itself
    assert np.isfinite(m["train_loss"]) and tr.optimizer.steps_done() == 4
    saved = {}
    monkeypatch.setattr(torch, "save", lambda obj, path: saved.update(obj))
    tr.save_checkpoint(0, is_best=True)
    assert set(saved) == TODAY_KEYS | {"cond_drop_prob"} and saved["cond_drop_prob"] == 0.25
    tr.stepper.close()


def test_generator_ddim_and_guidance(psg, golden):
    from oracle import hashgen
    from pokemon_sprite_generator_amd import guidance, imaging
    from tests import text_cases as TC
    from tests import text_grad_cases as GC
    from tests.test_generate_gpu import StandInUNet, noise_fn
    vae = psg.PokemonVAE(latent_dim=8, text_dim=256)
    vae.load_state_dict(hashgen.fill_unet_state({k: tuple(v.shape) for k, v in vae.state_dict().items()}, 11, "stress"))
    te = psg.TextEncoder(bert_config=TC.bert_config(2), hidden_dim=256, finetune_strategy="none")
    te.load_state_dict(GC.state_dict(te), strict=True)
    gen = psg.SpriteGenerator(vae.to(DEV), StandInUNet().to(DEV), te.to(DEV))
    g = golden("text_encoder_grad.npz")
    tokens = (torch.from_numpy(g["M_input_ids"])[:2], torch.from_numpy(g["M_attention_mask"])[:2])
    got = gen.generate_from_text(tokens, sampler="ddim", num_inference_steps=3, guidance_scale=2, noise_fn=noise_fn)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 215, 215, 3) and got.is_cuda
    # by hand: the empty description at the prompts' length, the linear schedule, ddim_sample, decode
    text = gen.text_encoder.encode_ids(*tokens)
    S = text.shape[1]
    ids, mask = guidance.null_text_tokens(gen.text_encoder, S, like=tokens)
    assert ids.shape == (1, S) and mask.tolist() == [[1, 1] + [0] * (S - 2)] and int(ids[0, 0]) == int(tokens[0][0, 0])
    null = gen.text_encoder.encode_ids(ids, mask)[0]
    abar = torch.cumprod(1.0 - torch.linspace(0.0001, 0.02, 1000), dim=0)
    lat = psg.ddim_sample(gen.unet, text, abar, num_steps=3, guidance_scale=2.0, null_text=null, noise_fn=noise_fn)
    assert torch.equal(got, imaging.to_uint8(gen.vae.decode(lat, text)))
    plain = gen.generate_from_text(tokens, num_inference_steps=3, noise_fn=noise_fn)
    guided = gen.generate_from_text(tokens, num_inference_steps=3, noise_fn=noise_fn, guidance_scale=2)
    lat_g = psg.gradio_ddpm_sample(gen.unet, text, 3, noise_fn=noise_fn, guidance_scale=2.0, null_text=null)
    assert torch.equal(guided, imaging.to_uint8(gen.vae.decode(lat_g, text))) and not torch.equal(got, plain)
    with pytest.raises(psg.PsgError, match="sampler"):
        gen.generate_from_text(tokens, sampler="plms", num_inference_steps=3, noise_fn=noise_fn)
