"""-m gpu: FinalTrainer - stage 3's epochs, the phase switch, validation, checkpoint, resume and sample sheet around
FinalStepper - against a twin that drives a second FinalStepper over a second identical loader by hand.

Setup (tests/trainer_cases.py): the 8 fixture sprites split 5 / 2 / 1, batch 2; the generator of tests/test_final_joint_gpu.py
(frozen VAE encoder, trainable decoder, a small stand-in for the U-Net, a 2-layer BERT without dropout), tests/clip_ref.py's
"hook" CLIP with a stand-in tokenizer; final_epochs 2, phase1_epochs 1; fp32; `torch.manual_seed` in front of each run.

The trainer and the twin launch the same deterministic kernels on the same inputs: metrics and parameters are compared with
== / torch.equal.  The cached CLIP text features are compared with `text_features` of each training batch the same way: the
text tower is causal and pools at the EOS, so a row depends on its own tokens only, not on how far its batch is padded."""
import pytest
import torch

from tests import trainer_cases as TCs

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("loss", "l1_loss", "mse_loss")
CKPT_KEYS = {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "config", "global_step", "best_val_loss",
             "training_phase"}                          # final_trainer.py:646-655


@pytest.fixture(scope="module")
def psg():
    import pokemon_sprite_generator_amd as m
    from pokemon_sprite_generator_amd import _lib
    _lib.init(0)
    yield m
    m.ops.GradSink.unregister_all()
    m.ops.WeightCache.clear()


@pytest.fixture(scope="module")
def world(psg):
    return TCs.world(psg)


def _trainer(psg, world, tmp, name, clip="cached"):
    comps = {"generator": TCs.generator(psg, world), "clip_loss": None if clip is None else TCs.clip(psg, world, tokenizer=clip == "cached")}
    return psg.FinalTrainer(TCs.config(tmp), "unused_vae.pth", "unused_diffusion.pth", name, components=comps, compute_dtype=torch.float32)


def _chunked_features(clip, dataset):
    """The trainer's set-up restated: text_features of every dataset row in chunks of the batch size."""
    texts = [dataset.meta(i)["full_description"] for i in range(len(dataset))]
    return torch.cat([clip.text_features(clip.tokenize(texts[lo:lo + TCs.BATCH]).to(DEV)) for lo in range(0, len(texts), TCs.BATCH)], 0)


def _by_hand(st, loaders, clip, feats, cfg):
    """What FinalTrainer.train() does to a stepper, written out: [(phase, train means + clip mean, validation means)]."""
    out = []
    tc = cfg["training"]
    for epoch in range(tc["final_epochs"]):
        if epoch == tc["phase1_epochs"] and st.training_phase == "text_encoder":
            st.switch_to_joint_training()
        st.epoch = epoch
        st.generator.train()
        loaders["train"].set_epoch(epoch)
        rows, terms = [], []
        for b in loaders["train"]:
            kw = {}
            if clip is not None:
                def term(recon, idx):
                    terms.append(clip.forward_features(recon, feats[idx]))
                    return terms[-1]
                kw = dict(clip_loss=term, clip_weight=tc["clip_weight"], texts=b["index"])
            rows.append(st.train_step(b["image"], b["input_ids"], b["attention_mask"], **kw))
        train = TCs.mean_of(rows, KEYS, len(rows))
        clip_sum = torch.zeros(1, device=DEV)
        for t in terms:
            clip_sum += t.detach().reshape(1)
        train.append(float(clip_sum) / len(rows))
        st.generator.eval()
        vrows = [st.validate_step(b["image"], b["input_ids"], b["attention_mask"]) for b in loaders["val"]]
        out.append((st.training_phase, train, TCs.mean_of(vrows, KEYS, len(vrows))))
        st.end_epoch()
    return out


def _run(psg, world, tmp, name, clip):
    tr = _trainer(psg, world, tmp, name, clip)
    start = TCs.snapshot(tr.generator)
    log = TCs.record(tr, after_epoch=lambda t, e: (t.training_phase, TCs.snapshot(t.generator.vae_decoder)))
    torch.manual_seed(TCs.SEED)
    tr.train()
    own = TCs.snapshot(tr.generator)
    gen = TCs.generator(psg, world)
    twin = psg.FinalStepper(gen, config=TCs.config(tmp))
    twin_clip = None if clip is None else TCs.clip(psg, world)
    loaders = TCs.loaders(psg)
    feats = None if clip is None else _chunked_features(twin_clip, loaders["train"].dataset)
    torch.manual_seed(TCs.SEED)
    hand = _by_hand(twin, loaders, twin_clip, feats, TCs.config(tmp))
    torch.cuda.synchronize()
    return {"trainer": tr, "log": log, "start": start, "own": own, "twin": TCs.snapshot(gen), "hand": hand, "tmp": tmp}


@pytest.fixture(scope="module")
def with_clip(psg, world, tmp_path_factory):
    return _run(psg, world, tmp_path_factory.mktemp("stage3_clip"), "clip", "cached")


@pytest.fixture(scope="module")
def without_clip(psg, world, tmp_path_factory):
    return _run(psg, world, tmp_path_factory.mktemp("stage3_plain"), "plain", None)


def test_phase_switch_and_what_moves(psg, with_clip):
    r = with_clip
    tr, start = r["trainer"], r["start"]
    assert [(k, e) for k, e, _ in r["log"]] == [("train", 0), ("state", 0), ("val", 0), ("train", 1), ("state", 1), ("val", 1)]
    (phase0, dec0), (phase1, dec1) = r["log"][1][2], r["log"][4][2]
    assert phase0 == "text_encoder" and phase1 == "joint" == tr.training_phase
    for n, p in dec0.items():                                             # epoch 0: the decoder is frozen
        assert torch.equal(p, start["vae_decoder." + n]), n
    moved = sum(not torch.equal(p, dec0[n]) for n, p in dec1.items())
    assert moved >= len(dec1) - 2, (moved, len(dec1))                      # (two biases have an exactly zero gradient: vae_decoder_ref.ZERO_GRAD)
    assert any(not torch.equal(r["own"][n], start[n]) for n in start if n.startswith("text_encoder."))
    for n in start:                                                       # never stepped: the encoder and the U-Net
        if n.startswith(("vae_encoder.", "unet.")):
            assert torch.equal(r["own"][n], start[n]), n
    assert [g["name"] for g in tr.optimizer.param_groups] == ["text_encoder", "vae_decoder"]
    assert tr.current_epoch == 2 and tr.global_step == 4 and (tr.log_dir / "final_training.log").exists()


@pytest.mark.parametrize("which", ["with_clip", "without_clip"])
def test_metrics_equal_the_hand_driven_twin_bit_for_bit(psg, which, request):
    r = request.getfixturevalue(which)
    for epoch in range(2):
        tm, vm = [m for k, e, m in r["log"] if e == epoch and k in ("train", "val")]
        assert set(tm) == {"loss", "l1_loss", "mse_loss", "clip_loss"} and set(vm) == {"loss", "l1_loss", "mse_loss"}
        phase, train, val = r["hand"][epoch]
        got_t, got_v = [tm[k] for k in KEYS + ("clip_loss",)], [vm[k] for k in KEYS]
        print(f"{which} epoch {epoch} ({phase}): train {got_t} twin {train}; val {got_v} twin {val}")
        assert got_t == train and got_v == val, epoch
        assert phase == ("text_encoder", "joint")[epoch]
        if which == "with_clip":
            assert -1.0 <= tm["clip_loss"] <= 1.0 and tm["clip_loss"] != 0.0
            # the total holds the term: L1 + 0.1 MSE + 0.1 CLIP, up to the rounding of the means
            want = tm["l1_loss"] + 0.1 * tm["mse_loss"] + 0.1 * tm["clip_loss"]
            assert abs(tm["loss"] - want) <= 1e-5 * abs(want), (tm, want)
        else:
            assert tm["clip_loss"] == 0.0
        assert abs(vm["loss"] - (vm["l1_loss"] + 0.1 * vm["mse_loss"])) <= 1e-5 * vm["loss"]     # validation: no CLIP term
    for n, p in r["own"].items():
        assert torch.equal(p, r["twin"][n]), n


def test_cached_clip_features_equal_the_per_batch_text_tower(psg, world, with_clip):
    tr = with_clip["trainer"]
    clip, feats = tr.clip_loss, tr.clip_text_features
    ds = tr.data_loaders["train"].dataset
    assert feats is not None and tuple(feats.shape) == (len(ds), 32) and not feats.requires_grad
    assert torch.equal(feats, _chunked_features(clip, ds))
    lengths, worst = set(), 0.0
    tr.data_loaders["train"].set_epoch(0)
    for batch in list(tr.data_loaders["train"]) + list(tr.data_loaders["val"]):
        ids = clip.tokenize(batch["full_description"]).to(DEV)
        lengths.add(ids.shape[1])
        own = clip.text_features(ids)
        cached = feats[batch["index"]]
        worst = max(worst, float((own.float() - cached.float()).abs().max()))
        print(f"rows {batch['index'].tolist()} padded to {ids.shape[1]}: max |per-batch - cached| {worst:.3e}")
        assert torch.equal(own, cached), batch["index"].tolist()
    assert len(lengths) > 1                                               # the batches are padded to different lengths
    # a trainer whose CLIP has no tokenizer keeps no table of features (the per-batch path)
    plain = TCs.clip(psg, world, tokenizer=False)
    tr2 = psg.FinalTrainer(TCs.config(with_clip["tmp"]), "-", "-", "no_tokenizer", components={
        "generator": tr.generator, "clip_loss": plain, "data_loaders": tr.data_loaders}, compute_dtype=torch.float32)
    assert tr2.clip_text_features is None


def test_joint_checkpoint_resumes_in_the_joint_phase(psg, world, with_clip):
    tr, tmp = with_clip["trainer"], with_clip["tmp"]
    path = tr.checkpoint_dir / "final_best_model.pth"
    assert path.exists()                                                  # epoch 0 at the latest was a best
    first = torch.load(path, map_location="cpu")
    vals = [m["loss"] for k, e, m in with_clip["log"] if k == "val"]
    assert set(first) == CKPT_KEYS and first["best_val_loss"] == min(vals) == tr.best_val_loss
    assert first["epoch"] == vals.index(min(vals)) and first["global_step"] == 2 * (first["epoch"] + 1)
    assert first["training_phase"] == ("text_encoder", "joint")[first["epoch"]]
    tr.save_checkpoint(1, is_best=True)                                   # the state after the joint epoch, whichever was best
    ck = torch.load(path, map_location="cpu")
    assert set(ck) == CKPT_KEYS and ck["training_phase"] == "joint" and ck["epoch"] == 1 and ck["global_step"] == 4
    assert set(ck["model_state_dict"]) == set(tr.generator.state_dict())
    assert {k.split(".")[0] for k in ck["model_state_dict"]} == {"vae_encoder", "vae_decoder", "unet", "text_encoder"}
    assert [g["name"] for g in ck["optimizer_state_dict"]["param_groups"]] == ["text_encoder", "vae_decoder"]
    again = _trainer(psg, world, tmp, "again")
    assert again.training_phase == "text_encoder"
    again.load_checkpoint(str(path))
    assert again.training_phase == "joint" and again.current_epoch == 1 and again.global_step == 4
    assert all(p.requires_grad for p in again.generator.vae_decoder.parameters())
    for n, p in TCs.snapshot(again.generator).items():
        assert torch.equal(p, with_clip["own"][n]), n
    results = []
    for t in (tr, again):
        torch.manual_seed(TCs.SEED + 1)
        tm, vm = t.train_epoch(1), t.validate_epoch(1)
        results.append((tm, vm, TCs.snapshot(t.generator)))
    assert results[0][0] == results[1][0] and results[0][1] == results[1][1]
    assert all(torch.equal(results[0][2][n], results[1][2][n]) for n in results[0][2])
    assert any(not torch.equal(results[0][2]["vae_decoder." + n], p) for n, p in with_clip["log"][4][2][1].items())


def test_sample_sheet(psg, with_clip):
    from PIL import Image
    import numpy as np
    tr = with_clip["trainer"]
    assert sorted(p.name for p in tr.sample_dir.iterdir()) == ["final_epoch_0000.png", "final_epoch_0001.png"]
    sheet = np.asarray(Image.open(tr.sample_dir / "final_epoch_0000.png"))
    batch = next(iter(tr.data_loaders["val"]))
    assert sheet.shape == (2 * TCs.SIDE, 2 * TCs.SIDE, 3)
    real = psg.imaging.to_uint8(batch["image"]).cpu().numpy()
    for k in range(2):
        assert np.array_equal(sheet[:TCs.SIDE, k * TCs.SIDE:(k + 1) * TCs.SIDE], real[k]), k
    assert not np.array_equal(sheet[:TCs.SIDE], sheet[TCs.SIDE:])


def test_missing_clip_names_the_key(psg, world, tmp_path):
    with pytest.raises(psg.PsgError, match="mi355x.clip_path"):
        psg.FinalTrainer(TCs.config(tmp_path), "-", "-", "none", components={"generator": TCs.generator(psg, world)})
