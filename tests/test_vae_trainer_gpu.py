"""-m gpu: VAETrainer - stage 1's epochs, validation, best-model checkpoint, resume and sample sheet around VAEStepper -
against a twin that drives a second VAEStepper, built from the same state dicts, over a second identical loader by hand.

Setup (tests/trainer_cases.py): the 8 fixture sprites split 5 / 2 / 1, batch 2, 2 epochs (2 train batches each, one validation
batch); PokemonVAE with hashgen "stress" weights, a 2-layer BERT without dropout, tests/vgg_ref.py's VGG16, everything fp32 and
injected through `components`; `torch.manual_seed` in front of each run (the reparameterisation noise comes from torch's
default generator; the shuffle and the augmentations from the loader's own, seeded by the epoch).

The trainer and the twin launch the same deterministic kernels on the same inputs: the epoch means, both validation dicts
and every parameter afterwards are compared with torch.equal / ==, not with a tolerance."""
import pytest
import torch

from tests import trainer_cases as TCs

pytestmark = pytest.mark.gpu
DEV = "cuda"
TRAIN_KEYS = ("total_loss", "reconstruction_loss", "kl_loss")
CKPT_KEYS = {"epoch", "vae_state_dict", "text_encoder_state_dict", "optimizer_state_dict", "scheduler_state_dict", "config",
             "global_step", "best_val_loss"}            # vae_trainer.py:517-526


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


def _trainer(psg, world, tmp, name):
    vae, te, crit = TCs.vae_parts(psg, world)
    return psg.VAETrainer(TCs.config(tmp), name, components={"vae": vae, "text_encoder": te, "criterion": crit},
                          compute_dtype=torch.float32)


def _params(st):
    out = {"vae." + n: p.detach().clone() for n, p in st.vae.named_parameters()}
    out.update({"text." + n: p.detach().clone() for n, p in st.text_encoder.named_parameters()})
    return out


def _by_hand(st, loaders, epochs):
    """What VAETrainer.train() does to a stepper, written out: [(train means, validation means, kl weights of the epoch)]."""
    out = []
    for epoch in epochs:
        st.epoch = epoch
        st.vae.train(), st.text_encoder.train()
        loaders["train"].set_epoch(epoch)
        rows = [st.train_step(b["image"], b["input_ids"], b["attention_mask"]) for b in loaders["train"]]
        assert len(rows) == TCs.TRAIN_BATCHES
        train = TCs.mean_of(rows, TRAIN_KEYS, len(rows))
        st.vae.eval(), st.text_encoder.eval()
        vrows = [st.validate_step(b["image"], b["input_ids"], b["attention_mask"]) for b in loaders["val"]]
        val = TCs.mean_of(vrows, TRAIN_KEYS, len(vrows))
        st.end_epoch()
        out.append((train, val, [r["kl_weight"] for r in rows + vrows]))
    return out


@pytest.fixture(scope="module")
def runs(psg, world, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("stage1")
    tr = _trainer(psg, world, tmp, "own")
    assert tr.current_epoch == 0 and tr.global_step == 0 and tr.best_val_loss == float("inf")
    assert set(next(iter(tr.data_loaders["val"]))) >= {"input_ids", "attention_mask", "index"}     # the loader got the tokenizer
    start = _params(tr.stepper)
    log = TCs.record(tr)
    torch.manual_seed(TCs.SEED)
    tr.train()
    own_params = _params(tr.stepper)
    # the twin: a second stepper from the same state dicts, a second loader, the loop by hand
    vae, te, crit = TCs.vae_parts(psg, world)
    twin = psg.VAEStepper(vae, te, crit, config=TCs.config(tmp))
    assert all(torch.equal(a, b) for a, b in zip(start.values(), _params(twin).values()))
    torch.manual_seed(TCs.SEED)
    hand = _by_hand(twin, TCs.loaders(psg), range(2))
    torch.cuda.synchronize()
    return {"tmp": tmp, "trainer": tr, "log": log, "start": start, "own_params": own_params, "twin": twin, "hand": hand,
            "twin_params": _params(twin)}


def test_train_equals_the_hand_driven_twin_bit_for_bit(psg, runs):
    log, hand, tr = runs["log"], runs["hand"], runs["trainer"]
    assert [(k, e) for k, e, _ in log] == [("train", 0), ("val", 0), ("train", 1), ("val", 1)]
    for epoch in range(2):
        tm, vm = log[2 * epoch][2], log[2 * epoch + 1][2]
        assert set(tm) == {"loss", "recon_loss", "kl_loss", "epoch_time", "avg_batch_time"} and set(vm) == {"loss", "recon_loss", "kl_loss"}
        got_t, got_v = [tm[k] for k in ("loss", "recon_loss", "kl_loss")], [vm[k] for k in ("loss", "recon_loss", "kl_loss")]
        print(f"epoch {epoch}: train {got_t} twin {hand[epoch][0]}; val {got_v} twin {hand[epoch][1]}")
        assert got_t == hand[epoch][0] and got_v == hand[epoch][1], epoch
        assert all(v > 0 for v in got_t[:2] + got_v[:2])
        assert tm["epoch_time"] > 0 and tm["avg_batch_time"] == tm["epoch_time"] / TCs.TRAIN_BATCHES
    assert log[0][2]["loss"] != log[2][2]["loss"]
    moved = 0
    for n, p in runs["own_params"].items():
        assert torch.equal(p, runs["twin_params"][n]), n
        moved += not torch.equal(p, runs["start"][n])
    assert moved > 200                                                    # (214 VAE parameters and the text encoder's last layers)
    assert tr.current_epoch == 2 and tr.global_step == 4 == runs["twin"].global_step
    assert tr.stepper.learning_rates() == runs["twin"].learning_rates()   # both schedulers took two epoch steps
    assert (tr.log_dir / "vae_training.log").exists()


def test_kl_weight_follows_the_annealing(psg, runs):
    """kl_anneal_start 0, kl_anneal_end 2, weights 0 -> 1e-4: epoch 0 trains and validates at 0, epoch 1 at 5e-5."""
    weights = [w for _, _, ws in runs["hand"] for w in ws]
    assert weights == pytest.approx([0.0] * 3 + [5e-5] * 3, rel=1e-12, abs=0.0)
    tr = runs["trainer"]
    assert [tr.get_kl_weight(e) for e in range(4)] == pytest.approx([0.0, 5e-5, 1e-4, 1e-4], rel=1e-12, abs=0.0)
    # the reported total of epoch 1 holds the annealed weight: total - (recon + 0.1 * perceptual) = 5e-5 * kl is not checked
    # through the means (the perceptual part is not reported); the stepper's own test does that per step.  Here: the trainer
    # ran epoch 1 at the stepper's epoch 1 - its means equal the twin's, which asserted the weights above.
    assert runs["log"][2][2]["kl_loss"] == runs["hand"][1][0][2]


def test_checkpoint_keys_resume_and_stage3_loading(psg, world, runs, monkeypatch):
    tr, tmp = runs["trainer"], runs["tmp"]
    path = tr.checkpoint_dir / "vae_best_model.pth"
    assert path.exists() and sorted(p.name for p in tr.checkpoint_dir.iterdir()) == ["vae_best_model.pth"]
    ck = torch.load(path, map_location="cpu")
    assert set(ck) == CKPT_KEYS
    vals = [runs["log"][1][2]["loss"], runs["log"][3][2]["loss"]]
    print(f"validation losses {vals}, checkpoint of epoch {ck['epoch']}")
    assert ck["best_val_loss"] == min(vals) == tr.best_val_loss
    assert ck["epoch"] == vals.index(min(vals)) == 1 and ck["global_step"] == 4
    assert ck["config"] == tr.config and [g["name"] for g in ck["optimizer_state_dict"]["param_groups"]] == ["vae", "text_encoder"]
    for n, p in runs["own_params"].items():
        part, key = n.split(".", 1)
        assert torch.equal(ck["vae_state_dict" if part == "vae" else "text_encoder_state_dict"][key], p.cpu()), n
    # resume: a fresh trainer from the original weights takes the checkpoint and runs the epoch the reference would re-run
    again = _trainer(psg, world, tmp, "again")
    again.load_checkpoint(str(path))
    assert again.current_epoch == 1 and again.global_step == 4 and again.best_val_loss == ck["best_val_loss"]
    assert again.stepper.optimizer.steps_done() == 4 and again.stepper.learning_rates() == tr.stepper.learning_rates()
    results = []
    for t in (tr, again):                              # the uninterrupted trainer goes on from its own state, the resumed from the file
        torch.manual_seed(TCs.SEED + 1)
        tm, vm = t.train_epoch(1), t.validate_epoch(1)
        results.append(([tm[k] for k in ("loss", "recon_loss", "kl_loss")], vm, _params(t.stepper)))
    assert results[0][0] == results[1][0] and results[0][1] == results[1][1]
    assert all(torch.equal(results[0][2][n], results[1][2][n]) for n in results[0][2])
    assert again.global_step == 6 == tr.global_step
    assert any(not torch.equal(results[0][2][n], runs["own_params"][n]) for n in results[0][2])
    # stage 3 reads the file: FinalPokemonGenerator.from_checkpoints, its U-Net replaced by a small stand-in
    from pokemon_sprite_generator_amd import final
    unet = TCs.small_unet(psg)
    torch.save({"unet_state_dict": unet.state_dict()}, tmp / "diffusion.pth")
    monkeypatch.setattr(final, "UNet", lambda **kw: TCs.small_unet(psg))
    gen = psg.FinalPokemonGenerator.from_checkpoints(str(path), str(tmp / "diffusion.pth"), tr.config["model"], trainable_decoder=True,
                                                     bert_config=TCs.bert_config(), finetune_strategy="minimal")
    got = dict(gen.state_dict())
    for k, v in ck["vae_state_dict"].items():
        assert k.startswith(("encoder.", "decoder."))
        assert torch.equal(got["vae_" + k].cpu(), v), k                      # encoder.x -> vae_encoder.x, decoder.x -> vae_decoder.x
    for k, v in ck["text_encoder_state_dict"].items():
        assert torch.equal(got["text_encoder." + k], v), k
    again.stepper.arena.release(), again.stepper.params.release()


def test_sample_sheet(psg, runs):
    from PIL import Image
    import numpy as np
    tr = runs["trainer"]
    assert sorted(p.name for p in tr.sample_dir.iterdir()) == ["vae_epoch_0000.png", "vae_epoch_0001.png"]
    sheet = np.asarray(Image.open(tr.sample_dir / "vae_epoch_0000.png"))
    batch = next(iter(tr.data_loaders["val"]))
    n = batch["image"].shape[0]
    assert n == 2 and sheet.shape == (3 * TCs.SIDE, n * TCs.SIDE, 3) and sheet.dtype == np.uint8
    real = psg.imaging.to_uint8(batch["image"]).cpu().numpy()              # [n, H, W, 3]
    for k in range(n):
        assert np.array_equal(sheet[:TCs.SIDE, k * TCs.SIDE:(k + 1) * TCs.SIDE], real[k]), k
    rows = [sheet[r * TCs.SIDE:(r + 1) * TCs.SIDE] for r in range(3)]
    assert not np.array_equal(rows[0], rows[1]) and not np.array_equal(rows[1], rows[2])


def test_missing_vgg_weights_name_the_key(psg, world, tmp_path):
    vae, te, _ = TCs.vae_parts(psg, world)
    with pytest.raises(psg.PsgError, match="mi355x.vgg_state_dict"):
        psg.VAETrainer(TCs.config(tmp_path), "none", components={"vae": vae, "text_encoder": te})
