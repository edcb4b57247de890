"""-m gpu: stage 2 with the resident token table.  `ImprovedDiffusionTrainer` builds this package's loader with its text
encoder's tokenizer (`mi355x.gpu_data`, this package's TextEncoder, one process), the batches carry input_ids / attention_mask,
and `_encode` on them returns the embeddings of the string path, torch.equal: the ids and the padded length are the
tokenizer's.  The trainer is built from a stage-1 checkpoint written by `VAETrainer.save_checkpoint`, which must load as it is.
The U-Net is replaced by a small stand-in (`_encode` never calls it; building the real one takes longer than the test)."""
import pytest
import torch

from tests import trainer_cases as TCs

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def psg():
    import pokemon_sprite_generator_amd as m
    from pokemon_sprite_generator_amd import _lib
    _lib.init(0)
    yield m
    m.ops.GradSink.unregister_all()
    m.ops.WeightCache.clear()


def test_encode_from_the_table_equals_the_string_path(psg, tmp_path, monkeypatch):
    from pokemon_sprite_generator_amd import trainer as trainer_mod
    monkeypatch.setattr(trainer_mod, "UNet", lambda **kw: TCs.small_unet(psg))
    world = TCs.world(psg)
    vae, te, crit = TCs.vae_parts(psg, world)
    stage1 = psg.VAETrainer(TCs.config(tmp_path), "stage1", components={"vae": vae, "text_encoder": te, "criterion": crit},
                            compute_dtype=torch.float32)
    stage1.save_checkpoint(0, is_best=True)
    path = stage1.checkpoint_dir / "vae_best_model.pth"
    stage1.stepper.arena.release(), stage1.stepper.params.release()

    cfg = TCs.config(tmp_path, diffusion_epochs=1)
    cfg["mi355x"] = {"gpu_data": True, "dtype": "bf16"}
    cfg["optimization"].update(max_grad_norm=1.0, scheduler="constant")
    tok = TCs.bert_tokenizer()
    comps = {"TextEncoder": lambda model_name, hidden_dim: psg.TextEncoder(bert_config=TCs.bert_config(), hidden_dim=hidden_dim, tokenizer=tok)}
    tr = psg.ImprovedDiffusionTrainer(cfg, str(path), "stage2", components=comps)
    # the stage-1 checkpoint loaded as it is: the frozen text encoder and both halves of the VAE hold its tensors
    for k, v in tr.text_encoder.state_dict().items():
        assert torch.equal(v.cpu(), world["te"][k]), k
    for k, v in tr.vae_encoder.state_dict().items():
        assert torch.equal(v.cpu(), world["vae"]["encoder." + k]), k
    for k, v in tr.vae_decoder.state_dict().items():
        assert torch.equal(v.cpu(), world["vae"]["decoder." + k]), k
    assert tr.data_loaders["train"].tokens is not None and tr.data_loaders["val"].tokens is tr.data_loaders["train"].tokens
    batch = next(iter(tr.data_loaders["val"]))
    assert {"input_ids", "attention_mask", "index"} <= set(batch)
    want = tok(batch["full_description"], return_tensors="pt", padding=True, truncation=True, max_length=256)
    assert torch.equal(batch["input_ids"].cpu(), want["input_ids"])
    calls = []
    encode_ids = tr.text_encoder.encode_ids
    tr.text_encoder.encode_ids = lambda ids, mask, tt=None: calls.append(tuple(ids.shape)) or encode_ids(ids, mask, tt)
    tokenize = tr.text_encoder.tokenize
    tr.text_encoder.tokenize = lambda texts: calls.append("tokenizer") or tokenize(texts)
    torch.manual_seed(3)
    latent, emb, flag = tr._encode(batch)
    assert calls == [tuple(want["input_ids"].shape)]                      # no tokenizer call on the table's path
    strings = {k: v for k, v in batch.items() if k not in ("input_ids", "attention_mask", "index")}
    torch.manual_seed(3)
    latent_s, emb_s, flag_s = tr._encode(strings)
    assert calls[1] == "tokenizer"
    assert tuple(emb.shape) == (2, want["input_ids"].shape[1], 256) and torch.equal(emb, emb_s)
    assert torch.equal(latent, latent_s) and int(flag) == int(flag_s) == 0
    tr.stepper.close()
