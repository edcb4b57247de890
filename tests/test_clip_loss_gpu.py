"""-m gpu: `psg.CLIPLoss` end to end against the float64 restatement of tests/clip_ref.py - a tiny configuration, the real
ViT-B/32 widths with one layer per tower (every launch shape of the full model once), the state-dict round trip, and the hook:
FinalStepper.train_step(..., clip_loss=clip, texts=ids).  Bounds: `clip_ref.bar` (four times torch's CPU error in the same
precision on the same case, floored at 1e-6)."""
import pytest
import torch

from tests import clip_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def psg():
    import pokemon_sprite_generator_amd as m
    from pokemon_sprite_generator_amd import _lib
    _lib.init(0)
    return m


def _clip(psg, name, dt, sd=None):
    sd = {"model." + k: v for k, v in (sd or R.state_dict(name)).items()}
    return psg.CLIPLoss(R.CONFIGS[name], state_dict=sd, compute_dtype=dt, device=DEV)


@pytest.mark.parametrize("prec", list(R.PRECISIONS))
@pytest.mark.parametrize("case", list(R.LOSS_CASES))
def test_loss_and_image_gradient(psg, case, prec):
    name, B, H, S = R.LOSS_CASES[case]
    clip = _clip(psg, name, R.PRECISIONS[prec], R.loss_state_dict(case))      # (text_projection rebuilt: cosines away from 0)
    img, ids = R.loss_inputs(case)
    img = img.to(DEV).requires_grad_(True)
    out = clip(img, ids.to(DEV))
    assert out.dtype == torch.float32 and out.dim() == 0 and out.requires_grad
    out.backward()
    assert all(p.grad is None for p in clip.parameters())
    errs = R.errors(dict(loss=out.detach(), grad=img.grad), ("loss", case))
    key = ("loss", case, prec)
    print(f"{key}: loss {float(out.detach()):.6f}, " + ", ".join(f"{n} {e:.3e} (bar {R.bar(key, n):.3e})" for n, e in errs.items()))
    for n, e in errs.items():
        assert e <= R.bar(key, n), f"{key} {n}: {e:.3e} > {R.bar(key, n):.3e}"
    # no gradient asked: the same value under no_grad, nothing recorded; the cached text side gives it again
    val = clip(img.detach(), ids)                                      # (ids on the host are moved)
    assert not val.requires_grad and torch.equal(val, out.detach())
    te = clip.text_features(ids.to(DEV))
    assert not te.requires_grad and tuple(te.shape) == (B, R.CONFIGS[name]["projection_dim"])
    assert torch.equal(clip.forward_features(img.detach(), te), out.detach())


def test_second_eos_rule(psg):
    """eos_token_id != 2: the pooled row is the first position that holds it."""
    clip = _clip(psg, "eos", torch.float32)
    ids = R.token_ids("eos", 2, 8)
    got = clip.text_features(ids.to(DEV))
    ref = R.text(ids, R.state_dict("eos"), R.CONFIGS["eos"])
    assert R.rel(got, ref) < 1e-5
    wrong = R.text(ids, R.state_dict("eos"), dict(R.CONFIGS["eos"], text_config=dict(R.CONFIGS["eos"]["text_config"], eos_token_id=2)))
    assert R.rel(wrong, ref) > 1e-2


def test_state_dict_round_trip(psg):
    a = _clip(psg, "tiny", torch.float32)
    sd = a.state_dict()
    assert set(sd) == {"model." + k for k in R.state_shapes(R.CONFIGS["tiny"])}
    b = psg.CLIPLoss(R.CONFIGS["tiny"], compute_dtype=torch.float32).to(DEV)
    b.load_state_dict({k: v.cpu() for k, v in sd.items()})
    name, B, H, S = R.LOSS_CASES["tiny"]
    img, ids = R.image("tiny", B, H).to(DEV), R.token_ids(name, B, S).to(DEV)
    assert torch.equal(a(img, ids), b(img, ids))
    with pytest.raises(psg.PsgError):
        a(img.cpu(), ids)
    with pytest.raises(psg.PsgError, match="tokenizer"):
        a(img, ["a green creature"] * B)
    with pytest.raises(psg.PsgError):
        a(torch.zeros(B, 3, 80, 80, device=DEV), ids)                  # larger than the model's 64: not built


def test_final_stepper_takes_the_loss(psg, golden):
    """The hook of final.py: train_step(images, ids, mask, clip_loss=clip, clip_weight=w, texts=clip_ids) - the returned loss is
    the reconstruction loss plus w times the separately computed CLIP loss of the same reconstruction, and the text encoder's
    gradients differ from the step without it."""
    from pokemon_sprite_generator_amd import ops
    from tests import final_cases as FC
    from tests.test_final_gpu import _generator
    g = golden("text_encoder_grad.npz")
    ids, mask = torch.from_numpy(g["M_input_ids"])[:2].to(DEV), torch.from_numpy(g["M_attention_mask"])[:2].to(DEV)
    images = FC.inputs("b2")[2].to(DEV)
    gen, _ = _generator(psg, torch.float32)
    gen.eval()                                                          # no dropout: the reconstruction is the same every call
    te = gen.text_encoder
    clip = _clip(psg, "hook", torch.float32)
    clip_ids = R.token_ids("hook", 2, 8).to(DEV)
    w = 0.7
    with torch.no_grad():
        recon = gen.encode_and_decode_ids(images, ids, mask)
        rec_total = ops.recon_loss(recon, images)[0]
        clip_alone = clip(recon, clip_ids)
    assert -1.0 <= float(clip_alone) <= 1.0 and float(clip_alone) != 0.0

    st = psg.FinalStepper(gen, lr=0.0)                                  # lr = 0: the parameters stay, the steps are comparable

    def step(**kw):
        out = st.train_step(images, ids, mask, **kw)
        return out, {n: p.grad.detach().clone() for n, p in te.named_parameters() if p.grad is not None}
    plain, g_plain = step()
    both, g_both = step(clip_loss=clip, clip_weight=w, texts=clip_ids)
    # (the no_grad reconstruction runs the decoder's inference launches: the same arithmetic, not promised to be the same bits)
    assert abs(float(plain["loss"]) - float(rec_total)) <= 1e-5 * float(rec_total)
    want = float(plain["loss"]) + w * float(clip_alone)
    assert abs(float(both["loss"]) - want) <= 1e-5 * abs(want), (float(both["loss"]), want)
    assert torch.equal(both["l1_loss"], plain["l1_loss"]) and torch.equal(both["mse_loss"], plain["mse_loss"])
    assert g_plain and set(g_both) == set(g_plain)
    assert all(bool(torch.isfinite(v).all()) for v in g_both.values())
    assert any(not torch.equal(g_both[n], g_plain[n]) for n in g_plain)
    assert all(p.grad is None for p in clip.parameters())
    val = st.validate_step(images, ids, mask, clip_loss=clip, clip_weight=w, texts=clip_ids)
    assert not val["loss"].requires_grad and abs(float(val["loss"]) - float(both["loss"])) <= 1e-5 * abs(float(both["loss"]))
