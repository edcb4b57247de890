"""-m gpu: stage 3 on the MI355X kernels - the text encoder trained through the frozen VAE decoder (final_trainer.py:215-236,
:425-485).  The decoder's data gradients against the reference VAEDecoder's own backward (tests/golden/final_grad.npz,
tools/make_golden_final.py), the untouched inference path, frozen-means-frozen, and three optimisation steps end to end with
step one checked against a CPU run of the same chain (tests.final_cases.bert_encode + oracle.vae_oracle)."""
import ctypes as C

import pytest
import torch

from oracle import hashgen, vae_oracle as V
from oracle.make_golden_vae import SEED_W, vae_inputs
from tests import final_cases as FC
from tests import text_cases as TC
from tests import text_grad_cases as GC
from tests.util import maxrel, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ("conv_fwd", "conv_dgrad", "wgrad", "attn", "gn")           # psg_common.h ProfKind
# Profiled launches (convolution, GroupNorm, attention) of one no_grad VAEDecoder.forward on the parent commit, counted from
# its forward: latent_proj 1; per block two ResNetBlocks (2 convs each, + the 1x1 shortcut where the width changes: blocks
# 2-5) and the attention block's q / k / v / proj = 8 convs in block 1, 9 in blocks 2-5; final conv 1 -> 46 convolutions;
# 5 GroupNorms per block + the final one -> 26; 5 attention cores.
PARENT_DECODE_LAUNCHES = {"conv_fwd": 46, "conv_dgrad": 0, "wgrad": 0, "attn": 5, "gn": 26}


@pytest.fixture(scope="module")
def psg():
    import pokemon_sprite_generator_amd as m
    from pokemon_sprite_generator_amd import _lib
    _lib.init(0)
    return m


def _profiled(fn):
    """({kind: launches}, {kind: ms}) of the profiled kernel families over fn()."""
    from pokemon_sprite_generator_amd import _lib
    lib = _lib.init(0)
    _lib.check(lib.psg_profile_begin(), "psg_profile_begin")
    fn()
    torch.cuda.synchronize()
    n = len(KINDS)
    ms, work, cnt = (C.c_double * n)(), (C.c_double * n)(), (C.c_int64 * n)()
    _lib.check(lib.psg_profile_end(ms, work, cnt, n), "psg_profile_end")
    return {k: int(cnt[i]) for i, k in enumerate(KINDS)}, {k: float(ms[i]) for i, k in enumerate(KINDS)}


def _decoder(psg, dt, state=None):
    dec = psg.VAEDecoder(8, 256, 3, compute_dtype=dt)
    sd = state(dec) if state else FC.decoder_state({k: v.shape for k, v in dec.state_dict().items()})
    dec.load_state_dict(sd)
    for p in dec.parameters():
        p.requires_grad = False
    return dec.to(DEV), sd


def _grads(psg, dec, case):
    from pokemon_sprite_generator_amd import ops
    lat, text, img = (t.to(DEV) for t in FC.inputs(case))
    lat.requires_grad_(True), text.requires_grad_(True)
    recon = dec(lat, text)
    assert recon.requires_grad and recon.dtype == torch.float32 and tuple(recon.shape) == (lat.shape[0], 3, 215, 215)
    total, l1, mse = ops.recon_loss(recon, img)
    total.backward()
    assert all(p.grad is None for p in dec.parameters())
    return torch.stack([total.detach(), l1, mse]), text.grad, lat.grad


@pytest.mark.parametrize("case", sorted(FC.CASES))
def test_decoder_gradients_match_reference_fp32(psg, golden, case):
    """Loss scalars within 1e-4 relative; d loss / d text and d loss / d latent within 1e-3, max-abs over max-abs."""
    g = golden("final_grad.npz")
    dec, _ = _decoder(psg, torch.float32)
    losses, dtext, dlat = _grads(psg, dec, case)
    ref = torch.from_numpy(g[f"{case}_loss"])
    e_loss = float(((losses.cpu() - ref).abs() / ref.abs()).max())
    e_t, e_l = maxrel(dtext, torch.from_numpy(g[f"{case}_dtext"])), maxrel(dlat, torch.from_numpy(g[f"{case}_dlatent"]))
    print(f"case {case} fp32: loss rel {e_loss:.2e}, dtext {e_t:.2e}, dlatent {e_l:.2e}")
    assert e_loss < 1e-4, (losses.tolist(), ref.tolist())
    assert e_t < 1e-3 and e_l < 1e-3, (e_t, e_l)


def test_decoder_text_gradient_bf16(psg, golden):
    """bf16 decoder against the same fp32 fixture: rel-L2 < 4e-2 (the project's bf16 train bar), each sample's norm within 2 %."""
    g = golden("final_grad.npz")
    dec, _ = _decoder(psg, torch.bfloat16)
    _, dtext, _ = _grads(psg, dec, "b2")
    ref = torch.from_numpy(g["b2_dtext"])
    e = rel_l2(dtext, ref)
    norms = [(float(dtext[b].double().norm()), float(ref[b].double().norm())) for b in range(ref.shape[0])]
    print(f"bf16: dtext rel-L2 {e:.3e}; per-sample norms (got, ref) {norms}")
    assert e < 4e-2, e
    for got, want in norms:
        assert abs(got - want) < 0.02 * want, (got, want)


def test_inference_path_is_untouched(psg):
    """Under no_grad the decoder runs the parent's launches (counted) and gives the same bits before and after a differentiable
    call on the same module; with grad mode on but no input requiring grad it runs them too."""
    dec, _ = _decoder(psg, torch.float32, lambda d: hashgen.fill_unet_state({k: tuple(v.shape) for k, v in d.state_dict().items()}, SEED_W + 1, "stress"))
    _, _, lat, text = vae_inputs()
    lat, text = lat.to(DEV), text.to(DEV)
    with torch.no_grad():
        before = dec(lat, text)
        counts, _ = _profiled(lambda: dec(lat, text))
    assert counts == PARENT_DECODE_LAUNCHES, counts
    t = text.clone().requires_grad_(True)
    dec(lat, t).square().mean().backward()
    assert t.grad is not None and float(t.grad.abs().max()) > 0
    with torch.no_grad():
        after = dec(lat, text)
    assert torch.equal(before, after)
    out = dec(lat, text)                                  # grad mode on, nothing requires grad: the inference launches
    assert not out.requires_grad and torch.equal(out, before)
    counts2, _ = _profiled(lambda: dec(lat, text))
    assert counts2 == PARENT_DECODE_LAUNCHES, counts2


def _generator(psg, dt):
    c = GC.CASES["M"]
    te = psg.TextEncoder(bert_config=TC.bert_config(c["layers"]), hidden_dim=c["hidden_dim"], finetune_strategy=c["strategy"], compute_dtype=dt,
                         trainable=True)
    te.load_state_dict(GC.state_dict(te), strict=True)
    enc, dec = psg.VAEEncoder(3, 8, compute_dtype=dt), psg.VAEDecoder(8, 256, 3, compute_dtype=dt)
    esd = hashgen.fill_unet_state({k: tuple(v.shape) for k, v in enc.state_dict().items()}, 11, "stress")
    dsd = FC.decoder_state({k: v.shape for k, v in dec.state_dict().items()})
    enc.load_state_dict(esd), dec.load_state_dict(dsd)
    gen = psg.FinalPokemonGenerator(enc, dec, None, te).to(DEV)
    eps = (hashgen.uniform((2, 8, 27, 27), FC.SEED_IN, hashgen.name_id("final.e2e.eps")) * 3.0 ** 0.5).to(DEV)
    raw = gen.vae_encoder.forward
    gen.vae_encoder.forward = lambda x: raw(x, eps=eps)            # the reparameterisation draw, fixed for the comparison
    return gen, dsd


def test_three_train_steps_end_to_end(psg, golden):
    g = golden("text_encoder_grad.npz")
    ids, mask = torch.from_numpy(g["M_input_ids"])[:2], torch.from_numpy(g["M_attention_mask"])[:2]
    tt = torch.from_numpy(g["M_token_type_ids"])[:2]
    images = FC.inputs("b2")[2].to(DEV)
    gen, dsd = _generator(psg, torch.float32)
    te = gen.text_encoder
    st = psg.FinalStepper(gen, lr=1e-3)
    assert sorted(id(p) for p in st.params) == sorted(id(p) for p in te.parameters() if p.requires_grad)
    before = {n: p.detach().clone() for n, p in gen.named_parameters()}
    sd0 = {k: v.detach().cpu().clone() for k, v in te.state_dict().items()}
    latent = gen.vae_encoder(images)[0].cpu()

    # the text encoder's own weight-gradient launches: the same encoder alone, forward + backward
    def alone():
        y = te.encode_ids(ids, mask)
        y.square().mean().backward()
    te_counts, _ = _profiled(alone)
    for p in te.parameters():
        p.grad = None
    assert te_counts["wgrad"] > 0

    res = {}
    counts, _ = _profiled(lambda: res.update(st.train_step(images, ids, mask)))
    assert set(res) == {"loss", "l1_loss", "mse_loss", "grad_norm"} and all(v.is_cuda and v.numel() == 1 for v in res.values())
    assert counts["wgrad"] == te_counts["wgrad"], (counts, te_counts)          # no VAE weight gradient was launched
    proj_grad = te.projection.weight.grad.detach().cpu().clone()
    gn1 = float(res["grad_norm"])
    outs = [res]
    for _ in range(2):
        outs.append(st.train_step(images, ids, mask))
    for r in outs:
        assert all(bool(torch.isfinite(v)) for v in r.values()), r
    for n, p in gen.named_parameters():
        same = torch.equal(p.detach(), before[n])
        if n.startswith("text_encoder.") and p.requires_grad and not n.startswith("text_encoder.bert.pooler."):
            assert not same, n
        else:
            assert same, n
        if not n.startswith("text_encoder."):
            assert p.grad is None and not p.requires_grad, n

    # step one on the CPU: BERT restatement -> oracle decoder (the GPU encoder's latent) -> L1 + 0.1 MSE -> backward
    torch.set_num_threads(8)
    train = set(GC.trainable_names(te))
    sd = {k: v.clone().requires_grad_(k in train) for k, v in sd0.items()}
    emb = FC.bert_encode(sd, te.bert.config, ids, mask, tt, 256)
    total, l1, mse = FC.recon_loss(V.vae_decode(dsd, latent, emb), images.cpu())
    total.backward()
    ref = sd["projection.weight"].grad * min(1.0, 1.0 / (gn1 + 1e-6))          # clip_grad_norm_(1.0), as the step applied it
    total, l1, mse = total.detach(), l1.detach(), mse.detach()
    e_loss = abs(float(outs[0]["loss"]) - float(total)) / float(total)
    e_g = maxrel(proj_grad, ref)
    print(f"step 1: loss {float(outs[0]['loss']):.6f} (CPU {float(total):.6f}, rel {e_loss:.2e}); grad_norm {gn1:.4e}; "
          f"projection.weight.grad max-abs/max-abs {e_g:.2e}; losses {[float(r['loss']) for r in outs]}")
    assert e_loss < 1e-3, e_loss
    assert abs(float(outs[0]["l1_loss"]) - float(l1)) < 1e-3 * float(l1) and abs(float(outs[0]["mse_loss"]) - float(mse)) < 1e-3 * float(mse)
    assert e_g < 1e-3, e_g
    val = st.validate_step(images, ids, mask)
    assert set(val) == {"loss", "l1_loss", "mse_loss"} and bool(torch.isfinite(val["loss"])) and not val["loss"].requires_grad


def test_joint_phase_is_not_built(psg):
    gen, _ = _generator(psg, torch.float32)
    with pytest.raises(psg.PsgError, match="joint phase not built"):
        gen.unfreeze_vae_decoder()
    lat, text, _ = (t.to(DEV) for t in FC.inputs("s20"))
    text.requires_grad_(True)
    gen.vae_decoder.block3_attn.k.weight.requires_grad = True
    with pytest.raises(psg.PsgError, match="requires_grad"):
        gen.vae_decoder(lat, text)
    with torch.no_grad():                                 # the inference path does not care
        assert gen.vae_decoder(lat, text).shape == (1, 3, 215, 215)
