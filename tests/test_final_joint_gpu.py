"""-m gpu: stage 3's joint phase (final_trainer.py:590-642) - FinalStepper with the text encoder and the VAE decoder under ONE
clip norm and their own learning rates, update="grouped" (one arena, one norm pass, one clip + AdamW launch:
psg_adamw_groups_sets_f32) against its own twin, update="torch" (torch.optim.AdamW, one clip_grad_norm_ over everything
stepped), and step 1 against a CPU run of the same chain.

Setup (the world of tests/test_vae_stepper_gpu.py): VAEEncoder and VAEDecoder(8, 256, trainable=True) with that file's hashgen
"stress" weights, a 2-layer TextEncoder(hidden_dim=256, trainable=True, finetune_strategy="minimal") with
tests/text_grad_cases.py's weights and no dropout; batch 1, one 215 x 215 image, 20 tokens (13 real), the encoder's eps fixed,
fp32.  lr 1e-4 (text encoder), 1e-5 (decoder, the 0.1 x default), weight decay 0.01, cosine schedule over 5 epochs, max norm
0.02 (the clip is active in every joint step).

Both steppers take one text-encoder-phase step and end the epoch; the twin takes the grouped stepper's weights, both switch and
take three joint steps.  Step 1: losses and the three
norms at relative 1e-5, every stepped parameter at max-rel < 2e-6 - except the two decoder biases of
tests.vae_decoder_ref.ZERO_GRAD, whose exact gradient is zero: |delta p| <= 1.01 * lr * (1 + weight_decay * |p|).  Steps 2 and
3: the worst per-parameter max-rel, bounded at 4 x the figure measured on MI355X, no tighter than 2e-6 (DESIGN §21's
convention for optimizer feedback).

Measured on MI355X.  Joint step 1: losses and norms equal to the 7 digits printed, worst per-parameter max-rel 1.1e-7
(text_encoder.bert.encoder.layer.0.output.LayerNorm.weight).  Step 2: 5.3e-7, step 3: 6.9e-7 (text_encoder.projection.weight both
times); the three norms of the two runs still agree to the 7 digits printed.  Step 1 against the CPU chain: the three norms to
5e-7, the applied gradients (exp_avg / 0.1) of projection.weight, block3_resnet1.conv1.weight and block2_attn.k.weight to
2.1e-6 / 2.1e-6 / 1.2e-6 with the shared coefficient 0.5; the groups' own coefficients would have been 1.0 (text: 2 x the shared
one) and 0.514 (decoder: 1.029 x).  bf16 joint step: grad_norm 1.3e-3, grad_norm_text 2.0e-3, grad_norm_decoder 1.3e-3 from the
fp32 run's.
"""
import ctypes as C

import pytest
import torch

from oracle import hashgen, vae_oracle as V
from tests import final_cases as FC, text_cases as TC, text_grad_cases as TG, vae_decoder_ref as R
from tests.util import h, maxrel

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, WD = 1e-4, 0.01
DLR = LR * 0.1
MAX_NORM = 0.02                        # below the joint steps' gradient norms (0.038, 0.026, 0.023 measured): the clip is active
BAR = 2e-6
LOSS_BAR = 1e-5
CPU_BAR = 1e-3                         # tests/test_final_gpu.py::test_three_train_steps_end_to_end's
STEP23_MEASURED = 6.91e-7               # worst per-parameter max-rel against the twin after joint steps 2 and 3 (MI355X)
BF16_NORMS_MEASURED = (1.31e-3, 2.01e-3, 1.29e-3)  # |norm_bf16 / norm_fp32 - 1| of grad_norm, grad_norm_text, grad_norm_decoder (MI355X)
BF16_NORM_BAR = 5e-2                   # tests/test_vae_stepper_gpu.py's
ZERO = {"vae_decoder." + n for n in R.ZERO_GRAD}
SEED = 77
S, S_REAL = 20, 13
NORMS = ("grad_norm", "grad_norm_text", "grad_norm_decoder")
KINDS = ("conv_fwd", "conv_dgrad", "wgrad", "attn", "gn")           # psg_common.h ProfKind


@pytest.fixture(scope="module")
def psg():
    import pokemon_sprite_generator_amd as m
    from pokemon_sprite_generator_amd import _lib
    _lib.init(0)
    yield m
    m.ops.GradSink.unregister_all()
    m.ops.WeightCache.clear()


def _bert_config():
    return dict(TC.bert_config(2), hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)


def _wgrad_launches(fn):
    """Weight-gradient launches over fn(), as tests/test_final_gpu.py counts them."""
    from pokemon_sprite_generator_amd import _lib
    lib = _lib.init(0)
    _lib.check(lib.psg_profile_begin(), "psg_profile_begin")
    fn()
    torch.cuda.synchronize()
    n = len(KINDS)
    ms, work, cnt = (C.c_double * n)(), (C.c_double * n)(), (C.c_int64 * n)()
    _lib.check(lib.psg_profile_end(ms, work, cnt, n), "psg_profile_end")
    return int(cnt[KINDS.index("wgrad")])


@pytest.fixture(scope="module")
def world(psg):
    """The state dicts and the batch, made once and left unchanged."""
    vae = psg.PokemonVAE(8, 256, trainable=True)
    vae_sd = hashgen.fill_unet_state({k: tuple(v.shape) for k, v in vae.state_dict().items()}, SEED, "stress")
    te = psg.TextEncoder(bert_config=_bert_config(), hidden_dim=256, trainable=True, finetune_strategy="minimal")
    ids = hashgen.randint((1, S), SEED, hashgen.name_id("vaestep.ids"), 0, _bert_config()["vocab_size"])
    mask = torch.zeros(1, S, dtype=torch.int64)
    mask[:, :S_REAL] = 1
    batch = (h((1, 3, 215, 215), "vaestep.img", 1.0).to(DEV), ids.to(DEV), mask.to(DEV))
    return {"enc": {k[8:]: v for k, v in vae_sd.items() if k.startswith("encoder.")},
            "dec": {k[8:]: v for k, v in vae_sd.items() if k.startswith("decoder.")}, "te": TG.state_dict(te),
            "cfg": te.bert.config, "batch": batch, "eps": h((1, 8, 27, 27), "vaestep.eps", 1.0).to(DEV)}


def _generator(psg, world, dtype=torch.float32, trainable=True, unet=None, model_state=None):
    te = psg.TextEncoder(bert_config=_bert_config(), hidden_dim=256, compute_dtype=dtype, trainable=True, finetune_strategy="minimal")
    enc, dec = psg.VAEEncoder(3, 8, compute_dtype=dtype), psg.VAEDecoder(8, 256, 3, compute_dtype=dtype, trainable=trainable)
    te.load_state_dict(world["te"]), enc.load_state_dict(world["enc"]), dec.load_state_dict(world["dec"])
    gen = psg.FinalPokemonGenerator(enc, dec, unet, te).to(DEV)
    if model_state is not None:
        gen.load_state_dict(model_state)
    raw, eps = gen.vae_encoder.forward, world["eps"]
    gen.vae_encoder.forward = lambda x: raw(x, eps=eps)            # the reparameterisation draw, fixed for the comparison
    return gen


def _stepper(psg, gen, update, **kw):
    kw.setdefault("scheduler", "cosine")
    kw.setdefault("max_grad_norm", MAX_NORM)
    return psg.FinalStepper(gen, lr=LR, weight_decay=WD, update=update, final_epochs=5, **kw)


def _params(gen):
    return {n: p.detach().clone() for n, p in gen.named_parameters()}


def _stepped(st):
    ids = {id(p) for p in st.text_params + st.decoder_params}
    return {n for n, p in st.generator.named_parameters() if id(p) in ids}


def _scalars(r):
    return {k: v.detach().clone() for k, v in r.items()}


def _small_unet(psg):
    """Stands in for the U-Net: the generator and the stepper only ever touch its parameters."""
    torch.manual_seed(5)
    return psg.UNetBlock(64, 64, 128, 256, has_attention=True, num_heads=4)


def _release(st):
    if st.arena is not None:
        st.arena.release()
        st.param_arena.release()


@pytest.fixture(scope="module")
def runs(psg, world):
    """One text-encoder-phase step, the end of an epoch, the switch and three joint steps of the grouped stepper and of its
    torch twin; a checkpoint after the third joint step, and a fourth grouped step."""
    batch = world["batch"]
    out = {"steps": []}
    gens = [_generator(psg, world, unet=_small_unet(psg)) for _ in range(2)]
    te = gens[0].text_encoder

    def alone():                                           # the text encoder's own weight-gradient launches
        te.encode_ids(batch[1], batch[2]).square().mean().backward()
    out["te_wgrad"] = _wgrad_launches(alone)
    for p in te.parameters():
        p.grad = None
    own, twin = _stepper(psg, gens[0], "grouped"), _stepper(psg, gens[1], "torch")
    out.update(own=own, twin=twin, start=_params(gens[0]))
    assert all(torch.equal(a, b) for a, b in zip(out["start"].values(), _params(gens[1]).values()))
    res = {}
    out["text_wgrad"] = _wgrad_launches(lambda: res.update(own.train_step(*batch)))
    out["text_step"] = (_scalars(res), _params(gens[0]), {n: p.grad for n, p in gens[0].vae_decoder.named_parameters()})
    twin.train_step(*batch)
    for st in (own, twin):
        st.end_epoch()
    out["lr_before_switch"] = own.learning_rates()
    # the joint phase starts from the same state dicts: the twin takes the grouped stepper's weights (the two text-phase steps
    # differ in their last bits, which would feed back into the joint steps' gradients)
    gens[1].load_state_dict({k: v.detach().clone() for k, v in gens[0].state_dict().items()})
    psg.ops.WeightCache.invalidate()
    gens[1].text_encoder.drop_prepared()
    own.switch_to_joint_training(), twin.switch_to_joint_training()
    assert all(torch.equal(a, b) for a, b in zip(_params(gens[0]).values(), _params(gens[1]).values()))
    out["switched"] = {"params": _params(gens[0]), "steps_done": own.optimizer.steps_done(), "m_any": bool(own.optimizer._m.any()),
                       "v_any": bool(own.optimizer._v.any()), "lrs": own.learning_rates(), "twin_lrs": twin.learning_rates(),
                       "names": [g["name"] for g in own.optimizer.param_groups], "twin_state": len(twin.optimizer.state),
                       "unet": {n: p.detach().clone() for n, p in gens[0].unet.named_parameters()},
                       "unet_requires_grad": all(p.requires_grad for p in gens[0].unet.parameters())}
    out["stepped"] = _stepped(own)
    for _ in range(3):
        ro, rt = own.train_step(*batch), twin.train_step(*batch)
        out["steps"].append((_scalars(ro), _scalars(rt), _params(gens[0]), _params(gens[1])))
    out["validate"] = _scalars(own.validate_step(*batch))
    out["checkpoint"] = own.state_dict()
    out["step4"] = (_scalars(own.train_step(*batch)), _params(gens[0]), own.optimizer._m.clone(), own.optimizer._v.clone())
    torch.cuda.synchronize()
    return out


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def test_trainable_decoder_unfreezes_and_is_a_default_one_until_then(psg, world, runs):
    """Fails without the joint phase.  Before the switch a trainable-but-frozen decoder is a default decoder: the same bits from
    the same text-phase step, no VAE weight-gradient launch, no decoder gradient, no decoder parameter moved."""
    assert callable(psg.FinalStepper.switch_to_joint_training)
    gen = _generator(psg, world)
    assert not gen.vae_decoder.live_weights()
    gen.unfreeze_vae_decoder()
    assert gen.vae_decoder.live_weights() and all(p.requires_grad for p in gen.vae_decoder.parameters())
    # the same text-phase step with a default VAEDecoder loaded from the same state dict
    plain_gen = _generator(psg, world, trainable=False)
    assert not plain_gen.vae_decoder.trainable
    plain = _stepper(psg, plain_gen, "grouped")
    want = _scalars(plain.train_step(*world["batch"]))
    got, params, dec_grads = runs["text_step"]
    assert set(got) == set(want) == {"loss", "l1_loss", "mse_loss", "grad_norm"}
    for k in want:
        assert torch.equal(got[k], want[k]), k
    plain_params = _params(plain_gen)
    moved = 0
    for n, p in plain_params.items():
        assert torch.equal(params[n], p), n
        if n.startswith("text_encoder."):
            moved += not torch.equal(p, runs["start"][n])
        else:
            assert torch.equal(p, runs["start"][n]), n
    assert moved == len(runs["own"].text_params)
    assert runs["text_wgrad"] == runs["te_wgrad"] > 0, (runs["text_wgrad"], runs["te_wgrad"])
    assert len(dec_grads) == 144 and all(g is None for g in dec_grads.values())
    _release(plain)


def test_switch_semantics(psg, runs):
    sw, own = runs["switched"], runs["own"]
    assert sw["steps_done"] == 0 and not sw["m_any"] and not sw["v_any"] and sw["twin_state"] == 0
    assert sw["names"] == ["text_encoder", "vae_decoder"]
    assert runs["lr_before_switch"][0] < LR                                  # the cosine schedule had moved ...
    assert sw["lrs"] == sw["twin_lrs"] == (LR, DLR)                          # ... and restarted at the base learning rates
    for n, p in runs["text_step"][1].items():
        assert torch.equal(p, sw["params"][n]), n                            # re-binding to the new arena moved no value
    assert own.training_phase == "joint" and own.epoch == 1 and own.global_step == 5
    # the U-Net: unfrozen, never reached by a gradient, never moved
    assert sw["unet_requires_grad"] and len(sw["unet"]) > 0
    for st in (runs["own"], runs["twin"]):
        for n, p in st.generator.unet.named_parameters():
            assert p.requires_grad and p.grad is None and torch.equal(p.detach(), sw["unet"][n]), n
    assert not any(n.startswith("unet.") for n in runs["stepped"])


def test_joint_step_1_against_the_torch_twin(psg, runs):
    ro, rt, po, pt = runs["steps"][0]
    assert set(ro) == set(rt) == {"loss", "l1_loss", "mse_loss"} | set(NORMS)
    for k in sorted(ro):
        assert ro[k].is_cuda and ro[k].dim() == 0 and rt[k].is_cuda and rt[k].dim() == 0, k        # device scalars
        print(f"joint step 1 {k}: own {float(ro[k]):.6e} twin {float(rt[k]):.6e}")
        assert _rel(ro[k], rt[k]) < LOSS_BAR and float(rt[k]) > 0, k
    assert float(ro["grad_norm"]) > MAX_NORM                                  # the shared clip is active
    stepped, start = runs["stepped"], runs["switched"]["params"]
    assert len([n for n in stepped if n.startswith("vae_decoder.")]) == 144 and ZERO <= stepped
    assert any(n.startswith("text_encoder.") for n in stepped)
    lr = {"vae_decoder": DLR, "text_encoder": LR}
    worst, excepted = (0.0, ""), set()
    for n in sorted(po):
        if n not in stepped:                                   # the VAE encoder, the text encoder's frozen layers and the pooler
            assert torch.equal(po[n], start[n]) and torch.equal(pt[n], start[n]), n
            continue
        assert not torch.equal(po[n], start[n]), f"{n} did not move"
        if n in ZERO:
            excepted.add(n)
            d, bound = (po[n] - start[n]).abs(), 1.01 * lr[n.split(".")[0]] * (1 + WD * start[n].abs())
            assert bool((d <= bound).all()), (n, float(d.max()))
            continue
        e = maxrel(po[n], pt[n])
        worst = max(worst, (e, n))
        assert e < BAR, (n, e)
    print(f"joint step 1 worst per-parameter max-rel against the twin {worst[0]:.2e} ({worst[1]})")
    assert excepted == ZERO


def test_joint_steps_2_and_3_against_the_torch_twin(psg, runs):
    """Measured on MI355X: 5.33e-7 after step 2, 6.91e-7 after step 3 (text_encoder.projection.weight) = STEP23_MEASURED; the bound
    is 4 x that (2.8e-6)."""
    bound = max(4 * STEP23_MEASURED, BAR)
    worst = []
    for i in (1, 2):
        ro, rt, po, pt = runs["steps"][i]
        worst.append(max((maxrel(po[n], pt[n]), n) for n in runs["stepped"] if n not in ZERO))
        print(f"joint step {i + 1} worst per-parameter max-rel against the twin {worst[-1][0]:.2e} ({worst[-1][1]}), bound {bound:.1e}")
        for k in ("loss",) + NORMS:
            print(f"joint step {i + 1} {k}: own {float(ro[k]):.6e} twin {float(rt[k]):.6e}")
        assert float(ro["loss"]) != float(runs["steps"][i - 1][0]["loss"])                     # the weights moved the loss
    assert max(worst)[0] < bound, worst


@pytest.fixture(scope="module")
def cpu_step(psg, world):
    """Joint step 1 on the CPU: BERT restatement -> oracle decoder (the GPU encoder's latent) -> L1 + 0.1 MSE -> backward."""
    torch.set_num_threads(8)
    gen = _generator(psg, world)
    images, ids, mask = world["batch"]
    with torch.no_grad():
        latent = gen.vae_encoder(images)[0].cpu()
    te = gen.text_encoder
    train = {n for n, p in te.named_parameters() if p.requires_grad and not n.startswith("bert.pooler.")}
    tsd = {k: v.clone().requires_grad_(k in train) for k, v in world["te"].items()}
    dsd = {k: v.clone().requires_grad_(True) for k, v in world["dec"].items()}
    emb = FC.bert_encode(tsd, world["cfg"], ids.cpu(), mask.cpu(), torch.zeros_like(ids.cpu()), 256)
    total, l1, mse = FC.recon_loss(V.vae_decode(dsd, latent, emb), images.cpu())
    total.backward()
    tg = {k: v.grad for k, v in tsd.items() if k in train}
    dg = {k: v.grad for k, v in dsd.items()}
    assert all(g is not None for g in tg.values()) and all(g is not None for g in dg.values())
    nt = float(torch.stack([g.double().norm() for g in tg.values()]).norm())
    nd = float(torch.stack([g.double().norm() for g in dg.values()]).norm())
    return {"gen": gen, "text": tg, "dec": dg, "norm_text": nt, "norm_dec": nd, "norm": (nt * nt + nd * nd) ** 0.5, "loss": float(total)}


def test_the_clip_is_shared_step_1_against_the_cpu(psg, world, cpu_step):
    """max_grad_norm is half the CPU run's total norm, so the clip is active; what the kernel applied (the first moment after
    step 1 is (1 - beta1) * coef * g) is the CPU gradient times the SHARED coefficient."""
    c = cpu_step
    max_norm = 0.5 * c["norm"]
    st = _stepper(psg, c["gen"], "grouped", max_grad_norm=max_norm)
    st.switch_to_joint_training()
    r = st.train_step(*world["batch"])
    got = {k: float(r[k]) for k in NORMS}
    print(f"CPU norms: total {c['norm']:.6e} text {c['norm_text']:.6e} decoder {c['norm_dec']:.6e}; GPU {got}; max_grad_norm {max_norm:.6e}")
    assert got["grad_norm"] > max_norm                                        # the clip is active
    assert abs(float(r["loss"]) - c["loss"]) < CPU_BAR * c["loss"]
    for k, want in zip(NORMS, (c["norm"], c["norm_text"], c["norm_dec"])):
        assert abs(got[k] - want) < CPU_BAR * want, (k, got[k], want)
    sq = got["grad_norm_text"] ** 2 + got["grad_norm_decoder"] ** 2
    assert abs(got["grad_norm"] ** 2 - sq) < 1e-5 * sq
    shared = min(1.0, max_norm / (got["grad_norm"] + 1e-6))
    own = {"text": min(1.0, max_norm / (got["grad_norm_text"] + 1e-6)), "dec": min(1.0, max_norm / (got["grad_norm_decoder"] + 1e-6))}
    # a per-group coefficient is off by the ratio of the norms - far outside the bar for at least one of the groups
    assert max(own["text"] / shared, own["dec"] / shared) > 1 + 100 * CPU_BAR, (own, shared)
    cpu_coef = min(1.0, max_norm / (c["norm"] + 1e-6))
    gen = c["gen"]
    picks = [(gen.text_encoder.projection.weight, c["text"]["projection.weight"], "text"),
             (gen.vae_decoder.block3_resnet1.conv1.weight, c["dec"]["block3_resnet1.conv1.weight"], "dec"),
             (gen.vae_decoder.block2_attn.k.weight, c["dec"]["block2_attn.k.weight"], "dec")]
    for p, ref, group in picks:
        assert p.grad.data_ptr() == st.arena.views[[id(q) for q in st.arena.params].index(id(p))].data_ptr()     # from the arena
        e_g = maxrel(p.grad * shared, ref * cpu_coef)
        applied = st.optimizer.state[p]["exp_avg"] / (1 - 0.9)
        e_m = maxrel(applied, ref * cpu_coef)
        print(f"{tuple(p.shape)} ({group}): arena gradient x shared coef {e_g:.2e}, applied gradient (exp_avg / 0.1) {e_m:.2e}; "
              f"own coef / shared {own[group] / shared:.4f}")
        assert e_g < CPU_BAR and e_m < CPU_BAR, (e_g, e_m)
    _release(st)


def test_no_stale_operand_after_the_raw_pointer_updates(psg, world, runs):
    """validate_step after three joint steps == validate_step of freshly built modules holding the checkpoint's weights."""
    gen = _generator(psg, world, trainable=False, model_state={k: v for k, v in runs["checkpoint"]["model_state_dict"].items()
                                                                 if not k.startswith("unet.")})
    got = psg.FinalStepper(gen).validate_step(*world["batch"])
    assert set(got) == set(runs["validate"]) == {"loss", "l1_loss", "mse_loss"}
    for k, v in runs["validate"].items():
        assert torch.equal(v, got[k]), k
    assert not torch.equal(runs["validate"]["loss"], runs["steps"][0][0]["loss"])


def test_checkpoint_resume_is_bitwise(psg, world, runs):
    ck = runs["checkpoint"]
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "global_step", "best_val_loss",
                       "training_phase"}
    assert ck["training_phase"] == "joint" and ck["global_step"] == 4 and ck["epoch"] == 1
    assert [g["name"] for g in ck["optimizer_state_dict"]["param_groups"]] == ["text_encoder", "vae_decoder"]
    gen = _generator(psg, world, unet=_small_unet(psg))
    again = _stepper(psg, gen, "grouped")
    assert again.training_phase == "text_encoder"
    again.load_state_dict(ck)                                                  # switches first
    assert again.training_phase == "joint" and again.optimizer.steps_done() == 3 and again.learning_rates() == runs["own"].learning_rates()
    r = _scalars(again.train_step(*world["batch"]))
    want, params, m, v = runs["step4"]
    for k, x in want.items():
        assert torch.equal(x, r[k]), k
    got = _params(gen)
    for n in params:
        assert torch.equal(params[n], got[n]), n
    assert torch.equal(m, again.optimizer._m) and torch.equal(v, again.optimizer._v)
    _release(again)


def test_a_second_loss_term(psg, world):
    """clip_loss / clip_weight in the joint phase: both gradient paths into the reconstruction are summed, in both updates."""
    clip = lambda recon, texts: recon.square().mean()
    res = []
    for update in ("grouped", "torch"):
        gen = _generator(psg, world)
        st = _stepper(psg, gen, update)
        st.switch_to_joint_training()
        start = _params(gen)
        res.append((_scalars(st.train_step(*world["batch"], clip_loss=clip, clip_weight=0.1, texts=None)), _params(gen), _stepped(st), start))
        _release(st)
    (ro, po, stepped, start), (rt, pt, _, _) = res
    plain = _generator(psg, world)
    base = psg.FinalStepper(plain).validate_step(*world["batch"])
    assert float(ro["loss"]) > float(base["loss"])                             # the second term is in the total
    for k in sorted(ro):
        print(f"second loss term {k}: own {float(ro[k]):.6e} twin {float(rt[k]):.6e}")
        assert _rel(ro[k], rt[k]) < LOSS_BAR, k
    for n in sorted(stepped):
        assert not torch.equal(po[n], start[n]), f"{n} did not move"
        if n in ZERO:
            d, bound = (po[n] - start[n]).abs(), 1.01 * DLR * (1 + WD * start[n].abs())
            assert bool((d <= bound).all()), (n, float(d.max()))
            continue
        e = maxrel(po[n], pt[n])
        assert e < BAR, (n, e)


def test_one_bf16_joint_step(psg, world, runs):
    """Measured on MI355X: |norm_bf16 / norm_fp32 - 1| = 1.31e-3 (grad_norm), 2.01e-3 (grad_norm_text), 1.29e-3 (grad_norm_decoder):
    BF16_NORMS_MEASURED."""
    gen = _generator(psg, world, dtype=torch.bfloat16)
    st = _stepper(psg, gen, "grouped")
    st.train_step(*world["batch"])                         # the fp32 run's sequence: a text-phase step, the epoch's end, the switch
    st.end_epoch()
    st.switch_to_joint_training()
    start = _params(gen)
    r = st.train_step(*world["batch"])
    for k in ("loss", "l1_loss", "mse_loss") + NORMS:
        assert bool(torch.isfinite(r[k])), k
    after = _params(gen)
    for n in _stepped(st):
        if n not in ZERO:
            assert not torch.equal(after[n], start[n]), f"{n} did not move"
    fp32 = runs["steps"][0][0]
    for k in NORMS:
        e = _rel(r[k], fp32[k])
        print(f"bf16 {k}: {float(r[k]):.6e} against fp32 {float(fp32[k]):.6e}: {e:.2e}")
        assert e < BF16_NORM_BAR, (k, e)
    _release(st)
