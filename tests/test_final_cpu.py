"""CPU suite of stage 3 (the text encoder trained through the frozen VAE decoder): the new C-ABI entries are declared, bound
and exported; the fixture tests/golden/final_grad.npz (reference VAEDecoder forward + backward, tools/make_golden_final.py) is
reproduced by oracle.vae_oracle under autograd on this machine; the stage-3 surface carries the reference's names."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import vae_oracle as V
from tests import final_cases as FC
from tests import text_cases as TC
from tests import text_grad_cases as GC
from tests.util import maxrel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["psg_attn_bwd_longq", "psg_attn_bwd_longq_workspace_bytes", "psg_recon_loss_f32", "psg_recon_loss_workspace_bytes"]
A16 = 0x1000


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_new_symbols_declared_exported_and_bound(lib):
    from pokemon_sprite_generator_amd import _lib
    txt = open(os.path.join(ROOT, "include", "psg_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, body), f"{n} not declared in include/psg_hip.h"
        assert hasattr(lib, n), f"libpsg_hip.so does not export {n}"
        assert n in _lib.SIGNATURES, n
    # each new entry cites the reference lines it implements
    assert "vae_decoder.py:49-65" in txt and "final_trainer.py:215-236" in txt and "final_trainer.py:425-440" in txt


def _longq(lib, B=2, heads=8, L=729, S=32, d=8, drop=0.0, dt=1, ld=64, ws=A16, ws_bytes=1 << 30, q=A16):
    return lib.psg_attn_bwd_longq(q, ld, A16, 2 * ld, A16, 2 * ld, A16, ld, A16, ld, A16, A16, A16, ld, A16, 2 * ld, A16, 2 * ld,
                                  B, heads, L, S, d, 1.0, drop, 0, dt, ws, ws_bytes, None)


def test_longq_argument_validation_without_gpu(lib):
    """Bad arguments are refused on the host before any launch."""
    assert _longq(lib, drop=0.1) == -6 and b"drop_p" in lib.psg_last_error()                  # PSG_ERR_ARG: no dropout here
    assert _longq(lib, q=None) == -6
    assert _longq(lib, dt=7) == -2
    assert _longq(lib, d=12) == -1 and _longq(lib, S=257) == -1 and _longq(lib, L=0) == -1    # PSG_ERR_SHAPE
    assert _longq(lib, ld=60) == -1 and _longq(lib, q=A16 + 2) == -3
    need = lib.psg_attn_bwd_longq_workspace_bytes(2, 8, 729, 32, 8)
    assert need >= 2 * 8 * 2 * 32 * 8 * 4                                                     # at least one fp32 [2][S][d] per (b, head)
    assert _longq(lib, ws_bytes=need - 1) == -4 and _longq(lib, ws=None) == -4                # PSG_ERR_WORKSPACE
    assert lib.psg_attn_bwd_longq_workspace_bytes(2, 8, 0, 32, 8) < 0
    # the size is a function of the shape alone, and grows with the number of slabs only
    assert lib.psg_attn_bwd_longq_workspace_bytes(2, 8, 729, 32, 8) == need
    assert lib.psg_attn_bwd_longq_workspace_bytes(4, 8, 46225, 32, 4) <= 64 << 20
    assert lib.psg_recon_loss_f32(None, A16, None, A16, 10, 1.0, 0.1, A16, None) == -6
    assert lib.psg_recon_loss_f32(A16, A16, None, A16, 0, 1.0, 0.1, A16, None) == -1
    assert lib.psg_recon_loss_workspace_bytes() > 0


def test_fixture_exists_and_has_every_case(golden):
    assert os.path.exists(os.path.join(ROOT, "tests", "golden", "final_grad.npz"))
    g = golden("final_grad.npz")
    for case, (B, S) in FC.CASES.items():
        assert g[f"{case}_loss"].shape == (3,) and g[f"{case}_dtext"].shape == (B, S, 256) and g[f"{case}_dlatent"].shape == (B, 8, 27, 27)
        tot, l1, mse = (float(v) for v in g[f"{case}_loss"])
        assert abs(tot - (l1 + 0.1 * mse)) < 1e-6 * tot


@pytest.mark.parametrize("case", sorted(FC.CASES))
def test_oracle_under_autograd_reproduces_the_fixture(golden, case):
    """oracle.vae_oracle.vae_decode + the L1 + 0.1 MSE loss, differentiated by torch on this machine, against the reference's
    recorded loss and gradients: 1e-5, max-abs over max-abs."""
    import pokemon_sprite_generator_amd as psg
    g = golden("final_grad.npz")
    torch.set_num_threads(8)
    sd = FC.decoder_state({k: v.shape for k, v in psg.VAEDecoder().state_dict().items()})
    lat, text, img = FC.inputs(case)
    lat.requires_grad_(True), text.requires_grad_(True)
    losses = FC.recon_loss(V.vae_decode(sd, lat, text), img)
    losses[0].backward()
    e = [maxrel(torch.stack(losses), torch.from_numpy(g[f"{case}_loss"])), maxrel(text.grad, torch.from_numpy(g[f"{case}_dtext"])),
         maxrel(lat.grad, torch.from_numpy(g[f"{case}_dlatent"]))]
    print(f"case {case}: oracle vs fixture: loss {e[0]:.2e}, dtext {e[1]:.2e}, dlatent {e[2]:.2e}")
    assert max(e) < 1e-5, e


def test_bert_restatement_is_pinned_to_the_reference_fixture(golden):
    """tests.final_cases.bert_encode (the CPU text encoder of the end-to-end GPU check) against the reference module's recorded
    output and gradients of case M (tests/golden/text_encoder_grad.npz)."""
    from tests.util import check_digest
    g = golden("text_encoder_grad.npz")
    c = GC.CASES["M"]
    from pokemon_sprite_generator_amd.text_encoder import TextEncoder
    enc = TextEncoder(bert_config=TC.bert_config(c["layers"]), hidden_dim=c["hidden_dim"], finetune_strategy=c["strategy"], trainable=True)
    sd = {k: v.clone().requires_grad_(k in set(GC.trainable_names(enc))) for k, v in GC.state_dict(enc).items()}
    ids, mask, tt = (torch.from_numpy(g[f"M_{k}"]) for k in ("input_ids", "attention_mask", "token_type_ids"))
    y = FC.bert_encode(sd, enc.bert.config, ids, mask, tt, c["hidden_dim"])
    assert maxrel(y[:, :, ::GC.COL_STRIDE["M"]], torch.from_numpy(g["M_out_cols"])) < 1e-5
    (y * GC.cotangent("M", y.shape)).sum().backward()
    for n in ("projection.weight", "bert.encoder.layer.1.attention.self.value.weight", "bert.encoder.layer.2.output.dense.weight"):
        check_digest(sd[n].grad, g[f"M_grad_d::{n}"], g[f"M_grad_s::{n}"], 1e-4, what=n)


def test_stage3_surface_has_the_reference_names():
    import pokemon_sprite_generator_amd as psg
    G = psg.FinalPokemonGenerator
    for m in ("forward", "encode_and_decode", "encode_and_decode_ids", "unfreeze_vae_decoder", "freeze_vae_decoder", "unfreeze_unet",
              "freeze_unet", "from_checkpoints"):
        assert callable(getattr(G, m)), m
    for m in ("train_step", "validate_step"):
        assert callable(getattr(psg.FinalStepper, m)), m
    c = GC.CASES["M"]
    te = psg.TextEncoder(bert_config=TC.bert_config(1), hidden_dim=c["hidden_dim"], finetune_strategy="none", trainable=True)
    gen = G(psg.VAEEncoder(), psg.VAEDecoder(), psg.UNet(), te)
    keys = set(k.split(".")[0] for k in gen.state_dict())
    assert keys == {"vae_encoder", "vae_decoder", "unet", "text_encoder"}
    frozen = [p for m in (gen.vae_encoder, gen.vae_decoder, gen.unet) for p in m.parameters()]
    assert frozen and not any(p.requires_grad for p in frozen)
    assert any(p.requires_grad for p in gen.text_encoder.parameters())
    with pytest.raises(psg.PsgError, match="joint phase not built"):
        gen.unfreeze_vae_decoder()
    with pytest.raises(psg.PsgError, match="joint phase not built"):
        gen.unfreeze_unet()
    gen.freeze_vae_decoder(), gen.freeze_unet()
    assert not any(p.requires_grad for p in frozen)
    with pytest.raises(psg.PsgError):                    # no CPU fallback on the differentiable path either
        gen.vae_decoder(torch.zeros(1, 8, 27, 27), torch.zeros(1, 4, 256, requires_grad=True))
