"""CPU suite for the VAE encoder's training path: host-side validation of psg_conv4s2_dgrad / psg_conv4s2_wgrad /
psg_reparam_bwd_f32, the VAEEncoder(trainable=...) parameter flags, and the references of the GPU tests checked against
themselves - the kernel-level bound (tests/gemm_ref.check on tests/conv4s2_ref's cases) holds torch's own fp32 kernels and
rejects planted defects; the module-level fp64 oracle gradients are reproduced by torch fp32 to a tenth of the fp32 bar, and
torch bf16's distance from them is recorded in tests/golden/vae_encoder_grad_bf16.json for the GPU test's bf16 bar."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from tests import conv4s2_ref as R
from tests import gemm_ref
from tests.util import maxrel, rel_l2

from pokemon_sprite_generator_amd._lib import OK, ERR_SHAPE, ERR_DTYPE, ERR_ALIGN, ERR_WORKSPACE, ERR_ARG

P = 0x10000            # a 16-byte aligned non-null "pointer": validation never dereferences


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def _dgrad(lib, g=P, ldg=32, wd=P, dx=P, lddx=16, B=2, Hi=7, Wi=9, Cin=16, Ho=3, Wo=4, Cout=32, pad=1, dtype=1):
    return lib.psg_conv4s2_dgrad(g, ldg, wd, dx, lddx, B, Hi, Wi, Cin, Ho, Wo, Cout, pad, dtype, None)


def _wgrad(lib, x=P, ldx=16, g=P, ldg=32, dw=P, layout=0, cin_real=16, dbias=P, B=2, Hi=7, Wi=9, Cin=16, Ho=3, Wo=4, Cout=32, pad=1,
           acc=0, accb=0, dtype=1, ws=P, ws_bytes=1 << 30):
    return lib.psg_conv4s2_wgrad(x, ldx, g, ldg, dw, layout, cin_real, dbias, B, Hi, Wi, Cin, Ho, Wo, Cout, pad, acc, accb, dtype, ws, ws_bytes, None)


def test_dgrad_argument_validation(lib):
    for null in ("g", "wd", "dx"):
        assert _dgrad(lib, **{null: None}) == ERR_ARG and b"null" in lib.psg_last_error()
    assert _dgrad(lib, dtype=7) == ERR_DTYPE and b"dtype" in lib.psg_last_error()
    for pad in (0, 3):
        assert _dgrad(lib, pad=pad) == ERR_ARG and b"pad" in lib.psg_last_error()
    assert _dgrad(lib, Ho=4) == ERR_SHAPE and b"(H+2p-4)/2+1" in lib.psg_last_error()
    assert _dgrad(lib, pad=2) == ERR_SHAPE                                   # 7x9 pad 2 gives 4x5, not 3x4
    assert _dgrad(lib, Cin=12, lddx=16) == ERR_SHAPE and b"multiples of 8" in lib.psg_last_error()
    assert _dgrad(lib, Cout=36, ldg=40) == ERR_SHAPE and b"multiples of 8" in lib.psg_last_error()
    assert _dgrad(lib, ldg=24) == ERR_SHAPE and b"leading dimension of g" in lib.psg_last_error()
    assert _dgrad(lib, lddx=8) == ERR_SHAPE and b"leading dimension of dx" in lib.psg_last_error()
    assert _dgrad(lib, g=P + 8) == ERR_ALIGN and _dgrad(lib, dx=P + 4) == ERR_ALIGN and _dgrad(lib, wd=P + 2) == ERR_ALIGN
    assert _dgrad(lib, ldg=36) == ERR_ALIGN                                   # bf16 rows of 72 bytes
    assert _dgrad(lib, B=0) == ERR_SHAPE


def test_wgrad_argument_validation(lib):
    for null in ("x", "g", "dw"):
        assert _wgrad(lib, **{null: None}) == ERR_ARG and b"null" in lib.psg_last_error()
    assert _wgrad(lib, dtype=2) == ERR_DTYPE
    assert _wgrad(lib, pad=0) == ERR_ARG and _wgrad(lib, pad=4) == ERR_ARG
    assert _wgrad(lib, Wo=5) == ERR_SHAPE and b"(H+2p-4)/2+1" in lib.psg_last_error()
    assert _wgrad(lib, Cin=20, ldx=24, cin_real=20) == ERR_SHAPE and _wgrad(lib, Cout=20) == ERR_SHAPE
    assert _wgrad(lib, ldx=8) == ERR_SHAPE and b"leading dimension of x" in lib.psg_last_error()
    assert _wgrad(lib, ldg=16) == ERR_SHAPE and b"leading dimension of g" in lib.psg_last_error()
    assert _wgrad(lib, x=P + 8) == ERR_ALIGN and _wgrad(lib, g=P + 2) == ERR_ALIGN and _wgrad(lib, ldx=20) == ERR_ALIGN
    assert _wgrad(lib, dtype=0, ldx=18) == ERR_ALIGN                          # fp32 rows of 72 bytes
    for bad in (0, -1, 17):
        assert _wgrad(lib, cin_real=bad) == ERR_ARG and b"cin_real" in lib.psg_last_error()
    assert _wgrad(lib, layout=2) == ERR_ARG and b"dw_layout" in lib.psg_last_error()
    need = lib.psg_conv4s2_wgrad_workspace_bytes(2, 3, 4, 16, 32, 1)
    assert need > 0
    assert _wgrad(lib, ws_bytes=need - 1) == ERR_WORKSPACE and b"workspace" in lib.psg_last_error()
    assert _wgrad(lib, ws=None) == ERR_WORKSPACE
    assert _wgrad(lib, ws=P + 4, ws_bytes=need) == ERR_ALIGN
    assert lib.psg_reparam_bwd_f32(None, P, P, P, P, 0, 16, None) == ERR_ARG
    assert lib.psg_reparam_bwd_f32(P, P, P, None, None, 0, 16, None) == ERR_ARG
    assert lib.psg_reparam_bwd_f32(P, None, P, P, P, 0, 16, None) == ERR_ARG
    assert lib.psg_reparam_bwd_f32(P, None, None, P, None, 0, 0, None) == OK    # n = 0: nothing to do


def test_workspace_query_is_positive_and_monotone_in_the_split_count(lib):
    try:
        assert lib.psg_conv4s2_wgrad_workspace_bytes(32, 107, 107, 8, 32, 7) == -1 and b"dtype" in lib.psg_last_error()
        assert lib.psg_conv4s2_wgrad_workspace_bytes(32, 107, 107, 12, 32, 1) == -1
        assert lib.psg_conv4s2_wgrad_workspace_bytes(0, 107, 107, 8, 32, 1) == -1
        for (B, Ho, Cin, Cout) in ((32, 107, 8, 32), (32, 53, 32, 64), (32, 27, 64, 128), (3, 3, 8, 32)):
            prev = 0
            for n in (1, 2, 3, 4, 8, 16, 64):
                assert lib.psg_conv4s2_wgrad_set_splits(n) == OK
                b = lib.psg_conv4s2_wgrad_workspace_bytes(B, Ho, Ho, Cin, Cout, 1)
                assert b >= prev and b > 0 and b % ((Cout * 16 * Cin + Cout) * 4) == 0, (B, Ho, Cin, Cout, n, b)
                if n == 1:
                    assert b == (Cout * 16 * Cin + Cout) * 4
                prev = b
            lib.psg_conv4s2_wgrad_set_splits(0)
            b = lib.psg_conv4s2_wgrad_workspace_bytes(B, Ho, Ho, Cin, Cout, 0)
            assert 0 < b <= 256 * (Cout * 16 * Cin + Cout) * 4
    finally:
        lib.psg_conv4s2_wgrad_set_splits(0)


def test_trainable_flag_sets_the_parameter_flags():
    import pokemon_sprite_generator_amd as psg
    frozen, train = psg.VAEEncoder(), psg.VAEEncoder(3, 8, trainable=True)
    assert len(list(frozen.parameters())) == 70 and not any(p.requires_grad for p in frozen.parameters())
    assert len(list(train.parameters())) == 70 and all(p.requires_grad for p in train.parameters())
    assert frozen.trainable is False and train.trainable is True
    assert list(frozen.state_dict()) == list(train.state_dict())
    with pytest.raises(psg.PsgError):                                       # no CPU fallback on either path
        train(torch.zeros(1, 3, 23, 27))
    with pytest.raises(psg.PsgError):
        frozen(torch.zeros(1, 3, 23, 27))
    vae = psg.PokemonVAE()                                                  # the frozen VAE is what it was
    assert vae.encoder.trainable is False


# ------------------------------------------------------------------------------------------ the kernel-level bound
@pytest.mark.parametrize("name", sorted(R.DGRAD_CASES))
def test_dgrad_bound_holds_torch_fp32_and_rejects_planted_defects(name):
    B, Hi, Wi, pad, Cin, Cout, _ = R.DGRAD_CASES[name]
    g, w = R.dgrad_inputs(name, torch.float32)
    ref, S = gemm_ref.conv_dgrad(g, w, (Hi, Wi), stride=2, pad=pad)
    t = F.conv_transpose2d(g.permute(0, 3, 1, 2), w, stride=2, padding=pad, output_padding=((Hi + 2 * pad - 4) % 2, (Wi + 2 * pad - 4) % 2))
    worst = gemm_ref.check(t.permute(0, 2, 3, 1), ref, S, torch.float32, f"{name} torch fp32", 4 * Cout)
    print(f"{name}: torch fp32 conv_transpose2d err/bound {worst:.3f}")
    for dtype in (torch.float32, torch.bfloat16):
        g, w = R.dgrad_inputs(name, dtype)
        ref, S = gemm_ref.conv_dgrad(g, w, (Hi, Wi), stride=2, pad=pad)
        gemm_ref.check(ref.to(dtype), ref, S, dtype, f"{name} rounded reference", 4 * Cout)       # the reference alone passes
        w2 = w.clone()
        w2[:, :, 2, 1] = 0                                                                    # one tap dropped
        bad, _ = gemm_ref.conv_dgrad(g, w2, (Hi, Wi), stride=2, pad=pad)
        with pytest.raises(AssertionError):
            gemm_ref.check(bad.to(dtype), ref, S, dtype, f"{name} tap dropped", 4 * Cout)
        # pad 1 computed as pad 2 (and 2 as 1): the same g spread with the other padding - the grid on which that is consistent
        # is two pixels smaller / larger - laid over the true grid from the top left corner
        other = 3 - pad
        H2, W2 = Hi + 2 * (pad - other), Wi + 2 * (pad - other)
        if H2 >= 1 and W2 >= 1 and R.out_hw(H2, W2, other) == R.out_hw(Hi, Wi, pad):
            off, _ = gemm_ref.conv_dgrad(g, w, (H2, W2), stride=2, pad=other)
            bad = torch.zeros_like(ref)
            hh, ww = min(Hi, H2), min(Wi, W2)
            bad[:, :hh, :ww] = off[:, :hh, :ww]
            with pytest.raises(AssertionError):
                gemm_ref.check(bad.to(dtype), ref, S, dtype, f"{name} pad {pad} as pad {other}", 4 * Cout)


def _shift_pad(x):
    """x as a kernel gathering with pad + 1 would see it: every tap one pixel up and left."""
    return F.pad(x, (0, 0, 1, 0, 1, 0))[:, :x.shape[1], :x.shape[2]]


@pytest.mark.parametrize("name", sorted(R.WGRAD_CASES))
def test_wgrad_bound_holds_torch_fp32_and_rejects_planted_defects(name, lib):
    B, Hi, Wi, pad, Cin, cin_real, Cout, _, _, pins, _ = R.WGRAD_CASES[name]
    Ho, Wo = R.out_hw(Hi, Wi, pad)
    M = B * Ho * Wo
    x, g = R.wgrad_inputs(name, torch.float32)
    ref, S = R.wgrad_ref(x, g, pad)
    wt = torch.zeros(Cout, Cin, 4, 4, requires_grad=True)
    F.conv2d(x.permute(0, 3, 1, 2), wt, stride=2, padding=pad).backward(g.permute(0, 3, 1, 2))
    worst = gemm_ref.check(wt.grad, ref, S, torch.float32, f"{name} torch fp32", M)
    print(f"{name}: torch fp32 conv2d weight gradient err/bound {worst:.3f}")
    for dtype in (torch.float32, torch.bfloat16):
        x, g = R.wgrad_inputs(name, dtype)
        ref, S = R.wgrad_ref(x, g, pad)
        gemm_ref.check(ref.float(), ref, S, torch.float32, f"{name} rounded reference", M)
        bad, _ = R.wgrad_ref(_shift_pad(x), g, pad)                                              # pad p computed as pad p + 1
        with pytest.raises(AssertionError):
            gemm_ref.check(bad.float(), ref, S, torch.float32, f"{name} pad off by one", M)
        bad = ref.clone()
        bad[:, :, 1, 3] = 0                                                                   # one tap dropped
        with pytest.raises(AssertionError):
            gemm_ref.check(bad.float(), ref, S, torch.float32, f"{name} tap dropped", M)
        n = max(pins)
        rps = -(-(-(-M // n)) // 16) * 16                                                     # rows per slab: whole 16-row steps
        if rps < M:
            bad, _ = R.wgrad_ref(x, g, pad, rows=slice(0, (M - 1) // rps * rps))                 # the last M split omitted
            with pytest.raises(AssertionError):
                gemm_ref.check(bad.float(), ref, S, torch.float32, f"{name} last split omitted", M)
        if cin_real < Cin:                                                                    # cin_real ignored: rows of Cin written
            bad = ref.reshape(-1)[:Cout * cin_real * 16].reshape(Cout, cin_real, 4, 4)
            with pytest.raises(AssertionError):
                gemm_ref.check(bad.float(), ref[:, :cin_real], S[:, :cin_real], torch.float32, f"{name} cin_real ignored", M)
    # every split pin of the case really gives that many slabs (the GPU test relies on it for its uneven split)
    try:
        for n in pins:
            lib.psg_conv4s2_wgrad_set_splits(n)
            assert lib.psg_conv4s2_wgrad_workspace_bytes(B, Ho, Wo, Cin, Cout, 1) == n * (Cout * 16 * Cin + Cout) * 4
    finally:
        lib.psg_conv4s2_wgrad_set_splits(0)


# -------------------------------------------------------------------------------------------- the module-level reference
def test_module_reference_fp32_is_a_tenth_of_the_bar_and_bf16_is_recorded():
    import pokemon_sprite_generator_amd as psg
    enc = psg.VAEEncoder(3, 8)
    sd = R.encoder_state({k: tuple(v.shape) for k, v in enc.state_dict().items()})
    img, eps, G = R.encoder_inputs()
    ref, ref_out = R.oracle_run(sd, img, eps, G, torch.float64)
    assert len(ref) == 70
    assert tuple(ref_out[0].shape) == (2, 8, 3, 4)
    sibling = float(ref[R.ZERO_GRAD_SIBLING].abs().max())
    assert float(ref[R.ZERO_GRAD].abs().max()) < 1e-12 * sibling                 # zero in exact arithmetic; fp64 leaves ~1e-17
    f32, f32_out = R.oracle_run(sd, img, eps, G, torch.float32)
    worst = max((maxrel(f32[k], ref[k]), k) for k in ref if k != R.ZERO_GRAD)
    print(f"torch fp32 vs fp64: worst per-parameter max-rel {worst[0]:.2e} ({worst[1]}); |{R.ZERO_GRAD}| fp32 "
          f"{float(f32[R.ZERO_GRAD].abs().max()):.2e}, sibling {sibling:.2e}")
    assert worst[0] < 1e-4, worst                                                # a tenth of the fp32 bar (1e-3)
    assert all(maxrel(a, b) < 1e-4 for a, b in zip(f32_out, ref_out))
    assert float(f32[R.ZERO_GRAD].abs().max()) <= 1e-3 * sibling
    b16, _ = R.oracle_run(sd, img, eps, G, torch.bfloat16)
    rec = {k: float(f"{rel_l2(b16[k], ref[k]):.3e}") for k in sorted(ref) if k != R.ZERO_GRAD}
    rec[R.ZERO_GRAD] = float(f"{float(b16[R.ZERO_GRAD].abs().max()) / sibling:.3e}")           # on its sibling's scale
    with open(R.GOLDEN_BF16, "w") as f:
        json.dump({"what": "torch bf16 autograd of oracle.vae_oracle.vae_encode vs its fp64 run: per-parameter gradient rel-L2 "
                           f"({R.ZERO_GRAD}: max |g| / max |fp64 gradient of {R.ZERO_GRAD_SIBLING}|); inputs of tests/conv4s2_ref.py",
                   "rel_l2": rec}, f, indent=1, sort_keys=True)
        f.write("\n")
    assert set(R.load_bf16_golden()["rel_l2"]) == set(ref)
