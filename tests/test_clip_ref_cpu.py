"""CPU suite for the CLIP loss: the float64 restatement the GPU tests compare against (tests/clip_ref.py) is held against
transformers' own CLIPModel and F.interpolate, the recorded precision baseline against a re-measurement, the comparator against
planted defects; plus what of `psg.CLIPLoss` needs no device: state-dict keys, from_pretrained, the text cleaning, the EOS
rules, argument validation.  The second half holds the element-wise references and bounds of tests/clip_cases.py: they equal
torch (SDPA, F.interpolate, autograd) in float64, their measured constants are re-measured, the fp32 evaluation in the header's
order stays inside the counted bound, and fifteen planted kernel defects are rejected, each at the smallest case that shows it."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

from tests import clip_ref as R


def _hf(name):
    """(CLIPModel in float64 with its own random weights, its state dict) for CONFIGS[name]."""
    transformers = pytest.importorskip("transformers")
    c = R.CONFIGS[name]
    cfg = transformers.CLIPConfig(text_config=dict(c["text_config"], bos_token_id=1, pad_token_id=0), vision_config=dict(c["vision_config"]),
                                  projection_dim=c["projection_dim"])
    torch.manual_seed(7)
    m = transformers.CLIPModel(cfg).double().eval()
    with torch.no_grad():                               # transformers initialises every bias to 0 and every LayerNorm to (1, 0)
        for k, p in m.named_parameters():
            if k.endswith(".bias") or "norm" in k:
                p.add_(0.1 * torch.randn_like(p))
    return m, {k: v.detach().clone() for k, v in m.state_dict().items()}


@pytest.mark.parametrize("name", ["tiny", "eos"])
def test_restatement_equals_transformers(name):
    """Loss and d loss / d pixel_values of the restatement against CLIPModel.forward in float64, both EOS-pooling rules."""
    m, sd = _hf(name)
    c = R.CONFIGS[name]
    S = c["vision_config"]["image_size"]
    ids = R.token_ids(name, 2, 8)
    assert len(set(R.eos_index(ids, c["text_config"]["eos_token_id"]).tolist())) == 2          # EOS at different places
    pv = R.prep(R.image(name, 2, S - 7), S).detach()
    a = pv.clone().requires_grad_(True)
    out = m(input_ids=ids, pixel_values=a, attention_mask=torch.ones_like(ids))
    la = R.cosine(out.image_embeds, out.text_embeds.detach())
    la.backward()
    la = la.detach()
    b = pv.clone().requires_grad_(True)
    lb = R.cosine(R.vision(b, sd, c), R.text(ids, sd, c).detach())
    lb.backward()
    lb = lb.detach()
    assert abs(float(la) - float(lb)) <= 1e-10 * max(1.0, abs(float(la))), (float(la), float(lb))
    assert R.rel(b.grad, a.grad) <= 1e-10
    assert float(a.grad.abs().max()) > 0


def test_padding_mask_cannot_reach_text_embeds():
    """Padding follows the pooled EOS position and the tower is causal: the processor's mask changes nothing, in transformers
    and in the restatement - so the kernels need a causal mask only, no key lengths."""
    m, sd = _hf("tiny")
    c = R.CONFIGS["tiny"]
    ids = R.token_ids("tiny", 2, 8)
    at = R.eos_index(ids, 2)
    mask = torch.arange(8)[None, :] <= at[:, None]
    assert not bool(mask.all())
    with torch.no_grad():
        full = m.get_text_features(input_ids=ids, attention_mask=torch.ones_like(ids))
        part = m.get_text_features(input_ids=ids, attention_mask=mask.long())
    full, part = (getattr(t, "pooler_output", t) for t in (full, part))
    assert float((full - part).abs().max()) <= 1e-12
    assert float((R.text(ids, sd, c) - R.text(ids, sd, c, key_mask=mask)).abs().max()) <= 1e-12
    assert float((R.text(ids, sd, c) - full).abs().max()) <= 1e-10


@pytest.mark.parametrize("Hi,S", sorted({(h, s) for h, s, _ in R.PREP_CASES if h != s} | {(57, 64), (1, 8), (3, 16)}))
def test_resize_is_the_antialiased_bicubic_of_f_interpolate(Hi, S):
    x = R.u((2, 3, Hi, Hi), f"resize.{Hi}").double()
    M = R.resize_matrix(Hi, S)
    mine = torch.einsum("oh,bchw,pw->bcop", M, x, M)
    ref = F.interpolate(x, size=(S, S), mode="bicubic", align_corners=False, antialias=True)
    assert float((mine - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert float((M.sum(1) - 1).abs().max()) <= 1e-14 and int((M != 0).sum(1).max()) <= 4
    if Hi >= 8:                                          # a = -0.75 (torch's plain 'bicubic') is another filter
        other = F.interpolate(x, size=(S, S), mode="bicubic", align_corners=False)
        assert float((other - ref).abs().max()) > 1e-3


def test_eos_rules():
    ids = torch.tensor([[5, 9, 63, 63, 63], [7, 63, 0, 0, 0], [3, 40, 63, 40, 0]])
    assert R.eos_index(ids, 2).tolist() == [2, 1, 2]                 # the highest id, its first occurrence
    assert R.eos_index(ids, 40).tolist() == [0, 0, 1]                # the first position that holds the id (0 when there is none)


def test_text_cleaning_is_the_references():
    from pokemon_sprite_generator_amd.clip_loss import clean_text
    text = ["[NAME] is a small [MASK] green creature", "[MASK]", "no marks here", "a  double space [NAME]"]
    ref = [" ".join([w for w in t.split(" ") if w not in ["[MASK]", "[NAME]"]]) for t in text]           # clip_loss.py:49
    assert clean_text(text) == ref and ref[0] == "is a small green creature" and ref[1] == ""


def test_state_dict_keys_are_clipmodels_and_position_ids_are_ignored():
    import pokemon_sprite_generator_amd as psg
    m, sd = _hf("tiny")
    clip = psg.CLIPLoss(R.CONFIGS["tiny"])
    mine = clip.state_dict()
    assert set(mine) == {"model." + k for k in sd if not k.endswith("position_ids")}
    assert set(mine) == {"model." + k for k in R.state_shapes(R.CONFIGS["tiny"])}
    assert all(tuple(mine["model." + k].shape) == tuple(v.shape) for k, v in sd.items() if not k.endswith("position_ids"))
    full = {"model." + k: v.float() for k, v in sd.items()}
    full["model.text_model.embeddings.position_ids"] = torch.arange(16)[None]            # what some transformers versions save
    full["model.vision_model.embeddings.position_ids"] = torch.arange(17)[None]
    clip.load_state_dict(full)                                                           # strict
    assert torch.equal(clip.model.visual_projection.weight, sd["visual_projection.weight"].float())
    assert all(not p.requires_grad for p in clip.parameters())
    assert sum(p.numel() for p in clip.parameters()) == sum(p.numel() for p in m.parameters())
    # a CLIPConfig is accepted as well as a dict
    clip2 = psg.CLIPLoss(m.config)
    assert clip2.model.config == clip.model.config


def test_from_pretrained_reads_a_saved_directory(tmp_path):
    import pokemon_sprite_generator_amd as psg
    m, sd = _hf("tiny")
    m.float().save_pretrained(str(tmp_path))
    clip = psg.CLIPLoss.from_pretrained(str(tmp_path))
    assert clip.tokenizer is None                                                        # no tokenizer files in the directory
    got = clip.state_dict()
    for k, v in m.state_dict().items():
        if not k.endswith("position_ids"):
            assert torch.equal(got["model." + k], v.float()), k
    with pytest.raises(psg.PsgError, match="tokenizer"):
        clip.tokenize(["a green creature"])

    class Tok:                                           # a caller-supplied tokenizer sees the CLEANED text
        def __call__(self, text, **kw):
            self.seen, self.kw = text, kw
            return {"input_ids": torch.tensor([[3, 4, 63]] * len(text))}
    clip.tokenizer = Tok()
    ids = clip.tokenize(["[NAME] a green creature"])
    assert clip.tokenizer.seen == ["a green creature"] and ids.dtype == torch.int64 and clip.tokenizer.kw["padding"] is True


def test_cpu_tensors_are_refused():
    import pokemon_sprite_generator_amd as psg
    from pokemon_sprite_generator_amd import ops
    clip = psg.CLIPLoss(R.CONFIGS["tiny"])
    ids = R.token_ids("tiny", 1, 8)
    with pytest.raises(psg.PsgError):
        clip(torch.zeros(1, 3, 64, 64), ids)
    with pytest.raises(psg.PsgError):
        clip.text_features(ids)
    with pytest.raises(psg.PsgError):
        clip(torch.zeros(1, 3, 64, 64), ["no tokenizer"])
    with pytest.raises(psg.PsgError):
        ops.clip_prep(torch.zeros(1, 3, 8, 8), 16, 8)
    with pytest.raises(psg.PsgError):
        ops.cosine_loss(torch.zeros(2, 8), torch.zeros(2, 8))
    with pytest.raises(psg.PsgError):
        ops.attention_causal(torch.zeros(1, 4, 96), 2)


# ---- the comparator ---------------------------------------------------------------------------------------------
REL_TOL = 0.25            # another CPU may give other low bits; an entry is an error figure of one or two significant digits
INERT = R.BAR_FLOOR / R.BAR_FACTOR     # an entry below this cannot move its bar off the floor


def test_baseline_table_covers_every_case():
    assert set(R.BASELINE_ERR) == set(R.baseline_keys())


@pytest.mark.parametrize("key", R.baseline_keys(), ids=lambda k: "-".join(str(x) for x in k))
def test_baseline_err_is_torchs_own_error(key):
    """Every recorded value against a re-measurement: |measured - recorded| <= REL_TOL * recorded, or both so far under the
    bars' floor that neither can move a bar."""
    got, rec = R.measure(key), R.BASELINE_ERR[key]
    assert set(got) == set(rec)
    for n, v in got.items():
        assert abs(v - rec[n]) <= REL_TOL * rec[n] or max(v, rec[n]) < INERT, f"{key} {n}: measured {v:.3e}, recorded {rec[n]:.3e}"


@pytest.mark.parametrize("defect", [dict(cubic_a=-0.75), dict(causal=False), dict(act="gelu")], ids=["cubic-a", "no-causal-mask", "gelu-erf"])
def test_comparator_rejects_a_planted_defect(defect):
    """The float64 restatement with ONE thing wrong misses the fp32 bars by far: torch's non-antialiased cubic (a = -0.75), a
    text tower without the causal mask, GELU-erf in place of quick-GELU."""
    cfg = R.CONFIGS[R.LOSS_CASES["tiny"][0]]
    out, grad = R.loss(*R.loss_inputs("tiny"), R.loss_state_dict("tiny"), cfg, **defect)
    e = R.errors(dict(loss=out, grad=grad), ("loss", "tiny"))
    key = ("loss", "tiny", "fp32")
    assert e["grad"] > 100 * R.bar(key, "grad"), e
    assert e["loss"] > 100 * R.bar(key, "loss"), e
    sound = R.errors(dict(zip(("loss", "grad"), R.loss(*R.loss_inputs("tiny"), R.loss_state_dict("tiny"), cfg))), ("loss", "tiny"))
    assert sound["grad"] == 0.0 and sound["loss"] == 0.0


def test_comparator_rejects_the_wrong_cubic_at_the_kernel():
    Hi, S, P = 13, 16, 8
    img, dy = R.prep_inputs(Hi, S, P, 1)
    rows = R.patch_rows(R.prep(img, S, torch.float64, cubic_a=-0.75), P)
    e = R.errors(dict(fwd=rows, bwd=R.reference(("prep", Hi, S, P, 1))["bwd"]), ("prep", Hi, S, P, 1))
    assert e["fwd"] > 100 * R.bar(("prep", Hi, S, P, 1, "fp32"), "fwd") and e["bwd"] == 0.0


def test_patch_rows_are_the_flattened_conv():
    """Row r, column c P^2 + ky P + kx of the patch rows times the flattened Conv2d weight is the patch embedding."""
    pv = R.u((2, 3, 16, 16), "rows.pv").double()
    w = R.u((5, 3, 8, 8), "rows.w").double()
    ref = F.conv2d(pv, w, stride=8).flatten(2).transpose(1, 2)
    assert R.rel(R.patch_rows(pv, 8) @ w.reshape(5, -1).t(), ref) <= 1e-14
    rows = R.patch_rows(pv, 8)
    assert float(rows[1, 3, 2 * 64 + 5 * 8 + 6]) == float(pv[1, 2, 8 + 5, 8 + 6])         # patch 3 = (row 1, column 1)


# ---- argument validation: host checks, no launch ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


P16 = C.c_void_p(0x1000)
SHAPE, DTYPE, ALIGN, ARG = -1, -2, -3, -6


def test_clip_prep_argument_validation(lib):
    f, g = lib.psg_clip_prep_fwd, lib.psg_clip_prep_bwd
    assert f(None, P16, 192, 1, 8, 8, 16, 8, 0.5, 0.5, 0, None) == ARG and b"null" in lib.psg_last_error()
    assert f(P16, P16, 192, 1, 17, 17, 16, 8, 0.5, 0.5, 0, None) == SHAPE                  # Hi > S: needs the antialias window
    assert f(P16, P16, 192, 1, 8, 9, 16, 8, 0.5, 0.5, 0, None) == SHAPE                    # Hi != Wi: needs the centre crop
    assert f(P16, P16, 192, 1, 8, 8, 18, 8, 0.5, 0.5, 0, None) == SHAPE                    # S % P != 0
    assert f(P16, P16, 100, 1, 8, 8, 16, 8, 0.5, 0.5, 0, None) == SHAPE                    # row stride below 3 P^2
    assert f(P16, P16, 192, 1, 8, 8, 16, 8, 0.5, 0.5, 7, None) == DTYPE
    assert g(P16, 192, None, 1, 8, 8, 16, 8, 0.5, 0, None) == ARG
    assert g(P16, 192, P16, 1, 17, 17, 16, 8, 0.5, 0, None) == SHAPE
    assert g(P16, 192, P16, 1, 8, 9, 16, 8, 0.5, 0, None) == SHAPE
    assert g(P16, 192, P16, 1, 8, 8, 18, 8, 0.5, 0, None) == SHAPE


def test_causal_attention_and_cosine_argument_validation(lib):
    f = lib.psg_attn_fwd_causal
    ok = dict(B=2, heads=2, L=8, S=8, d=16)

    def call(q=P16, ld=96, drop=0.0, dtype=0, **kw):
        a = dict(ok, **kw)
        return f(q, ld, P16, ld, P16, ld, P16, 32, None, a["B"], a["heads"], a["L"], a["S"], a["d"], 0.25, drop, 0, dtype, None)
    assert call(q=None) == ARG
    assert call(L=8, S=9) == SHAPE and call(L=129, S=129) == SHAPE and call(d=24) == SHAPE and call(d=128) == SHAPE
    assert call(drop=0.1) == ARG and call(dtype=5) == DTYPE
    assert call(ld=30) == SHAPE and call(q=C.c_void_p(0x1004)) == ALIGN
    h = lib.psg_cosine_loss
    assert h(None, 8, P16, 8, None, 0, P16, 2, 8, 0, None) == ARG
    assert h(P16, 8, P16, 8, None, 0, P16, 2, 6, 0, None) == SHAPE and h(P16, 6, P16, 8, None, 0, P16, 2, 8, 0, None) == SHAPE
    assert h(P16, 8, P16, 8, P16, 4, P16, 2, 8, 0, None) == SHAPE and h(P16, 8, P16, 8, None, 0, P16, 2, 8, 3, None) == DTYPE


def test_unknown_activation_is_refused(lib):
    from pokemon_sprite_generator_amd import _lib
    assert _lib.ACT_QUICK_GELU == 5
    assert lib.psg_epilogue_bwd(P16, 8, P16, 8, P16, 8, 4, 8, 6, 1.0, 0.0, 0, 0, None) == ARG and b"act" in lib.psg_last_error()
    d = _lib.ConvDesc()
    d.x = d.w = d.y = 0x1000
    d.B, d.Hi, d.Wi, d.Cin, d.Ho, d.Wo, d.Cout = 1, 1, 1, 8, 1, 1, 8
    d.ksize, d.stride, d.pad, d.ldx, d.ldy, d.act = 1, 1, 0, 8, 8, 6
    assert lib.psg_conv_fwd_workspace_bytes(C.byref(d)) < 0 and b"act" in lib.psg_last_error()
    d.act = 5
    assert lib.psg_conv_fwd_workspace_bytes(C.byref(d)) >= 0


@pytest.mark.parametrize("case", list(R.LOSS_CASES))
def test_loss_cases_are_not_a_cancellation(case):
    """The loss cases rebuild text_projection so that the case's texts and images agree (clip_ref.loss_state_dict): every
    cosine is well away from 0, so the loss's relative error measures the arithmetic; nothing else of the state dict moves."""
    name = R.LOSS_CASES[case][0]
    sd, plain, cfg = R.loss_state_dict(case), R.state_dict(name), R.CONFIGS[name]
    assert [k for k in sd if not torch.equal(sd[k], plain[k])] == ["text_projection.weight"]
    assert torch.equal(sd["text_projection.weight"], R.bf16_exact(sd["text_projection.weight"]))
    img, ids = R.loss_inputs(case)
    cos = (F.normalize(R.vision(R.prep(img, cfg["vision_config"]["image_size"]), sd, cfg), dim=-1) * F.normalize(R.text(ids, sd, cfg), dim=-1)).sum(-1)
    assert float(cos.min()) > 0.5 and float(R.reference(("loss", case))["loss"]) < -0.5


# ---- the element-wise references, bounds and constants of tests/clip_cases.py ---------------------------------------------
from tests import attn_ref  # noqa: E402
from tests import clip_cases as KC  # noqa: E402

CLIP_REPORT = os.environ.get("PSG_CLIP_REPORT")      # optional: append the measured figures to this file


def _report(line):
    if CLIP_REPORT:
        with open(CLIP_REPORT, "a") as f:
            f.write(line + "\n")


def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("name", ["f32.d16.L1", "f32.d32.L3", "bf16.d16.L65", "f32.d64.L65.b1h1", "f32.d32.L77.hot", "f32.d64.L128"])
def test_causal_reference_is_sdpa_in_float64(name):
    import numpy as np
    c, r = KC.CAUSAL_BY_NAME[name], KC.causal_reference(name)
    B, L, H, d = c["B"], c["L"], c["heads"], c["d"]
    Q, Kk, V = (t.double().view(B, L, H, d).transpose(1, 2) for t in KC.causal_operands(name))
    sc = float(np.float32(c["scale"]))
    want = F.scaled_dot_product_attention(Q, Kk, V, is_causal=True, scale=sc).transpose(1, 2).reshape(B, L, H * d)
    assert float((r.o - want).abs().max()) <= 1e-13 * float(want.abs().max())
    s = (Q @ Kk.transpose(2, 3) * sc).masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), float("-inf"))
    assert float((r.lse - torch.logsumexp(s, -1)).abs().max()) <= 1e-12 * max(1.0, float(r.lse.abs().max()))
    assert torch.equal(r.o[:, 0], KC.causal_operands(name)[2][:, 0].double())            # row 0 is v[0]
    assert bool((r.o_mag >= 0).all()) and bool((r.lse_mag > 0).all())
    # the non-causal reference is untouched by the new argument
    qq, kk, vv = KC.causal_operands(name)
    full = attn_ref.reference(qq, kk, vv, H, c["scale"], attn_ref.VALU, False)
    assert torch.equal(full.o[:, L - 1], attn_ref.reference(qq, kk, vv, H, c["scale"], attn_ref.VALU, False, causal=True).o[:, L - 1])


def test_hot_causal_cases_need_the_running_maximum():
    """max |s| > 100 in every hot case: exp(s) alone overflows fp32 (at 88.7) - and does, evaluated that way."""
    import numpy as np
    hot = [c for c in KC.CAUSAL if c["hot"]]
    assert {(c["dtype"], c["d"]) for c in hot} == {(dn, d) for dn in KC.DTYPES for d in KC.CAUSAL_D} and all(c["L"] == 77 for c in hot)
    for c in hot:
        B, L, H, d = c["B"], c["L"], c["heads"], c["d"]
        Q, Kk, _ = (t.double().view(B, L, H, d).transpose(1, 2) for t in KC.causal_operands(c["name"]))
        s = (Q @ Kk.transpose(2, 3) * c["scale"]).masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), 0.0)
        assert float(s.max()) > 100.0 and float(s.min()) < -100.0, (c["name"], float(s.max()), float(s.min()))
        assert not bool(torch.isfinite(torch.exp(s.float())).all())


def test_causal_constant_is_four_times_the_measured_error():
    """C_CAUSAL = 4 x the larger of the smallest passing c of torch's fp32 masked softmax and of the header's sequential
    description in numpy fp32, each re-measured here within 25 %; both pass every case at C_CAUSAL by construction."""
    ct, at_t, cs, at_s = KC.measure_c_causal()
    _report(f"c_causal torch {ct:.4g} at {at_t}, sequential {cs:.4g} at {at_s}; recorded {R.C_CAUSAL_TORCH} / {R.C_CAUSAL_SEQ}, C_CAUSAL {R.C_CAUSAL:.4g}")
    assert abs(ct - R.C_CAUSAL_TORCH) <= REL_TOL * R.C_CAUSAL_TORCH, (ct, at_t)
    assert abs(cs - R.C_CAUSAL_SEQ) <= REL_TOL * R.C_CAUSAL_SEQ, (cs, at_s)
    assert R.C_CAUSAL == 4.0 * max(R.C_CAUSAL_TORCH, R.C_CAUSAL_SEQ)


def test_cosine_constant_is_four_times_torchs_own_error():
    c, at = KC.measure_c_cos()
    _report(f"c_cos torch {c:.4g} at {at}; recorded {R.C_COS_TORCH}, C_COS {R.C_COS:.4g}")
    assert abs(c - R.C_COS_TORCH) <= REL_TOL * R.C_COS_TORCH, (c, at)
    assert R.C_COS == 4.0 * R.C_COS_TORCH


@pytest.mark.parametrize("Hi,S,P", KC.PREP_SHAPES)
def test_prep_references_equal_autograd(Hi, S, P):
    """prep_fwd_ref / prep_bwd_ref against F.interpolate(antialias=True) and autograd in fp64, for every (a, b) of the table."""
    B = 3
    img, dy = KC.prep_operands(Hi, S, P, B)
    mean = torch.tensor(R.MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    inv = torch.tensor(R._inv_std(), dtype=torch.float64).view(1, 3, 1, 1)
    for a, b in KC.PREP_AB:
        a, b = R._f32(a), R._f32(b)
        x = img.double().requires_grad_(True)
        v = a * x + b
        if Hi != S:
            v = F.interpolate(v, size=(S, S), mode="bicubic", align_corners=False, antialias=True)
        rows = R.rows_of((v - mean) * inv, P)
        (rows * dy.double()).sum().backward()
        ref, mag = R.prep_fwd_ref(img, S, P, a, b)
        assert float((ref - rows.detach()).abs().max()) <= 1e-12 * float(mag.max())
        assert bool((mag >= ref.abs() * (1 - 1e-12)).all())
        g, M = R.prep_bwd_ref(dy, B, Hi, S, P, a)
        assert float((g - x.grad).abs().max()) <= 1e-12 * float(M.max()) and bool((M >= g.abs() * (1 - 1e-12)).all())
        if Hi == 1:                                      # every output is the one pixel: the full sum over all S * S outputs
            want = a * inv.view(1, 3) * R.pixels_of(dy.double(), B, S, P).sum((-1, -2))
            assert float((g.view(B, 3) - want).abs().max()) <= 1e-13 * float(M.max())
    assert torch.equal(R.pixels_of(R.rows_of(v.detach(), P), B, S, P), v.detach())


def test_prep_fp32_evaluation_in_the_headers_order_uses_under_half_the_bound():
    """K_PREP counts roundings; the numpy-fp32 evaluation in the header's order (the taps of a window row first, then the rows)
    must stay below half of K_PREP 2^-24 Mag on every case."""
    worst, at = 0.0, None
    for (Hi, S, P) in KC.PREP_SHAPES:
        for B in KC.PREP_BATCHES:
            img, _ = KC.prep_operands(Hi, S, P, B)
            for a, b in KC.PREP_AB:
                ref, mag = R.prep_fwd_ref(img, S, P, a, b)
                w = R.check_bound(R.prep_fwd_f32(img, S, P, a, b), ref, R.prep_fwd_bound(mag), f"prep {Hi}->{S} P{P} B{B} a{a} b{b}")
                if w > worst:
                    worst, at = w, (Hi, S, P, B, a, b)
    _report(f"prep_f32_header_order worst {worst:.4f} at {at} (K_PREP {R.K_PREP})")
    assert R.K_PREP == 17 and worst <= 0.5, (worst, at)


@pytest.mark.parametrize("kind", KC.COS_KINDS)
def test_cosine_reference_equals_autograd(kind):
    for B, D in ((5, 8), (9, 260), (2, 4)):
        u, v = KC.cosine_operands(B, D, kind, "f32")
        r = R.cosine_ref(u, v)
        out, du = R.cosine_torch(u, v, torch.float64)
        assert abs(float(out) - float(r.loss)) <= 1e-13
        assert float((du - r.du).abs().max()) <= 1e-12 * float(r.du.abs().max())
        assert bool((r.du_mag >= 0).all()) and float(r.loss_mag) > 0
        for row in KC.planted_rows(B):
            if kind == "tiny_u":
                assert 0.0 < float(r.nu[row]) < R.COS_EPS
                for dn in KC.DTYPES:                     # still below eps and not zero as a launch of either dtype reads it
                    assert 0.0 < float(KC.cosine_operands(B, D, kind, dn)[0][row].double().norm()) < R.COS_EPS
            if kind in ("zero_u", "tiny_u"):             # du = -v^ / (eps B): of order 1e12
                want = -(v[row].double() / v[row].double().norm()) / (R.COS_EPS * B)
                assert float((r.du[row] - want).abs().max()) <= 1e-12 * float(want.abs().max()) and float(want.abs().max()) > 1e10
            if kind == "zero_v":
                assert bool((r.du[row] == 0).all())
            if kind == "neg":
                assert abs(float(r.cos[row]) + 1.0) <= 1e-6


# ---- planted defects, each on the smallest case that shows it --------------------------------------------------------------
def _causal_emulate(name, defect=None):
    """psg_attn_fwd_causal in fp64 on the case's operands, stored like the launch's, with one defect."""
    c = KC.CAUSAL_BY_NAME[name]
    B, L, H, d = c["B"], c["L"], c["heads"], c["d"]
    Q, Kk, V = (t.double().view(B, L, H, d).transpose(1, 2) for t in KC.causal_operands(name))
    if defect == "head_neighbour":                       # head h reads K and V at head h - 1's offset
        Kk, V = Kk.roll(1, 1), V.roll(1, 1)
    live = torch.ones(L, L, dtype=torch.bool).tril()
    if defect == "diagonal_left_out":                    # s < l (row 0 keeps its one key)
        live = torch.ones(L, L, dtype=torch.bool).tril(-1)
        live[0, 0] = True
    if defect == "next_key_let_in":                      # s <= l + 1
        live = torch.ones(L, L, dtype=torch.bool).tril(1)
    s = (Q @ Kk.transpose(2, 3) * float(torch.tensor(c["scale"], dtype=torch.float32))).masked_fill(~live, float("-inf"))
    o = (torch.softmax(s, -1) @ V).transpose(1, 2).reshape(B, L, H * d)
    lse = torch.logsumexp(s, -1)
    if defect == "lse_without_maximum":
        lse = lse - s.amax(-1)
    if defect == "second_wave_zero":
        o[:, 64:], lse[:, :, 64:] = 0.0, 0.0
    return KC.causal_store(o, lse, name)


CAUSAL_DEFECTS = {"diagonal_left_out": "L2", "next_key_let_in": "L2", "head_neighbour": "L1", "second_wave_zero": "L65", "lse_without_maximum": "L1"}


@pytest.mark.parametrize("dn", list(KC.DTYPES))
@pytest.mark.parametrize("defect", sorted(CAUSAL_DEFECTS))
def test_causal_comparator_rejects_planted_defect(defect, dn):
    name = f"{dn}.d16.{CAUSAL_DEFECTS[defect]}"
    worst = KC.causal_check(*_causal_emulate(name), name, name)
    assert all(w <= 1.0 for w in worst.values())
    bad = _causal_emulate(name, defect)
    assert _fails(lambda: KC.causal_check(*bad, name, name)), f"{defect} passes at {name}"
    _report(f"defect causal {defect} rejected at {name}")


def _axis(n_in, n_out, how):
    """clip_ref.resize_matrix with one thing wrong."""
    if how == "cubic_a":
        return R.resize_matrix(n_in, n_out, -0.75)
    scale = n_in / n_out
    M = torch.zeros(n_out, n_in, dtype=torch.float64)
    for o in range(n_out):
        c = scale * (o + 0.5)
        lo, hi = max(int(c - 1.5), 0), min(int(c + 2.5), n_in)
        w = [R.keys_cubic(j + 0.5 - c, -0.5) for j in range(lo, hi)]
        tot = 1.0 if how == "no_renorm" else sum(w)
        for j, x in zip(range(lo, hi), w):
            jj = j + 1 if how == "shift" else j       # the window one sample further on
            if jj < n_in:
                M[o, jj] = x / tot
    return M


def _prep_emulate(Hi, S, P, B, a, b, defect=None):
    """(patch rows, dimg) in fp64 with one defect."""
    img, dy = KC.prep_operands(Hi, S, P, B)
    W = _axis(Hi, S, defect) if defect in ("cubic_a", "no_renorm", "shift") else None
    rows, _ = R.prep_fwd_ref(img, S, P, a, b, W)
    G = S // P
    if defect == "ky_kx_swapped":
        rows = rows.view(-1, 3, P, P).transpose(2, 3).reshape(-1, 3 * P * P)
    if defect == "wy_wx_swapped":                        # the x weights on the rows and the y weights on the columns: the transpose
        rows = R.rows_of(R.pixels_of(rows, B, S, P).transpose(2, 3).contiguous(), P)
    g = dy
    if defect == "bwd_neighbour_output":                 # the gather reads the dy of output ox + 1
        px = R.pixels_of(dy.double(), B, S, P)
        g = R.rows_of(torch.cat([px[..., 1:], px[..., -1:]], -1), P)
    dimg, _ = R.prep_bwd_ref(g, B, Hi, S, P, a)
    return rows.float(), dimg.float()


PREP_DEFECTS = {"cubic_a": (2, 16, 8), "no_renorm": (1, 16, 8), "shift": (1, 16, 8), "ky_kx_swapped": (2, 16, 8), "wy_wx_swapped": (2, 16, 8),
                "bwd_neighbour_output": (1, 16, 8)}


def _prep_verify(got, Hi, S, P, B, a, b):
    img, dy = KC.prep_operands(Hi, S, P, B)
    ref, mag = R.prep_fwd_ref(img, S, P, a, b)
    g, M = R.prep_bwd_ref(dy, B, Hi, S, P, a)
    return (R.check_bound(got[0], ref, R.prep_fwd_bound(mag), "prep fwd"), R.check_bound(got[1], g, R.prep_bwd_bound(M), "prep bwd"))


@pytest.mark.parametrize("defect", sorted(PREP_DEFECTS))
def test_prep_comparator_rejects_planted_defect(defect):
    Hi, S, P = PREP_DEFECTS[defect]
    assert (Hi, S, P) in KC.PREP_SHAPES
    a, b = KC.PREP_AB[0]
    assert max(_prep_verify(_prep_emulate(Hi, S, P, 1, a, b), Hi, S, P, 1, a, b)) <= 1.0
    bad = _prep_emulate(Hi, S, P, 1, a, b, defect)
    assert _fails(lambda: _prep_verify(bad, Hi, S, P, 1, a, b)), f"{defect} passes at {(Hi, S, P)}"
    if Hi == 2 and defect != "cubic_a":                  # ... and the smaller case cannot show it: one pixel, every output the same
        small = _prep_emulate(1, S, P, 1, a, b, defect)
        assert max(_prep_verify(small, 1, S, P, 1, a, b)) <= 1.0
    _report(f"defect prep {defect} rejected at {(Hi, S, P)}")


def _cosine_emulate(B, D, kind, dn, defect=None):
    u, v = (t.double() for t in KC.cosine_operands(B, D, kind, dn))
    n = (D // 256) * 256 if defect == "last_pass_dropped" and D > 256 and D % 256 else D
    nu, nv = u[:, :n].norm(dim=-1, keepdim=True), v[:, :n].norm(dim=-1, keepdim=True)
    den = nu.clamp_min(R.COS_EPS) * nv.clamp_min(R.COS_EPS)
    cos = (u[:, :n] * v[:, :n]).sum(-1, keepdim=True) / den
    rows = cos[:4] if defect == "second_row_dropped" else cos
    out = -rows.sum() / B
    gate = torch.ones_like(nu, dtype=torch.bool) if defect == "gate_missing" else nu > R.COS_EPS
    du = -(v / den - torch.where(gate, cos * u / (nu * nu).clamp_min(1e-300), torch.zeros_like(u)))
    if defect != "no_inv_b":
        du = du / B
    return out.float(), du.to(KC.DTYPES[dn])


COSINE_DEFECTS = {"second_row_dropped": (5, 4, "none"), "last_pass_dropped": (1, 260, "none"), "gate_missing": (2, 4, "tiny_u"), "no_inv_b": (2, 4, "none")}


@pytest.mark.parametrize("dn", list(KC.DTYPES))
@pytest.mark.parametrize("defect", sorted(COSINE_DEFECTS))
def test_cosine_comparator_rejects_planted_defect(defect, dn):
    B, D, kind = COSINE_DEFECTS[defect]
    assert B in KC.COS_B and D in KC.COS_D
    worst = KC.cosine_check(*_cosine_emulate(B, D, kind, dn), B, D, kind, dn, "clean")
    assert all(w <= 1.0 for w in worst.values())
    bad = _cosine_emulate(B, D, kind, dn, defect)
    assert _fails(lambda: KC.cosine_check(*bad, B, D, kind, dn, defect)), f"{defect} passes at {(B, D, kind)}"
    _report(f"defect cosine {defect} rejected at {dn} B{B} D{D} {kind}")


def test_cosine_comparator_wants_exact_zeros_for_a_zero_v_row():
    out, du = _cosine_emulate(5, 8, "zero_v", "f32")
    KC.cosine_check(out, du, 5, 8, "zero_v", "f32", "clean")
    du[4, 3] = 1e-30
    assert _fails(lambda: KC.cosine_check(out, du, 5, 8, "zero_v", "f32", "speck"))
