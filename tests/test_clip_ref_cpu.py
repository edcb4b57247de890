"""CPU suite for the CLIP loss: the float64 restatement the GPU tests compare against (tests/clip_ref.py) is held against
transformers' own CLIPModel and F.interpolate, the recorded precision baseline against a re-measurement, the comparator against
planted defects; plus what of `psg.CLIPLoss` needs no device: state-dict keys, from_pretrained, the text cleaning, the EOS
rules, argument validation."""
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
