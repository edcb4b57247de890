"""-m gpu: the sprite loader kernels (csrc/sprites.hip) against the fp64 specification and the reference chain on PIL
(tests/sprite_ref.py), their bitwise guarantees, and `create_data_loaders` end to end, down to one train step of
`ImprovedDiffusionTrainer` built without injected loaders.

Tolerances come from tests/sprite_ref.py and never from the kernels' output: the augment kernel is allowed 4 x the error
of the same specification evaluated in numpy fp32 (FP32_EVAL_MAX), the contrast mean (n_ambiguous * 255 + E) / S^2 with
E = 4 x FP32_SUM_ERR_MAX; ambiguous pixels (a rotation coordinate within 2e-4 of an integer) are left out, under a cap
of 1 % of a case's pixels."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import hashgen
from tests import sprite_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = R.all_cases()
SEMI = os.path.join(R.SPRITE_DIR, "descriptions_semicolon.csv")


@pytest.fixture(scope="module")
def D():
    from pokemon_sprite_generator_amd import _lib, data
    _lib.init(0)
    return data


def _inputs(name, S):
    r = R.reference(name, S)
    src = torch.from_numpy(np.array(R.fixture_array(S))).to(DEV)
    return r, src, torch.from_numpy(np.array(r["idx"])).to(DEV), torch.from_numpy(np.array(r["params"])).to(DEV)


def _normalised(u8_nhwc):
    """ToTensor + Normalize of stored pixels, on the CPU like the reference: ((u8.float() / 255) - 0.5) / 0.5."""
    x = u8_nhwc[..., :3].permute(0, 3, 1, 2).contiguous().cpu()
    return ((x.float() / 255) - 0.5) / 0.5


@pytest.mark.parametrize("name,S", CASES)
def test_contrast_mean_vs_fp64(D, name, S):
    r, src, idx, params = _inputs(name, S)
    got = D.contrast_mean(src, idx, params).cpu().double().numpy()
    E = 4.0 * R.FP32_SUM_ERR_MAX
    for k in range(5):
        if r["params"][k, 9] == 1:                    # no contrast op: the kernel may write anything
            continue
        bound = (int(r["namb"][k]) * 255.0 + E) / (S * S)
        err = abs(got[k] - r["mean"][k])
        print(f"{name} S={S} sample {k}: mean {r['mean'][k]:.6f} err {err:.3e} bound {bound:.3e} (ambiguous {int(r['namb'][k])})")
        assert r["namb"][k] <= R.AMBIG_CAP * S * S
        assert err <= bound, (name, S, k, err, bound)


@pytest.mark.parametrize("name,S", CASES)
def test_augment_vs_fp64(D, name, S):
    r, src, idx, params = _inputs(name, S)
    mean = torch.from_numpy(r["mean"].astype(np.float32)).to(DEV)          # the reference mean: the two kernels are judged separately
    got = D.augment(src, idx, params, mean=mean).cpu().double().numpy()
    assert got.shape == (5, 3, S, S)
    tol = 4.0 * R.FP32_EVAL_MAX
    for k in range(5):
        amb = r["ambig"][k]
        assert amb.mean() <= R.AMBIG_CAP, (name, S, k, amb.mean())
        err = np.abs(got[k] - r["out"][k])[:, ~amb].max()
        print(f"{name} S={S} sample {k}: max err {err:.3e} tol {tol:.3e} (ambiguous {amb.mean() * 100:.3f} %)")
        assert err <= tol, (name, S, k, err, tol)
    assert got.min() >= -1.0 and got.max() <= 1.0


@pytest.mark.parametrize("name,S", CASES)
def test_two_runs_are_bitwise_equal(D, name, S):
    _, src, idx, params = _inputs(name, S)
    m1, m2 = D.contrast_mean(src, idx, params), D.contrast_mean(src, idx, params)
    contrast = params[:, 9] != 1
    assert torch.equal(m1[contrast], m2[contrast])
    assert torch.equal(D.augment(src, idx, params, mean=m1), D.augment(src, idx, params, mean=m2))


def test_identity_is_bitwise_totensor_normalize(D):
    for S in (215, 33):
        src = torch.from_numpy(np.array(R.fixture_array(S))).to(DEV)
        idx = torch.tensor(R.IDX + [1, 1, 4], device=DEV)
        got = D.augment(src, idx, D.identity_params(len(idx), S, DEV))
        assert torch.equal(got.cpu(), _normalised(src[idx]))
        # the same row built by the case table and by draw-side code
        assert torch.equal(D.identity_params(1, S)[0], torch.from_numpy(R.make_row(S)))


@pytest.mark.parametrize("name,S", CASES)
def test_augment_vs_pil_chain(D, name, S):
    """The whole pipeline (the kernel's own mean) against the reference chain on PIL; the bound is the reference's measured
    uint8 quantisation plus the fp32 tolerance."""
    r, src, idx, params = _inputs(name, S)
    got = D.augment(src, idx, params).cpu().double().numpy()
    d = np.abs(got - R.pil_case(name, S).astype(np.float64))
    d[np.broadcast_to(r["ambig_pil"][:, None], d.shape)] = 0.0
    assert r["ambig_pil"].mean(axis=(1, 2)).max() <= R.AMBIG_CAP
    print(f"{name} S={S}: max |kernel - PIL chain| {d.max():.5f} bound {R.PIL_QUANT_MAX + 4 * R.FP32_EVAL_MAX:.5f}")
    assert d.max() <= R.PIL_QUANT_MAX + 4.0 * R.FP32_EVAL_MAX


def test_out_of_range_index_is_nan_not_a_fault(D):
    src = torch.from_numpy(np.array(R.fixture_array(33))).to(DEV)
    idx = torch.tensor([0, 8, -1, 7], device=DEV)
    params = torch.from_numpy(R.rows(R.cases(33)["all_contrast_middle"][:4], 33)).to(DEV)
    out = D.augment(src, idx, params)
    assert torch.isnan(out[1]).all() and torch.isnan(out[2]).all() and torch.isfinite(out[0]).all() and torch.isfinite(out[3]).all()


def test_host_wrappers_refuse_what_the_kernels_cannot_take(D):
    import pokemon_sprite_generator_amd as psg
    src = torch.zeros(2, 8, 8, 4, dtype=torch.uint8, device=DEV)
    idx, p = torch.zeros(3, dtype=torch.int64, device=DEV), D.identity_params(3, 8, DEV)
    with pytest.raises(psg.PsgError):
        D.augment(src.cpu(), idx.cpu(), p.cpu())
    with pytest.raises(psg.PsgError):
        D.augment(src[:, :, :, :3], idx, p)
    with pytest.raises(psg.PsgError):
        D.augment(src, idx.int(), p)
    with pytest.raises(psg.PsgError):
        D.augment(src, idx, p[:, :15])
    assert D.augment(src, idx, p).shape == (3, 3, 8, 8)


# ---- end to end ----------------------------------------------------------------------------------------------------------
def test_create_data_loaders_end_to_end(D):
    tr, va, te = D.create_data_loaders(SEMI, R.SPRITE_DIR, batch_size=2, val_split=0.25, test_split=0.13, seed=5)
    assert (len(tr), len(va), len(te)) == (2, 1, 1)
    ds = tr.dataset
    by_number = {r["national_number"]: k for k, r in enumerate(ds.rows)}

    def epoch(loader, e):
        loader.set_epoch(e)
        return list(loader)

    e0 = epoch(tr, 0)
    assert len(e0) == 2
    for b in e0:
        assert set(b) == {"image", "description", "full_description", "national_number", "name"}
        img = b["image"]
        assert img.shape == (2, 3, 215, 215) and img.dtype == torch.float32 and img.device == ds.device and img.is_cuda
        assert float(img.min()) >= -1.0 and float(img.max()) <= 1.0
        assert len(b["description"]) == len(b["full_description"]) == len(b["name"]) == 2 and b["national_number"].dtype == torch.int64
        for k in range(2):
            assert b["full_description"][k] == f"Pokemon named {b['name'][k]}. {b['description'][k]}."
    seen = [int(n) for b in e0 for n in b["national_number"]]
    assert len(set(seen)) == 4 and set(by_number[n] for n in seen) <= set(tr.indices)
    # the next iteration is the next epoch; the same seed and epoch give the same batches, from a loader built anew as well
    e1 = list(tr)
    assert tr.epoch == 2
    assert any(not torch.equal(a["image"], b["image"]) for a, b in zip(e0, e1))
    again = epoch(tr, 0)
    other = epoch(D.create_data_loaders(SEMI, R.SPRITE_DIR, batch_size=2, val_split=0.25, test_split=0.13, seed=5)[0], 0)
    for a, b, c in zip(e0, again, other):
        assert torch.equal(a["image"], b["image"]) and torch.equal(a["image"], c["image"])
        assert a["name"] == b["name"] == c["name"] and torch.equal(a["national_number"], c["national_number"])
    # val / test: sequential, un-augmented, bitwise ToTensor + Normalize of the stored pixels
    for loader in (va, te):
        batches = list(loader) + list(loader)                      # (the epoch does not matter)
        assert len(batches) == 2 * len(loader)
        got = torch.cat([b["image"] for b in batches[:len(loader)]])
        assert [int(n) for b in batches[:len(loader)] for n in b["national_number"]] == [ds.rows[k]["national_number"] for k in loader.indices]
        assert torch.equal(got.cpu(), _normalised(ds.images[torch.tensor(loader.indices, device=ds.device)]))


class _TextStub:
    def __call__(self, descriptions):
        rows = [hashgen.uniform((32, 256), 77, hashgen.name_id(d)) * math.sqrt(3.0) for d in descriptions]
        return torch.stack(rows).to(DEV)


class _VAEStub:
    """images [B, 3, 215, 215] -> (latent, mu, logvar) with [B, 8, 27, 27] latents that depend on the image."""

    def __call__(self, images):
        assert images.is_cuda and images.shape[1:] == (3, 215, 215)
        lat = torch.nn.functional.adaptive_avg_pool2d(images, 27)
        lat = torch.cat([lat, -lat, lat[:, :2] * 0.5], dim=1)
        return lat, lat, lat


def test_trainer_builds_its_own_loaders_and_trains_a_step(D, tmp_path):
    import pokemon_sprite_generator_amd as psg
    config = {
        "experiment_dir": str(tmp_path),
        "model": {"bert_model": "stub", "text_embedding_dim": 256, "latent_dim": 8, "num_timesteps": 1000, "beta_start": 0.0001, "beta_end": 0.02},
        "data": {"csv_path": SEMI, "image_dir": R.SPRITE_DIR, "batch_size": 2, "image_size": 215, "num_workers": 0, "pin_memory": False,
                 "val_split": 0.25, "test_split": 0.13},
        "training": {"diffusion_epochs": 1, "log_every": 1, "save_every": 1, "sample_every": 1000},
        "optimization": {"optimizer": "adamw", "learning_rate": 3e-4, "weight_decay": 0.01, "max_grad_norm": 1.0, "scheduler": "cosine"},
    }
    comps = {"text_encoder": _TextStub(), "vae_encoder": _VAEStub()}        # no "data_loaders": the trainer resolves its own
    tr = psg.ImprovedDiffusionTrainer(config, "unused.pth", "sprites", components=comps, compute_dtype=torch.bfloat16)
    assert isinstance(tr.data_loaders["train"], D.SpriteLoader) and tr._component("create_data_loaders") is D.create_data_loaders
    assert (len(tr.data_loaders["train"]), len(tr.data_loaders["val"]), len(tr.data_loaders["test"])) == (2, 1, 1)
    tr.data_loaders["train"].indices = tr.data_loaders["train"].indices[:2]   # one step: the smallest batch, once
    m = tr.train_epoch(0)
    assert math.isfinite(m["train_loss"]) and m["train_loss"] > 0
    assert tr.optimizer.steps_done() == 1
