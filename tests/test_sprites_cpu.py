"""CPU suite of the sprite loader (pokemon_sprite_generator_amd/data.py, csrc/sprites.hip): CSV parsing, description
strings, the split, loader lengths, the augmentation draws, the float specification against the reference chain on PIL
(tests/sprite_ref.py), and the new ABI entries' argument validation.  Nothing here launches a kernel."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests import sprite_ref as R

SEMI = os.path.join(R.SPRITE_DIR, "descriptions_semicolon.csv")
TAB = os.path.join(R.SPRITE_DIR, "pokemon_tab.csv")


@pytest.fixture(scope="module")
def data():
    from pokemon_sprite_generator_amd import data as D
    return D


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


# ---- CSV, descriptions, files ----------------------------------------------------------------------------------------
def test_semicolon_csv_is_numbered_from_one(data):
    rows = data.read_rows(SEMI)
    assert [r["national_number"] for r in rows] == list(range(1, 11))
    assert rows[0]["english_name"] == "Bulbasaur" and rows[3]["english_name"] == "Charmander"
    assert rows[0]["description"].startswith(" A squat, dinosaur-like creature")       # (stripped by clean_description)


def test_tab_csv_with_header_drops_rows_without_description(data):
    rows = data.read_rows(TAB)                                   # utf-16 with a byte-order mark, row 6 has no description
    assert [r["national_number"] for r in rows] == [1, 2, 3, 4, 5, 7, 8, 9, 10]
    assert rows[0]["english_name"] == "Bulbasaur" and "seed on its back" in rows[0]["description"]


@pytest.mark.parametrize("encoding", ["utf-8", "utf-16", "latin-1"])
@pytest.mark.parametrize("shape", ["semicolon", "tab"])
def test_three_encodings_two_shapes(data, tmp_path, encoding, shape):
    name, desc = "Flabébé", "Pokémon of the café; small"        # (the `;` inside quotes must not split the field)
    if shape == "semicolon":
        text = f'Pikachu; a mouse\n{name};"{desc}"\nNodesc;\n'
    else:
        text = f"national_number\tgen\tenglish_name\tdescription\n25\tI\tPikachu\t a mouse\n669\tVI\t{name}\t{desc}\n7\tI\tNodesc\t\n"
    p = tmp_path / "d.csv"
    p.write_bytes(text.encode(encoding))
    rows = data.read_rows(str(p))
    assert [r["english_name"] for r in rows] == ["Pikachu", name]
    assert rows[1]["description"] == desc
    assert [r["national_number"] for r in rows] == ([1, 2] if shape == "semicolon" else [25, 669])


def test_missing_columns_raise(data, tmp_path):
    p = tmp_path / "d.csv"
    p.write_text("national_number\tname\n1\tx\n")
    with pytest.raises(ValueError, match="Missing required columns"):
        data.read_rows(str(p))


def test_description_strings(data):
    assert data.clean_description('  "A quoted one."  ') == "A quoted one."
    assert data.clean_description(" plain ") == "plain"
    assert data.clean_description('"') == ""                                            # the reference's slice does the same
    assert data.create_full_description("Mew", ' "Pink." ') == "Pokemon named Mew. Pink.."
    assert data.create_full_description("Mew", "  ") == "Pokemon named Mew."


def test_dataset_filters_missing_files_and_composites(data):
    ds = data.SpriteDataset(SEMI, R.SPRITE_DIR, device="cpu")
    assert [r["national_number"] for r in ds.rows] == R.FIXTURE_NUMBERS                 # 004.png and 010.png do not exist
    assert tuple(ds.images.shape) == (8, 215, 215, 4) and ds.images.dtype == torch.uint8
    assert np.array_equal(ds.images.numpy(), R.fixture_array(215))
    m = ds.meta(3)
    assert m["national_number"] == 5 and m["name"] == "Charmeleon" and m["full_description"].startswith("Pokemon named Charmeleon. ")
    assert m["description"] == m["description"].strip() and m["full_description"].endswith(".")
    from PIL import Image
    rgba = np.asarray(Image.open(os.path.join(R.SPRITE_DIR, "001.png")).convert("RGBA")).astype(np.int64)
    part = (rgba[..., 3] > 0) & (rgba[..., 3] < 255)
    assert part.sum() > 100                                                              # a fixture with partial alpha
    want = (rgba[..., :3] * rgba[..., 3:] + 255 * (255 - rgba[..., 3:])) / 255.0
    assert np.abs(ds.images.numpy()[0, :, :, :3] - want).max() <= 1.0                    # composited on white
    black = data.SpriteDataset(SEMI, R.SPRITE_DIR, device="cpu", background_color="black")
    assert black.images[0, 0, 0, :3].tolist() == [0, 0, 0] and ds.images[0, 0, 0, :3].tolist() == [255, 255, 255]
    with pytest.raises(FileNotFoundError):
        data.SpriteDataset(SEMI, R.SPRITE_DIR, device="cpu", filter_missing=False)


def test_other_modes_and_sizes_are_composited_and_resized_once(data, tmp_path):
    from PIL import Image
    rng = np.random.default_rng(0)
    la = Image.fromarray(rng.integers(0, 256, (20, 20, 2), dtype=np.uint8), "LA")
    idx = rng.integers(0, 4, (40, 40), dtype=np.uint8)
    idx[:20, :20] = 0                                        # a block of the transparent entry
    pal = Image.fromarray(idx, "P")
    pal.putpalette([255, 0, 0, 0, 255, 0, 0, 0, 255, 9, 9, 9])
    rgb = Image.fromarray(rng.integers(0, 256, (20, 20, 3), dtype=np.uint8), "RGB")
    la.save(tmp_path / "001.png"); pal.save(tmp_path / "002.png", transparency=0); rgb.save(tmp_path / "003.png")
    (tmp_path / "d.csv").write_text("a;x\nb;y\nc;z\n")
    ds = data.SpriteDataset(str(tmp_path / "d.csv"), str(tmp_path), image_size=20, device="cpu", background_color=(10, 20, 30))
    for k, n in enumerate(("001", "002", "003")):
        ref = R.composite(str(tmp_path / f"{n}.png"), (10, 20, 30))
        if ref.size != (20, 20):
            ref = ref.resize((20, 20), Image.BILINEAR)
        assert np.array_equal(ds.images[k, :, :, :3].numpy(), np.asarray(ref)), n
    assert (ds.images[1, :, :, :3].numpy().reshape(-1, 3) == (10, 20, 30)).all(1).any()   # the transparent palette entry


# ---- split and loaders -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total,val,test,seed", [(898, 0.1, 0.1, 42), (8, 0.15, 0.05, 7), (101, 0.2, 0.0, 0)])
def test_split_equals_random_split(data, total, val, test, seed):
    tr, va, te = data.split_indices(total, val, test, seed)
    sizes = [total - int(total * val) - int(total * test), int(total * val), int(total * test)]
    ref = torch.utils.data.random_split(range(total), sizes, generator=torch.Generator().manual_seed(seed))
    assert [tr, va, te] == [list(p.indices) for p in ref]
    assert sorted(tr + va + te) == list(range(total))


def test_loader_lengths_and_contract(data):
    tr, va, te = data.create_data_loaders(SEMI, R.SPRITE_DIR, batch_size=3, val_split=0.25, test_split=0.13, device="cpu")
    assert (len(tr.indices), len(va.indices), len(te.indices)) == (5, 2, 1)
    assert (len(tr), len(va), len(te)) == (1, 1, 1)                        # 5 // 3 with drop_last; ceil(2 / 3); ceil(1 / 3)
    assert tr.augment and tr.drop_last and not va.augment and not va.drop_last
    ds = tr.dataset
    assert len(data.SpriteLoader(ds, range(8), 3, augment=False, drop_last=False)) == 3
    assert len(data.SpriteLoader(ds, range(8), 3, augment=True, drop_last=True)) == 2
    assert len(data.SpriteLoader(ds, [], 3, augment=False, drop_last=False)) == 0
    import pokemon_sprite_generator_amd as psg
    assert psg.create_data_loaders is data.create_data_loaders
    with pytest.raises(psg.PsgError):                                      # batches are made by the kernels or not at all
        next(iter(va))


# ---- the draws ---------------------------------------------------------------------------------------------------------
def test_draw_params_ranges_and_crop_validity(data):
    S, B = 215, 4096
    p = data.draw_params(B, S, generator=torch.Generator().manual_seed(1)).double()
    assert p.shape == (B, 16) and data.draw_params(3, S).dtype == torch.float32
    assert set(p[:, 0].tolist()) == {0.0, 1.0} and 0.45 < p[:, 0].mean() < 0.55
    assert set(p[:, 7].tolist()) == set(float(k) for k in range(24))
    for k in (8, 9, 10):
        assert 0.9 - 1e-6 <= p[:, k].min() < 0.91 and 1.09 < p[:, k].max() <= 1.1 + 1e-6
    assert -0.05 - 1e-7 <= p[:, 11].min() < -0.045 and 0.045 < p[:, 11].max() <= 0.05 + 1e-7
    i, j, h, w = (p[:, k] for k in (12, 13, 14, 15))
    assert (p[:, 12:] == p[:, 12:].round()).all()
    assert (i >= 0).all() and (j >= 0).all() and (h > 0).all() and (w > 0).all() and (i + h <= S).all() and (j + w <= S).all()
    assert h.min() >= math.floor(0.9 * S) and (i > 0).any() and (j > 0).any()
    # the rotation is PIL's matrix of an angle in [-10, 10]: a = e = cos, b = -d = sin(-angle), centre S / 2 fixed
    a, b, c, d, e, f = (p[:, k] for k in range(1, 7))
    assert torch.allclose(a, e) and torch.allclose(b, -d) and torch.allclose(a * a + b * b, torch.ones_like(a), atol=1e-6)
    ang = torch.rad2deg(torch.atan2(d, a))
    assert -10 - 1e-4 <= ang.min() < -9.5 and 9.5 < ang.max() <= 10 + 1e-4
    assert torch.allclose(a * S / 2 + b * S / 2 + c, torch.full_like(a, S / 2), atol=1e-4)
    assert torch.allclose(d * S / 2 + e * S / 2 + f, torch.full_like(a, S / 2), atol=1e-4)
    # seeded: the same generator state gives the same rows
    q = data.draw_params(B, S, generator=torch.Generator().manual_seed(1)).double()
    assert torch.equal(p, q)


def test_rotation_coefficients_are_pils(data):
    angles = [0.0, 3.0, 7.3, 10.0, -10.0, -7.3, 1e-3]
    for S in (215, 33):
        got = data.rotation_coefficients(torch.tensor(angles, dtype=torch.float64), S)
        want = torch.tensor([R.rotation_coeffs(a, S) for a in angles], dtype=torch.float64)
        assert torch.allclose(got, want, rtol=0, atol=1e-12)
        assert torch.equal(got.float()[0], torch.tensor([1.0, 0, 0, 0, 1, 0]))
    assert torch.equal(data.identity_params(2, 215)[1], torch.from_numpy(R.make_row(215)))


def test_first_valid_of_ten_equals_a_python_loop(data):
    S, B = 215, 2000
    w, h = data.crop_candidates(B, S, generator=torch.Generator().manual_seed(3))
    assert w.shape == (B, 10) and ((w > S) | (h > S)).any() and ((w <= S) & (h <= S)).any()
    ui, uj = torch.rand(B, dtype=torch.float64), torch.rand(B, dtype=torch.float64)
    i, j, hs, ws = data.pick_crop(w, h, S, ui, uj)
    for n in range(B):
        want = (S, S)
        for k in range(10):
            if 0 < w[n, k] <= S and 0 < h[n, k] <= S:
                want = (int(w[n, k]), int(h[n, k]))
                break
        assert (int(ws[n]), int(hs[n])) == want
        assert int(i[n]) == min(int(float(ui[n]) * (S - want[1] + 1)), S - want[1]) and int(j[n]) == min(int(float(uj[n]) * (S - want[0] + 1)), S - want[0])
    # candidates are round(sqrt(area * ratio)) of an area in [0.9, 1] S^2 and a ratio in [0.9, 1.1]
    assert w.min() >= round(S * math.sqrt(0.81)) - 1 and w.max() <= round(S * math.sqrt(1.1)) + 1
    assert ((w * h).double() / (S * S)).min() > 0.88 and ((w * h).double() / (S * S)).max() < 1.02


def test_fallback_fires_only_when_all_ten_fail(data):
    S = 215
    bad, good = torch.full((10,), S + 1), torch.full((10,), 200)
    w = torch.stack([bad, bad, torch.cat([bad[:9], good[:1]]), good, torch.zeros(10, dtype=torch.int64)])
    h = torch.stack([good, bad, torch.cat([bad[:9], good[:1]]), good, good])
    h[2, :9] = 200                                           # row 2: nine tries fail on w alone, the tenth is valid
    u = torch.full((5,), 0.999999, dtype=torch.float64)
    i, j, hs, ws = data.pick_crop(w, h, S, u, u)
    assert ws.tolist() == [S, S, 200, 200, S] and hs.tolist() == [S, S, 200, 200, S]      # rows 0, 1, 4: the whole image
    assert i.tolist() == [0, 0, 15, 15, 0] and j.tolist() == [0, 0, 15, 15, 0]            # the largest offsets: i + h = S


# ---- the specification against the reference chain ---------------------------------------------------------------------
def test_ambiguous_pixels_stay_under_the_cap():
    for name, S in R.all_cases():
        r = R.reference(name, S)
        for k in range(5):
            assert r["ambig"][k].mean() <= R.AMBIG_CAP and r["ambig_pil"][k].mean() <= R.AMBIG_CAP, (name, S, k)
    assert max(R.reference(n, 33)["ambig"].mean() for n in R.cases(33)) == 0.0
    assert 0.003 < R.reference("rotate", 215)["ambig"].mean(axis=(1, 2)).max() < 0.004


def test_fixed_point_map_is_what_pil_rotates_by():
    """sprite_ref.pil_fixed_map is not a guess: it reproduces Image.rotate(NEAREST) pixel for pixel."""
    from PIL import Image
    for S, angles in ((215, (3.0, 7.3, 10.0, -10.0, -7.3)), (33, (3.0, 10.0, -10.0))):
        img = R.fixture_images(S)[2]
        a = np.asarray(img)
        for ang in angles:
            sx, sy, inside = R.pil_fixed_map(ang, S)
            emu = np.where(inside[..., None], a[np.clip(sy, 0, S - 1), np.clip(sx, 0, S - 1)], 0)
            assert np.array_equal(emu, np.asarray(img.rotate(ang, Image.NEAREST, False, None, fillcolor=(0, 0, 0))))
            n = int(R.pil_floor_differs(ang, R.make_row(S, angle=ang), S).sum())
            assert n <= 0.005 * S * S, (S, ang, n)           # 16.16 rounding moves a few boundaries, not the rotation


def test_specification_equals_pil_chain_up_to_its_quantisation():
    """max |fp64 specification - PIL chain| over fixtures x cases, ambiguous pixels excluded.  Measured: 0.0793 in output
    units (10.1 levels; all ops with contrast first), the one-op cases 0.0078 (one level) except hue, 0.0596.  The limit
    16/255*2 = 0.1255 was fixed before measuring: above it the restatement is wrong."""
    worst, per_case = 0.0, {}
    for name, S in R.all_cases():
        r = R.reference(name, S)
        d = np.abs(R.pil_case(name, S).astype(np.float64) - r["out"])
        d[np.broadcast_to(r["ambig_pil"][:, None], d.shape)] = 0.0
        per_case[(name, S)] = float(d.max())
        worst = max(worst, per_case[(name, S)])
    print("spec vs PIL chain, max per case:", {k: round(v, 5) for k, v in per_case.items()})
    assert worst <= R.QUANT_LIMIT, per_case
    for name in ("identity", "flip", "rotate"):              # no arithmetic on pixel values: only pil_chain's fp32 normalise differs
        assert per_case[(name, 215)] <= 1e-7, name
    assert worst <= R.PIL_QUANT_MAX and worst > 0.99 * R.PIL_QUANT_MAX, worst       # the recorded constant is the measured one


def test_recorded_fp32_constants_are_the_measured_ones():
    e_aug, e_sum = R.measure_fp32()
    print("fp32 vs fp64 evaluation of the specification:", e_aug, "luma sum:", e_sum)
    assert e_aug <= R.FP32_EVAL_MAX and e_aug > 0.95 * R.FP32_EVAL_MAX
    assert 0.5 * R.FP32_SUM_ERR_MAX <= e_sum <= R.FP32_SUM_ERR_MAX          # (numpy's pairwise order may differ between builds)


def test_identity_specification_is_totensor_normalize():
    r = R.reference("identity", 215)
    src = torch.from_numpy(R.fixture_array(215)[R.IDX][..., :3].copy()).permute(0, 3, 1, 2)
    want = ((src.float() / 255) - 0.5) / 0.5
    assert np.array_equal(r["out32"], want.numpy())


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_sprite_entries_reject_bad_arguments_without_gpu(lib):
    ok = 0x1000
    assert lib.psg_sprite_augment(None, 8, ok, ok, ok, ok, 4, 215, None) == -6
    assert b"null" in lib.psg_last_error()
    for bad in range(6):
        args = [ok] * 5
        if bad < 5:
            args[bad if bad < 1 else bad] = None
            a = [args[0], 8, args[1], args[2], args[3], args[4], 4, 215, None]
            assert lib.psg_sprite_augment(*a) == -6, bad
    assert lib.psg_sprite_contrast_mean(ok, 8, None, ok, ok, 4, 215, None) == -6
    assert lib.psg_sprite_contrast_mean(ok, 8, ok, None, ok, 4, 215, None) == -6
    assert lib.psg_sprite_contrast_mean(ok, 8, ok, ok, None, 4, 215, None) == -6
    for N, B, S in ((0, 4, 215), (8, 0, 215), (8, 4, 0), (-1, 4, 215), (8, -2, 215), (8, 4, -215), (8, 4, 5000), (8, 70000, 215)):
        assert lib.psg_sprite_augment(ok, N, ok, ok, ok, ok, B, S, None) == -1, (N, B, S)
        assert lib.psg_sprite_contrast_mean(ok, N, ok, ok, ok, B, S, None) == -1, (N, B, S)
    assert lib.psg_sprite_augment(ok + 2, 8, ok, ok, ok, ok, 4, 215, None) == -3       # the source is read a dword per pixel
