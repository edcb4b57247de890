"""CPU suite for the imaging end of the generation path: the numpy restatement of PIL's 8-bit LANCZOS resample against PIL
itself (0 mismatching bytes), `imaging.lanczos_coeffs` against the restatement's tables entry for entry, host-side argument
validation of the three new entry points, and CPU tensors refused."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import imaging_ref as R


@pytest.fixture(scope="module")
def lib():
    from pokemon_sprite_generator_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def _pil_resize(img_hwc, out_hw):
    Image = pytest.importorskip("PIL.Image")
    mode = {1: "L", 3: "RGB", 4: "CMYK"}[img_hwc.shape[2]]            # (CMYK: four plain channels - RGBA would premultiply)
    pil = Image.fromarray(img_hwc[:, :, 0] if mode == "L" else img_hwc, mode)
    out = np.asarray(pil.resize((out_hw[1], out_hw[0]), Image.Resampling.LANCZOS))
    return out[:, :, None] if mode == "L" else out


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_restatement_matches_pil(name):
    pytest.importorskip("PIL")
    img, out_hw = R.content(name), R.SHAPES[name][4]
    got = R.resample(img, out_hw)
    assert got.shape == (img.shape[0],) + tuple(out_hw) + (img.shape[3],) and got.dtype == np.uint8
    for b in range(img.shape[0]):
        want = _pil_resize(img[b], out_hw)
        assert int((got[b] != want).sum()) == 0, f"{name}[{b}]: {(got[b] != want).sum()} bytes differ from PIL"
    if name in ("up_7x5", "up_96", "c4_b2"):
        assert got.min() == 0 and got.max() == 255                     # (an upscale of 0 / 255 content overshoots into both clamps)


def test_restatement_single_channel_matches_pil():
    pytest.importorskip("PIL")
    img = R.content("up_96")[:, :, :, :1]
    assert int((R.resample(img, (50, 131))[0] != _pil_resize(img[0], (50, 131))).sum()) == 0


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_lanczos_coeffs_equal_the_restatement(name):
    from pokemon_sprite_generator_amd import imaging
    H, W, _, _, (Hout, Wout) = R.SHAPES[name]
    for n_in, n_out in ((W, Wout), (H, Hout)):
        want, got = R.coeff_tables(n_in, n_out), imaging.lanczos_coeffs(n_in, n_out)
        if n_in == n_out:
            assert want is None and got is None
            continue
        assert got[2] == want[2]
        for g, w in zip(got[:2], want[:2]):
            assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w)
        bounds, coef, kmax = got
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds[:, 0] + bounds[:, 1] <= n_in).all()
        assert bounds[:, 1].max() <= kmax and all((coef[i, n:] == 0).all() for i, n in enumerate(bounds[:, 1]))
        assert (np.abs(coef.sum(1) - (1 << 22)) <= kmax).all()         # every row sums to one, up to its taps' roundings
    assert imaging.lanczos_coeffs(4096, 215)[2] == 117                 # the table width of a 4096-wide input


def test_lanczos_coeffs_rejects_bad_sizes():
    from pokemon_sprite_generator_amd import imaging
    with pytest.raises(ValueError):
        imaging.lanczos_coeffs(0, 215)
    with pytest.raises(ValueError):
        imaging.lanczos_coeffs(215, -1)


def _i32(a):
    a = np.ascontiguousarray(a, np.int32)
    return a, a.ctypes.data


def test_resample_validation_without_gpu(lib):
    """psg_resample_u8 rejects bad arguments on the host, before any launch (no device is needed to get the code)."""
    P = 0x1000                                                          # a non-null stand-in: never dereferenced on these paths
    keep, xb = _i32([[0, 3], [1, 3]])                                   # 4 -> 2 columns, table width 3
    keep2, yb = _i32([[0, 2]] * 3)                                      # 2 -> 3 rows, table width 2

    def call(src=P, u8=P, f32=0, lut=0, B=1, Hin=2, Win=4, Cc=3, Hout=3, Wout=2, xbh=xb, xbd=P, xc=P, kx=3, ybh=yb, ybd=P, yc=P, ky=2,
             ws=P, ws_bytes=1 << 20):
        return lib.psg_resample_u8(src, u8, f32, lut, B, Hin, Win, Cc, Hout, Wout, xbh, xbd, xc, kx, ybh, ybd, yc, ky, ws, ws_bytes, None)

    assert call(src=0) == -6 and b"null" in lib.psg_last_error()
    assert call(u8=0, f32=0) == -6
    assert call(f32=P, lut=0) == -6                                     # the fp32 output without its table
    assert call(f32=P, lut=P, Cc=2) == -6                               # ... or with fewer than three channels
    assert call(xbd=0) == -6 and call(xc=0) == -6 and call(ybh=0) == -6 and call(yc=0) == -6
    for kw in ({"B": 0}, {"Hin": 0}, {"Win": -1}, {"Hout": 0}, {"Wout": 0}, {"Cc": 0}, {"Cc": 5}, {"kx": -1}, {"ky": -2},
               {"kx": 0}, {"ky": 0}, {"B": 70000}, {"Hin": 1 << 20}):      # (a skipped pass between different sizes)
        assert call(**kw) == -1, kw
    assert b"skipped" in lib.psg_last_error() or b"large" in lib.psg_last_error()
    for bad in ([[0, 3], [2, 3]], [[-1, 3], [1, 3]], [[0, 4], [1, 3]], [[0, 3], [1, -1]], [[4, 1], [1, 3]]):
        k, p = _i32(bad)
        assert call(xbh=p) == -1 and b"horizontal bounds row" in lib.psg_last_error(), bad
    k, p = _i32([[0, 2], [0, 2], [1, 2]])
    assert call(ybh=p) == -1 and b"vertical bounds row 2" in lib.psg_last_error()
    assert call(ws=0) == -4 and call(ws_bytes=1 * 2 * 2 * 3 - 1) == -4
    del keep, keep2


def test_image_to_u8_and_latent_mix_validation_without_gpu(lib):
    P = 0x1000
    assert lib.psg_image_to_u8(0, 1, 1, 1, 1, P, 1, 2, 2, None) == -6 and b"null" in lib.psg_last_error()
    assert lib.psg_image_to_u8(P, 1, 1, 1, 1, 0, 1, 2, 2, None) == -6
    for B, H, W in ((0, 2, 2), (1, 0, 2), (1, 2, -3), (70000, 2, 2), (1, 70000, 2)):
        assert lib.psg_image_to_u8(P, 12, 4, 2, 1, P, B, H, W, None) == -1
    assert lib.psg_image_to_u8(P, 12, -4, 2, 1, P, 1, 2, 2, None) == -1 and b"stride" in lib.psg_last_error()
    assert lib.psg_latent_mix_f32(0, P, 0.5, 0.5, P, 8, None) == -6
    assert lib.psg_latent_mix_f32(P, 0, 0.5, 0.5, P, 8, None) == -6
    assert lib.psg_latent_mix_f32(P, P, 0.5, 0.5, 0, 8, None) == -6
    assert lib.psg_latent_mix_f32(P, P, 0.5, 0.5, P, 0, None) == -1 and lib.psg_latent_mix_f32(P, P, 0.5, 0.5, P, -4, None) == -1


def test_cpu_tensors_are_refused():
    import pokemon_sprite_generator_amd as psg
    from pokemon_sprite_generator_amd import imaging
    with pytest.raises(psg.PsgError):
        imaging.resize_lanczos(torch.zeros(7, 5, 3, dtype=torch.uint8))
    with pytest.raises(psg.PsgError):
        imaging.to_uint8(torch.zeros(1, 3, 4, 4))
    with pytest.raises(psg.PsgError):
        imaging.mix_latent(torch.zeros(1, 8, 27, 27), torch.zeros(1, 8, 27, 27), 0.7)
    with pytest.raises(psg.PsgError):
        imaging.pil_to_tensor(np.zeros((7, 5, 3), np.uint8), device="cpu")
    assert psg.SpriteGenerator.__module__ == "pokemon_sprite_generator_amd.generate"


def test_host_restatements_of_the_pointwise_ops():
    """The references the GPU tests compare with, on values whose result is known."""
    img = torch.tensor([-1.0, -0.5, 0.0, 1.0, 3.0, -3.0, float("inf"), float("-inf"), -0.99, 0.99, 0.999, 0.0])
    got = R.image_to_u8(img.reshape(3, 2, 2))
    assert got.shape == (2, 2, 3) and got.dtype == np.uint8
    assert got.transpose(2, 0, 1).reshape(-1).tolist() == [0, 63, 127, 255, 255, 0, 255, 0, 1, 253, 254, 127]
    a, b = torch.full((4,), 2.0), torch.full((4,), -1.0)
    assert torch.equal(R.mix(a, b, 0.0), a) and torch.equal(R.mix(a, b, 1.0), b)
    n = R.normalise(np.array([[[[0, 255, 51, 9]]]], np.uint8))
    assert n.shape == (1, 3, 1, 1) and n.reshape(-1).tolist() == [-1.0, 1.0, float((np.float32(51) / np.float32(255) - np.float32(0.5)) * np.float32(2))]
