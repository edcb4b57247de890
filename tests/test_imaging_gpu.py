"""-m gpu: the imaging kernels (csrc/imaging.hip) bit for bit - psg_resample_u8 against the numpy restatement of PIL's 8-bit
LANCZOS resample (tests/imaging_ref.py) and against PIL itself with 0 mismatching bytes, its fused fp32 output against the
reference's ToTensor + normalise on the CPU, psg_image_to_u8 against tensor_to_pil's numpy chain, psg_latent_mix_f32 against
torch on the CPU."""
import functools

import numpy as np
import pytest
import torch

from tests import imaging_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def imaging():
    from pokemon_sprite_generator_amd import _lib, imaging as m
    _lib.init(0)
    return m


@functools.lru_cache(maxsize=None)
def _expected(name):
    """(input, restatement's bytes) of a shape, computed once and shared (read-only) by the tests that need it."""
    img = R.content(name)
    want = R.resample(img, R.SHAPES[name][4])
    img.setflags(write=False), want.setflags(write=False)
    return img, want


def _mismatches(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return int((got != want).sum())


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_resample_equals_the_restatement_and_pil(imaging, name):
    img, want = _expected(name)
    Hout, Wout = R.SHAPES[name][4]
    u8, f32 = imaging.resize_lanczos(torch.from_numpy(img.copy()).to(DEV), (Wout, Hout), normalize="both")
    got = u8.cpu().numpy()
    bad = _mismatches(got, want)
    print(f"{name}: {bad} of {want.size} bytes differ from the restatement")
    assert bad == 0
    assert torch.equal(f32.cpu(), R.normalise(want)), "fp32 output is not ((u8 / 255.0) - 0.5) * 2 bit for bit"
    try:
        from PIL import Image
    except ImportError:
        return
    mode = {3: "RGB", 4: "CMYK"}[img.shape[3]]                          # (CMYK: four plain channels - RGBA would premultiply)
    for b in range(img.shape[0]):
        pil = np.asarray(Image.fromarray(img[b], mode).resize((Wout, Hout), Image.Resampling.LANCZOS))
        assert _mismatches(got[b], pil) == 0, f"{name}[{b}] differs from PIL"


def test_each_output_alone_and_a_3d_input(imaging):
    """Either output may be absent (a null pointer in the launch); a [H, W, C] input gives results without the batch dimension."""
    img, want = _expected("near_identity")
    src = torch.from_numpy(img.copy()).to(DEV)
    u8 = imaging.resize_lanczos(src, (215, 215), normalize=False)
    f32 = imaging.resize_lanczos(src, (215, 215), normalize=True)
    assert u8.dtype == torch.uint8 and _mismatches(u8.cpu().numpy(), want) == 0
    assert f32.shape == (1, 3, 215, 215) and torch.equal(f32.cpu(), R.normalise(want))
    one = imaging.resize_lanczos(src[0], (215, 215), normalize=True)
    assert one.shape == (3, 215, 215) and torch.equal(one, f32[0])
    img7, want7 = _expected("identity")
    f7 = imaging.resize_lanczos(torch.from_numpy(img7.copy()).to(DEV), (215, 215))         # the copy path, fp32 only
    assert torch.equal(f7.cpu(), R.normalise(img7)) and np.array_equal(img7, want7)


def test_resample_from_an_odd_base_address(imaging):
    """Byte loads only: an image that starts at an odd address inside a larger buffer (rows of 111 bytes) gives the same bytes."""
    img, want = _expected("odd_stride")
    buf = torch.zeros(img.size + 3, dtype=torch.uint8, device=DEV)
    for off in (1, 3):
        view = buf[off:off + img.size].view(img.shape)
        view.copy_(torch.from_numpy(img.copy()))
        assert view.data_ptr() % 2 == 1 and view.is_contiguous()
        assert _mismatches(imaging.resize_lanczos(view, (215, 215), normalize=False).cpu().numpy(), want) == 0


def test_one_and_two_channel_images(imaging):
    img = R.content("up_96")
    for C in (1, 2):
        sub = np.ascontiguousarray(img[..., :C])
        got = imaging.resize_lanczos(torch.from_numpy(sub).to(DEV), (131, 50), normalize=False).cpu().numpy()
        assert _mismatches(got, R.resample(sub, (50, 131))) == 0


def test_pil_to_tensor_equals_the_reference_chain(imaging):
    """gradio_app.py:440-454 on the host (PIL resize, numpy, torch) against pil_to_tensor, bit for bit, from a PIL image, an
    array and a tensor; a non-RGB image is converted first."""
    Image = pytest.importorskip("PIL.Image")
    rgb = np.random.default_rng(3).integers(0, 256, (180, 300, 3), dtype=np.uint8)
    pil = Image.fromarray(rgb, "RGB")
    ref = torch.from_numpy(np.array(pil.resize((215, 215), Image.Resampling.LANCZOS))).float() / 255.0
    ref = (ref.permute(2, 0, 1) - 0.5) * 2
    for source in (pil, rgb, torch.from_numpy(rgb), torch.from_numpy(rgb).to(DEV)):
        got = imaging.pil_to_tensor(source, device=DEV)
        assert got.shape == (3, 215, 215) and got.dtype == torch.float32 and got.is_cuda
        assert torch.equal(got.cpu(), ref)
    rgba = Image.fromarray(np.random.default_rng(4).integers(0, 256, (64, 48, 4), dtype=np.uint8), "RGBA")
    grey = Image.fromarray(rgb[:, :, 0], "L")
    for im in (rgba, grey):
        assert torch.equal(imaging.pil_to_tensor(im, device=DEV), imaging.pil_to_tensor(im.convert("RGB"), device=DEV))
    assert torch.equal(imaging.pil_to_tensor(rgb[:, :, 0], device=DEV), imaging.pil_to_tensor(grey, device=DEV))
    small = imaging.pil_to_tensor(pil, size=64, device=DEV)
    assert small.shape == (3, 64, 64)


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 3, 215, 215)])
@pytest.mark.parametrize("layout", ["contiguous", "channels_last"])
def test_to_uint8_equals_the_numpy_chain(imaging, shape, layout):
    img = R.u8_image(shape)
    want = np.stack([R.image_to_u8(img[b]) for b in range(shape[0])])
    dev = img.to(DEV)
    if layout == "channels_last":
        dev = dev.contiguous(memory_format=torch.channels_last)
        assert dev.stride(1) == 1
    got = imaging.to_uint8(dev)
    assert got.dtype == torch.uint8 and got.is_cuda and got.is_contiguous()
    assert _mismatches(got.cpu().numpy(), want) == 0
    assert torch.equal(imaging.to_uint8(dev[0]), got[0])
    if shape[2] == 215:                                                  # every listed value took part, and both clamps
        assert set(R.u8_values().tolist()) <= set(img.reshape(-1).tolist()) and want.min() == 0 and want.max() == 255


def test_to_uint8_nan_is_zero(imaging):
    img = torch.full((1, 3, 4, 6), float("nan"))
    img[0, 1, 2, 3] = 1.0
    got = imaging.to_uint8(img.to(DEV)).cpu()
    assert int(got[0, 2, 3, 1]) == 255 and int(got.sum()) == 255


@pytest.mark.parametrize("s", [0.0, 0.3, 0.7, 1.0])
def test_mix_latent_equals_torch_cpu(imaging, s):
    g = torch.Generator().manual_seed(11)
    a, b = torch.randn(2, 8, 27, 27, generator=g), torch.randn(2, 8, 27, 27, generator=g)
    got = imaging.mix_latent(a.to(DEV), b.to(DEV), s)
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), R.mix(a, b, s))
    odd = imaging.mix_latent(a.reshape(-1)[1:].to(DEV)[2:], b.reshape(-1)[3:].to(DEV), s)      # unaligned base, n % 4 != 0
    assert torch.equal(odd.cpu(), R.mix(a.reshape(-1)[3:], b.reshape(-1)[3:], s))
