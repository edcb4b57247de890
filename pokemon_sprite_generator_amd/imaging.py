"""The two ends of the demo's generation path (gradio_app.py:394-465), on the device: an uploaded image in, the latent /
noise blend, uint8 sprites out.  The kernels are csrc/imaging.hip, specified in include/psg_hip.h.

  * `pil_to_tensor` (:440-454): PIL's `resize((215, 215), Image.Resampling.LANCZOS)` + ToTensor + `(t - 0.5) * 2` as
    `resize_lanczos` - the 8-bit separable resample of PIL's Resample.c, integer arithmetic end to end, so the bytes are PIL's
    for any input size; the normalisation is a 256-entry table of the reference's own expression applied in the last pass.
  * `mix_latent` (:426): `latent * (1 - s) + noise * s`.
  * `to_uint8` / `tensor_to_pil` (:456-465): `(t + 1) / 2`, clamp, `* 255`, truncate, HWC - one launch per batch and no
    host copy until an image is asked for as a PIL object.

`lanczos_coeffs` restates PIL's `precompute_coeffs` + `normalize_coeffs_8bpc` for the LANCZOS filter on the host in double
precision (libm's sin through `math.sin`, as the C code calls it); tests/imaging_ref.py restates it again, independently, and
both are held to PIL itself.

One deviation from the reference, documented in DESIGN.md: an image whose mode is not RGB is converted to RGB BEFORE the
resize (what the demo's `gr.Image(image_mode="RGB")` does ahead of the reference); the reference's own order for a bare RGBA
image resizes with premultiplied alpha first.
"""
import functools
import math

import numpy as np
import torch

from . import _lib

PRECISION_BITS = 32 - 8 - 2          # PIL's 8-bit resample: coefficients are 22-bit fixed point
LANCZOS_SUPPORT = 3.0


def _lanczos(v):
    if not (-3.0 <= v < 3.0):
        return 0.0
    if v == 0.0:
        return 1.0
    a, b = v * math.pi, (v / 3) * math.pi
    return (math.sin(a) / a) * (math.sin(b) / b)


@functools.lru_cache(maxsize=64)
def lanczos_coeffs(in_size: int, out_size: int):
    """(bounds int32 [out, 2] = (first input index, tap count), coef int32 [out, kmax] zero-padded, kmax) of PIL's LANCZOS
    resample from in_size to out_size samples, or None when the sizes are equal (PIL skips that pass).  The arrays are
    read-only (the result is cached per size pair)."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise ValueError(f"lanczos_coeffs: sizes must be positive, got {in_size} -> {out_size}")
    if in_size == out_size:
        return None
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = LANCZOS_SUPPORT * fs
    kmax = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs                                          # (PIL multiplies by the reciprocal)
    bounds = np.zeros((out_size, 2), np.int32)
    coef = np.zeros((out_size, kmax), np.int32)
    for i in range(out_size):
        center = (i + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))         # int(): toward zero, as the C cast
        xmax = min(in_size, int(center + support + 0.5))
        n = xmax - xmin
        w = [_lanczos((x + xmin - center + 0.5) * ss) for x in range(n)]
        total = 0.0
        for v in w:                                        # summed in tap order
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        bounds[i] = (xmin, n)
        coef[i, :n] = [int(v * (1 << PRECISION_BITS) + (0.5 if v >= 0 else -0.5)) for v in w]
    bounds.setflags(write=False)
    coef.setflags(write=False)
    return bounds, coef, kmax


_dev_tables = {}      # (in, out, device index) -> (bounds host, bounds device, coef device, kmax)
_dev_lut = {}         # device index -> fp32 [256]


def _tables(in_size, out_size, device):
    key = (int(in_size), int(out_size), device.index)
    if key not in _dev_tables:
        t = lanczos_coeffs(in_size, out_size)
        if t is None:
            _dev_tables[key] = (None, None, None, 0)
        else:
            _dev_tables[key] = (t[0], torch.from_numpy(t[0].copy()).to(device), torch.from_numpy(t[1].copy()).to(device), t[2])
    return _dev_tables[key]


def _lut(device):
    """ToTensor + normalise of every byte value, by the reference's own expressions (gradio_app.py:450-452) on the host."""
    if device.index not in _dev_lut:
        t = torch.arange(256, dtype=torch.uint8).float() / 255.0
        _dev_lut[device.index] = ((t - 0.5) * 2).to(device)
    return _dev_lut[device.index]


def _device_of(t, what):
    if not t.is_cuda:
        raise _lib.PsgError(f"{what} needs GPU tensors: the HIP kernels are the only implementation")
    return torch.device("cuda", t.device.index if t.device.index is not None else torch.cuda.current_device())


def _host_ptr(a):
    return None if a is None else a.ctypes.data


def resize_lanczos(src_u8, size=(215, 215), normalize=True):
    """psg_resample_u8 with PIL's LANCZOS tables.  src_u8: uint8 GPU tensor [H, W, C] or [B, H, W, C], C in 1..4; size:
    (width, height), as `Image.resize` takes it.  normalize=True: fp32 [B, 3, height, width] = ((byte / 255) - 0.5) * 2 of
    the first three channels (C >= 3); False: the resized bytes, uint8 [B, height, width, C]; "both": (bytes, fp32).  A 3-d
    input gives results without the batch dimension."""
    if not isinstance(src_u8, torch.Tensor):
        raise TypeError("resize_lanczos: src_u8 must be a tensor")
    dev = _device_of(src_u8, "resize_lanczos")
    if src_u8.dtype != torch.uint8 or src_u8.dim() not in (3, 4):
        raise _lib.PsgError(f"resize_lanczos: src must be a uint8 [H, W, C] or [B, H, W, C] tensor, got {src_u8.dtype} {tuple(src_u8.shape)}")
    if normalize not in (True, False, "both"):
        raise ValueError("resize_lanczos: normalize must be True, False or 'both'")
    single = src_u8.dim() == 3
    src = (src_u8[None] if single else src_u8).contiguous()
    B, Hin, Win, C = src.shape
    Wout, Hout = (int(s) for s in size)
    if not 1 <= C <= 4 or min(B, Hin, Win, Hout, Wout) <= 0:
        raise _lib.PsgError(f"resize_lanczos: shape {tuple(src.shape)} -> {(Hout, Wout)} needs positive sizes and C in 1..4")
    want_u8, want_f32 = normalize is not True, normalize is not False
    if want_f32 and C < 3:
        raise _lib.PsgError(f"resize_lanczos: the normalised output takes three channels, the image has {C}")
    lib = _lib.init(dev.index)
    xbh, xb, xc, kx = _tables(Win, Wout, dev)
    ybh, yb, yc, ky = _tables(Hin, Hout, dev)
    out_u8 = torch.empty(B, Hout, Wout, C, dtype=torch.uint8, device=dev) if want_u8 else None
    out_f32 = torch.empty(B, 3, Hout, Wout, dtype=torch.float32, device=dev) if want_f32 else None
    ws_bytes = B * Hin * Wout * C if kx and ky else 0
    ws = _lib.workspace(ws_bytes, dev) if ws_bytes else None
    with torch.cuda.device(dev):
        _lib.check(lib.psg_resample_u8(_lib.ptr(src), _lib.ptr(out_u8), _lib.ptr(out_f32), _lib.ptr(_lut(dev) if want_f32 else None),
                                       B, Hin, Win, C, Hout, Wout, _host_ptr(xbh), _lib.ptr(xb), _lib.ptr(xc), kx,
                                       _host_ptr(ybh), _lib.ptr(yb), _lib.ptr(yc), ky, _lib.ptr(ws), ws_bytes, _lib.stream_ptr()),
                   "psg_resample_u8")
    outs = [o[0] if single else o for o in (out_u8, out_f32) if o is not None]
    return outs[0] if len(outs) == 1 else tuple(outs)


def _as_u8_hwc(image, device):
    """uint8 [H, W, C] or [B, H, W, C] on `device`, C = 3 or 4, from a PIL image, a numpy array or a tensor."""
    if hasattr(image, "mode") and hasattr(image, "convert"):               # a PIL image
        if image.mode != "RGB":
            image = image.convert("RGB")
        image = np.array(image)
    if isinstance(image, np.ndarray):
        image = torch.from_numpy(np.array(image))                          # (a writable, contiguous copy)
    if not isinstance(image, torch.Tensor):
        raise TypeError(f"pil_to_tensor: expected a PIL image, a numpy array or a tensor, got {type(image).__name__}")
    if image.dtype != torch.uint8:
        raise _lib.PsgError(f"pil_to_tensor: pixel data must be uint8, got {image.dtype}")
    if image.dim() == 2:
        image = image[:, :, None]
    if image.dim() not in (3, 4) or image.shape[-1] not in (1, 3, 4):
        raise _lib.PsgError(f"pil_to_tensor: expected [H, W], [H, W, C] or [B, H, W, C] with C in (1, 3, 4), got {tuple(image.shape)}")
    if image.shape[-1] == 1:                                               # grey -> RGB, as convert("RGB") of an "L" image
        image = image.expand(*image.shape[:-1], 3)
    return image.to(device).contiguous()


def pil_to_tensor(image, size: int = 215, device=None):
    """gradio_app.py:440-454: fp32 [3, size, size] in [-1, 1] on the device ([B, 3, size, size] for a 4-d array / tensor) from
    an upload of any size.  A PIL image whose mode is not RGB is converted with `.convert("RGB")` BEFORE the resize (see the
    module docstring); an array or tensor is uint8 [H, W], [H, W, 3] or [H, W, 4] (the fourth channel is ignored, as
    `convert("RGB")` drops it).  device=None: the tensor's own GPU, else the current one."""
    if device is None:
        if isinstance(image, torch.Tensor) and image.is_cuda:
            device = image.device
        elif torch.cuda.is_available():
            device = torch.device("cuda", torch.cuda.current_device())
        else:
            raise _lib.PsgError("pil_to_tensor needs a GPU: the HIP kernels are the only implementation")
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.PsgError("pil_to_tensor needs a GPU device: the HIP kernels are the only implementation")
    return resize_lanczos(_as_u8_hwc(image, device), (size, size), normalize=True)


def to_uint8(images):
    """tensor_to_pil's arithmetic (gradio_app.py:458-464) for a batch, on the device: fp32 [B, 3, H, W] (any strides: NCHW and
    channels_last go in without a copy) -> uint8 [B, H, W, 3]; [3, H, W] -> [H, W, 3]."""
    dev = _device_of(images, "to_uint8")
    single = images.dim() == 3
    img = images[None] if single else images
    if img.dim() != 4 or img.shape[1] != 3 or img.numel() == 0:
        raise _lib.PsgError(f"to_uint8: expected [B, 3, H, W] or [3, H, W], got {tuple(images.shape)}")
    img = img.detach()
    if img.dtype != torch.float32:
        img = img.float()
    B, _, H, W = img.shape
    sb, sc, sh, sw = img.stride()
    lib = _lib.init(dev.index)
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.psg_image_to_u8(_lib.ptr(img), sb, sc, sh, sw, _lib.ptr(out), B, H, W, _lib.stream_ptr()), "psg_image_to_u8")
    return out[0] if single else out


def tensor_to_pil(image):
    """gradio_app.py:456-465: one fp32 [3, H, W] image (or an already converted uint8 [H, W, 3] one) -> PIL RGB image."""
    from PIL import Image                      # lazy: importing the package needs neither PIL nor a GPU
    if image.dtype != torch.uint8:
        image = to_uint8(image)
    if image.dim() != 3 or image.shape[-1] != 3:
        raise _lib.PsgError(f"tensor_to_pil: expected one [3, H, W] image or its uint8 [H, W, 3] form, got {tuple(image.shape)}")
    return Image.fromarray(image.cpu().numpy())


def save_sheet(rows, path):
    """Monitoring grid: `rows` is a list of [n, 3, H, W] tensors in [-1, 1] (one H x W for all); each goes through `to_uint8`
    and becomes one row of the sheet, its n images side by side (a shorter row ends in white).  Laid out on the device,
    written as a PNG with PIL.  Returns the uint8 [len(rows) * H, n_max * W, 3] sheet."""
    from PIL import Image                      # lazy: importing the package needs neither PIL nor a GPU
    if not rows:
        raise _lib.PsgError("save_sheet: no rows")
    u8 = [to_uint8(r) for r in rows]                                   # [n, H, W, 3] each
    H, W = u8[0].shape[1:3]
    if any(tuple(r.shape[1:3]) != (H, W) for r in u8):
        raise _lib.PsgError(f"save_sheet: rows of different image sizes {[tuple(r.shape) for r in u8]}")
    n = max(r.shape[0] for r in u8)
    sheet = torch.full((len(u8), H, n, W, 3), 255, dtype=torch.uint8, device=u8[0].device)
    for k, r in enumerate(u8):
        sheet[k, :, :r.shape[0]] = r.to(sheet.device).permute(1, 0, 2, 3)
    sheet = sheet.reshape(len(u8) * H, n * W, 3)
    Image.fromarray(sheet.cpu().numpy()).save(str(path))
    return sheet


def mix_latent(latent, noise, strength: float):
    """gradio_app.py:426: latent * (1 - strength) + noise * strength in fp32, both scalars rounded to fp32 first (as torch
    applies a Python scalar to an fp32 tensor), every product and the sum rounded once.  `noise` is moved to the latent's device (an injected draw may come from the host)."""
    dev = _device_of(latent, "mix_latent")
    if noise.shape != latent.shape or latent.numel() == 0:
        raise _lib.PsgError(f"mix_latent: latent {tuple(latent.shape)} and noise {tuple(noise.shape)} must have one, non-empty shape")
    a = latent.detach().float().contiguous()
    b = noise.detach().to(device=dev, dtype=torch.float32).contiguous()
    out = torch.empty_like(a)
    lib = _lib.init(dev.index)
    with torch.cuda.device(dev):
        _lib.check(lib.psg_latent_mix_f32(_lib.ptr(a), _lib.ptr(b), float(1 - strength), float(strength), _lib.ptr(out), a.numel(),
                                          _lib.stream_ptr()), "psg_latent_mix_f32")
    return out
