"""References for the sprite loader kernels (pokemon_sprite_generator_amd/csrc/sprites.hip, data.py).

(i)  `spec_mean` / `spec_augment`: the float specification of the two kernels (include/psg_hip.h, "Sprite batches")
     restated in numpy, generic in the float type: fp64 is the reference the kernels are judged by, fp32 (same
     expressions, same order) measures what fp32 evaluation alone costs - the kernels' tolerance comes from that, never
     from their own output.
(ii) `pil_chain`: the reference's train pipeline on PIL itself - the calls torchvision's PIL backend makes for
     RandomHorizontalFlip, RandomRotation, ColorJitter, RandomResizedCrop, ToTensor, Normalize (torchvision is not
     installed where this runs; the calls are restated from its documented behaviour).  One deliberate difference: a
     hue shift of exactly 0 skips the HSV round trip (torchvision quantises to 8-bit HSV even then), so that the
     one-op cases isolate one op; a drawn hue is never 0.
(iii) `cases(S)`: the case table.

An output pixel is AMBIGUOUS when, for any of its four taps, the rotation's xin or yin lies within AMBIG_EPS of an
integer: fp32 and fp64 may floor it differently there, and so may PIL, which steps through the affine map in 16.16 fixed
point.  Ambiguous pixels are left out of element-wise comparisons, under a cap of AMBIG_CAP of a case's pixels.
"""
import functools
import itertools
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SPRITE_DIR = os.path.join(HERE, "golden", "sprites")
NP = 16
ORDERS = list(itertools.permutations(range(4)))      # 0 brightness, 1 contrast, 2 saturation, 3 hue
AMBIG_EPS = 2e-4
AMBIG_CAP = 0.01
IDX = [5, 0, 7, 2, 6]                                # non-monotone rows of the 8 fixture sprites
FIXTURE_NUMBERS = [1, 2, 3, 5, 6, 7, 8, 9]           # NNN.png present under golden/sprites (4 and 10 are missing on purpose)

# ---- measured constants (tests/test_sprites_cpu.py recomputes and compares them; DESIGN.md quotes them) -------------
# max |fp64 specification - PIL chain| in output units over fixtures x cases, ambiguous pixels excluded: the reference's
# own uint8 quantisation (a truncating blend per colour op, 8-bit H/S/V, two rounded resize passes).  "Ambiguous" here
# includes the pixels where PIL's fixed-point rotation reads another source pixel (pil_floor_differs: up to 19 of 46225
# pixels of the rotated image; with them in, the maximum is a sprite's outline against its background, 1.37).  It must stay
# below QUANT_LIMIT = 16/255*2, or the restatement is wrong.
QUANT_LIMIT = 16.0 / 255.0 * 2.0
PIL_QUANT_MAX = 0.07933       # 10.1 of 255 levels (all ops, contrast first; the hue op alone: 0.0596)
# max |fp32 evaluation - fp64 evaluation| of spec_augment over the case table (S = 215 and S = 33), ambiguous pixels
# excluded; the kernel's tolerance is 4x this (a different but equivalent operation order).
FP32_EVAL_MAX = 2.05e-5
# max over the table's samples of |fp32 sum - fp64 sum| of the contrast-mean luma sum; the mean kernel's E is 4x this.
FP32_SUM_ERR_MAX = 1.15        # of sums near 1e7: 2.5e-5 of a level in the mean


# ---------------------------------------------------------------------------------------------------------------------
# parameter rows
# ---------------------------------------------------------------------------------------------------------------------
def rotation_coeffs(angle, S):
    """The inverse affine PIL's Image.rotate(angle, expand=False, center=None) builds (PIL/Image.py), in Python floats."""
    angle = angle % 360.0
    if angle == 0:
        return (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    cx = cy = S / 2
    ang = -math.radians(angle)
    m = [round(math.cos(ang), 15), round(math.sin(ang), 15), 0.0, round(-math.sin(ang), 15), round(math.cos(ang), 15), 0.0]
    m[2] = m[0] * -cx + m[1] * -cy + m[2] + cx
    m[5] = m[3] * -cx + m[4] * -cy + m[5] + cy
    return tuple(m)


def make_row(S, flip=0, angle=0.0, order=(0, 1, 2, 3), b=1.0, c=1.0, s=1.0, hue=0.0, crop=None):
    i, j, h, w = crop if crop is not None else (0, 0, S, S)
    return np.array([flip, *rotation_coeffs(angle, S), ORDERS.index(tuple(order)), b, c, s, hue, i, j, h, w], dtype=np.float32)


def cases(S):
    """name -> list of 5 per-sample dicts (keyword arguments of make_row and pil_chain)."""
    wmin, mid = int(0.9 * S), int(round(math.sqrt(0.9) * S))
    ang = [3.0, 7.3, 10.0, -10.0, -7.3] if S == 215 else [0.0, 3.0, 10.0, -10.0, 3.0]
    crops = [(0, S - wmin, S, wmin), (S - wmin, 0, wmin, S), (S - wmin, S - wmin, wmin, wmin), (S - mid, 0, mid, mid), (1, S - mid, mid - 1, mid)]
    fb, fc, fs, fh = [0.9, 1.1, 1.1, 0.9, 1.05], [1.1, 0.9, 0.9, 1.1, 0.95], [0.9, 1.1, 0.9, 1.1, 1.03], [-0.05, 0.05, 0.05, -0.05, 0.02]
    flips = [1, 0, 1, 1, 0]

    def all_ops(orders):
        return [dict(flip=flips[k], angle=ang[k], order=orders[k], b=fb[k], c=fc[k], s=fs[k], hue=fh[k], crop=crops[k]) for k in range(5)]

    t = {
        "all_contrast_first": all_ops([(1, 0, 2, 3), (1, 2, 3, 0), (1, 3, 0, 2), (1, 0, 3, 2), (1, 3, 2, 0)]),
        "all_contrast_middle": all_ops([(3, 0, 1, 2), (0, 1, 3, 2), (2, 3, 1, 0), (3, 1, 2, 0), (0, 2, 1, 3)]),
        "all_contrast_last": all_ops([(2, 3, 0, 1), (0, 2, 3, 1), (3, 2, 0, 1), (3, 0, 2, 1), (0, 3, 2, 1)]),
    }
    if S != 215:
        return t
    t.update({
        "identity": [dict() for _ in range(5)],
        "flip": [dict(flip=f) for f in flips],
        "rotate": [dict(angle=a) for a in ang],
        "brightness": [dict(b=v, order=ORDERS[3 * k]) for k, v in enumerate(fb)],
        "contrast": [dict(c=v, order=ORDERS[5 * k + 1]) for k, v in enumerate(fc)],
        "saturation": [dict(s=v, order=ORDERS[4 * k + 2]) for k, v in enumerate(fs)],
        "hue": [dict(hue=v, order=ORDERS[5 * k + 3]) for k, v in enumerate(fh)],
        "crop": [dict(crop=c) for c in crops],
    })
    return t


def rows(case, S):
    return np.stack([make_row(S, **kw) for kw in case])


# ---------------------------------------------------------------------------------------------------------------------
# fixture sprites
# ---------------------------------------------------------------------------------------------------------------------
def composite(path, background=(255, 255, 255)):
    """The reference's _load_image_with_background (src/data/dataset_improved.py:124-140)."""
    from PIL import Image
    img = Image.open(path)
    if img.mode in ("RGBA", "LA") or (img.mode == "P" and "transparency" in img.info):
        bg = Image.new("RGB", img.size, background)
        bg.paste(img, mask=(img.convert("RGBA") if img.mode == "P" else img).split()[-1])
        return bg
    return img.convert("RGB")


@functools.lru_cache(maxsize=None)
def fixture_images(S=215):
    """The 8 fixture sprites as PIL RGB images, composited on white (S != 215: resized once with PIL BILINEAR)."""
    from PIL import Image
    out = []
    for n in FIXTURE_NUMBERS:
        img = composite(os.path.join(SPRITE_DIR, f"{n:03d}.png"))
        out.append(img if img.size == (S, S) else img.resize((S, S), Image.BILINEAR))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fixture_array(S=215):
    """uint8 [8, S, S, 4]: the resident layout (R, G, B, unused)."""
    a = np.zeros((len(FIXTURE_NUMBERS), S, S, 4), np.uint8)
    for k, img in enumerate(fixture_images(S)):
        a[k, :, :, :3] = np.asarray(img)
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------------------------------------------------------------
# (i) the float specification, generic in the float type
# ---------------------------------------------------------------------------------------------------------------------
def _clip(v, dt):
    return np.minimum(np.maximum(v, dt(0)), dt(255))


def _luma(r, g, b, dt):
    return (dt(19595) * r + dt(38470) * g + dt(7471) * b) / dt(65536)


def _hue_shift(r, g, b, shift, dt):
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    delta = np.where(grey, dt(1), maxc - minc)
    s = delta / np.where(grey, dt(1), maxc)
    rc, gc, bc = (maxc - r) / delta, (maxc - g) / delta, (maxc - b) / delta
    h = np.where(r == maxc, bc - gc, np.where(g == maxc, dt(2) + rc - bc, dt(4) + gc - rc))
    h = h / dt(6)
    h = h - np.floor(h)
    h = h + shift
    h = h - np.floor(h)
    h6 = h * dt(6)
    fi = np.floor(h6)
    f = h6 - fi
    i = fi.astype(np.int64) % 6
    p, q, t = maxc * (dt(1) - s), maxc * (dt(1) - s * f), maxc * (dt(1) - s * (dt(1) - f))
    R = np.choose(i, [maxc, q, p, p, t, maxc])
    G = np.choose(i, [t, maxc, maxc, q, p, p])
    B = np.choose(i, [p, p, t, maxc, maxc, q])
    return np.where(grey, r, R), np.where(grey, g, G), np.where(grey, b, B)


def _colour_ops(r, g, b, row, mean, dt, to_contrast=False):
    fb, fc, fs, fh = (dt(row[k]) for k in (8, 9, 10, 11))
    for op in ORDERS[int(row[7])]:
        if op == 0:
            if fb != 1:
                r, g, b = _clip(fb * r, dt), _clip(fb * g, dt), _clip(fb * b, dt)
        elif op == 1:
            if to_contrast:
                break
            if fc != 1:
                m = dt(mean)
                r, g, b = _clip(m + fc * (r - m), dt), _clip(m + fc * (g - m), dt), _clip(m + fc * (b - m), dt)
        elif op == 2:
            if fs != 1:
                l = _luma(r, g, b, dt)
                r, g, b = _clip(l + fs * (r - l), dt), _clip(l + fs * (g - l), dt), _clip(l + fs * (b - l), dt)
        elif fh != 0:
            r, g, b = _hue_shift(r, g, b, fh, dt)
    return r, g, b


def _rotated(img, row, dt):
    """(r, g, b, ambiguous) of the flipped + rotated image, [S, S] each, indexed [v, u]."""
    S = img.shape[0]
    a, b, c, d, e, f = (dt(row[k]) for k in range(1, 7))
    uc = (np.arange(S).astype(dt) + dt(0.5))[None, :]
    vc = (np.arange(S).astype(dt) + dt(0.5))[:, None]
    xin, yin = a * uc + b * vc + c, d * uc + e * vc + f
    fx, fy = np.floor(xin), np.floor(yin)
    inside = (fx >= 0) & (fx < S) & (fy >= 0) & (fy < S)
    sx, sy = np.where(inside, fx, 0).astype(np.int64), np.where(inside, fy, 0).astype(np.int64)
    if row[0] != 0:
        sx = S - 1 - sx
    px = img[sy, sx].astype(dt)
    r, g, bl = (np.where(inside, px[..., k], dt(0)) for k in range(3))
    amb = (np.abs(xin - np.rint(xin)) < AMBIG_EPS) | (np.abs(yin - np.rint(yin)) < AMBIG_EPS)
    return r, g, bl, amb


def pil_fixed_map(angle, S):
    """(sx, sy, inside), int64 / bool [S, S] indexed [v, u]: the source pixel PIL's Image.rotate(angle, NEAREST) reads.  PIL
    does not evaluate xin = a(u+.5) + b(v+.5) + c per pixel: for an image this small it rounds the six coefficients to 16.16
    fixed point (the half-pixel offsets folded into c and f) and steps through the map with integer additions
    (libImaging/Geometry.c, affine_fixed), so near an integer it may floor differently from ANY float evaluation."""
    a = rotation_coeffs(angle, S)
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))
    a0, a1, a3, a4 = fix(a[0]), fix(a[1]), fix(a[3]), fix(a[4])
    a2, a5 = fix(a[2] + a[0] * 0.5 + a[1] * 0.5), fix(a[5] + a[3] * 0.5 + a[4] * 0.5)
    u, v = np.arange(S, dtype=np.int64)[None, :], np.arange(S, dtype=np.int64)[:, None]
    sx, sy = (a2 + u * a0 + v * a1) >> 16, (a5 + u * a3 + v * a4) >> 16
    return sx, sy, (sx >= 0) & (sx < S) & (sy >= 0) & (sy < S)


def pil_floor_differs(angle, row, S):
    """bool [S, S]: pixels of the rotated image where PIL's fixed-point map and the fp64 specification read different source
    pixels - the reference legitimately flooring differently, like an ambiguous pixel."""
    sx, sy, inside = pil_fixed_map(angle, S)
    a, b, c, d, e, f = (np.float64(row[k]) for k in range(1, 7))
    uc, vc = (np.arange(S) + 0.5)[None, :], (np.arange(S) + 0.5)[:, None]
    fx, fy = np.floor(a * uc + b * vc + c), np.floor(d * uc + e * vc + f)
    fin = (fx >= 0) & (fx < S) & (fy >= 0) & (fy < S)
    return (inside != fin) | (inside & fin & ((sx != fx) | (sy != fy)))


def spec_mean(src, idx, params, dt=np.float64):
    """(mean [B], luma sum [B], n_ambiguous [B]); samples whose contrast factor is 1 get 0."""
    B, S = len(idx), src.shape[1]
    mean, total, namb = np.zeros(B, dt), np.zeros(B, dt), np.zeros(B, np.int64)
    for k in range(B):
        row = params[k]
        if row[9] == 1:
            continue
        r, g, b, amb = _rotated(src[idx[k]], row, dt)
        r, g, b = _colour_ops(r, g, b, row, 0, dt, to_contrast=True)
        total[k] = np.sum(_luma(r, g, b, dt), dtype=dt)
        mean[k] = total[k] / dt(S * S)
        namb[k] = int(amb.sum())
    return mean, total, namb


def spec_augment(src, idx, params, mean, dt=np.float64, also=None):
    """(out [B, 3, S, S], ambiguous [B, S, S]).  `mean` [B] is given (the two kernels are judged separately).  also: bool
    [B, S, S], further pixels of the ROTATED image to treat as ambiguous (carried through the four taps)."""
    B, S = len(idx), src.shape[1]
    out, ambig = np.zeros((B, 3, S, S), dt), np.zeros((B, S, S), bool)
    for k in range(B):
        row = params[k]
        r, g, b, amb = _rotated(src[idx[k]], row, dt)
        if also is not None:
            amb = amb | also[k]
        chans = _colour_ops(r, g, b, row, mean[k], dt)           # per pixel of the rotated image: the same value at every tap that reads it
        ci, cj, ch, cw = (int(row[n]) for n in (12, 13, 14, 15))
        o = np.arange(S).astype(dt) + dt(0.5)
        cx, cy = o * dt(cw) / dt(S) - dt(0.5), o * dt(ch) / dt(S) - dt(0.5)
        x0, y0 = np.floor(cx), np.floor(cy)
        wx, wy = (cx - x0)[None, :], (cy - y0)[:, None]
        xa, xb = (np.clip(x0.astype(np.int64) + n, 0, cw - 1) + cj for n in (0, 1))
        ya, yb = (np.clip(y0.astype(np.int64) + n, 0, ch - 1) + ci for n in (0, 1))
        one = dt(1)
        for c, p in enumerate(chans):
            top = (one - wx) * p[ya][:, xa] + wx * p[ya][:, xb]
            bot = (one - wx) * p[yb][:, xa] + wx * p[yb][:, xb]
            v = (one - wy) * top + wy * bot
            out[k, c] = (v / dt(255) - dt(0.5)) / dt(0.5)
        ambig[k] = amb[ya][:, xa] | amb[ya][:, xb] | amb[yb][:, xa] | amb[yb][:, xb]
    return out, ambig


@functools.lru_cache(maxsize=None)
def reference(name, S):
    """The fp64 reference of one case, computed once and shared: dict(params, idx, mean, total, namb, out, ambig,
    ambig_pil, mean32, total32, out32); the *32 entries are the same restatement evaluated in fp32 (given the fp64 mean);
    ambig_pil adds the pixels where PIL's fixed-point rotation reads another source pixel (comparisons with pil_chain)."""
    src, idx = fixture_array(S), IDX
    case = cases(S)[name]
    params = rows(case, S)
    mean, total, namb = spec_mean(src, idx, params)
    out, ambig = spec_augment(src, idx, params, mean)
    differs = np.stack([pil_floor_differs(kw.get("angle", 0.0), params[k], S) for k, kw in enumerate(case)])
    _, ambig_pil = spec_augment(src, idx, params, mean, also=differs)
    mean32, total32, _ = spec_mean(src, idx, params, np.float32)
    out32, _ = spec_augment(src, idx, params, mean.astype(np.float32), np.float32)
    r = dict(params=params, idx=np.array(idx, np.int64), mean=mean, total=total, namb=namb, out=out, ambig=ambig, ambig_pil=ambig_pil, mean32=mean32, total32=total32,
             out32=out32)
    for v in r.values():
        v.setflags(write=False)
    return r


def all_cases():
    return [(n, 215) for n in cases(215)] + [(n, 33) for n in cases(33)]


def measure_fp32():
    """(max |fp32 - fp64| of the augment restatement outside ambiguous pixels, max |fp32 - fp64| of the luma sums) over the table."""
    e_aug = e_sum = 0.0
    for name, S in all_cases():
        r = reference(name, S)
        keep = ~np.broadcast_to(r["ambig"][:, None], r["out"].shape)
        e_aug = max(e_aug, float(np.abs(r["out32"].astype(np.float64) - r["out"])[keep].max()))
        e_sum = max(e_sum, float(np.abs(r["total32"].astype(np.float64) - r["total"]).max()))
    return e_aug, e_sum


# ---------------------------------------------------------------------------------------------------------------------
# (ii) the reference chain on PIL
# ---------------------------------------------------------------------------------------------------------------------
def pil_chain(img, S, flip=0, angle=0.0, order=(0, 1, 2, 3), b=1.0, c=1.0, s=1.0, hue=0.0, crop=None):
    """float32 [3, S, S]: what the reference's train loader yields for the RGB image `img` under these draws."""
    from PIL import Image, ImageEnhance
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    img = img.rotate(angle, Image.NEAREST, False, None, fillcolor=(0, 0, 0))
    for op in order:
        if op == 0:
            img = ImageEnhance.Brightness(img).enhance(b)
        elif op == 1:
            img = ImageEnhance.Contrast(img).enhance(c)
        elif op == 2:
            img = ImageEnhance.Color(img).enhance(s)
        elif hue != 0:
            h, sat, val = img.convert("HSV").split()
            np_h = np.array(h, dtype=np.uint8)
            with np.errstate(over="ignore"):
                np_h += np.int32(hue * 255).astype(np.uint8)
            img = Image.merge("HSV", (Image.fromarray(np_h, "L"), sat, val)).convert("RGB")
    i, j, h, w = crop if crop is not None else (0, 0, S, S)
    img = img.crop((j, i, j + w, i + h)).resize((S, S), Image.BILINEAR)
    t = np.asarray(img).astype(np.float32).transpose(2, 0, 1) / np.float32(255)
    return (t - np.float32(0.5)) / np.float32(0.5)


def pil_case(name, S):
    """float32 [5, 3, S, S]: pil_chain over one case on the fixture sprites IDX selects."""
    imgs = fixture_images(S)
    return np.stack([pil_chain(imgs[IDX[k]], S, **kw) for k, kw in enumerate(cases(S)[name])])
