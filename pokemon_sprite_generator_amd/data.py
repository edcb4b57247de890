"""Sprite batches from a device-resident dataset: the reference's `src.data.create_data_loaders` without torchvision,
pandas or DataLoader workers.

The reference (src/data/dataset_improved.py) decodes and augments every sprite per sample with PIL in DataLoader workers:
alpha composite, RandomHorizontalFlip, RandomRotation(10), ColorJitter(0.1, 0.1, 0.1, 0.05), RandomResizedCrop(scale
0.9-1, ratio 0.9-1.1), ToTensor, Normalize.  Here every PNG is decoded and composited ONCE (`SpriteDataset`), the whole
set lives on the device as uint8 [N, S, S, 4], and a batch is two launches in the training stream: the per-sample
contrast mean and one fused gather/augment/normalise kernel (csrc/sprites.hip, specified in include/psg_hip.h).

torchvision is not installed where this package is built and tested, so the augmentation's distributions and geometry
(`draw_params`) are restated from torchvision's documented behaviour and from the source of the installed PIL, not
imported; tests/sprite_ref.py holds the same chain on PIL itself and the bound the two are held to.

Deviations from the reference, both documented in DESIGN.md:
  * a source that is not image_size x image_size is resized once at load time (PIL BILINEAR); the reference augments
    at the original size and resizes after (4 of the 898 sprites);
  * the float chain drops the reference's intermediate uint8 roundings (a truncating blend per colour op, 8-bit HSV,
    rounded resize passes) and keeps its clipping.
"""
import csv
import io
import math
import os
from typing import Tuple, Union

import torch

from . import _lib

NUM_PARAMS = _lib.ABI.constants["PSG_SPRITE_PARAMS"]     # the row layout is described in include/psg_hip.h
# what pandas.read_csv reads as a missing value (the reference drops rows whose description is missing)
_NA = frozenset(["", "#N/A", "#N/A N/A", "#NA", "-1.#IND", "-1.#QNAN", "-NaN", "-nan", "1.#IND", "1.#QNAN", "<NA>", "N/A", "NA",
                 "NULL", "NaN", "None", "n/a", "nan", "null"])
_REQUIRED = ("national_number", "english_name", "description")


# ---------------------------------------------------------------------------------------------------------------------
# CSV and PNG (host, once)
# ---------------------------------------------------------------------------------------------------------------------
def parse_background_color(background_color) -> Tuple[int, int, int]:
    if isinstance(background_color, str):
        named = {"white": (255, 255, 255), "black": (0, 0, 0), "gray": (128, 128, 128), "grey": (128, 128, 128)}
        if background_color.lower() not in named:
            raise ValueError(f"Unknown background color: {background_color}")
        return named[background_color.lower()]
    if isinstance(background_color, (tuple, list)) and len(background_color) == 3:
        return tuple(int(c) for c in background_color)
    raise ValueError(f"Invalid background color format: {background_color}")


def _decode(raw: bytes) -> str:
    """utf-8, then utf-16, then latin-1, like the reference's nested fallbacks.  utf-16 is only tried on a byte-order mark:
    without one Python decodes any even number of bytes as utf-16 and a latin-1 file would come out as noise."""
    try:
        return raw.decode("utf-8")
    except UnicodeDecodeError:
        pass
    if raw[:2] in (b"\xff\xfe", b"\xfe\xff"):
        try:
            return raw.decode("utf-16")
        except UnicodeDecodeError:
            pass
    return raw.decode("latin-1")


def read_rows(csv_path):
    """[{national_number, english_name, description}] of the two shapes the reference accepts: the 2-column `;` file without
    a header (numbered from 1 in file order) and the tab-separated file with a header.  Rows without a description are dropped."""
    with open(csv_path, "rb") as fh:
        text = _decode(fh.read())
    text = text.lstrip("\ufeff")
    recs = [r for r in csv.reader(io.StringIO(text, newline=""), delimiter=";") if r]
    rows = []
    if recs and len(recs[0]) == 2:
        for n, r in enumerate(recs, start=1):
            if len(r) != 2:
                raise ValueError(f"{csv_path}: line {n} has {len(r)} fields, expected 2")
            rows.append({"national_number": n, "english_name": r[0], "description": r[1]})
    else:
        recs = [r for r in csv.reader(io.StringIO(text, newline=""), delimiter="\t") if r]
        header = recs[0] if recs else []
        missing = [c for c in _REQUIRED if c not in header]
        if missing:
            raise ValueError(f"Missing required columns: {missing}. Available columns: {list(header)}")
        col = {c: header.index(c) for c in _REQUIRED}
        for r in recs[1:]:
            get = lambda c: r[col[c]] if col[c] < len(r) else ""
            rows.append({"national_number": int(get("national_number")), "english_name": get("english_name"),
                         "description": get("description")})
    return [r for r in rows if r["description"] not in _NA]


def clean_description(description) -> str:
    """The reference's _clean_description (:205-214)."""
    if description is None:
        return ""
    description = str(description).strip()
    if description.startswith('"') and description.endswith('"'):
        description = description[1:-1]
    return description


def create_full_description(name, description) -> str:
    """The reference's _create_full_description (:216-226)."""
    parts = [f"Pokemon named {name}"]
    description = clean_description(description)
    if description:
        parts.append(description)
    return ". ".join(parts) + "."


def load_image_with_background(image_path, background_color=(255, 255, 255)):
    """The reference's _load_image_with_background (:124-140): transparency is composited on the background colour."""
    from PIL import Image                      # lazy: importing the package needs neither PIL nor a GPU
    img = Image.open(image_path)
    if img.mode in ("RGBA", "LA") or (img.mode == "P" and "transparency" in img.info):
        background = Image.new("RGB", img.size, tuple(background_color))
        alpha = (img.convert("RGBA") if img.mode == "P" else img).split()[-1]
        background.paste(img, mask=alpha)
        return background
    return img.convert("RGB")


class SpriteDataset:
    """The whole sprite set, decoded once and resident on `device` as `images`: uint8 [N, S, S, 4] (R, G, B, unused).

    device=None is the current GPU.  A CPU device holds the array for inspection; batches need the GPU (the kernels are the
    only implementation)."""

    def __init__(self, csv_path: str, image_dir: str, image_size: int = 215, filter_missing: bool = True,
                 background_color: Union[str, Tuple[int, int, int]] = "white", device=None):
        import numpy as np
        from PIL import Image
        self.csv_path, self.image_dir, self.image_size = csv_path, image_dir, int(image_size)
        self.background_color = parse_background_color(background_color)
        if device is None:
            if not torch.cuda.is_available():
                raise _lib.PsgError("SpriteDataset(device=None) needs a GPU; pass device='cpu' to only parse and decode")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        rows = read_rows(csv_path)
        if filter_missing:
            rows = [r for r in rows if os.path.exists(self._get_image_path(r["national_number"]))]
        self.rows = rows
        S = self.image_size
        host = np.zeros((len(rows), S, S, 4), np.uint8)
        for k, r in enumerate(rows):
            img = load_image_with_background(self._get_image_path(r["national_number"]), self.background_color)
            if img.size != (S, S):
                img = img.resize((S, S), Image.BILINEAR)
            host[k, :, :, :3] = np.asarray(img)
        self.images = torch.from_numpy(host).to(self.device)
        self.device = self.images.device                 # ("cuda" -> the device index the array landed on)

    def _get_image_path(self, national_number: int) -> str:
        return os.path.join(self.image_dir, f"{int(national_number):03d}.png")

    def __len__(self) -> int:
        return len(self.rows)

    def meta(self, i: int):
        r = self.rows[int(i)]
        return {"description": clean_description(r["description"]),
                "full_description": create_full_description(r["english_name"], r["description"]),
                "national_number": int(r["national_number"]), "name": str(r["english_name"])}


# ---------------------------------------------------------------------------------------------------------------------
# the two kernels
# ---------------------------------------------------------------------------------------------------------------------
def _check(src, idx, params):
    if not (src.is_cuda and idx.is_cuda and params.is_cuda):
        raise _lib.PsgError("sprite batches need GPU tensors: the HIP kernels are the only implementation")
    if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[1] != src.shape[2] or src.shape[3] != 4 or not src.is_contiguous():
        raise _lib.PsgError(f"sprites: src must be a contiguous uint8 [N, S, S, 4] tensor, got {src.dtype} {tuple(src.shape)}")
    B = idx.shape[0]
    if idx.dtype != torch.int64 or idx.dim() != 1 or not idx.is_contiguous():
        raise _lib.PsgError("sprites: idx must be a contiguous int64 [B] tensor")
    if params.dtype != torch.float32 or tuple(params.shape) != (B, NUM_PARAMS) or not params.is_contiguous():
        raise _lib.PsgError(f"sprites: params must be a contiguous fp32 [{B}, {NUM_PARAMS}] tensor, got {params.dtype} {tuple(params.shape)}")
    return src.shape[0], B, src.shape[1]


def contrast_mean(src, idx, params):
    """psg_sprite_contrast_mean: fp32 [B], the mean luma the contrast op of each sample blends with."""
    N, B, S = _check(src, idx, params)
    lib = _lib.init(src.device.index)
    mean = torch.empty(B, dtype=torch.float32, device=src.device)
    _lib.check(lib.psg_sprite_contrast_mean(_lib.ptr(src), N, _lib.ptr(idx), _lib.ptr(params), _lib.ptr(mean), B, S, _lib.stream_ptr()),
               "psg_sprite_contrast_mean")
    return mean


def augment(src, idx, params, mean=None):
    """psg_sprite_augment: fp32 [B, 3, S, S] in [-1, 1].  mean=None: contrast_mean(src, idx, params) is launched first."""
    N, B, S = _check(src, idx, params)
    lib = _lib.init(src.device.index)
    if mean is None:
        mean = contrast_mean(src, idx, params)
    if mean.dtype != torch.float32 or tuple(mean.shape) != (B,) or not mean.is_cuda or not mean.is_contiguous():
        raise _lib.PsgError(f"sprites: mean must be a contiguous fp32 [{B}] GPU tensor")
    out = torch.empty(B, 3, S, S, dtype=torch.float32, device=src.device)
    _lib.check(lib.psg_sprite_augment(_lib.ptr(src), N, _lib.ptr(idx), _lib.ptr(params), _lib.ptr(mean), _lib.ptr(out), B, S,
                                      _lib.stream_ptr()), "psg_sprite_augment")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# text inputs: the token ids of every description, resident like the images
# ---------------------------------------------------------------------------------------------------------------------
MAX_LENGTH = 256       # the reference TextEncoder's truncation


def tokenize_rows(texts, tokenizer, max_length: int = MAX_LENGTH):
    """[[id, ...]] - the reference's tokenizer call per text (truncation at max_length, special tokens as the tokenizer adds
    them), no padding."""
    return [list(tokenizer(t, truncation=True, max_length=max_length)["input_ids"]) for t in texts]


def padded_batch(rows, pad_id: int, S: int = None):
    """Host restatement of psg_token_batch over lists of ids: (input_ids, attention_mask) int64 [B, S], S = the longest row."""
    S = max(len(r) for r in rows) if S is None else S
    ids = torch.full((len(rows), S), int(pad_id), dtype=torch.int64)
    mask = torch.zeros(len(rows), S, dtype=torch.int64)
    for b, r in enumerate(rows):
        n = min(len(r), S)
        ids[b, :n] = torch.tensor(r[:n], dtype=torch.int64)
        mask[b, :n] = 1
    return ids, mask


def token_batch(table, lens, idx, S: int, pad_id: int):
    """psg_token_batch: (input_ids, attention_mask) int64 [B, S] and kv_len int32 [B] of the rows `idx` of `table`."""
    if not (table.is_cuda and lens.is_cuda and idx.is_cuda):
        raise _lib.PsgError("token batches need GPU tensors: the HIP kernel is the only implementation")
    if table.dtype != torch.int32 or table.dim() != 2 or not table.is_contiguous():
        raise _lib.PsgError(f"tokens: table must be a contiguous int32 [N, L] tensor, got {table.dtype} {tuple(table.shape)}")
    N, L = table.shape
    if lens.dtype != torch.int32 or tuple(lens.shape) != (N,) or not lens.is_contiguous():
        raise _lib.PsgError(f"tokens: lens must be a contiguous int32 [{N}] tensor")
    if idx.dtype != torch.int64 or idx.dim() != 1 or not idx.is_contiguous():
        raise _lib.PsgError("tokens: idx must be a contiguous int64 [B] tensor")
    B, S = idx.shape[0], int(S)
    lib = _lib.init(table.device.index)
    ids = torch.empty(B, S, dtype=torch.int64, device=table.device)
    mask = torch.empty(B, S, dtype=torch.int64, device=table.device)
    kv_len = torch.empty(B, dtype=torch.int32, device=table.device)
    _lib.check(lib.psg_token_batch(_lib.ptr(table), _lib.ptr(lens), N, L, _lib.ptr(idx), B, S, int(pad_id), _lib.ptr(ids),
                                   _lib.ptr(mask), _lib.ptr(kv_len), _lib.stream_ptr()), "psg_token_batch")
    return ids, mask, kv_len


class TokenTable:
    """The tokenizer's ids of `dataset.meta(i)["full_description"]` for every row, made once on the host: `table` int32 [N, L]
    on the dataset's device (right-padded with `pad_id`, L the longest row), `lens` int32 [N] there, `lens_host` a list.
    `batch` then gives what `tokenizer(texts, padding=True, truncation=True, max_length=max_length)` returns for a batch's
    texts, from one launch and no host work."""

    def __init__(self, dataset, tokenizer, max_length: int = MAX_LENGTH):
        pad = getattr(tokenizer, "pad_token_id", None)
        self.pad_id = 0 if pad is None else int(pad)
        self.max_length = int(max_length)
        rows = tokenize_rows([dataset.meta(i)["full_description"] for i in range(len(dataset))], tokenizer, self.max_length)
        self.lens_host = [len(r) for r in rows]
        host, _ = padded_batch(rows, self.pad_id) if rows else (torch.zeros(0, 1, dtype=torch.int64), None)
        self.table = host.to(torch.int32).to(dataset.device)
        self.lens = torch.tensor(self.lens_host, dtype=torch.int32).to(dataset.device)

    def __len__(self) -> int:
        return len(self.lens_host)

    def batch(self, idx_dev, rows_host):
        """(input_ids, attention_mask) int64 [B, S] of the dataset rows `idx_dev` (int64, device); `rows_host` are the same
        rows on the host, from which the padded length S = the longest of them comes without a device read."""
        S = max(self.lens_host[int(r)] for r in rows_host)
        ids, mask, _ = token_batch(self.table, self.lens, idx_dev, S, self.pad_id)
        return ids, mask


# ---------------------------------------------------------------------------------------------------------------------
# the draws (pure torch on the given device, no host sync)
# ---------------------------------------------------------------------------------------------------------------------
def identity_params(B: int, S: int, device="cpu"):
    """[B, 16] rows that leave the image as stored: the val / test path."""
    row = [0, 1, 0, 0, 0, 1, 0, 0, 1, 1, 1, 0, 0, 0, S, S]
    return torch.tensor(row, dtype=torch.float32, device=device).repeat(B, 1)


def rotation_coefficients(angle, S: int):
    """fp64 [B, 6]: the inverse affine PIL's Image.rotate(angle, expand=False, center=None) builds (PIL/Image.py): centre S/2,
    cos and sin rounded to 15 decimals, the same operation order; angle 0 is the identity."""
    angle = torch.remainder(angle.to(torch.float64), 360.0)
    rad = -torch.deg2rad(angle)
    cos, sin = torch.round(torch.cos(rad), decimals=15), torch.round(torch.sin(rad), decimals=15)
    c0 = S / 2
    a, b, d, e = cos, sin, -sin, cos
    c = (a * -c0 + b * -c0 + 0.0) + c0
    f = (d * -c0 + e * -c0 + 0.0) + c0
    m = torch.stack([a, b, c, d, e, f], dim=1)
    ident = torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], dtype=torch.float64, device=angle.device)
    return torch.where((angle == 0)[:, None], ident, m)


def crop_candidates(B: int, S: int, generator=None, device="cpu"):
    """(w, h) int64 [B, 10]: RandomResizedCrop's ten tries per sample - area S*S*U(0.9, 1), log-ratio U(log 0.9, log 1.1),
    w = round(sqrt(area * ratio)), h = round(sqrt(area / ratio))."""
    kw = dict(dtype=torch.float64, device=device, generator=generator)
    area = S * S * (0.9 + 0.1 * torch.rand(B, 10, **kw))
    lo, hi = math.log(0.9), math.log(1.1)
    ratio = torch.exp(lo + (hi - lo) * torch.rand(B, 10, **kw))
    w = torch.round(torch.sqrt(area * ratio)).to(torch.int64)
    h = torch.round(torch.sqrt(area / ratio)).to(torch.int64)
    return w, h


def pick_crop(w, h, S: int, ui, uj):
    """(i, j, h, w) int64 [B]: the first candidate with 0 < w <= S and 0 < h <= S, else the whole image (the reference's
    fallback for a square image); i ~ randint(0, S - h + 1), j ~ randint(0, S - w + 1) from the uniforms ui, uj in [0, 1)."""
    valid = (w > 0) & (w <= S) & (h > 0) & (h <= S)
    first = torch.argmax(valid.to(torch.int64), dim=1, keepdim=True)          # the first maximum: the first valid try
    found = valid.any(dim=1)
    full = torch.full_like(first[:, 0], S)
    ws, hs = torch.where(found, w.gather(1, first)[:, 0], full), torch.where(found, h.gather(1, first)[:, 0], full)
    i = torch.minimum(torch.floor(ui * (S - hs + 1)).to(torch.int64), S - hs)
    j = torch.minimum(torch.floor(uj * (S - ws + 1)).to(torch.int64), S - ws)
    return i, j, hs, ws


def draw_params(B: int, S: int, generator=None, device="cpu"):
    """fp32 [B, 16]: one augmentation per sample with torchvision's distributions - flip with p = 0.5; angle ~ U(-10, 10); the
    order of the colour ops uniform over the 24 permutations (randperm(4)); brightness, contrast, saturation ~ U(0.9, 1.1);
    hue ~ U(-0.05, 0.05); RandomResizedCrop as in crop_candidates / pick_crop.  Everything is drawn and computed in fp64 and
    rounded to fp32 once."""
    kw = dict(dtype=torch.float64, device=device, generator=generator)
    u = torch.rand(B, 9, **kw)
    flip = (u[:, 0] < 0.5).to(torch.float64)
    rot = rotation_coefficients(-10.0 + 20.0 * u[:, 1], S)
    order = torch.floor(u[:, 2] * 24).clamp_(max=23)
    colour = 0.9 + 0.2 * u[:, 3:6]
    hue = -0.05 + 0.1 * u[:, 6]
    w, h = crop_candidates(B, S, generator, device)
    i, j, hs, ws = pick_crop(w, h, S, u[:, 7], u[:, 8])
    cols = [flip[:, None], rot, order[:, None], colour, hue[:, None]] + [t.to(torch.float64)[:, None] for t in (i, j, hs, ws)]
    return torch.cat(cols, dim=1).to(torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# loaders
# ---------------------------------------------------------------------------------------------------------------------
def split_indices(total: int, val_split: float, test_split: float, seed: int):
    """(train, val, test) index lists: exactly torch.utils.data.random_split(range(total), [train, val, test],
    generator=torch.Generator().manual_seed(seed)) with the reference's sizes."""
    test_size, val_size = int(total * test_split), int(total * val_split)
    train_size = total - val_size - test_size
    parts = torch.utils.data.random_split(range(total), [train_size, val_size, test_size],
                                          generator=torch.Generator().manual_seed(seed))
    return tuple(list(p.indices) for p in parts)


class SpriteLoader:
    """Batches of the reference's dict - image (fp32 [B, 3, S, S] on the dataset's device), description, full_description,
    national_number (int64 tensor), name - over `indices` of a SpriteDataset.  With `tokens` (a TokenTable of the dataset) a
    batch also carries input_ids, attention_mask (int64 [B, S], the tokenizer's padded batch of full_description) and index
    (int64 [B], the dataset rows), all on the device.

    augment=True: shuffled and augmented from generators seeded `seed + epoch`, so every data-parallel rank sees the same
    global batches (ddp.ShardedLoader slices them).  The epoch advances by one per iteration; `set_epoch` pins it."""

    def __init__(self, dataset, indices, batch_size: int, augment: bool, drop_last: bool, seed: int = 42, tokens=None):
        self.dataset, self.indices, self.batch_size, self.tokens = dataset, list(indices), int(batch_size), tokens
        self.augment, self.drop_last, self.seed, self.epoch = bool(augment), bool(drop_last), int(seed), 0
        if self.batch_size <= 0:
            raise ValueError("batch_size must be positive")

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    def __len__(self) -> int:
        n = len(self.indices)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        ds, dev, S = self.dataset, self.dataset.device, self.dataset.image_size
        epoch, self.epoch = self.epoch, self.epoch + 1
        order, gen = self.indices, None
        if self.augment:
            perm = torch.randperm(len(order), generator=torch.Generator().manual_seed(self.seed + epoch)).tolist()
            order = [order[k] for k in perm]
            gen = torch.Generator(device=dev).manual_seed(self.seed + epoch)
        order_dev = torch.tensor(order, dtype=torch.int64).to(dev)               # one upload per epoch
        for n in range(len(self)):
            lo, hi = n * self.batch_size, min((n + 1) * self.batch_size, len(order))
            idx = order_dev[lo:hi]
            if self.augment:
                image = augment(ds.images, idx, draw_params(hi - lo, S, gen, dev))
            else:                                                                # no contrast op: its mean is never read
                image = augment(ds.images, idx, identity_params(hi - lo, S, dev), mean=torch.zeros(hi - lo, device=dev))
            meta = [ds.meta(k) for k in order[lo:hi]]
            batch = {key: [m[key] for m in meta] for key in ("description", "full_description", "name")}
            batch["national_number"] = torch.tensor([m["national_number"] for m in meta], dtype=torch.int64)
            batch["image"] = image
            if self.tokens is not None:
                batch["input_ids"], batch["attention_mask"] = self.tokens.batch(idx, order[lo:hi])
                batch["index"] = idx
            yield batch


def create_data_loaders(csv_path: str, image_dir: str, batch_size: int = 32, val_split: float = 0.1, test_split: float = 0.1,
                        image_size: int = 215, num_workers: int = 4, pin_memory: bool = True, seed: int = 42,
                        background_color: Union[str, Tuple[int, int, int]] = "white", device=None, tokenizer=None):
    """The reference's create_data_loaders (src/data/dataset_improved.py:228-317): (train, val, test).  The same split (seed),
    train shuffled + augmented with drop_last, val / test sequential and un-augmented.  num_workers and pin_memory are
    accepted and ignored: there are no workers and nothing to pin.  `tokenizer`: the three loaders share one TokenTable of
    the dataset and their batches carry input_ids / attention_mask / index."""
    dataset = SpriteDataset(csv_path, image_dir, image_size=image_size, background_color=background_color, device=device)
    train, val, test = split_indices(len(dataset), val_split, test_split, seed)
    tokens = None if tokenizer is None else TokenTable(dataset, tokenizer)
    return (SpriteLoader(dataset, train, batch_size, augment=True, drop_last=True, seed=seed, tokens=tokens),
            SpriteLoader(dataset, val, batch_size, augment=False, drop_last=False, seed=seed, tokens=tokens),
            SpriteLoader(dataset, test, batch_size, augment=False, drop_last=False, seed=seed, tokens=tokens))
