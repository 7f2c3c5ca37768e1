"""CLIP image pre-processing for `forward_image(list_of_paths)` (avssl/model/kwClip.py:504-519 -> ClipModel.prep_image, clip_official.py:151-164 ->
the `preprocess` that `clip.load` returns = clip/clip.py `_transform(n_px)` [3P openai/CLIP]):

    Resize(n_px, BICUBIC)  ->  CenterCrop(n_px)  ->  convert("RGB")  ->  ToTensor()  ->  Normalize(CLIP mean, CLIP std)

torchvision is not installed; its PIL code path IS `Image.resize(..., BICUBIC)` + `Image.crop`, so the geometry below reproduces it with PIL alone:
the SHORTER side becomes n_px and the longer one int(n_px * long / short) (torchvision.transforms.functional.resize, int size), the crop window starts at
int(round((H - n_px) / 2)), int(round((W - n_px) / 2)) (center_crop).  The host part ends at uint8 HWC; scaling by 1/255 and the normalisation run on the
device (sc_image_normalize_u8) when the model lives there, so a batch crosses PCIe as bytes.  The second half of this file states the same geometry as an
integer plan that the device executes on the decoded bytes (sc_image_prep_u8), with PIL's result on every byte; then only the decode stays on the host."""
import functools
import math
from typing import List, NamedTuple, Sequence, Union

import numpy as np
import torch

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def clip_resize_center_crop_u8(img, n_px: int = 224) -> np.ndarray:
    """PIL image (any mode / size) -> uint8 [n_px, n_px, 3], the geometric half of clip's `_transform`."""
    from PIL import Image
    w, h = img.size
    if not (w == h == n_px):
        if w <= h:
            nw, nh = n_px, int(n_px * h / w)
        else:
            nw, nh = int(n_px * w / h), n_px
        if (nw, nh) != (w, h):
            img = img.resize((nw, nh), Image.BICUBIC)
        top, left = int(round((nh - n_px) / 2.0)), int(round((nw - n_px) / 2.0))
        img = img.crop((left, top, left + n_px, top + n_px))
    return np.asarray(img.convert("RGB"), dtype=np.uint8)


# ---- the same geometry as an integer plan the device executes (csrc/image_prep.hip, ops.image_prep) ---------------------------------------------------
# Pillow's 8-bit resampler is a pure integer algorithm once its coefficient tables exist: fixed-point weights with 22 fractional bits, an int32 accumulator
# that starts at one half, an arithmetic shift and a clamp to a byte; the horizontal pass runs first and the vertical pass works on ITS uint8 result.  The
# tables are restated here from that public algorithm (Pillow is third-party and not vendored) and checked byte for byte against the installed Pillow by
# tests/test_image_prep_host.py.  Only BICUBIC on 8-bit RGB / L images is restated; every other mode keeps the PIL path above.
PRECISION_BITS = 22          # 32 - 8 (pixel) - 2 (head room): Pillow's 8 bits-per-channel fixed point


def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@functools.lru_cache(maxsize=256)
def resample_coeffs(in_size: int, out_size: int):
    """Bicubic tables of one axis: (coef int32 [out, ksize], bounds int32 [out, 2] = (first input pixel, number of taps) per output pixel).  Cached per size
    pair; the arrays are read-only.  The weight sum is the SEQUENTIAL double sum in tap order (a pairwise sum rounds differently and moves a coefficient by
    one unit in rare cases)."""
    if in_size <= 0 or out_size <= 0:
        raise ValueError(f"resample_coeffs: sizes must be positive, got {in_size} -> {out_size}")
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    coef = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        coef[xx, :xmax] = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w]
        bounds[xx] = (xmin, xmax)
    coef.setflags(write=False)
    bounds.setflags(write=False)
    return coef, bounds


class ClipWindowPlan(NamedTuple):
    """What the device computes for one w x h image: the n_px x n_px window at (left, top) of the nw x nh resize, and nothing outside it."""
    w: int
    h: int
    n_px: int
    nw: int
    nh: int
    left: int
    top: int
    hpass: bool          # the horizontal pass runs (nw != w)
    vpass: bool          # the vertical pass runs (nh != h)
    row0: int            # first and last INPUT row the window needs: the horizontal pass produces exactly these
    row1: int


@functools.lru_cache(maxsize=4096)
def clip_window_plan(w: int, h: int, n_px: int) -> ClipWindowPlan:
    """The geometry of `clip_resize_center_crop_u8` as a plan: same sizes, same crop origin (Python's round-half-to-even)."""
    if w <= 0 or h <= 0 or n_px <= 0:
        raise ValueError(f"clip_window_plan: sizes must be positive, got {w} x {h} -> {n_px}")
    if w == h == n_px:
        return ClipWindowPlan(w, h, n_px, w, h, 0, 0, False, False, 0, n_px - 1)
    if w <= h:
        nw, nh = n_px, int(n_px * h / w)
    else:
        nw, nh = int(n_px * w / h), n_px
    top, left = int(round((nh - n_px) / 2.0)), int(round((nw - n_px) / 2.0))
    row0, row1 = top, top + n_px - 1
    if nh != h:
        vb = resample_coeffs(h, nh)[1]
        row0, row1 = int(vb[top, 0]), int(vb[top + n_px - 1, 0] + vb[top + n_px - 1, 1] - 1)
    return ClipWindowPlan(w, h, n_px, nw, nh, left, top, nw != w, nh != h, row0, row1)


def execute_plan_numpy(img: np.ndarray, n_px: int) -> np.ndarray:
    """The plan run on the host in numpy (int64 accumulate): uint8 [h, w, 3] or [h, w] -> uint8 [n_px, n_px, 3].  The statement the device kernel is
    checked against on the CPU; not a data path."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3):
        raise ValueError(f"execute_plan_numpy: need uint8 [h, w, 3] or [h, w], got {img.dtype} {img.shape}")
    h, w = img.shape[:2]
    p = clip_window_plan(w, h, n_px)
    half = 1 << (PRECISION_BITS - 1)
    x = img.reshape(h, w, -1)[p.row0:p.row1 + 1].astype(np.int64)
    if p.hpass:
        coef, bounds = resample_coeffs(w, p.nw)
        cols = []
        for xx in range(p.left, p.left + n_px):
            x0, cnt = bounds[xx]
            acc = half + np.tensordot(x[:, x0:x0 + cnt], coef[xx, :cnt].astype(np.int64), axes=([1], [0]))
            cols.append(np.clip(acc >> PRECISION_BITS, 0, 255))
        x = np.stack(cols, axis=1)
    else:
        x = x[:, p.left:p.left + n_px]
    if p.vpass:
        coef, bounds = resample_coeffs(h, p.nh)
        rows = []
        for yy in range(p.top, p.top + n_px):
            y0, cnt = bounds[yy]
            acc = half + np.tensordot(coef[yy, :cnt].astype(np.int64), x[y0 - p.row0:y0 - p.row0 + cnt], axes=([0], [0]))
            rows.append(np.clip(acc >> PRECISION_BITS, 0, 255))
        x = np.stack(rows, axis=0)
    out = x.astype(np.uint8)
    return np.ascontiguousarray(np.broadcast_to(out, (n_px, n_px, 3)))


GEOM_FIELDS = 10          # SC_IMAGE_PREP_GEOM: w, h, C, left, top, row0, row1, passes, htab, vtab
HPASS, VPASS = 1, 2       # SC_IMAGE_PREP_HPASS / SC_IMAGE_PREP_VPASS


class ImageBatchPlan(NamedTuple):
    """The arguments of sc_image_prep_u8 for one ragged batch, as host arrays (include/speechclip_hip.h has the layout)."""
    images: list                 # uint8 arrays, C-contiguous, [h, w, 3] or [h, w]
    offsets: np.ndarray          # int64 [2, B]: byte offset of each image in the packed buffer, byte offset of its workspace share
    geom: np.ndarray             # int32 [B, GEOM_FIELDS]
    tables: np.ndarray           # int32 [T]: one record (in, out, ksize, bounds, coef) per distinct size pair
    packed_bytes: int
    workspace_bytes: int


def as_u8_image(img) -> np.ndarray:
    """A decoded image as `load_images_raw` returns it (array or host tensor) -> C-contiguous uint8 [h, w, 3] or [h, w]; anything else is refused."""
    if isinstance(img, torch.Tensor):
        if img.is_cuda:
            raise ValueError("image_prep takes host images (the batch crosses PCIe once, packed)")
        img = img.numpy()
    if not isinstance(img, np.ndarray) or img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3) or img.size == 0:
        raise ValueError(f"image_prep needs uint8 images [h, w, 3] (RGB) or [h, w] (L), got {getattr(img, 'dtype', type(img))} {getattr(img, 'shape', '')}")
    return np.ascontiguousarray(img)


def plan_image_batch(images: Sequence, n_px: int, pad_bytes: int = 0, plans: Sequence[ClipWindowPlan] = None) -> ImageBatchPlan:
    """Plans, tables and offsets of one batch.  `pad_bytes` bytes are left free in front of every image and behind the last one (tests fill them with 255 so
    that a read outside an image shows in the result); `plans` replaces clip_window_plan per image (tests: geometries CLIP's rule never produces)."""
    imgs = [as_u8_image(im) for im in images]
    B = len(imgs)
    offsets = np.zeros((2, B), dtype=np.int64)
    geom = np.zeros((B, GEOM_FIELDS), dtype=np.int32)
    recs, where, tlen = [], {}, 0

    def table(in_size, out_size):
        nonlocal tlen
        if (in_size, out_size) not in where:
            coef, bounds = resample_coeffs(in_size, out_size)
            rec = np.concatenate([np.array([in_size, out_size, coef.shape[1]], dtype=np.int32), bounds.reshape(-1), coef.reshape(-1)])
            where[(in_size, out_size)] = tlen
            recs.append(rec)
            tlen += rec.size
        return where[(in_size, out_size)]

    pos, ws = 0, 0
    for b, im in enumerate(imgs):
        h, w = im.shape[:2]
        C = 1 if im.ndim == 2 else 3
        p = clip_window_plan(w, h, n_px) if plans is None else plans[b]
        if (p.w, p.h, p.n_px) != (w, h, n_px):
            raise ValueError(f"image {b}: plan for {p.w} x {p.h} -> {p.n_px}, image is {w} x {h} -> {n_px}")
        pos += pad_bytes
        offsets[0, b], offsets[1, b] = pos, ws
        pos += im.size
        geom[b] = (w, h, C, p.left, p.top, p.row0, p.row1, (HPASS if p.hpass else 0) | (VPASS if p.vpass else 0),
                   table(w, p.nw) if p.hpass else 0, table(h, p.nh) if p.vpass else 0)
        if p.hpass:
            ws += (p.row1 - p.row0 + 1) * n_px * C
    tables = np.concatenate(recs) if recs else np.zeros(0, dtype=np.int32)
    return ImageBatchPlan(imgs, offsets, geom, tables, pos + pad_bytes, ws)


def load_images_raw(paths: Sequence[str], n_px: int = 224) -> List[np.ndarray]:
    """Decode only: one uint8 array per file, [h, w, 3] for mode RGB and [h, w] for mode L, at the file's own size.  A file of any other mode (P, 1, RGBA, LA,
    CMYK, I;16 ...) comes back as the [n_px, n_px, 3] result of `clip_resize_center_crop_u8`: PIL resamples those modes differently and they are not
    restated, and an n_px x n_px RGB array has the identity plan."""
    from PIL import Image
    out = []
    for p in paths:
        with Image.open(p) as im:
            if im.mode in ("RGB", "L"):
                out.append(np.asarray(im, dtype=np.uint8))
            else:
                out.append(clip_resize_center_crop_u8(im, n_px))
    return out


def load_images_u8(paths: Sequence[str], n_px: int = 224) -> torch.Tensor:
    """-> uint8 [B, n_px, n_px, 3] (host)."""
    from PIL import Image
    out = np.empty((len(paths), n_px, n_px, 3), dtype=np.uint8)
    for i, p in enumerate(paths):
        with Image.open(p) as im:
            out[i] = clip_resize_center_crop_u8(im, n_px)
    return torch.from_numpy(out)


def normalize_u8(u8: torch.Tensor, device: Union[str, torch.device] = "cpu") -> torch.Tensor:
    """uint8 [B, H, W, 3] -> f32 [B, 3, H, W] = (x / 255 - mean) / std on `device`: the HIP kernel on a GPU; plain tensor arithmetic on the host
    (DataLoader workers run this on CPUs -- data layer, avssl/data/base_dataset.py:101-108 -- not the hot path)."""
    device = torch.device(device)
    if device.type == "cuda":
        from .. import ops
        return ops.image_normalize_u8(u8.to(device, non_blocking=True).contiguous(), CLIP_MEAN, CLIP_STD)
    x = u8.to(torch.float32).div_(255.0).permute(0, 3, 1, 2)
    mean, std = torch.tensor(CLIP_MEAN).view(1, 3, 1, 1), torch.tensor(CLIP_STD).view(1, 3, 1, 1)
    return ((x - mean) / std).contiguous()


def clip_preprocess(n_px: int = 224):
    """The callable `clip.load` returns as `preprocess` (ClipModel.image_preprocess, clip_official.py:50): PIL image -> f32 [3, n_px, n_px]."""
    def _preprocess(img) -> torch.Tensor:
        return normalize_u8(torch.from_numpy(clip_resize_center_crop_u8(img, n_px).copy())[None])[0]
    return _preprocess
