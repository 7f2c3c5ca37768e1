"""The case list of the image hand-over tests (test_image_prep_host.py, test_image_prep_gpu.py): (w, h, n_px), each in mode RGB and mode L, random bytes from
a fixed seed.  The smallest shapes that reach every branch: identity; crop only (with the odd margin 3, where half-to-even and floor differ); upscale; downscale
with 151 coefficients per output pixel; one-pixel sides; windows at both edges of the bounds tables.  Images and their PIL crops are computed once per
process and are read-only."""
import functools
import zlib

import numpy as np

CASES_16 = [(16, 16, 16), (17, 16, 16), (19, 16, 16), (16, 40, 16), (31, 17, 16), (2, 3, 16), (1, 5, 16), (5, 1, 16), (600, 640, 16), (640, 600, 16)]
CASES_32 = [(37, 91, 32), (1000, 40, 32), (40, 1000, 32), (33, 47, 32), (64, 64, 32), (20, 20, 32), (100, 60, 32)]
CASES_224 = [(500, 375, 224), (375, 500, 224), (224, 300, 224), (225, 224, 224), (100, 60, 224)]          # on the GPU only
CASES_CPU = CASES_16 + CASES_32


@functools.lru_cache(maxsize=None)
def case_image(w, h, mode):
    rng = np.random.default_rng(zlib.crc32(f"{w}x{h}{mode}".encode()))
    img = rng.integers(0, 256, size=(h, w, 3) if mode == "RGB" else (h, w), dtype=np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _pil_crop(w, h, mode, n):
    from PIL import Image
    from speechclip_amd.data.image_transforms import clip_resize_center_crop_u8
    out = clip_resize_center_crop_u8(Image.fromarray(case_image(w, h, mode), mode), n).copy()
    out.setflags(write=False)
    return out


def pil_crop(img, n):
    """uint8 [n, n, 3]: the existing host function on a case image."""
    h, w = img.shape[:2]
    return _pil_crop(w, h, "RGB" if img.ndim == 3 else "L", n)
