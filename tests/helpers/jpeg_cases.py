"""Pictures and cached reference encodings shared by the JPEG tests (the definition against PIL on the CPU, the kernel against
the definition on the GPU)."""
import functools

import numpy as np

from tests.helpers import jpeg_ref

# (H, W): below and at the MCU; partial MCUs on both sides; two rows, wide (one restart marker); nine rows (RSTm wraps past 7)
SIZES = [(1, 1), (8, 8), (16, 16), (37, 51), (40, 56), (17, 300), (144, 176)]
QUALITIES = [10, 75, 95]
EXTRA = [((40, 56), 1), ((40, 56), 50)]                 # the ends of the quality rule's two branches, at one size
CONTENTS = ("noise", "ramp", "flat0", "flat255", "blocks", "pixels")
CASES = [(hw, q) for hw in SIZES for q in QUALITIES] + EXTRA


def picture(kind, h, w):
    """uint8 [h, w, 3] BGR"""
    y, x = np.mgrid[0:h, 0:w]
    if kind == "noise":
        return np.random.default_rng(1000 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "ramp":
        return np.stack([(3 * x + y) % 256, (x + 5 * y) % 256, (2 * x + 2 * y) % 256], axis=-1).astype(np.uint8)
    if kind == "flat0":
        return np.zeros((h, w, 3), np.uint8)
    if kind == "flat255":
        return np.full((h, w, 3), 255, np.uint8)
    if kind == "blocks":                                 # black / white 8 x 8 checkerboard
        return np.repeat((((y // 8 + x // 8) & 1) * 255).astype(np.uint8)[..., None], 3, axis=-1)
    if kind == "pixels":                                 # 1-pixel checkerboard
        return np.repeat((((y + x) & 1) * 255).astype(np.uint8)[..., None], 3, axis=-1)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def reference(kind, h, w, quality):
    """(bytes, stats) of jpeg_ref.encode for picture(kind, h, w)"""
    stats = jpeg_ref.new_stats()
    return jpeg_ref.encode(picture(kind, h, w), quality, stats), stats


def psnr(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    mse = float((d * d).mean())
    return 99.0 if mse == 0 else 10 * np.log10(255.0 * 255.0 / mse)
