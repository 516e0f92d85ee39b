"""JPEG files shared by the decoder's tests (the definition against PIL on the CPU, the kernels against the definition on the
GPU): written by Pillow at test time, and by the project's own encoder's definition (tests/helpers/jpeg_ref.py)."""
import functools
import io

import numpy as np
from PIL import Image

from tests.helpers import jpeg_decode_ref, jpeg_ref

SUBSAMPLINGS = {"444": 0, "422": 1, "420": 2}
WRITERS = {"plain": {}, "optimize": {"optimize": True}, "dri_row": {"restart_marker_rows": 1}, "dri_3": {"restart_marker_blocks": 3}}


def picture(kind, h, w, seed=0):
    """uint8 [h, w, 3] BGR: noise, ramps, or 8 x 8 flats"""
    rng = np.random.default_rng(100000 * seed + 1000 * h + w)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "ramp":
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([(3 * x + y) % 256, (x + 5 * y) % 256, (2 * x + 2 * y) % 256], axis=-1).astype(np.uint8)
    if kind == "flats":
        small = rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8, 3), dtype=np.uint8)
        return np.repeat(np.repeat(small, 8, axis=0), 8, axis=1)[:h, :w].copy()
    raise ValueError(kind)


def pil_file(bgr, quality, sampling, writer="plain", **more):
    """the JPEG file Pillow writes for a BGR picture; ``sampling``: "444" / "422" / "420" / "gray" (the picture's channel 0)"""
    buf = io.BytesIO()
    if sampling == "gray":
        Image.fromarray(np.ascontiguousarray(bgr[..., 0])).save(buf, "JPEG", quality=quality, **WRITERS[writer], **more)
    else:
        Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(buf, "JPEG", quality=quality, subsampling=SUBSAMPLINGS[sampling],
                                                                   **WRITERS[writer], **more)
    return buf.getvalue()


def pil_decode(data):
    """Pillow's decode of a file: uint8 [H, W, 3] BGR"""
    with Image.open(io.BytesIO(data)) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8)[..., ::-1])


@functools.lru_cache(maxsize=None)
def case(kind, h, w, quality, sampling, writer="plain", seed=0):
    """(file bytes, the definition's BGR picture of it): computed once, shared, not to be written to"""
    data = own_file(kind, h, w, quality, seed) if writer == "own" else pil_file(picture(kind, h, w, seed), quality, sampling, writer)
    bgr = jpeg_decode_ref.decode(data)[0]
    bgr.setflags(write=False)
    return data, bgr


def own_file(kind, h, w, quality, seed=0):
    """the file of the project's encoder (its definition): 4:2:0, one restart interval per MCU row"""
    return jpeg_ref.encode(picture(kind, h, w, seed), quality)


# the GPU test's grid: the smallest sizes that can go wrong - below, at and across the MCU, partial MCUs on both sides, widths
# 2 and 4 (chroma at most 2 wide: replication) and 5 (its first neighbour), and one size of several chunks
SIZES = [(1, 1), (8, 8), (16, 16), (17, 33), (37, 51), (9, 2), (9, 4), (9, 5)]
LARGE = (144, 176)
