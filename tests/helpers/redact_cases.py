"""Inputs for the redaction kernel's tests: packed region tables (include/frhip.h fr_redact_u8) built by hand or from a seed, with
garbage in every slot behind a frame's count, and the expected pictures from tests/helpers/redact_ref.py."""
import numpy as np

from tests.helpers import redact_ref

SIZES = [(1, 1), (3, 5), (8, 8), (17, 33), (37, 51), (70, 133)]        # H, W; the last: three tiles each way at block 16 .. 64
BLOCKS = [2, 3, 5, 7, 16, 64]
BIG = 1 << 20


def noise(rng, n, H, W):
    return rng.integers(0, 256, (n, H, W, 3), dtype=np.int64).astype(np.uint8)


def shapes_of_regions(H, W):
    """One region list per entry, each a frame's worth: the shapes the kernel has to get right on an H x W picture."""
    cx, cy = W // 2, H // 2
    return [
        [(cx, cy, cx, cy)],                                                      # 1 x 1
        [(1, 1, max(1, W - 2), max(1, H - 2))],                                  # cuts cells on all four sides (block > 1)
        [(0, 0, W - 1, H - 1)],                                                  # the whole picture
        [(-5, -7, cx, cy)], [(cx, cy, W + 9, H + 4)],                            # partly outside: negative corners, past W / H
        [(-BIG, -BIG, BIG, BIG)], [(-BIG, cy, BIG, cy)], [(cx, -BIG, cx, BIG)],  # +-2^20: around it, a row, a column
        [(W, 0, W + 20, H)], [(-30, -30, -1, -1)], [(0, H, W, H + 50)],          # wholly outside
        [(-(1 << 24), 0, -BIG - 1, H)],                                          # beyond the clamp, outside
        [(0, 0, W // 3, H - 1), (W // 3 - 2, 0, W - 1, H // 2)],                 # two that overlap
        [(cx, 0, W - 1, cy)] * 2,                                                # the same region twice
    ]


def pack(per_frame, cap, seed=0, counts=None):
    """``per_frame``: per frame a list of rectangles -> (counts int32 [n], regions int32 [n, cap, 4]).  Every slot behind a
    frame's count is seeded garbage: nothing there may be read.  ``counts`` overrides the counts."""
    rng = np.random.default_rng(seed)
    n = len(per_frame)
    regions = rng.integers(-2 ** 31, 2 ** 31 - 1, (n, cap, 4), dtype=np.int64).astype(np.int32)
    cnt = np.zeros(n, np.int32)
    for f, rs in enumerate(per_frame):
        assert len(rs) <= cap
        cnt[f] = len(rs)
        if rs:
            regions[f, :len(rs)] = np.asarray(rs, np.int64).astype(np.int32)
    if counts is not None:
        cnt[:] = counts
    return cnt, regions


def random_regions(rng, count, H, W, spread=20):
    out = []
    for _ in range(count):
        xs, ys = np.sort(rng.integers(-spread, W + spread, 2)), np.sort(rng.integers(-spread, H + spread, 2))
        out.append((int(xs[0]), int(ys[0]), int(xs[1]), int(ys[1])))
    return out


def expected(frames, counts, regions, block, mode=0, colour=(0, 0, 0)):
    """redact_ref over a batch (an array or a list of frames): a list of uint8 [H, W, 3]"""
    return [redact_ref.redact_results(frames[f], counts[f], regions[f], block, mode, colour) for f in range(len(frames))]


def bgr_word(colour):
    b, g, r = (int(v) & 255 for v in colour)
    return b | (g << 8) | (r << 16)
