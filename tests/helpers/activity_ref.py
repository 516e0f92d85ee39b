"""The activity gate in NumPy: the definition the device kernels (csrc/frame_activity.hip) are pinned to, byte for byte.

Written from the specification, not from the kernel.  A frame is BGR ``uint8 [H,W,3]``.  In exact integers
(int64 here; every intermediate fits int32: a pixel term is at most 65 408, a cell sum at most 65 280)::

    L = (29*B + 150*G + 77*R + 128) >> 8          per pixel; 29 + 150 + 77 = 256, so L is 0 .. 255
    m = (sum of L over the cell + 128) >> 8       per 16 x 16 cell, stored as uint8

with ``gh = H // 16`` rows of ``gw = W // 16`` cells, row-major; remainder rows and columns belong to no cell.

``GateRef`` keeps, per camera slot, ``grid`` (the cell means of the last frame judged active), ``geom`` (its (H, W), (0, 0):
none) and ``idle`` (consecutive inactive judgments) and applies the rule literally, frame by frame.
"""
import numpy as np

WEIGHTS = (29, 150, 77)          # B, G, R
CELL = 16


def luma(bgr):
    """int64 [H,W]: the luma of every pixel"""
    p = np.asarray(bgr).astype(np.int64)
    return (WEIGHTS[0] * p[..., 0] + WEIGHTS[1] * p[..., 1] + WEIGHTS[2] * p[..., 2] + 128) >> 8


def cell_means(bgr):
    """uint8 [gh*gw]: the cell means of one frame, row-major (empty when the frame holds no whole cell)"""
    bgr = np.asarray(bgr)
    assert bgr.ndim == 3 and bgr.shape[2] == 3 and bgr.dtype == np.uint8
    gh, gw = bgr.shape[0] // CELL, bgr.shape[1] // CELL
    lum = luma(bgr[:gh * CELL, :gw * CELL])
    sums = lum.reshape(gh, CELL, gw, CELL).sum(axis=(1, 3))
    return ((sums + 128) >> 8).astype(np.uint8).reshape(-1)


class GateRef:
    """State arrays of ``slots`` camera slots with ``cells`` bytes per grid row, and the rule."""

    def __init__(self, slots, cells, thr=4, min_cells=2, max_idle=0):
        assert 0 <= thr <= 255 and min_cells >= 1 and max_idle >= 0
        self.S, self.C = int(slots), int(cells)
        self.thr, self.min_cells, self.max_idle = int(thr), int(min_cells), int(max_idle)
        self.grid = np.zeros((self.S, self.C), np.uint8)
        self.geom = np.zeros((self.S, 2), np.int32)
        self.idle = np.zeros(self.S, np.int32)

    def judge_one(self, frame, s):
        """(changed, active, cur) of one frame for slot ``s``; moves the state.  ``cur``: the frame's cell means, None when
        the means are not defined for it (no whole cell, or more cells than a grid row holds)."""
        H, W = frame.shape[:2]
        cells = (H // CELL) * (W // CELL)
        if H < CELL or W < CELL or cells > self.C:
            return -1, 1, None
        cur = cell_means(frame)
        if not 0 <= s < self.S:
            return -1, 1, cur
        if tuple(self.geom[s]) != (H, W):
            changed = -1
        else:
            diff = np.abs(cur.astype(np.int64) - self.grid[s, :cells].astype(np.int64))
            changed = int((diff > self.thr).sum())
        active = changed < 0 or changed >= self.min_cells or (self.max_idle > 0 and self.idle[s] >= self.max_idle)
        if active:
            self.grid[s, :cells] = cur
            self.geom[s] = (H, W)
            self.idle[s] = 0
        else:
            self.idle[s] += 1
        return changed, int(active), cur

    def judge(self, frames, slots):
        """A batch: (changed int32 [N], active int32 [N], [cur per frame]); every slot at most once."""
        named = [s for s in slots if 0 <= s < self.S]
        assert len(set(named)) == len(named), "two frames of one batch name one slot"
        out = [self.judge_one(f, int(s)) for f, s in zip(frames, slots)]
        return (np.array([o[0] for o in out], np.int32), np.array([o[1] for o in out], np.int32), [o[2] for o in out])
