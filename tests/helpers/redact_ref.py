"""The DEFINITION of face redaction (include/frhip.h fr_redact_u8), in NumPy integers: csrc/redact.hip is held to
these bytes with ``array_equal``.

One BGR ``uint8 [H, W, 3]`` picture, ``regions`` ``int32 [m, 4]`` of inclusive rectangles ``x1, y1, x2, y2`` (ordered; anywhere,
negative and past the picture included) and a ``block``:

* the grid of ``block x block`` cells is anchored at the picture's origin: pixel (x, y) lies in cell (x // block, y // block);
  the cells of the last column and row are cut at W and H, so a cell has n = cw * ch <= block^2 pixels;
* a pixel that no region holds keeps its bytes;
* mode 0, pixelate: a held pixel takes, per channel, ``(S + n // 2) // n`` with S the sum of the ORIGINAL bytes of its whole
  cell - the cell's pixels outside every region included;
* mode 1, fill: a held pixel takes ``colour``.

The grid does not depend on the regions, so overlapping regions, a region listed twice and any order of the list give the bytes
of the union.  Two forms are kept: ``redact`` (vectorised) and ``redact_loop`` (per pixel, as the rule reads);
tests/test_redact_ref_host.py holds them equal."""
import numpy as np

PIXELATE, FILL = 0, 1
COORD_LIMIT = 1 << 20          # coordinates beyond +-2^20 are clamped there, as the kernel clamps them


def _regions(regions):
    r = np.asarray(regions, np.int64).reshape(-1, 4)
    return np.clip(r, -COORD_LIMIT, COORD_LIMIT)


def held_mask(shape_hw, regions):
    """bool [H, W]: the pixels at least one region holds"""
    H, W = shape_hw
    m = np.zeros((H, W), bool)
    for x1, y1, x2, y2 in _regions(regions).tolist():
        xa, xb, ya, yb = max(x1, 0), min(x2, W - 1), max(y1, 0), min(y2, H - 1)
        if xa <= xb and ya <= yb:
            m[ya:yb + 1, xa:xb + 1] = True
    return m


def cell_means(frame, block):
    """uint8 [ceil(H / block), ceil(W / block), 3]: every cell's rounded mean, (S + n // 2) // n"""
    H, W, _ = frame.shape
    ys, xs = np.arange(H) // block, np.arange(W) // block
    s = np.zeros((ys[-1] + 1, xs[-1] + 1, 3), np.int64)
    n = np.zeros((ys[-1] + 1, xs[-1] + 1), np.int64)
    np.add.at(s, (ys[:, None], xs[None, :]), frame.astype(np.int64))
    np.add.at(n, (ys[:, None], xs[None, :]), 1)
    return ((s + (n // 2)[..., None]) // n[..., None]).astype(np.uint8)


def redact(frame, regions, block, mode=PIXELATE, colour=(0, 0, 0)):
    """``frame`` uint8 [H, W, 3] -> a new frame with the regions redacted (the vectorised form)"""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3 and block >= 1 and mode in (PIXELATE, FILL)
    H, W, _ = frame.shape
    out = frame.copy()
    m = held_mask((H, W), regions)
    if mode == FILL:
        out[m] = np.asarray(colour, np.int64) & 255
        return out
    full = cell_means(frame, block)[(np.arange(H) // block)[:, None], (np.arange(W) // block)[None, :]]
    out[m] = full[m]
    return out


def redact_loop(frame, regions, block, mode=PIXELATE, colour=(0, 0, 0)):
    """the same picture, pixel by pixel as the rule reads (slow: small pictures only)"""
    frame = np.asarray(frame)
    H, W, _ = frame.shape
    regs = _regions(regions).tolist()
    out = frame.copy()
    for y in range(H):
        for x in range(W):
            if not any(x1 <= x <= x2 and y1 <= y <= y2 for x1, y1, x2, y2 in regs):
                continue
            if mode == FILL:
                out[y, x] = [int(c) & 255 for c in colour]
                continue
            cy, cx = y // block * block, x // block * block
            cell = frame[cy:min(cy + block, H), cx:min(cx + block, W)].reshape(-1, 3).astype(np.int64)
            n = len(cell)
            out[y, x] = (cell.sum(0) + n // 2) // n
    return out


def redact_results(frame, counts_row, regions_row, block, mode=PIXELATE, colour=(0, 0, 0)):
    """one frame of a packed batch: the first ``counts_row`` regions of ``regions_row`` int32 [cap, 4] (clamped to 0 .. cap)"""
    k = max(0, min(int(counts_row), len(regions_row)))
    return redact(frame, np.asarray(regions_row)[:k], block, mode, colour)
