"""The DEFINITION of a face chip (include/frhip.h fr_face_chips_u8), in NumPy integers: csrc/face_chips.hip is
held to these bytes with ``array_equal``.

A chip is one record ``(frame, x0, y0, side)``: the square ``[x0, x0 + side) x [y0, y0 + side)`` of frame ``frame``, in frame
pixels, anywhere - partly or wholly outside the frame -, resampled to ``S x S`` BGR bytes.  A pixel outside the frame reads as
the fill colour.  With ``L = side``, on one axis, output ``j`` weighs source position ``p`` (relative to the square's origin):

* box regime, ``L >= S`` (the exact area average): a source pixel is S units long, an output pixel L; ``w`` is the overlap of
  ``[p S, (p + 1) S)`` with ``[j L, (j + 1) L)``; the weights of an output sum to ``T = L``;
* bilinear regime, ``L < S`` (half-pixel centres): ``n = (2 j + 1) L - S``, ``p = floor(n / 2 S)`` (toward minus infinity: -1 at
  the leading edge), ``t = n - 2 S p``; the taps are ``p`` (weight ``2 S - t``) and ``p + 1`` (weight ``t``), NOT clamped to the
  square: -1 and L read the frame's own neighbouring pixels; the weights sum to ``T = 2 S``.

The value is ``(sum_y sum_x w_y w_x pix + T^2 // 2) // T^2`` per channel: round half up, the identity at ``L == S``.  The largest
sum, ``255 * 4096^2 + 4096^2 // 2``, fits an unsigned 32-bit accumulator.

A record whose frame index is outside the batch, whose side is outside ``1 .. MAX_SIDE``, with a coordinate beyond ``+-2^20`` or
whose frame is missing (None, or with a non-positive side) gives a chip of pure fill colour.

``chip`` works from the frame's rows (a horizontal pass over the rows that exist, then the vertical one), never from an
``L x L`` square; ``chip_loop`` is the rule as it reads, per output pixel (slow: small cases only).
tests/test_chip_ref_host.py holds the two equal."""
import numpy as np

MAX_SIDE = 4096                # FR_CHIP_MAX_SIDE
MIN_SIZE, MAX_SIZE = 16, 256
COORD_LIMIT = 1 << 20


def axis_weights(L, S):
    """``(first, w)``: ``w`` int64 [S, m], the weight of source position ``first + k`` for output ``j`` in ``w[j, k]``, and the
    sum ``T`` of a row of it is L (box) or 2 S (bilinear)."""
    j = np.arange(S, dtype=np.int64)[:, None]
    if L >= S:
        p = np.arange(L, dtype=np.int64)[None, :]
        w = np.minimum((j + 1) * L, (p + 1) * S) - np.maximum(j * L, p * S)
        return 0, np.maximum(w, 0)
    n = (2 * j + 1) * L - S
    p0 = n // (2 * S)                                      # floor: -1 at the leading edge
    t = n - 2 * S * p0
    p = np.arange(-1, L + 1, dtype=np.int64)[None, :]
    return -1, (p == p0) * (2 * S - t) + (p == p0 + 1) * t


def valid_record(rec, nframes):
    f, x0, y0, side = (int(v) for v in rec)
    return 0 <= f < nframes and 1 <= side <= MAX_SIDE and abs(x0) <= COORD_LIMIT and abs(y0) <= COORD_LIMIT


def _frame_of(frames, rec):
    if not valid_record(rec, len(frames)):
        return None
    fr = frames[int(rec[0])]
    if fr is None:
        return None
    fr = np.asarray(fr)
    assert fr.dtype == np.uint8 and fr.ndim == 3 and fr.shape[2] == 3
    return fr if fr.shape[0] > 0 and fr.shape[1] > 0 else None


def _in_frame(first, w, origin, extent):
    """the columns of ``w`` whose source position lies inside ``[0, extent)``: (the frame's range a:b, w[:, those])"""
    a = max(origin + first, 0)
    b = min(origin + first + w.shape[1], extent)
    if a >= b:
        return 0, 0, w[:, :0]
    return a, b, w[:, a - origin - first:b - origin - first]


def chip(frames, rec, S, fill=(0, 0, 0)):
    """``frames``: a sequence of BGR uint8 [H, W, 3] pictures (None: a missing frame) -> uint8 [S, S, 3]"""
    assert MIN_SIZE <= S <= MAX_SIZE
    fillv = np.asarray([int(c) & 255 for c in fill], np.int64)
    fr = _frame_of(frames, rec)
    if fr is None:
        return np.broadcast_to(fillv.astype(np.uint8), (S, S, 3)).copy()
    _, x0, y0, L = (int(v) for v in rec)
    H, W, _ = fr.shape
    first, w = axis_weights(L, S)
    T = int(w[0].sum())
    xa, xb, wx = _in_frame(first, w, x0, W)
    ya, yb, wy = _in_frame(first, w, y0, H)
    rows = fr[ya:yb, xa:xb].astype(np.int64)                                    # the rows and columns that exist
    # horizontal pass: per existing row and output column the row sum, <= 255 T
    h = np.einsum("jx,yxc->yjc", wx, rows) + (T - wx.sum(1))[None, :, None] * fillv
    # vertical pass; a row outside the frame has the row sum T fill
    v = np.einsum("iy,yjc->ijc", wy, h) + (T - wy.sum(1))[:, None, None] * (T * fillv)
    assert v.max(initial=0) + T * T // 2 < 1 << 32
    return ((v + T * T // 2) // (T * T)).astype(np.uint8)


def chip_loop(frames, rec, S, fill=(0, 0, 0)):
    """the same chip, output pixel by output pixel as the rule reads"""
    fillv = [int(c) & 255 for c in fill]
    fr = _frame_of(frames, rec)
    out = np.empty((S, S, 3), np.uint8)
    if fr is None:
        out[:] = fillv
        return out
    _, x0, y0, L = (int(v) for v in rec)
    H, W, _ = fr.shape

    def taps(j):
        if L >= S:
            lo, hi = j * L, (j + 1) * L
            return [(p, min(hi, (p + 1) * S) - max(lo, p * S)) for p in range(lo // S, (hi + S - 1) // S)]
        n = (2 * j + 1) * L - S
        p = n // (2 * S)
        t = n - 2 * S * p
        return [(p, 2 * S - t), (p + 1, t)]
    T = L if L >= S else 2 * S
    for i in range(S):
        for j in range(S):
            acc = [0, 0, 0]
            for py, wy in taps(i):
                for px, wx in taps(j):
                    y, x = y0 + py, x0 + px
                    pix = fr[y, x] if 0 <= y < H and 0 <= x < W else fillv
                    for c in range(3):
                        acc[c] += wy * wx * int(pix[c])
            out[i, j] = [(a + T * T // 2) // (T * T) for a in acc]
    return out


def chips(frames, records, S, fill=(0, 0, 0)):
    """uint8 [F, S, S, 3]: every record's chip"""
    records = np.asarray(records, np.int64).reshape(-1, 4)
    out = np.empty((len(records), S, S, 3), np.uint8)
    for k, rec in enumerate(records):
        out[k] = chip(frames, rec, S, fill)
    return out
