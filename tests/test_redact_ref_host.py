"""tests/helpers/redact_ref.py, the definition csrc/redact.hip is held to, against itself (no GPU): its vectorised form and its
per-pixel form give equal bytes, pixels outside every region stay, a cell wholly inside a region carries one value, and the
largest cell of all-255 bytes does not overflow."""
import numpy as np
import pytest

from tests.helpers import redact_ref

SIZES = [(1, 1), (3, 5), (8, 8), (17, 33), (37, 51)]
BLOCKS = [2, 3, 5, 8, 64]


def _regions(H, W):
    return np.array([(-5, -5, 2, 2), (1, 1, 1, 1), (W // 2, H // 3, W + 9, H // 3 + 7), (W // 2 - 2, H // 3 + 3, W // 2 + 4, H + 3),
                     (W + 1, 0, W + 5, 5), (-(1 << 22), -9, -1, H + 9), (0, H, W, 1 << 22)], np.int32)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_two_forms_are_equal_and_pixels_outside_every_region_stay(hw, block):
    H, W = hw
    rng = np.random.default_rng(100 * H + block)
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.int64).astype(np.uint8)
    regs = _regions(H, W)
    keep = frame.copy()
    for mode in (redact_ref.PIXELATE, redact_ref.FILL):
        a = redact_ref.redact(frame, regs, block, mode, (7, 200, 255))
        b = redact_ref.redact_loop(frame, regs, block, mode, (7, 200, 255))
        assert a.dtype == np.uint8 and a.shape == frame.shape and np.array_equal(a, b)
        held = redact_ref.held_mask((H, W), regs)
        assert np.array_equal(a[~held], frame[~held])
        if mode == redact_ref.FILL:
            assert (a[held] == (7, 200, 255)).all()
    assert np.array_equal(frame, keep)                       # the input is not written
    # no region, and regions wholly outside: the frame as it is
    assert np.array_equal(redact_ref.redact(frame, np.zeros((0, 4), np.int32), block), frame)
    assert np.array_equal(redact_ref.redact(frame, [(W, 0, W + 9, H), (-9, -9, -1, -1)], block), frame)


def test_order_duplicates_and_overlap_give_the_union():
    rng = np.random.default_rng(3)
    frame = rng.integers(0, 256, (37, 51, 3), dtype=np.int64).astype(np.uint8)
    a, b = (4, 5, 30, 20), (18, 11, 47, 33)
    one = redact_ref.redact(frame, [a, b], 5)
    assert np.array_equal(one, redact_ref.redact(frame, [b, a], 5))
    assert np.array_equal(one, redact_ref.redact(frame, [a, b, a, a], 5))
    # applying the regions one after the other is NOT the definition where they share a cell: the second would average bytes the
    # first wrote - the in-place hazard the kernel must not have
    chained = redact_ref.redact(redact_ref.redact(frame, [a], 5), [b], 5)
    assert not np.array_equal(one, chained)


@pytest.mark.parametrize("block", [2, 3, 5, 16])
def test_a_cell_wholly_inside_a_region_carries_one_value(block):
    H, W = 37, 51
    rng = np.random.default_rng(block)
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.int64).astype(np.uint8)
    x1, y1, x2, y2 = 7, 4, 48, 33
    out = redact_ref.redact(frame, [(x1, y1, x2, y2)], block)
    whole = 0
    for cy in range(0, H, block):
        for cx in range(0, W, block):
            ye, xe = min(cy + block, H), min(cx + block, W)
            if cx >= x1 and xe - 1 <= x2 and cy >= y1 and ye - 1 <= y2:
                cell = out[cy:ye, cx:xe].reshape(-1, 3)
                assert (cell == cell[0]).all()
                src = frame[cy:ye, cx:xe].reshape(-1, 3).astype(np.int64)
                assert cell[0].tolist() == ((src.sum(0) + len(src) // 2) // len(src)).tolist()
                whole += 1
    assert whole >= 1
    # a cell the region cuts: its held pixels carry the mean of the WHOLE cell, its other pixels their own bytes
    cx, cy = x1 // block * block, y1 // block * block
    src = frame[cy:cy + block, cx:cx + block].reshape(-1, 3).astype(np.int64)
    assert out[y1, x1].tolist() == ((src.sum(0) + len(src) // 2) // len(src)).tolist()


def test_the_largest_cell_of_all_255_bytes_gives_255():
    frame = np.full((64, 64, 3), 255, np.uint8)
    out = redact_ref.redact(frame, [(0, 0, 63, 63)], 64)
    assert (out == 255).all()                                # n = 4096: S = 1 044 480 in no 8- or 16-bit sum
    assert np.array_equal(out, redact_ref.redact_loop(frame, [(0, 0, 63, 63)], 64))


def test_rounding_ties_go_up_for_even_and_odd_n():
    # n = 4, S = 2 -> (2 + 2) // 4 = 1; S = 1 -> 0;  n = 9 (odd, no exact tie): S = 4 -> (4 + 4) // 9 = 0, S = 5 -> 1
    f = np.zeros((2, 2, 3), np.uint8)
    f[0, 0] = (1, 1, 0)
    f[0, 1] = (1, 0, 0)
    assert redact_ref.redact(f, [(0, 0, 1, 1)], 2)[0, 0].tolist() == [1, 0, 0]
    g = np.zeros((3, 3, 3), np.uint8)
    g[0, 0] = (4, 5, 13)
    assert redact_ref.redact(g, [(0, 0, 2, 2)], 3)[1, 1].tolist() == [0, 1, 1]
