"""tests/helpers/chip_ref.py, the definition csrc/face_chips.hip is held to, against itself and against three outside anchors (no
GPU): its vectorised and its per-pixel form give equal bytes; the identity at L == S; fill outside the frame; the largest sum;
Pillow's BILINEAR within one level, Pillow's BOX within one level at integer ratios, and an independently written float64 area
average (an integral image interpolated at the fractional edges) with no mismatch at non-integer ratios."""
import time

import numpy as np
import pytest

from tests.helpers import chip_ref

H, W = 270, 480
FILL = (7, 200, 255)


def smooth_frame():
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.stack([127.5 + 127.5 * np.sin(x / 23.0 + y / 41.0), 255.0 * x / (W - 1), 127.5 + 127.5 * np.cos(y / 17.0) * np.sin(x / 31.0)],
                    axis=2).round().clip(0, 255).astype(np.uint8)


def noise_frame(seed=11):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


FRAMES = {"smooth": smooth_frame(), "noise": noise_frame()}


def origin(L, k=0):
    """a square of side L at least 2 pixels inside the frame, a different place per k"""
    return 2 + (37 * k) % (W - L - 3), 2 + (23 * k) % (H - L - 3)


@pytest.mark.parametrize("S", [16, 48])
def test_the_two_forms_are_equal(S):
    rng = np.random.default_rng(S)
    fr = rng.integers(0, 256, (33, 50, 3), dtype=np.uint8)
    recs = [(0, 3, 4, S), (0, -5, -3, 20), (0, 40, 20, 2 * S + 1), (0, 2, 2, 7), (0, 10, 10, 1), (0, -3, 30, S - 1), (0, -100, 0, 10),
            (0, 0, 0, 3 * S + 7), (0, 49, 32, S + 1), (0, -1, -1, 2), (0, 20, -40, 90)]
    for rec in recs:
        a, b = chip_ref.chip([fr], rec, S, FILL), chip_ref.chip_loop([fr], rec, S, FILL)
        assert a.dtype == np.uint8 and a.shape == (S, S, 3) and np.array_equal(a, b), rec


@pytest.mark.parametrize("S", [16, 112, 256])
def test_identity_at_side_equal_size(S):
    fr = FRAMES["noise"]
    for x0, y0 in ((0, 0), (5, 3), (W - S, H - S)):
        assert np.array_equal(chip_ref.chip([fr], (0, x0, y0, S), S), fr[y0:y0 + S, x0:x0 + S])
    # cut by the frame: the part that exists is the frame's, the rest is fill
    got = chip_ref.chip([fr], (0, -4, -6, S), S, FILL)
    assert np.array_equal(got[6:, 4:], fr[:S - 6, :S - 4]) and (got[:6] == FILL).all() and (got[:, :4] == FILL).all()


def test_fill_outside_the_frame_on_each_side_and_wholly_outside():
    fr = np.full((40, 60, 3), 90, np.uint8)
    S, L = 16, 32                                             # an output pixel is 2 x 2 source pixels
    fill = np.asarray(FILL)
    left = chip_ref.chip([fr], (0, -16, 4, L), S, FILL)
    assert (left[:, :8] == fill).all() and (left[:, 8:] == 90).all()
    right = chip_ref.chip([fr], (0, 44, 4, L), S, FILL)
    assert (right[:, :8] == 90).all() and (right[:, 8:] == fill).all()
    top = chip_ref.chip([fr], (0, 4, -16, L), S, FILL)
    assert (top[:8] == fill).all() and (top[8:] == 90).all()
    bottom = chip_ref.chip([fr], (0, 4, 24, L), S, FILL)
    assert (bottom[:8] == 90).all() and (bottom[8:] == fill).all()
    # an output pixel half inside: the rounded mean of frame and fill, (2 * 90 + 2 * c + 2) // 4
    half = chip_ref.chip([fr], (0, -15, 4, L), S, FILL)
    assert half[0, 7].tolist() == [(2 * 90 + 2 * c + 2) // 4 for c in FILL]
    for rec in ((0, 60, 0, L), (0, 0, 40, L), (0, -L, 0, L), (0, 0, -L, L), (0, 1 << 20, 5, L), (0, 5, -(1 << 20), 7)):
        assert (chip_ref.chip([fr], rec, S, FILL) == fill).all(), rec
    # the bilinear taps are not clamped to the square: a square's edge column blends with the frame's next pixel
    ramp = np.zeros((20, 20, 3), np.uint8)
    ramp[:, 10:] = 200
    up = chip_ref.chip([ramp], (0, 6, 6, 4), 16, FILL)         # columns 6 .. 9 are 0, the tap at 10 is 200
    assert up[0, 15, 0] > 0 and up[0, 0, 0] == 0


def test_records_no_picture_is_defined_for_are_fill():
    fr = noise_frame(3)[:33, :50]
    fill = np.asarray(FILL)
    for rec in ((-1, 0, 0, 20), (1, 0, 0, 20), (0, 0, 0, 0), (0, 0, 0, 4097), (0, (1 << 20) + 1, 0, 20), (0, 0, -(1 << 20) - 1, 20)):
        assert (chip_ref.chip([fr], rec, 16, FILL) == fill).all(), rec
    assert (chip_ref.chip([None, fr], (0, 0, 0, 20), 16, FILL) == fill).all()
    assert not (chip_ref.chip([None, fr], (1, 0, 0, 20), 16, FILL) == fill).all()
    assert (chip_ref.chip([np.zeros((0, 5, 3), np.uint8)], (0, 0, 0, 20), 16, FILL) == fill).all()
    assert chip_ref.chips([fr], [(0, 0, 0, 20), (5, 0, 0, 20)], 16, FILL).shape == (2, 16, 16, 3)


def test_the_largest_sum_by_hand_and_the_speed_of_a_4096_square():
    """side 4096 over all-255 pixels with a white fill: every weighted sum is 255 * 4096^2, plus 4096^2 // 2 for the rounding
    it is 255 * 2^24 + 2^23 - inside 2^32, outside 2^31 - and every byte is 255"""
    assert 2 ** 31 < 255 * 4096 ** 2 + 4096 ** 2 // 2 < 2 ** 32
    fr = np.full((64, 97, 3), 255, np.uint8)
    t0 = time.perf_counter()
    got = chip_ref.chip([fr], (0, -2000, -2000, 4096), 256, (255, 255, 255))
    took = time.perf_counter() - t0
    assert (got == 255).all() and took < 1.0, took
    for S in (16, 256):
        assert (chip_ref.chip([np.full((4096, 4, 3), 255, np.uint8)], (0, 0, 0, 4096), S, (255, 255, 255)) == 255).all()
    # and a black fill shows where the frame ends: output (0, 0) of S = 16 covers 256 x 256 source pixels, 64 x 97 of them white
    got = chip_ref.chip([fr], (0, 0, 0, 4096), 16)
    assert got[0, 0].tolist() == [(255 * 64 * 97 + 32768) // 65536] * 3 and not got[1:].any()


@pytest.mark.parametrize("S", [32, 112, 256])
@pytest.mark.parametrize("name", ["smooth", "noise"])
def test_bilinear_regime_is_within_one_level_of_pillow(name, S):
    from PIL import Image
    fr = FRAMES[name]
    img = Image.fromarray(fr, "RGB")
    for k, L in enumerate([S - 1, S // 2, S // 2 + 1, 20, 7, 1]):
        x0, y0 = origin(L, k)
        want = np.asarray(img.resize((S, S), Image.BILINEAR, box=(x0, y0, x0 + L, y0 + L))).astype(int)
        got = chip_ref.chip([fr], (0, x0, y0, L), S).astype(int)
        assert np.abs(got - want).max() <= 1, (name, S, L, int(np.abs(got - want).max()))


@pytest.mark.parametrize("S", [32, 112, 256])
@pytest.mark.parametrize("name", ["smooth", "noise"])
def test_box_regime_is_within_one_level_of_pillow_box_at_integer_ratios(name, S):
    from PIL import Image
    fr = FRAMES[name]
    img = Image.fromarray(fr, "RGB")
    ran = 0
    for k in (1, 2, 3, 5):
        L = k * S
        if L > H - 4:                                        # the square stays at least 2 pixels inside the frame
            continue
        x0, y0 = origin(L, k)
        want = np.asarray(img.resize((S, S), Image.BOX, box=(x0, y0, x0 + L, y0 + L))).astype(int)
        got = chip_ref.chip([fr], (0, x0, y0, L), S).astype(int)
        assert np.abs(got - want).max() <= 1, (name, S, L, int(np.abs(got - want).max()))
        if k == 1:
            assert np.array_equal(got, want)
        ran += 1
    assert ran >= 1


def float_area_average(fr, x0, y0, L, S):
    """float64 [S, S, 3]: the mean of the picture - a piecewise constant function, pixel (x, y) on [x, x + 1) x [y, y + 1) - over
    each output pixel's rectangle, from an integral image interpolated at the fractional edges x0 + j L / S"""
    I = np.zeros((fr.shape[0] + 1, fr.shape[1] + 1, 3))
    I[1:, 1:] = fr.astype(np.float64).cumsum(0).cumsum(1)

    def at(u):                                               # index and fraction of the real coordinates u
        i = np.floor(u).astype(int)
        return i, u - i
    ex = x0 + np.arange(S + 1) * (L / S)
    ey = y0 + np.arange(S + 1) * (L / S)
    (ix, fx), (iy, fy) = at(ex), at(ey)
    ix1, iy1 = np.minimum(ix + 1, fr.shape[1]), np.minimum(iy + 1, fr.shape[0])
    rows = I[iy] * (1 - fy)[:, None, None] + I[iy1] * fy[:, None, None]                   # [S + 1, W + 1, 3]
    F = rows[:, ix] * (1 - fx)[None, :, None] + rows[:, ix1] * fx[None, :, None]          # [S + 1, S + 1, 3]
    area = (L / S) ** 2
    return (F[1:, 1:] - F[1:, :-1] - F[:-1, 1:] + F[:-1, :-1]) / area


@pytest.mark.parametrize("LS", [(113, 112), (250, 112), (103, 32), (257, 256)], ids=lambda p: "%dto%d" % p)
def test_box_regime_equals_a_float64_area_average_at_non_integer_ratios(LS):
    L, S = LS
    fr = FRAMES["noise"]
    x0, y0 = origin(L, L)
    v = float_area_average(fr, x0, y0, L, S)
    near_tie = np.abs(v - np.floor(v) - 0.5) < 1e-6
    assert near_tie.mean() <= 0.001
    want = np.floor(v + 0.5).astype(int)
    got = chip_ref.chip([fr], (0, x0, y0, L), S).astype(int)
    assert int(((got != want) & ~near_tie).sum()) == 0
