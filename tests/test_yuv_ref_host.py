"""The host side of YUV 4:2:0 ingest (no GPU needed): the constants table of colour.py, the shape rule, and the NumPy
definition the device conversion is pinned to (tests/helpers/yuv_ref.py)."""
import numpy as np
import pytest

from tests.helpers import yuv_ref


def test_constants_table_is_the_specified_one():
    from facerecognition_infrenceengine_amd import colour
    want = {
        "bt601": (16, 1220542, 2116026, -409993, -852492, 1673527),
        "bt709": (16, 1220945, 2215014, -223608, -558796, 1879825),
        "jpeg": (0, 1048576, 1858077, -360853, -748826, 1470104),
    }
    assert colour.MATRICES == want
    assert yuv_ref.CONSTANTS == want
    assert colour.LAYOUTS == {"nv12": 0, "i420": 1}
    assert colour.check_pixel_format("bgr") == (None, None)
    assert colour.check_pixel_format("i420", "jpeg") == (1, want["jpeg"])
    with pytest.raises(ValueError, match="unknown pixel_format"):
        colour.check_pixel_format("yuyv")
    with pytest.raises(ValueError, match="unknown pixel_format"):
        colour.check_pixel_format("bgr", allow_bgr=False)
    with pytest.raises(ValueError, match="unknown matrix"):
        colour.check_pixel_format("nv12", "bt2020")


def test_every_intermediate_stays_inside_int32():
    """the extremes of the three sums over the whole (Y, U, V) cube, per matrix: the kernel computes in int32"""
    for name, (y_off, cy, cub, cug, cvg, cvr) in yuv_ref.CONSTANTS.items():
        ymax = (255 - y_off) * cy + (1 << 19)
        worst = 0
        for terms in ((cub,), (cug, cvg), (cvr,)):
            hi = ymax + sum(max(c * -128, c * 127) for c in terms)
            lo = (1 << 19) + sum(min(c * -128, c * 127) for c in terms)
            worst = max(worst, abs(hi), abs(lo))
        assert worst < 2 ** 31, (name, worst)                      # the largest is bt709's 5.74e8
        # and the check the C entry points make admits the row
        assert 255 * cy + (1 << 19) + 128 * max(abs(cub), abs(cug) + abs(cvg), abs(cvr)) < 2 ** 31


def test_bt601_is_within_one_of_the_rounded_float_definition():
    rng = np.random.default_rng(601)
    Y, U, V = (rng.integers(0, 256, 1_000_000, dtype=np.int64) for _ in range(3))
    got = yuv_ref.convert_triples(Y, U, V, "bt601")
    want = yuv_ref.float_bt601(Y, U, V)
    for g, w, c in zip(got, want, "BGR"):
        d = np.abs(g.astype(np.int16) - w.astype(np.int16))
        assert d.max() <= 1, (c, int(d.max()))
    # grey stays grey, black and white land where limited range puts them
    grey = yuv_ref.convert_triples(np.arange(256), 128, 128, "bt601")
    assert np.array_equal(grey[0], grey[1]) and np.array_equal(grey[1], grey[2])
    assert grey[0][16] == 0 and grey[0][235] == 255 and grey[0][0] == 0
    full = yuv_ref.convert_triples(np.arange(256), 128, 128, "jpeg")
    assert np.array_equal(full[0], np.arange(256)) and np.array_equal(full[2], np.arange(256))


@pytest.mark.parametrize("matrix", sorted(yuv_ref.CONSTANTS))
def test_nv12_and_i420_views_of_the_same_planes_convert_identically(matrix):
    rng = np.random.default_rng(7)
    for h, w in ((2, 2), (2, 6), (4, 10), (6, 32), (8, 34)):
        y = rng.integers(0, 256, (h, w), dtype=np.uint8)
        u = rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
        v = rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
        nv12, i420 = yuv_ref.pack(y, u, v, "nv12"), yuv_ref.pack(y, u, v, "i420")
        assert nv12.shape == i420.shape == (h * 3 // 2, w)
        for f, layout in ((nv12, "nv12"), (i420, "i420")):
            py, pu, pv = yuv_ref.planes(f, layout)
            assert np.array_equal(py, y) and np.array_equal(pu, u) and np.array_equal(pv, v)
        a, b = yuv_ref.yuv420_to_bgr(nv12, "nv12", matrix), yuv_ref.yuv420_to_bgr(i420, "i420", matrix)
        assert a.shape == (h, w, 3) and a.dtype == np.uint8 and np.array_equal(a, b)
        # nearest chroma, spelled out per pixel
        for yy in range(h):
            for xx in range(w):
                bgr = yuv_ref.convert_triples(int(y[yy, xx]), int(u[yy // 2, xx // 2]), int(v[yy // 2, xx // 2]), matrix)
                assert tuple(int(c) for c in bgr) == tuple(int(c) for c in a[yy, xx])
        if w > 2:
            assert not np.array_equal(nv12[h:], i420[h:])       # the two layouts do differ in memory


def test_odd_sizes_raise():
    from facerecognition_infrenceengine_amd import colour
    for shape in ((3, 3), (4, 4), (5, 4), (6, 5), (0, 4), (3,), (3, 2, 1)):      # [H*3/2, W]: 3 rows are H = 2, 4 or 5 rows no H
        with pytest.raises(ValueError):
            yuv_ref.frame_hw(shape)
        with pytest.raises(ValueError):
            colour.check_yuv_shape(shape)
    for shape, hw in (((3, 2), (2, 2)), ((6, 10), (4, 10)), ((1620, 1920), (1080, 1920))):
        assert yuv_ref.frame_hw(shape) == hw == colour.check_yuv_shape(shape)
    for h, w in ((3, 4), (4, 3), (0, 2), (2, -2)):
        with pytest.raises(ValueError):
            colour.check_yuv_size(h, w)
    with pytest.raises(ValueError, match="2 GiB"):
        colour.check_yuv_size(32768, 32768)
    with pytest.raises(ValueError):
        yuv_ref.yuv420_to_bgr(np.zeros((3, 3), np.uint8))
    with pytest.raises(ValueError):
        yuv_ref.bgr_to_yuv420(np.zeros((3, 4, 3), np.uint8))


def test_forward_helper_round_trips_flat_colours():
    """the input manufacturer is a sane inverse: flat patches come back within 2 of where they started"""
    rng = np.random.default_rng(3)
    for _ in range(50):
        c = rng.integers(16, 236, 3)
        bgr = np.broadcast_to(c.astype(np.uint8), (4, 6, 3))
        for layout in yuv_ref.LAYOUTS:
            back = yuv_ref.yuv420_to_bgr(yuv_ref.bgr_to_yuv420(bgr, layout), layout, "bt601")
            assert np.abs(back.astype(np.int16) - bgr.astype(np.int16)).max() <= 2, (c, layout)
