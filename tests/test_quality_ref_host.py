"""The NumPy definition of face quality (tests/helpers/quality_ref.py) against the properties the specification states
(DESIGN.md 4.5e).  No GPU."""
import numpy as np
import pytest

from tests.helpers import quality_ref as qr


def _random_rgb(seed):
    return np.random.default_rng(seed).integers(0, 256, (112, 112, 3), dtype=np.uint8)


def test_all_256_bytes_survive_the_f16_crop():
    u = np.arange(256, dtype=np.uint8)
    rgb = np.zeros((112, 112, 3), np.uint8)
    rgb[0, :, 0], rgb[1, :, 0], rgb[2, :32, 0] = u[:112], u[112:224], u[224:]
    crop = qr.crop_from_bytes(rgb)
    back = qr.crop_bytes(crop)
    assert np.array_equal(back, rgb.astype(np.int64))
    h = crop[..., 0].astype(np.float32)
    v = (h * np.float32(127.5)).astype(np.float32) + np.float32(127.5)
    assert np.abs(v - rgb[..., 0]).max() < 0.04                  # 0.031: far from the 0.5 that would move the rounding


def test_luma_weights_are_the_gates():
    from tests.helpers import activity_ref as ar
    rgb = _random_rgb(1)
    assert np.array_equal(qr.luma(qr.crop_from_bytes(rgb)), ar.luma(rgb[..., ::-1]))


@pytest.mark.parametrize("value", [0, 1, 127, 128, 255])
def test_constant_crop_has_no_contrast_and_no_sharpness(value):
    qi = qr.integer_metrics(qr.crop_from_bytes(np.full((112, 112, 3), value, np.uint8)))
    assert qi[0] == value and qi[1] == 0 and qi[2] == 0
    assert qi[3] == (qr.N if value <= 15 else 0) and qi[4] == (qr.N if value >= 240 else 0)
    assert (qi[5:] == 0).all()


def test_checkerboard_is_the_sharpest_crop():
    crop = qr.crop_from_bytes(qr.checkerboard())
    sL, sL2, sD, sD2, dark, bright = qr.sums(crop)
    assert sD2 == 6_658_560_000 > 2 ** 32 and sD == 0
    qi = qr.integer_metrics(crop)
    assert qi[2] == 1_040_400 == 1020 ** 2
    assert qi[0] == 128 and qi[1] == 16256 and qi[3] == qi[4] == qr.N // 2      # (3200 * 255 + 3200) // 6400; 127.5^2 floored


def test_ramps():
    for axis in (0, 1):
        qi = qr.integer_metrics(qr.crop_from_bytes(qr.ramp(axis)))
        assert qi[2] == 0                                        # a linear ramp has no Laplacian
        lo = 2 * (qr.Y0 if axis == 0 else qr.X0)
        vals = lo + 2 * np.arange(80)
        assert qi[0] == (int(vals.sum()) * 80 + qr.N // 2) // qr.N
        assert qi[1] == (qr.N * int((vals ** 2).sum()) * 80 - (int(vals.sum()) * 80) ** 2) // qr.N ** 2


def test_only_window_and_ring_are_read():
    rgb = _random_rgb(2)
    base = qr.integer_metrics(qr.crop_from_bytes(rgb))
    out = rgb.copy()
    keep = np.zeros((112, 112), bool)
    keep[qr.Y0 - 1:qr.Y1 + 1, qr.X0 - 1:qr.X1 + 1] = True
    out[~keep] ^= 0xFF                                            # every pixel outside window plus ring
    assert np.array_equal(qr.integer_metrics(qr.crop_from_bytes(out)), base)
    crop = qr.crop_from_bytes(rgb)
    crop[..., 3:] = np.float16(7)                                 # nor the padding channels
    assert np.array_equal(qr.integer_metrics(crop), base)


def test_the_ring_moves_sharp_and_nothing_else():
    rgb = _random_rgb(3)
    base = qr.integer_metrics(qr.crop_from_bytes(rgb))
    ring = np.zeros((112, 112), bool)
    ring[qr.Y0 - 1:qr.Y1 + 1, qr.X0 - 1:qr.X1 + 1] = True
    ring[qr.Y0:qr.Y1, qr.X0:qr.X1] = False
    out = rgb.copy()
    out[ring] ^= 0xFF
    got = qr.integer_metrics(qr.crop_from_bytes(out))
    assert got[2] != base[2]
    assert np.array_equal(np.delete(got, 2), np.delete(base, 2))
    # the four corners of the ring touch no window pixel's Laplacian
    corners = rgb.copy()
    for y in (qr.Y0 - 1, qr.Y1):
        for x in (qr.X0 - 1, qr.X1):
            corners[y, x] ^= 0xFF
    assert np.array_equal(qr.integer_metrics(qr.crop_from_bytes(corners)), base)


# ---------------------------------------------------------------------------------------------------- landmarks
def test_template_landmarks_pass_yaw_and_pitch():
    qf = qr.landmark_metrics(qr.TEMPLATE)
    d2, t, c, m = (float(v) for v in qf)
    assert abs(t / d2 - 0.500) < 1e-3 and abs(c / m - 0.495) < 1e-3 and m > 0
    crop = qr.crop_from_bytes(_random_rgb(4))
    _, _, verdict = qr.measure(crop[None], qr.TEMPLATE[None])
    assert verdict[0] & (qr.YAW | qr.PITCH) == 0
    # the same under a similarity of the frame: scaled, turned and moved landmarks
    a = np.deg2rad(33.0)
    R = np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]], np.float32)
    k = (qr.TEMPLATE @ R.T * np.float32(3.7) + np.float32([400, 250])).astype(np.float32)
    assert np.array_equal(R @ R.T > 0.5, np.eye(2, dtype=bool)) and np.linalg.det(R) > 0     # a proper rotation
    _, _, verdict = qr.measure(crop[None], k[None])
    assert verdict[0] & (qr.YAW | qr.PITCH) == 0


def test_mirrored_face_sets_pitch():
    k = qr.TEMPLATE.copy()
    k[:, 1] = np.float32(112) - k[:, 1]                           # upside down: nose and mouth above the eye line
    qf = qr.landmark_metrics(k)
    assert qf[3] <= 0
    assert qr.verdict_of(qr.integer_metrics(qr.crop_from_bytes(_random_rgb(5))), qf, qr.ACCEPT_ALL) == qr.PITCH
    # all five landmarks on one point: m == 0 is "not above zero" as well
    assert qr.verdict_of(np.zeros(8, np.int32), qr.landmark_metrics(np.ones((5, 2), np.float32)), qr.ACCEPT_ALL) == qr.PITCH


def test_operation_order_of_the_landmark_terms():
    """each term against float64 arithmetic rounded where the specification rounds"""
    rng = np.random.default_rng(6)
    for _ in range(50):
        k = rng.uniform(0, 2000, (5, 2)).astype(np.float32)
        f = np.float32
        ex, ey = f(k[1, 0] - k[0, 0]), f(k[1, 1] - k[0, 1])
        ax, ay = f(k[2, 0] - k[0, 0]), f(k[2, 1] - k[0, 1])
        mx, my = f(f(k[3, 0] + k[4, 0]) * f(0.5)) - k[0, 0], f(f(k[3, 1] + k[4, 1]) * f(0.5)) - k[0, 1]
        want = [f(f(float(ex) * float(ex)) + f(float(ey) * float(ey))), f(f(float(ax) * float(ex)) + f(float(ay) * float(ey))),
                f(f(float(ex) * float(ay)) - f(float(ey) * float(ax))), f(f(float(ex) * float(my)) - f(float(ey) * float(mx)))]
        assert np.array_equal(qr.landmark_metrics(k), np.array(want, np.float32))


# ---------------------------------------------------------------------------------------------------- thresholds at their edges
def _qi(mean=128, contrast=1000, sharp=1000, dark=0, bright=0):
    return np.array([mean, contrast, sharp, dark, bright, 0, 0, 0], np.int32)


FIT_QF = np.array([400.0, 200.0, 200.0, 400.0], np.float32)     # d2, t, c, m: t / d2 = c / m = 0.5


@pytest.mark.parametrize("bit,field,at,off", [
    (qr.DARK, "mean", 40, -1), (qr.BRIGHT, "mean", 215, +1), (qr.FLAT, "contrast", 100, -1), (qr.BLURRED, "sharp", 50, -1)])
def test_integer_thresholds_at_the_boundary(bit, field, at, off):
    lim = qr.Limits()
    assert qr.verdict_of(_qi(**{field: at}), FIT_QF, lim) == 0            # on the threshold: fit
    assert qr.verdict_of(_qi(**{field: at + off}), FIT_QF, lim) == bit    # one past it


def test_clip_threshold_counts_both_ends():
    lim = qr.Limits()
    assert qr.verdict_of(_qi(dark=1000, bright=600), FIT_QF, lim) == 0
    assert qr.verdict_of(_qi(dark=1000, bright=601), FIT_QF, lim) == qr.CLIPPED
    assert qr.verdict_of(_qi(dark=1601), FIT_QF, lim) == qr.CLIPPED


def test_eye_distance_threshold():
    lim = qr.Limits()                                             # min_eye2 = 144
    at = np.array([144.0, 72.0, 72.0, 144.0], np.float32)
    below = np.array([np.nextafter(np.float32(144), np.float32(0)), 72.0, 72.0, 144.0], np.float32)
    assert qr.verdict_of(_qi(), at, lim) == 0
    assert qr.verdict_of(_qi(), below, lim) & qr.SMALL


def test_yaw_threshold():
    lim = qr.Limits()                                             # |2 t - d2| > 0.5 d2
    d2 = np.float32(400)
    for t, bad in ((300.0, False), (100.0, False), (300.25, True), (99.75, True)):
        qf = np.array([d2, t, 200.0, 400.0], np.float32)
        assert bool(qr.verdict_of(_qi(), qf, lim) & qr.YAW) == bad, t
    assert qr.verdict_of(_qi(), np.array([d2, 1e9, 200.0, 400.0], np.float32), qr.ACCEPT_ALL) == 0     # infinity: switched off


def test_pitch_thresholds():
    lim = qr.Limits()                                             # 0.25 m <= c <= 0.75 m, m > 0
    m = np.float32(400)
    for c, bad in ((100.0, False), (300.0, False), (99.99, True), (300.01, True)):
        qf = np.array([400.0, 200.0, c, m], np.float32)
        assert bool(qr.verdict_of(_qi(), qf, lim) & qr.PITCH) == bad, c


def test_all_bits_and_empty_slots():
    lim = qr.Limits(clip_max=10)
    bad_qf = np.array([1.0, 5.0, -1.0, -1.0], np.float32)
    assert qr.verdict_of(_qi(mean=10, contrast=0, sharp=0, dark=6400), bad_qf, lim) == 255 - qr.BRIGHT
    assert qr.verdict_of(_qi(mean=250, contrast=0, sharp=0, bright=6400), bad_qf, lim) == 255 - qr.DARK
    assert qr.verdict_of(_qi(mean=100, contrast=0, sharp=0, bright=6400), bad_qf, lim.replace(mean_lo=200, mean_hi=50)) == 255
    crops = np.full((8, 112, 112, 8), np.nan, np.float16)
    kps = np.full((8, 5, 2), np.nan, np.float32)
    crops[0], kps[0] = qr.crop_from_bytes(_random_rgb(7)), qr.TEMPLATE
    crops[4:8], kps[4:8] = crops[0], qr.TEMPLATE
    qi, qf, verdict = qr.measure(crops, kps, qr.ACCEPT_ALL, counts=[1, 4], cap=4)
    assert list(verdict) == [0, -1, -1, -1, 0, 0, 0, 0]
    assert (qi[1:4] == 0).all() and (qf[1:4] == 0).all() and (qi[4:] == qi[0]).all()
