"""Face quality in NumPy: the definition the device kernel (csrc/face_quality.hip) is pinned to, byte for byte.

Written from the specification (include/frhip.h fr_face_quality_f16), not from the kernel.  A crop is the
``float16 [112,112,8]`` face that the alignment writes: channels 0..2 are R, G, B as ``(u - 127.5) / 127.5``.

* pixel: ``u = rint(h * 127.5f + 127.5f)`` per channel, two singly rounded float32 operations, clamped to 0 .. 255;
  ``L = (77 R + 150 G + 29 B + 128) >> 8``
* window: rows 20 .. 99, columns 16 .. 95 (n = 6400); the Laplacian ``D = 4 L - up - down - left - right`` also reads the
  one-pixel ring round it
* ``qi = (mean, contrast, sharp, dark, bright, 0, 0, 0)`` in exact integers (Python ints here: no width to overflow)
* ``qf = (d2, t, c, m)`` in ``np.float32`` scalars, one rounding per operation in the stated order
* the verdict mask against the thresholds of ``Limits``
"""
import numpy as np

SIZE = 112
Y0, Y1, X0, X1 = 20, 100, 16, 96            # the window: rows Y0 .. Y1 - 1, columns X0 .. X1 - 1
N = (Y1 - Y0) * (X1 - X0)                   # 6400
SMALL, DARK, BRIGHT, FLAT, BLURRED, CLIPPED, YAW, PITCH = 1, 2, 4, 8, 16, 32, 64, 128
REASONS = ((SMALL, "small"), (DARK, "dark"), (BRIGHT, "bright"), (FLAT, "flat"), (BLURRED, "blurred"), (CLIPPED, "clipped"),
           (YAW, "yaw"), (PITCH, "pitch"))
# the ArcFace template the alignment maps the landmarks to: left eye, right eye, nose, left mouth, right mouth
TEMPLATE = np.array([[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366], [41.5493, 92.3655], [70.7299, 92.2041]],
                    np.float32)
F = np.float32


class Limits:
    """The thresholds of the verdict; the defaults are ``FaceQuality``'s (min_eye2 = 12 * 12)."""

    def __init__(self, min_eye2=144.0, mean_lo=40, mean_hi=215, contrast_min=100, sharp_min=50, clip_max=1600, yaw_max=0.5,
                 pitch_lo=0.25, pitch_hi=0.75):
        self.min_eye2, self.yaw_max, self.pitch_lo, self.pitch_hi = F(min_eye2), F(yaw_max), F(pitch_lo), F(pitch_hi)
        self.mean_lo, self.mean_hi, self.contrast_min = int(mean_lo), int(mean_hi), int(contrast_min)
        self.sharp_min, self.clip_max = int(sharp_min), int(clip_max)

    def replace(self, **kw):
        d = dict(self.__dict__)
        d.update(kw)
        return Limits(**d)

    def args(self):
        """in the order of fr_face_quality_f16's scalar arguments"""
        return (float(self.min_eye2), self.mean_lo, self.mean_hi, self.contrast_min, self.sharp_min, self.clip_max,
                float(self.yaw_max), float(self.pitch_lo), float(self.pitch_hi))


# every test of the verdict switched off as far as thresholds can: bit 128 still needs m > 0
ACCEPT_ALL = Limits(0.0, 0, 255, 0, 0, N, np.inf, -np.inf, np.inf)


def crop_from_bytes(rgb):
    """uint8 [...,112,112,3] R, G, B -> the float16 [...,112,112,8] crop as the alignment writes it: ``(float32(u) - 127.5f) /
    127.5f`` rounded to float16, channels 3..7 zero"""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.shape[-3:] == (SIZE, SIZE, 3)
    out = np.zeros(rgb.shape[:-1] + (8,), np.float16)
    out[..., :3] = ((rgb.astype(np.float32) - F(127.5)) / F(127.5)).astype(np.float16)
    return out


def crop_bytes(crop):
    """float16 [...,8] -> int64 [...,3]: the bytes R, G, B"""
    h = np.asarray(crop)[..., :3].astype(np.float32)
    v = (h * F(127.5)).astype(np.float32) + F(127.5)
    return np.fmin(np.fmax(np.rint(v.astype(np.float32)), F(0)), F(255)).astype(np.int64)


def luma(crop):
    """int64 [112,112] of one crop"""
    u = crop_bytes(crop)
    return (77 * u[..., 0] + 150 * u[..., 1] + 29 * u[..., 2] + 128) >> 8


def sums(crop):
    """(sum L, sum L^2, sum D, sum D^2, dark, bright) over the window, Python ints"""
    L = luma(crop)
    w = L[Y0:Y1, X0:X1]
    D = 4 * w - L[Y0 - 1:Y1 - 1, X0:X1] - L[Y0 + 1:Y1 + 1, X0:X1] - L[Y0:Y1, X0 - 1:X1 - 1] - L[Y0:Y1, X0 + 1:X1 + 1]
    return (int(w.sum()), int((w * w).sum()), int(D.sum()), int((D * D).sum()), int((w <= 15).sum()), int((w >= 240).sum()))


def integer_metrics(crop):
    """qi: int32 [8]"""
    sL, sL2, sD, sD2, dark, bright = sums(crop)
    mean = (sL + N // 2) // N
    contrast = (N * sL2 - sL * sL) // (N * N)
    sharp = (N * sD2 - sD * sD) // (N * N)
    return np.array([mean, contrast, sharp, dark, bright, 0, 0, 0], np.int32)


def _cross(ax, ay, bx, by):
    return F(F(ax * by) - F(ay * bx))


def landmark_metrics(kps):
    """qf: float32 [4] = (d2, t, c, m) of float32 [5,2] landmarks"""
    k = np.asarray(kps, np.float32).reshape(5, 2)
    with np.errstate(all="ignore"):
        le, re, nose, lm, rm = (k[i] for i in range(5))
        ex, ey = F(re[0] - le[0]), F(re[1] - le[1])
        d2 = F(F(ex * ex) + F(ey * ey))
        ax, ay = F(nose[0] - le[0]), F(nose[1] - le[1])
        t = F(F(ax * ex) + F(ay * ey))
        mx, my = F(F(lm[0] + rm[0]) * F(0.5)), F(F(lm[1] + rm[1]) * F(0.5))
        c = _cross(ex, ey, ax, ay)
        m = _cross(ex, ey, F(mx - le[0]), F(my - le[1]))
    return np.array([d2, t, c, m], np.float32)


def verdict_of(qi, qf, lim):
    mean, contrast, sharp, dark, bright = (int(v) for v in qi[:5])
    d2, t, c, m = (F(v) for v in qf)
    v = 0
    with np.errstate(all="ignore"):
        if d2 < lim.min_eye2:
            v |= SMALL
        if mean < lim.mean_lo:
            v |= DARK
        if mean > lim.mean_hi:
            v |= BRIGHT
        if contrast < lim.contrast_min:
            v |= FLAT
        if sharp < lim.sharp_min:
            v |= BLURRED
        if dark + bright > lim.clip_max:
            v |= CLIPPED
        if np.abs(F(F(t + t) - d2)) > F(lim.yaw_max * d2):
            v |= YAW
        if not (m > 0) or c < F(lim.pitch_lo * m) or c > F(lim.pitch_hi * m):
            v |= PITCH
    return v


def measure(crops, kps, lim=None, counts=None, cap=None):
    """The whole entry: (qi int32 [S,8], qf float32 [S,4], verdict int32 [S]).  ``counts`` with ``cap``: the slot form - a slot
    without a face gives verdict -1 and zeros, and its crop and landmarks are not looked at."""
    lim = lim or Limits()
    crops, kps = np.asarray(crops), np.asarray(kps, np.float32)
    S = crops.shape[0]
    qi, qf, verdict = np.zeros((S, 8), np.int32), np.zeros((S, 4), np.float32), np.zeros(S, np.int32)
    for s in range(S):
        if counts is not None and not (s % cap < int(counts[s // cap])):
            verdict[s] = -1
            continue
        qi[s], qf[s] = integer_metrics(crops[s]), landmark_metrics(kps[s])
        verdict[s] = verdict_of(qi[s], qf[s], lim)
    return qi, qf, verdict


# ---------------------------------------------------------------------------------------------------- crops the tests share
def checkerboard():
    """uint8 [112,112,3]: 0 and 255 alternating in both directions, the sharpest crop there is"""
    y, x = np.mgrid[0:SIZE, 0:SIZE]
    return np.repeat((((y + x) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)


def ramp(axis):
    """uint8 [112,112,3]: grey rising by 2 per pixel along ``axis`` (0: down the rows, 1: along the columns)"""
    v = (np.arange(SIZE) * 2).astype(np.uint8)
    g = np.broadcast_to(v[:, None] if axis == 0 else v[None, :], (SIZE, SIZE))
    return np.repeat(g[..., None], 3, axis=2).copy()
