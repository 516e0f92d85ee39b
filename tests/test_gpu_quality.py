"""Face quality on the MI355X: fr_face_quality_f16 (csrc/face_quality.hip) against the NumPy definition of
tests/helpers/quality_ref.py, byte for byte - qi, qf and the verdict, with guard bytes round all three - and ``FaceQuality``
above it."""
import ctypes

import numpy as np
import pytest
import torch

from tests.helpers import quality_ref as qr

pytestmark = pytest.mark.gpu

GUARD, PATTERN = 64, 0xA5


class Out:
    """qi, qf and verdict of one call on the device, each between two runs of GUARD pattern bytes."""

    def __init__(self, S):
        self.S = S
        self.sizes = {"qi": S * 32, "qf": S * 16, "verdict": S * 4}
        self.buf = {k: torch.full((GUARD + n + GUARD,), PATTERN, dtype=torch.uint8, device="cuda") for k, n in self.sizes.items()}

    def ptr(self, name):
        return ctypes.c_void_p(self.buf[name].data_ptr() + GUARD)

    def host(self, name):
        raw = self.buf[name].cpu().numpy()
        n = self.sizes[name]
        assert (raw[:GUARD] == PATTERN).all() and (raw[GUARD + n:] == PATTERN).all(), f"guard bytes of {name} were written"
        body = raw[GUARD:GUARD + n]
        return {"qi": lambda: body.view(np.int32).reshape(self.S, 8), "qf": lambda: body.view(np.uint32).reshape(self.S, 4),
                "verdict": lambda: body.view(np.int32)}[name]()

    def untouched(self):
        return all((b.cpu().numpy() == PATTERN).all() for b in self.buf.values())


def _run(lib, crops, kps, lim, counts=None, cap=0):
    """one launch over host arrays -> (qi int32 [S,8], qf as uint32 bits [S,4], verdict int32 [S]) behind their guards"""
    from facerecognition_infrenceengine_amd import _lib
    S = crops.shape[0]
    c = torch.from_numpy(np.ascontiguousarray(crops).view(np.int16)).cuda()
    k = torch.from_numpy(np.ascontiguousarray(kps, np.float32).view(np.int32)).cuda()
    n = None if counts is None else torch.tensor(list(counts), dtype=torch.int32).cuda()
    out = Out(S)
    lib.fr_face_quality_f16(_lib.ptr(c), _lib.ptr(k), _lib.ptr(n), cap, S, out.ptr("qi"), out.ptr("qf"), out.ptr("verdict"),
                            *lim.args(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return out.host("qi"), out.host("qf"), out.host("verdict")


def _check(lib, crops, kps, lim, counts=None, cap=0):
    qi, qf, verdict = _run(lib, crops, kps, lim, counts, cap)
    wi, wf, wv = qr.measure(crops, kps, lim, counts, cap or None)
    assert np.array_equal(qi, wi), (qi, wi)
    assert np.array_equal(qf, wf.view(np.uint32)), (qf.view(np.float32), wf)
    assert np.array_equal(verdict, wv), (verdict, wv)
    return qi, qf.view(np.float32), verdict


def _random_crops(S, seed):
    rng = np.random.default_rng(seed)
    crops = qr.crop_from_bytes(rng.integers(0, 256, (S, 112, 112, 3), dtype=np.uint8))
    crops[..., 3:] = rng.standard_normal((S, 112, 112, 5)).astype(np.float16)       # the padding channels are not read
    scale = rng.uniform(0.2, 6.0, (S, 1, 1)).astype(np.float32)
    kps = (qr.TEMPLATE[None] * scale + rng.uniform(-3, 3, (S, 5, 2)) * scale + rng.uniform(0, 900, (S, 1, 2))).astype(np.float32)
    return crops, kps


@pytest.fixture(scope="module")
def shared():
    """37 random crops with their landmarks: the compact cases and the two-sizes case share them"""
    return _random_crops(37, 11)


@pytest.mark.parametrize("S", [1, 3, 37])
def test_compact_form_of_random_crops(lib, shared, S):
    crops, kps = shared
    qi, _, verdict = _check(lib, crops[:S], kps[:S], qr.Limits())
    assert (verdict >= 0).all() and (qi[:, 2] > 10000).all()               # byte noise is sharp


def test_same_rows_at_two_sizes(lib, shared):
    crops, kps = shared
    a = _run(lib, crops, kps, qr.Limits())
    b = _run(lib, crops[5:8], kps[5:8], qr.Limits())
    for x, y in zip(a, b):
        assert np.array_equal(x[5:8], y)


def test_flat_checkerboard_and_ramps(lib):
    rgb = np.stack([np.zeros((112, 112, 3), np.uint8), np.full((112, 112, 3), 255, np.uint8), qr.checkerboard(), qr.ramp(0),
                    qr.ramp(1)])
    crops, kps = qr.crop_from_bytes(rgb), np.repeat(qr.TEMPLATE[None], 5, axis=0)
    qi, _, verdict = _check(lib, crops, kps, qr.Limits())
    assert list(qi[0][:5]) == [0, 0, 0, qr.N, 0] and list(qi[1][:5]) == [255, 0, 0, 0, qr.N]
    assert qi[2][2] == 1_040_400                                            # sum D^2 = 6 658 560 000: a 32-bit sum fails here
    assert qi[3][2] == 0 and qi[4][2] == 0
    assert verdict[0] == qr.DARK | qr.FLAT | qr.BLURRED | qr.CLIPPED and verdict[1] == qr.BRIGHT | qr.FLAT | qr.BLURRED | qr.CLIPPED


def test_slot_form_skips_slots_without_a_face(lib):
    cap, counts = 4, (0, 1, 4)
    crops, kps = _random_crops(12, 12)
    bits16 = crops.view(np.uint16)
    kbits = kps.view(np.uint32)
    for s in range(12):
        if not s % cap < counts[s // cap]:                                  # NaN patterns: quiet, signalling, all ones
            bits16[s] = (0x7E00, 0x7D01, 0xFFFF)[s % 3]
            kbits[s] = (0x7FC00000, 0x7FA00001, 0xFFFFFFFF)[s % 3]
    qi, qf, verdict = _check(lib, crops, kps, qr.Limits(), counts, cap)
    assert list(verdict < 0) == [True] * 4 + [False] + [True] * 3 + [False] * 4
    assert (qi[verdict < 0] == 0).all() and (qf.view(np.uint32)[verdict < 0] == 0).all()
    # the faces of the slot form measure as they do in a compact list
    held = np.flatnonzero(verdict >= 0)
    a = _run(lib, crops[held], kps[held], qr.Limits())
    assert np.array_equal(a[0], qi[held]) and np.array_equal(a[2], verdict[held])


CASES = [(qr.SMALL, dict(min_eye2=1e6)), (qr.DARK, dict(mean_lo=200)), (qr.BRIGHT, dict(mean_hi=50)),
         (qr.FLAT, dict(contrast_min=16000)), (qr.BLURRED, dict(sharp_min=2_000_000)), (qr.CLIPPED, dict(clip_max=0)),
         (qr.YAW, dict(yaw_max=0.0)), (qr.PITCH, dict(pitch_lo=0.9, pitch_hi=0.9))]


def test_each_verdict_bit_alone_and_all_together(lib, shared):
    crops = shared[0][:2]
    kps = np.stack([qr.TEMPLATE, qr.TEMPLATE * np.float32(2.5) + np.float32(100)])
    _, _, verdict = _check(lib, crops, kps, qr.Limits())
    assert list(verdict) == [0, 0]                                          # the faces are fit under the defaults
    every = {}
    for bit, change in CASES:
        _, _, verdict = _check(lib, crops, kps, qr.Limits().replace(**change))
        assert list(verdict) == [bit, bit], (bit, verdict)
        every.update(change)
    _, _, verdict = _check(lib, crops, kps, qr.Limits().replace(**every))
    assert list(verdict) == [255, 255]
    upside = kps.copy()
    upside[:, :, 1] = np.float32(500) - upside[:, :, 1]                     # m <= 0: no threshold lets a mirrored face through
    _, _, verdict = _check(lib, crops, upside, qr.ACCEPT_ALL)
    assert list(verdict) == [qr.PITCH, qr.PITCH]


def test_refusals_return_invalid_without_a_launch(lib):
    from facerecognition_infrenceengine_amd import _lib
    raw = lib._c.fr_face_quality_f16                                        # the unchecked entry: its return value
    crops, kps = _random_crops(2, 13)
    c = torch.from_numpy(crops.view(np.int16)).cuda()
    k = torch.from_numpy(kps).cuda()
    n = torch.tensor([1], dtype=torch.int32).cuda()
    out = Out(2)
    ok = qr.Limits().args()

    def call(crops=c, kps=k, counts=None, cap=0, S=2, qi="qi", lim=ok):
        return raw(_lib.ptr(crops), _lib.ptr(kps), _lib.ptr(counts), cap, S, out.ptr(qi) if qi else None, out.ptr("qf"),
                   out.ptr("verdict"), *lim, _lib.stream_ptr())

    def lim(**kw):
        return qr.Limits().replace(**kw).args()
    nan, inf = float("nan"), float("inf")
    bad = [dict(S=-1), dict(S=65535 * 64 + 1), dict(counts=n, cap=0), dict(counts=n, cap=-2), dict(crops=None), dict(kps=None),
           dict(qi=None), dict(lim=lim(min_eye2=-1.0)), dict(lim=lim(min_eye2=nan)), dict(lim=lim(min_eye2=inf)),
           dict(lim=lim(mean_lo=-1)), dict(lim=lim(mean_lo=256)), dict(lim=lim(mean_hi=-1)), dict(lim=lim(mean_hi=256)),
           dict(lim=lim(contrast_min=-1)), dict(lim=lim(sharp_min=-1)), dict(lim=lim(clip_max=-1)), dict(lim=lim(clip_max=qr.N + 1)),
           dict(lim=lim(yaw_max=-0.5)), dict(lim=lim(yaw_max=nan)), dict(lim=lim(pitch_lo=0.8, pitch_hi=0.2)),
           dict(lim=lim(pitch_lo=nan)), dict(lim=lim(pitch_hi=nan))]
    for kw in bad:
        assert call(**kw) == -1, kw                                         # FR_E_INVALID
    odd = ctypes.c_void_p(c.data_ptr() + 8)                                 # crops off their 16-byte boundary
    assert raw(odd, _lib.ptr(k), None, 0, 1, out.ptr("qi"), out.ptr("qf"), out.ptr("verdict"), *ok, _lib.stream_ptr()) == -1
    assert raw(None, None, None, 0, 0, None, None, None, *ok, _lib.stream_ptr()) == 0       # S == 0: nothing is touched
    torch.cuda.synchronize()
    assert out.untouched()
    with pytest.raises(_lib.FrError, match="clip_max"):
        lib.fr_face_quality_f16(_lib.ptr(c), _lib.ptr(k), None, 0, 2, out.ptr("qi"), out.ptr("qf"), out.ptr("verdict"),
                                *lim(clip_max=7000), _lib.stream_ptr())
    assert call() == 0                                                      # and the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert not out.untouched()


def test_face_quality_object(lib, shared):
    from facerecognition_infrenceengine_amd.quality import FaceQuality
    crops, kps = shared
    q = FaceQuality(min_eye=20, sharp_min=500000)
    c = torch.from_numpy(crops[:8].view(np.int16)).cuda().view(torch.float16)
    k = torch.from_numpy(kps[:8]).cuda()
    counts = torch.tensor([2, 3], dtype=torch.int32).cuda()
    lim = qr.Limits(min_eye2=400.0, sharp_min=500000)
    for cnt, cap in ((None, None), (counts, 4)):
        qi, qf, verdict = (t.cpu().numpy() for t in q.measure_device(c, k, cnt, cap))
        wi, wf, wv = qr.measure(crops[:8], kps[:8], lim, None if cnt is None else [2, 3], cap)
        assert np.array_equal(qi, wi) and np.array_equal(qf.view(np.uint32), wf.view(np.uint32)) and np.array_equal(verdict, wv)
    d = q.describe(qi[0], qf[0], verdict[0])
    assert d["ok"] == (wv[0] == 0) and d["sharp"] == int(wi[0, 2]) and abs(d["eye_dist"] ** 2 - float(wf[0, 0])) < 1e-2 * wf[0, 0]
    assert q.describe(qi[3], qf[3], verdict[3]) == {"mean": 0, "contrast": 0, "sharp": 0, "dark": 0, "bright": 0, "eye_dist": 0.0,
                                                    "ok": False, "reasons": []}
    with pytest.raises(ValueError):
        q.measure_device(c, k, counts, None)
    with pytest.raises(ValueError):
        q.measure_device(c, k[:7])
