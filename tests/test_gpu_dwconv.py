"""fr_dw_conv_f16 and fr_det_conv_act_f16 on the MI355X, per element against float64 on the same f16 operands
(tests/helpers/mbf_ref.py).

Depthwise tolerance, derived: the operands are f16, so each product x * w is exact in f32.  The kernel adds the T = K * K
products into an f32 accumulator one by one (at most T roundings, each at most 2^-24 relative to a partial sum that never
exceeds A = sum |x * w| + |bias|), adds the bias (one more) and, under PReLU, multiplies by the slope (one more, and the error
made so far is scaled by |slope|): |v - r| <= s * (T + 2) * 2^-24 * A with s = max(1, |slope|).  The one rounding to f16 adds
at most half an ulp of the result: 2^-11 * |r| for a normal result, 2^-25 for a subnormal one.  Hence
    |y - r| <= max(2^-11 * |r|, 2^-25) + s * (T + 2) * 2^-24 * A.

Matrix-core convs: the bound tests/test_gpu_detect_precision.py and test_gpu_scrfd.py use - (K + 2) * 2^-24 * A for the
accumulation over K = Cin * k * k products, the bias and the residual (A includes |bias| and |residual|), times max(1, |slope|),
plus the f16 output rounding (none for the f32 output)."""
import numpy as np
import pytest
import torch

from facerecognition_infrenceengine_amd import _lib
from tests.helpers import mbf_ref

pytestmark = pytest.mark.gpu

DW_SHAPES = [  # N, H, W, C, K, stride, pad
    (1, 1, 1, 8, 3, 1, 1),          # all border
    (2, 5, 7, 8, 3, 1, 1),
    (3, 9, 6, 24, 3, 2, 1),         # odd and even stride-2 edges, C no multiple of 16
    (1, 14, 14, 136, 3, 1, 1),      # C no multiple of 64
    (2, 8, 8, 64, 3, 2, 1),
    (1, 16, 16, 64, 3, 2, 1),
    (3, 7, 7, 512, 7, 1, 0),        # global form
    (1, 56, 56, 128, 3, 1, 1),      # crosses every tile boundary
    (2, 19, 23, 16, 5, 2, 2),       # the generic-kernel band path: 5x5, stride 2
    (1, 9, 9, 8, 7, 1, 3),          # 7x7 with padding: not the global form
    (2, 7, 7, 16, 7, 1, 0),         # global form, C below a wave
    (1, 20, 33, 8, 3, 1, 0),        # no padding
]
GUARD = 64


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _operands(shape, seed):
    N, H, W, C, K, stride, pad = shape
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, H, W, C)).astype(np.float16)
    w = (rng.standard_normal((K * K, C)) / K).astype(np.float16)
    bias = rng.standard_normal(C).astype(np.float32)
    slope = np.array([-0.3, 0.0, 0.25, 1.5], dtype=np.float32)[rng.integers(0, 4, C)]
    return x, w, bias, slope


def _run_dw(x, w, bias, slope, K, stride, pad, act):
    N, H, W, C = x.shape
    Ho, Wo = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
    n = N * Ho * Wo * C
    buf = torch.full((n + 2 * GUARD,), -7.0, dtype=torch.float16, device="cuda")
    y = buf[GUARD:GUARD + n]
    xd, wd, bd, sd = _dev(x), _dev(w), _dev(bias), _dev(slope)
    _lib.load().fr_dw_conv_f16(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(sd) if act == 2 else None, _lib.ptr(y), N, H, W, C, K,
                               stride, pad, Ho, Wo, act, _lib.stream_ptr())
    out = buf.cpu().numpy()
    assert (out[:GUARD] == -7.0).all() and (out[GUARD + n:] == -7.0).all(), "guard band written"
    return out[GUARD:GUARD + n].reshape(N, Ho, Wo, C)


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("shape", DW_SHAPES, ids=lambda s: "-".join(str(v) for v in s))
def test_dw_conv_against_float64(shape, act):
    N, H, W, C, K, stride, pad = shape
    x, w, bias, slope = _operands(shape, seed=C * 100 + K * 10 + stride)
    got = _run_dw(x, w, bias, slope, K, stride, pad, act)
    want, A = mbf_ref.dw_ref(x, w, bias, slope, K, stride, pad, act)
    assert got.shape == want.shape and not np.isnan(got.astype(np.float64)).any()
    s = np.maximum(1.0, np.abs(slope.astype(np.float64))) if act == 2 else 1.0
    bound = np.maximum(2.0 ** -11 * np.abs(want), 2.0 ** -25) + s * (K * K + 2) * 2.0 ** -24 * A
    err = np.abs(got.astype(np.float64) - want)
    print(f"dw {shape} act {act}: max err {err.max():.3e}, max err / bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()
    if act == 1:
        assert (got >= 0).all()


@pytest.mark.parametrize("shape", [(3, 9, 6, 24, 3, 2, 1), (3, 7, 7, 512, 7, 1, 0), (3, 14, 14, 136, 3, 1, 1)],
                         ids=lambda s: "-".join(str(v) for v in s))
def test_dw_conv_bits_do_not_depend_on_the_batch(shape):
    N, H, W, C, K, stride, pad = shape
    x, w, bias, slope = _operands(shape, seed=7)
    together = _run_dw(x, w, bias, slope, K, stride, pad, 2)
    for i in range(N):
        alone = _run_dw(x[i:i + 1], w, bias, slope, K, stride, pad, 2)
        assert np.array_equal(alone[0].view(np.uint16), together[i].view(np.uint16)), i


def test_the_global_form_and_the_band_path_agree_bit_for_bit():
    """a 7 x 7 map under a 7 x 7 kernel, pad 0 (global path) is the centre pixel of the same map under pad 3 (band path)"""
    shape = (2, 7, 7, 64, 7, 1, 0)
    x, w, bias, slope = _operands(shape, seed=11)
    g = _run_dw(x, w, bias, slope, 7, 1, 0, 2)
    b = _run_dw(x, w, bias, slope, 7, 1, 3, 2)
    assert g.shape == (2, 1, 1, 64) and np.array_equal(g[:, 0, 0].view(np.uint16), b[:, 3, 3].view(np.uint16))


def test_dw_conv_refuses_bad_arguments():
    lib = _lib.load()
    x = torch.zeros((1, 8, 8, 16), dtype=torch.float16, device="cuda")
    w = torch.zeros((49, 16), dtype=torch.float16, device="cuda")
    b = torch.zeros(16, dtype=torch.float32, device="cuda")
    y = torch.zeros((1, 8, 8, 16), dtype=torch.float16, device="cuda")
    p, st = _lib.ptr, _lib.stream_ptr()
    with pytest.raises(_lib.FrError, match="does not follow"):
        lib.fr_dw_conv_f16(p(x), p(w), p(b), None, p(y), 1, 8, 8, 16, 3, 1, 1, 7, 8, 0, st)              # wrong Ho
    with pytest.raises(_lib.FrError, match="multiple of 8"):
        lib.fr_dw_conv_f16(p(x), p(w), p(b), None, p(y), 1, 8, 8, 12, 3, 1, 1, 8, 8, 0, st)              # C = 12
    with pytest.raises(_lib.FrError, match="kernel 4"):
        lib.fr_dw_conv_f16(p(x), p(w), p(b), None, p(y), 1, 8, 8, 16, 4, 1, 1, 7, 7, 0, st)              # K = 4
    with pytest.raises(_lib.FrError, match="needs the slope"):
        lib.fr_dw_conv_f16(p(x), p(w), p(b), None, p(y), 1, 8, 8, 16, 3, 1, 1, 8, 8, 2, st)              # act 2, no slope
    with pytest.raises(_lib.FrError, match="not supported"):
        lib.fr_dw_conv_f16(p(x), p(w), p(b), None, p(y), 1, 8, 8, 16, 3, 3, 1, 3, 3, 0, st)              # stride 3
    with pytest.raises(_lib.FrError, match="not supported"):
        lib.fr_dw_conv_f16(p(x), p(w), p(b), None, p(y), 1, 8, 8, 16, 3, 1, 2, 10, 10, 0, st)            # pad > K / 2
    torch.cuda.synchronize()
    assert not y.any()


# ------------------------------------------------------------------ the matrix-core conv with a choice of activation
ACT_CASES = [  # cin, cout, k, stride, H, W, N, residual, act, f32
    (64, 128, 1, 1, 9, 11, 2, False, 2, False),        # 1x1 expand + PReLU
    (128, 64, 1, 1, 9, 11, 2, True, 0, False),         # 1x1 project, linear, + residual
    (512, 512, 1, 1, 1, 1, 3, False, 0, True),         # the fully connected layer on a 1 x 1 map, f32 out
    (8, 64, 3, 2, 12, 12, 2, False, 2, False),         # the stem's shape: 3x3 stride 2 on 8 channels
    (64, 64, 1, 1, 7, 5, 1, True, 2, False),           # residual THEN PReLU: the epilogue's order
    (24, 40, 1, 1, 6, 6, 1, False, 2, False),          # widths that are no multiples of 16
]


def _run_conv(case, seed, entry):
    from facerecognition_infrenceengine_amd.scrfd import pack_conv
    cin, cout, k, stride, H, W, N, has_res, act, f32 = case
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float16).astype(np.float64)
    b = rng.standard_normal(cout).astype(np.float32)
    slope = np.array([-0.3, 0.0, 0.25, 1.5], dtype=np.float32)[rng.integers(0, 4, cout)]
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    packed, bias, cin_p, cout_w = pack_conv(w, b)
    x = np.zeros((N, H, W, cin_p), dtype=np.float16)
    x[..., :cin] = rng.standard_normal((N, H, W, cin)).astype(np.float16)
    ldo = cout if f32 else (cout + 7) // 8 * 8
    r = None
    if has_res:
        r = np.zeros((N, Ho, Wo, ldo), dtype=np.float16)
        r[..., :cout] = rng.standard_normal((N, Ho, Wo, cout)).astype(np.float16)
    sl = np.zeros(cout_w, dtype=np.float32)
    sl[:cout] = slope
    xd, wd, bd, sd, rd = _dev(x), _dev(packed), _dev(bias), _dev(sl), (_dev(r) if has_res else None)
    y = torch.full((N, Ho, Wo, ldo), float("nan"), dtype=torch.float32 if f32 else torch.float16, device="cuda")
    lib = _lib.load()
    if entry == "act":
        lib.fr_det_conv_act_f16(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(sd) if act == 2 else None, _lib.ptr(rd), _lib.ptr(y), N, H, W,
                                cin_p, cout_w, k, stride, pad, Ho, Wo, ldo, ldo, act, int(f32), 0, _lib.stream_ptr())
    else:
        assert act in (0, 1)
        lib.fr_det_conv_f16(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(rd), _lib.ptr(y), N, H, W, cin_p, cout_w, k, stride, pad, Ho, Wo,
                            ldo, ldo, act, int(f32), 0, _lib.stream_ptr())
    want, A = mbf_ref.conv_ref(x[..., :cin], w, b, slope, None if r is None else r[..., :cout], stride, pad, act)
    return y.cpu().numpy(), want, A, slope


@pytest.mark.parametrize("case", ACT_CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_det_conv_act_against_float64(case):
    cin, cout, k, stride, H, W, N, has_res, act, f32 = case
    got, want, A, slope = _run_conv(case, seed=cin + cout, entry="act")
    got = got.astype(np.float64)
    assert not np.isnan(got).any()
    if not f32:
        assert not got[..., cout:].any()
    got = got[..., :cout]
    s = np.maximum(1.0, np.abs(slope.astype(np.float64))) if act == 2 else 1.0
    bound = s * (cin * k * k + 2) * 2.0 ** -24 * A + (0.0 if f32 else np.maximum(2.0 ** -11 * np.abs(want), 2.0 ** -25))
    err = np.abs(got - want)
    print(f"act conv {case}: max err {err.max():.3e}, max err / bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("case", [(56, 88, 3, 2, 33, 47, 1, False, 1, False), (88, 88, 3, 1, 13, 21, 2, True, 1, False),
                                  (80, 20, 3, 1, 20, 20, 1, False, 0, True), (64, 128, 1, 1, 9, 11, 2, False, 1, False)],
                         ids=lambda c: "-".join(str(int(v)) for v in c))
def test_relu_through_the_new_entry_is_the_detector_conv_bit_for_bit(case):
    a = _run_conv(case, seed=5, entry="act")[0]
    b = _run_conv(case, seed=5, entry="det")[0]
    assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else np.uint16),
                                                 b.view(np.uint32 if b.dtype == np.float32 else np.uint16))
