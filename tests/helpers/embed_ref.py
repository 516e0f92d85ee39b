"""Float64 references for the embed net's conv kernels (conv_mfma.hip and the conv_*.hip family), plain numpy / torch on the
CPU, and the operand generators, case lists and float32 emulation that tests/test_embed_ref_host.py (CPU) and
tests/test_gpu_embed_pins.py (GPU) share.

Two instruments:
  * exact-integer operands (int_operands, int_stage_block): every product, partial sum and output is an integer that the
    number format holds exactly (f16 outputs |v| <= 2048, f32 partial sums < 2^24), so the kernel's result does not depend on
    K or on the order of summation and is compared bit for bit.  That this holds is asserted HERE, on the reference.
  * float64 with a derived per-element bound, where the output is f32 or K is small: `mag` is the same sum over absolute
    values, so (n roundings) * 2^-24 * mag bounds any order of n f32 operations.

Layouts are the engine's: activations NHWC, weights [Cout][tap][Cin] rows with the second input's [C2] columns appended, the
border-class bias a 3x3 table [(first / inner / last row) x (first / inner / last column)][Cout].  Operation order is the
kernels' (conv_epilogue): bias, PReLU, residual, one rounding."""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24          # unit roundoff of f32
U16 = 2.0 ** -11          # unit roundoff of f16
BK = 64                   # K step of conv_mfma_kernel (halves)


def out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def splitk_slices(nk, splitk):
    """K-step ranges [ks, ke) of the slices of the split-K mode: per = ceil(nk / splitk), slice z = [z * per, min(nk, (z + 1) *
    per)); a slice that starts at or past nk is empty (ks >= ke) and must write zeros."""
    per = -(-nk // splitk)
    return [(z * per, min(nk, (z + 1) * per)) for z in range(splitk)]


def border_class(n):
    c = np.ones(n, dtype=np.int64)
    c[0] = 0
    c[-1] = 2
    return c


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2)


def patches(x, k, stride, pad, x2=None):
    """im2col in the engine's K order: [B*Ho*Wo][(kh*k + kw)*Cin + ci], then the second input's channels at pixel
    (ho*stride, wo*stride)."""
    B, H, W, C = x.shape
    Ho, Wo = out_size(H, k, stride, pad), out_size(W, k, stride, pad)
    u = F.unfold(_nchw(x), k, padding=pad, stride=stride)                    # [B][C*k*k][Ho*Wo], channel-major
    p = u.reshape(B, C, k * k, Ho * Wo).permute(0, 3, 2, 1).reshape(B * Ho * Wo, k * k * C).numpy()
    if x2 is not None:
        p = np.concatenate([p, x2[:, ::stride, ::stride][:, :Ho, :Wo].reshape(B * Ho * Wo, -1)], 1)
    return np.ascontiguousarray(p)


def conv_ref(x, w, bias, bias_mode, slope, residual, stride, pad, x2=None, w2=None, krange=None, k=None):
    """(want, mag), float64 NHWC [B][Ho][Wo][Cout].  w: [Cout][k*k*Cin (+ C2)] rows (or the C2 columns apart in w2); the packed
    stem passes its 72 real columns and k = 3.  krange = (k0, k1): only columns [k0, k1) of the flattened row and no epilogue
    (one split-K slice; k0 >= k1 is an empty slice: zeros)."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    if w2 is not None:
        w = np.concatenate([w, np.asarray(w2, np.float64)], 1)
    if x2 is not None:
        x2 = np.asarray(x2, np.float64)
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    C2 = 0 if x2 is None else x2.shape[3]
    kmain = w.shape[1] - C2
    if k is None:
        k = int(round((kmain // Cin) ** 0.5))
    assert k * k * Cin == kmain, (k, Cin, w.shape)
    Ho, Wo = out_size(H, k, stride, pad), out_size(W, k, stride, pad)
    if krange is not None:
        assert bias is None and slope is None and residual is None
        k0, k1 = krange
        p = patches(x, k, stride, pad, x2)
        want = p[:, k0:k1] @ w[:, k0:k1].T
        mag = np.abs(p[:, k0:k1]) @ np.abs(w[:, k0:k1]).T
        return want.reshape(B, Ho, Wo, Cout), mag.reshape(B, Ho, Wo, Cout)

    def run(xx, ww, xx2):
        w4 = torch.from_numpy(np.ascontiguousarray(ww[:, :kmain].reshape(Cout, k, k, Cin))).permute(0, 3, 1, 2)
        o = F.conv2d(_nchw(xx), w4, None, stride, pad)
        if xx2 is not None:
            o2 = F.conv2d(_nchw(xx2), torch.from_numpy(np.ascontiguousarray(ww[:, kmain:]))[:, :, None, None], None, stride, 0)
            o = o + o2[:, :, :Ho, :Wo]
        return o.permute(0, 2, 3, 1).numpy()

    want = run(x, w, x2)
    mag = run(np.abs(x), np.abs(w), None if x2 is None else np.abs(x2))
    if bias is not None:
        bias = np.asarray(bias, np.float64)
        if bias_mode == 1:
            b = bias.reshape(3, 3, Cout)[border_class(Ho)][:, border_class(Wo)][None]
        else:
            b = bias.reshape(1, 1, 1, Cout)
        want = want + b
        mag = mag + np.abs(b)
    if slope is not None:
        s = np.asarray(slope, np.float64).reshape(1, 1, 1, Cout)
        want = np.where(want > 0, want, want * s)
        mag = mag * np.maximum(1.0, np.abs(s))
    if residual is not None:
        r = np.asarray(residual, np.float64)
        want = want + r
        mag = mag + np.abs(r)
    return want, mag


def conv_bound(K, mag, want=None):
    """K products summed in f32 in any order, + bias, PReLU multiply, residual: (K + 2) roundings at 2^-24 of the running
    magnitude; an f16 output adds its one rounding (half an ulp of |want|, 2^-25 below the normal range)."""
    b = (K + 2) * U32 * mag
    return b if want is None else b + U16 * np.abs(want) + 2.0 ** -25


def epilogue_ref(partial, bias, bias_mode, slope, residual, Ho, Wo):
    """fr_conv_splitk_epilogue: (want, mag) [M][Cout] from f32 partials [splitk][M][Cout]."""
    p = np.asarray(partial, np.float64)
    M, Cout = p.shape[1:]
    want, mag = p.sum(0), np.abs(p).sum(0)
    if bias is not None:
        bias = np.asarray(bias, np.float64)
        if bias_mode == 1:
            b = bias.reshape(3, 3, Cout)[border_class(Ho)][:, border_class(Wo)].reshape(Ho * Wo, Cout)
            b = b[np.arange(M) % (Ho * Wo)]
        else:
            b = bias.reshape(1, Cout)
        want = want + b
        mag = mag + np.abs(b)
    if slope is not None:
        s = np.asarray(slope, np.float64).reshape(1, Cout)
        want = np.where(want > 0, want, want * s)
        mag = mag * np.maximum(1.0, np.abs(s))
    if residual is not None:
        r = np.asarray(residual, np.float64).reshape(M, Cout)
        want = want + r
        mag = mag + np.abs(r)
    return want, mag


def epilogue_bound(splitk, mag, want):
    """splitk adds (from zero), bias, PReLU multiply, residual: splitk + 3 roundings in f32, then one to f16."""
    return (splitk + 3) * U32 * mag + U16 * np.abs(want) + 2.0 ** -25


def fc_tail_ref(partial, bias):
    """fr_fc_reduce_l2norm's embedding: (want, mag) [B][dim] = bias + sum over slices."""
    p = np.asarray(partial, np.float64)
    b = np.asarray(bias, np.float64)[None]
    return b + p.sum(0), np.abs(b) + np.abs(p).sum(0)


def fc_tail_bound(splitk, mag):
    return (splitk + 1) * U32 * mag


def normed_ref(embedding):
    e = np.asarray(embedding, np.float64)
    return e / np.sqrt((e * e).sum(1, keepdims=True))


def normed_bound(dim, want):
    """dim squares (one rounding each) summed in f32 (dim - 1 roundings, any order): the sum of squares is within (dim + 2) u
    relative with the square root's own rounding counted in, the root halves that, then the root's and the division's
    roundings and the second-order terms: ((dim + 2) / 2 + 3) u |want|.  sqrtf and / are correctly rounded in this build (hipcc's
    default for HIP; the Makefile sets -fno-fast-math)."""
    return ((dim + 2) / 2 + 3) * U32 * np.abs(want)


# ---------------------------------------------------------------- operands
def _f16(a):
    return a.astype(np.float16).astype(np.float64)


def _geometry(B, H, W, Cin, Cout, k, stride, pad, bias_mode, C2):
    return SimpleNamespace(B=B, H=H, W=W, Cin=Cin, Cout=Cout, k=k, stride=stride, pad=pad, bias_mode=bias_mode, C2=C2,
                           Ho=out_size(H, k, stride, pad), Wo=out_size(W, k, stride, pad), K=k * k * Cin + C2)


def float_operands(rng, B, H, W, Cin, Cout, k, stride, pad, bias_mode=0, bias=False, slope=False, residual=False, C2=0, w=None):
    """Random operands at the precision the kernel sees them (x, w, residual f16; bias, slope f32), as float64 arrays."""
    o = _geometry(B, H, W, Cin, Cout, k, stride, pad, bias_mode, C2)
    o.x = _f16(rng.standard_normal((B, H, W, Cin)))
    o.x2 = _f16(rng.standard_normal((B, H, W, C2))) if C2 else None
    o.w = _f16(rng.standard_normal((Cout, o.K)) * (2.0 / o.K) ** 0.5) if w is None else w
    o.bias = rng.standard_normal(9 * Cout if bias_mode == 1 else Cout).astype(np.float32).astype(np.float64) if bias else None
    o.slope = (rng.random(Cout) * 0.5).astype(np.float32).astype(np.float64) if slope else None
    o.residual = _f16(rng.standard_normal((B, o.Ho, o.Wo, Cout))) if residual else None
    return o


def int_weights(rng, Cout, K, var_x=2.0, sigma=30.0):
    """Sparse weights in {-1, 0, 1}: P(w != 0) = min(1/4, sigma^2 / (K var_x)), so a sum over K inputs of variance var_x has a
    standard deviation of at most sigma whatever K is."""
    p = min(0.25, sigma * sigma / (K * var_x))
    return rng.choice([-1.0, 1.0], (Cout, K)) * (rng.random((Cout, K)) < p)


def int_operands(rng, B, H, W, Cin, Cout, k, stride, pad, bias_mode=0, bias=False, slope=False, residual=False, C2=0, w=None,
                 partial=False, stem=False):
    """Integer operands: x in {-2 .. 2}, sparse w in {-1, 0, 1}, integer bias and residual, slope in {-1, 0, 1, 2} (an integer
    slope keeps every value an integer, and the slope of another channel still changes the result).  Returns the operands with
    .want (float64); asserts on it that the kernel's arithmetic is exact: every f32 partial sum is below 2^24 in magnitude
    (mag < 2^24) and, unless `partial` (f32 partials out), every output is an f16 integer (|want| <= 2048).  stem: only channels
    0 .. 2 of x and of each tap's weights are non-zero, as in the packed stem."""
    o = _geometry(B, H, W, Cin, Cout, k, stride, pad, bias_mode, C2)
    o.x = rng.integers(-2, 3, (B, H, W, Cin)).astype(np.float64)
    o.x2 = rng.integers(-2, 3, (B, H, W, C2)).astype(np.float64) if C2 else None
    o.w = int_weights(rng, Cout, o.K) if w is None else w
    if stem:
        o.x[..., 3:] = 0.0
        o.w = (rng.integers(-1, 2, (Cout, k * k, Cin)) * (np.arange(Cin) < 3)).reshape(Cout, o.K).astype(np.float64)
    o.bias = rng.integers(-8, 9, 9 * Cout if bias_mode == 1 else Cout).astype(np.float64) if bias else None
    o.slope = rng.integers(-1, 3, Cout).astype(np.float64) if slope else None
    o.residual = rng.integers(-16, 17, (B, o.Ho, o.Wo, Cout)).astype(np.float64) if residual else None
    if partial:
        return o
    o.want, mag = conv_ref(o.x, o.w, o.bias, bias_mode, o.slope, o.residual, stride, pad, x2=o.x2)
    assert_exact(o.want, mag)
    return o


def assert_exact(want, mag, limit=2048.0):
    """The condition under which a kernel's result is independent of summation order: checked on the reference."""
    assert np.array_equal(want, np.round(want)), "reference is not integral"
    assert mag.max() < 2.0 ** 24, mag.max()
    assert np.abs(want).max() <= limit, np.abs(want).max()
    assert np.abs(want).max() > 0


def int_stage_block(rng, B, HW, C):
    """One residual block of a stage kernel (fr_conv_stage14_f16 / fr_conv_stage28_f16) on integer operands: conv1 + 9-class bias
    + PReLU -> f16 map `mid`, conv2 + bias + block input.  conv2's weights are sparser (its input is conv1's output, not
    {-2 .. 2}); mid and the output are asserted to be f16 integers, so the whole block is exact."""
    o = SimpleNamespace(B=B, HW=HW, C=C)
    K = 9 * C
    o.x = rng.integers(-2, 3, (B, HW, HW, C)).astype(np.float64)
    o.w1 = int_weights(rng, C, K, sigma=10.0)
    o.b9 = rng.integers(-8, 9, 9 * C).astype(np.float64)
    o.slope = rng.integers(-1, 3, C).astype(np.float64)
    o.mid, mag = conv_ref(o.x, o.w1, o.b9, 1, o.slope, None, 1, 1)
    assert_exact(o.mid, mag)
    o.w2 = int_weights(rng, C, K, var_x=float((o.mid ** 2).mean()), sigma=60.0)
    o.b2 = rng.integers(-8, 9, C).astype(np.float64)
    o.want, mag = conv_ref(o.mid, o.w2, o.b2, 0, None, o.x, 1, 1)
    assert_exact(o.want, mag)
    return o


# ---------------------------------------------------------------- cases shared by the host test and the GPU pins
# B. split-K partials of fr_conv_nhwc_f16: B, H, W, Cin, Cout, k, stride, pad, splitk, C2
PARTIAL_CASES = [
    (1, 5, 9, 128, 128, 3, 1, 1, 6, 0),         # the engine's counts (_small_batch_splitk): Cin 128 -> 6 (<= 8 faces) and 2 (<= 48)
    (3, 7, 7, 128, 128, 3, 1, 1, 2, 0),
    (3, 5, 9, 256, 64, 3, 1, 1, 12, 0),         # Cin 256 -> 12 and 4; 64-cout tile, M = 135 of 256
    (1, 7, 7, 256, 256, 3, 1, 1, 4, 0),
    (1, 7, 7, 512, 128, 3, 1, 1, 24, 0),        # Cin 512 -> 24 and 8
    (3, 5, 9, 512, 128, 3, 1, 1, 8, 0),         # M = 135: a full 128-pixel tile across three images + 7 pixels
    (1, 5, 9, 128, 64, 3, 1, 1, 4, 0),          # ragged last slice: nk = 18 -> 5, 5, 5, 3
    (3, 7, 7, 64, 64, 3, 1, 1, 4, 0),           # empty slice: nk = 9 -> 3, 3, 3, 0
    (3, 13, 13, 128, 128, 3, 2, 1, 4, 64),      # x2 form: nk = 19 -> 5, 5, 5, 4, the last slice straddles nk_main = 18
    (3, 1, 1, 25088, 512, 1, 1, 0, 28, 0),      # the FC at its real shape: 28 slices of 14 K steps
    (130, 1, 1, 25088, 512, 1, 1, 0, 28, 0),    # two pixel tiles
    (3, 1, 1, 1920, 512, 1, 1, 0, 28, 0),       # short FC: nk = 30 -> 15 slices of 2, 13 empty
]

# C. fr_conv_splitk_epilogue: B = 3, Ho x Wo = 5 x 9 (M = 135; M * Cout / 4 = 2160 / 2295, no multiple of 256)
EPILOGUE_GEOM = (3, 5, 9)
EPILOGUE_SPLITK = (1, 2, 7, 24)
EPILOGUE_COUT = (64, 68)
EPILOGUE_FORMS = [(bias, slope, res) for bias in (None, 0, 1) for slope in (False, True) for res in (False, True)]

# D. fr_fc_reduce_l2norm: B, splitk, dim
FC_TAIL_CASES = [(1, 28, 512), (5, 28, 512), (4, 1, 512), (3, 8, 512), (3, 11, 512), (2, 28, 1024), (2, 5, 1280), (3, 3, 260),
                 (2, 2, 4)]


def case_seed(case):
    return sum((i + 1) * 7919 * int(v) for i, v in enumerate(case)) & 0x7fffffff


_fc_cache = {}


def fc_weights(kind, Cin):
    """The FC's [512][Cin] weights, made once per (kind, Cin): 12.8 M elements at the real shape."""
    if (kind, Cin) not in _fc_cache:
        rng = np.random.default_rng(Cin + (kind == "int"))
        if kind == "int":
            w = int_weights(rng, 512, Cin)
        else:
            w = _f16(rng.standard_normal((512, Cin), dtype=np.float32) * np.float32((2.0 / Cin) ** 0.5))
        _fc_cache[(kind, Cin)] = w
    return _fc_cache[(kind, Cin)]


def partial_operands(case, kind):
    B, H, W, Cin, Cout, k, stride, pad, splitk, C2 = case
    rng = np.random.default_rng(case_seed(case))
    w = fc_weights(kind, Cin) if k == 1 else None
    if kind == "int":
        return int_operands(rng, B, H, W, Cin, Cout, k, stride, pad, C2=C2, w=w, partial=True)
    return float_operands(rng, B, H, W, Cin, Cout, k, stride, pad, C2=C2, w=w)


def partial_refs(o, splitk, kind):
    """[(want, mag, K_slice)] per slice, [M][Cout]; for integer operands the exactness condition is asserted."""
    p = patches(o.x, o.k, o.stride, o.pad, o.x2)
    pa, wa = np.abs(p), np.abs(o.w)
    out = []
    for ks, ke in splitk_slices(o.K // BK, splitk):
        k0, k1 = ks * BK, max(ks, ke) * BK
        want, mag = p[:, k0:k1] @ o.w[:, k0:k1].T, pa[:, k0:k1] @ wa[:, k0:k1].T
        if kind == "int" and k1 > k0:
            assert_exact(want, mag, limit=2.0 ** 24 - 1)
        out.append((want, mag, k1 - k0))
    return out


def epilogue_operands(rng, splitk, Cout, bias_mode, slope, res, kind):
    B, Ho, Wo = EPILOGUE_GEOM
    M = B * Ho * Wo
    o = SimpleNamespace(splitk=splitk, M=M, Cout=Cout, Ho=Ho, Wo=Wo, bias_mode=bias_mode or 0)
    nb = 9 * Cout if bias_mode == 1 else Cout
    if kind == "int":
        o.partial = rng.integers(-40, 41, (splitk, M, Cout)).astype(np.float64)
        o.bias = None if bias_mode is None else rng.integers(-8, 9, nb).astype(np.float64)
        o.slope = rng.integers(-1, 3, Cout).astype(np.float64) if slope else None
        o.residual = rng.integers(-16, 17, (M, Cout)).astype(np.float64) if res else None
    else:
        o.partial = rng.standard_normal((splitk, M, Cout)).astype(np.float32).astype(np.float64)
        o.bias = None if bias_mode is None else rng.standard_normal(nb).astype(np.float32).astype(np.float64)
        o.slope = (rng.random(Cout) * 0.5).astype(np.float32).astype(np.float64) if slope else None
        o.residual = _f16(rng.standard_normal((M, Cout))) if res else None
    o.want, o.mag = epilogue_ref(o.partial, o.bias, o.bias_mode, o.slope, o.residual, Ho, Wo)
    if kind == "int":
        assert_exact(o.want, o.mag)
    return o


def fc_tail_operands(rng, B, splitk, dim, kind):
    o = SimpleNamespace(B=B, splitk=splitk, dim=dim)
    if kind == "int":
        o.partial = rng.integers(-1000, 1001, (splitk, B, dim)).astype(np.float64)
        o.bias = rng.integers(-8, 9, dim).astype(np.float64)
    else:
        o.partial = rng.standard_normal((splitk, B, dim)).astype(np.float32).astype(np.float64)
        o.bias = rng.standard_normal(dim).astype(np.float32).astype(np.float64)
    o.want, o.mag = fc_tail_ref(o.partial, o.bias)
    if kind == "int":
        assert_exact(o.want, o.mag, limit=2.0 ** 24 - 1)
    return o


# ---------------------------------------------------------------- float32 emulation of the kernels, with planted faults
def emulate_partials(o, splitk, fault=None):
    """The split-K mode of fr_conv_nhwc_f16 in float32: slice z = f32 matrix product over its K columns.  Faults: ("drop", s):
    K step s is skipped; "boundary": slice 0 takes the first step of slice 1 (the slices' sum stays right); "unwritten": an empty
    slice is left as it was (NaN)."""
    p = patches(o.x, o.k, o.stride, o.pad, o.x2).astype(np.float32)
    w = o.w.astype(np.float32)
    sl = splitk_slices(o.K // BK, splitk)
    if fault == "boundary":
        sl[0], sl[1] = (sl[0][0], sl[0][1] + 1), (sl[1][0] + 1, sl[1][1])
    out = np.full((splitk, p.shape[0], w.shape[0]), np.nan, np.float32)
    for z, (ks, ke) in enumerate(sl):
        if ks >= ke:
            if fault != "unwritten":
                out[z] = 0.0
            continue
        cols = np.concatenate([np.arange(s * BK, (s + 1) * BK) for s in range(ks, ke)
                               if not (isinstance(fault, tuple) and fault[1] == s)] or [np.arange(0)]).astype(np.int64)
        out[z] = p[:, cols] @ w[:, cols].T
    return out


def emulate_epilogue(partial, bias, bias_mode, slope, residual, Ho, Wo, fault=None):
    """fr_conv_splitk_epilogue in float32, slice after slice, -> f16.  Faults: "miss_slice" (the last slice is not added),
    "bias_col" (inner columns get the last column's class), "slope_prev" (the slope of channel c - 1), "res_neighbour" (the
    residual of pixel m + 1)."""
    p = np.asarray(partial, np.float32)
    splitk, M, Cout = p.shape
    v = np.zeros((M, Cout), np.float32)
    for z in range(splitk - (fault == "miss_slice")):
        v = v + p[z]
    if bias is not None:
        b = np.asarray(bias, np.float32)
        if bias_mode == 1:
            cc = border_class(Wo)
            if fault == "bias_col":
                cc[1:-1] = 2
            b = b.reshape(3, 3, Cout)[border_class(Ho)][:, cc].reshape(Ho * Wo, Cout)[np.arange(M) % (Ho * Wo)]
        v = v + b
    if slope is not None:
        s = np.asarray(slope, np.float32)
        if fault == "slope_prev":
            s = np.roll(s, 1)
        v = np.where(v > 0, v, v * s[None]).astype(np.float32)
    if residual is not None:
        r = np.asarray(residual, np.float32).reshape(M, Cout)
        if fault == "res_neighbour":
            r = np.roll(r, -1, 0)
        v = v + r
    return v.astype(np.float16)


def emulate_fc_tail(partial, bias, fault=None):
    """fr_fc_reduce_l2norm in sequential float32: (embedding, normed).  Faults: "miss_slice", "short_norm" (the norm over dim - 4
    columns)."""
    p = np.asarray(partial, np.float32)
    e = np.broadcast_to(np.asarray(bias, np.float32), p.shape[1:]).copy()
    for z in range(p.shape[0] - (fault == "miss_slice")):
        e = e + p[z]
    ss = np.zeros(e.shape[0], np.float32)
    for c in range(e.shape[1] - 4 * (fault == "short_norm")):
        ss = ss + e[:, c] * e[:, c]
    with np.errstate(divide="ignore", invalid="ignore"):          # dim = 4 with "short_norm": a norm over no column at all
        return e, e / np.sqrt(ss)[:, None]


def worst_ratio(err, bound):
    """max err / bound over the elements; an element with bound 0 (nothing was summed) must have err 0."""
    assert not np.isnan(err).any()
    z = bound == 0
    assert not err[z].any()
    return float(np.max(err[~z] / bound[~z])) if (~z).any() else 0.0
