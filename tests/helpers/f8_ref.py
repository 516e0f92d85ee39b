"""References for the fp8 (OCP e4m3) conv path of the embed net - fr_conv_nhwc_f8 (conv_halo_kernel<..., LEAN, F8>), fr_conv_stage14_f8,
fr_conv_stage14_f8_pack and the two quantisers - plain numpy on the CPU, with the operand generators and the float32 emulation
that tests/test_f8_ref_host.py (CPU) and tests/test_gpu_f8_pins.py (GPU) share.  Companion of tests/helpers/embed_ref.py.

Rounding to e4m3 is discontinuous, so a statistical comparison of codes is all a random-operand test can do.  The instrument here
makes every value BEFORE a rounding known exactly instead: inputs and weights on the e4m3 grid, scales and slopes powers of two,
bias / centre / residual multiples of a power of two.  All terms of an output's sum are then multiples of 2^-q, and while
mag * 2^q < 2^24 (mag = the sum of the terms' absolute values) every f32 partial sum, in any order, is exact - given that no
product falls out of the 13-bit window that the fp8 matrix instruction keeps inside a group of 8 channels (`misaligned`); the
roundings to f16 and to e4m3 - ties, subnormals, saturation - are deterministic functions of exact values and the outputs are
compared bit for bit.
Both the exactness conditions and the coverage conditions (each kind of rounding event occurs, on border pixels, in the last
pixel tile and inside) are asserted HERE, on the reference.

Operation order (include/frhip.h): acc * oscale + bias (9 border classes) -> PReLU -> + residual -> f16 (RNE);
y8 = e4m3((f16 - sub) * mul), saturating.  Layouts as in embed_ref: NHWC, weights [Cout][tap][Cin]."""
from types import SimpleNamespace

import numpy as np
import torch

from tests.helpers.embed_ref import U32, border_class, case_seed, conv_ref, patches

E4M3_MAX = 448.0
STEP_K = 128                                  # channels of one K step (one v_mfma_scale_f32_16x16x128_f8f6f4 per tap x 128 channels)


def seed_of(case):
    return case_seed(tuple(7 if v is None else v for v in case))


# ---------------------------------------------------------------- number formats
def _e4m3_step(m):
    """spacing of the e4m3 grid at magnitude m (<= 448): 2^(e - 3) in the binade [2^e, 2^(e+1)), 2^-9 below 2^-6"""
    _, e = np.frexp(np.maximum(m, 2.0 ** -9))
    return np.ldexp(1.0, np.maximum(e - 1, -6) - 3)


def e4m3(a):
    """float64 -> the nearest OCP e4m3 value (float64): ties to even, subnormal step 2^-9, saturating at +-448 (inf too)."""
    a = np.asarray(a, np.float64)
    m = np.minimum(np.abs(a), E4M3_MAX)
    step = _e4m3_step(m)
    return np.copysign(np.rint(m / step) * step, a)


def e4m3_trunc(a):
    """the same grid, rounded towards zero (a planted fault)"""
    a = np.asarray(a, np.float64)
    m = np.minimum(np.abs(a), E4M3_MAX)
    step = _e4m3_step(m)
    return np.copysign(np.floor(m / step) * step, a)


def e4m3_is_tie(a):
    m = np.minimum(np.abs(np.asarray(a, np.float64)), E4M3_MAX)
    q = m / _e4m3_step(m)
    return q - np.floor(q) == 0.5


def e4m3_values():
    """the 254 finite codes' values, in code order without the two NaN codes"""
    codes = np.array([c for c in range(256) if c & 0x7f != 0x7f], np.uint8)
    return torch.from_numpy(codes).view(torch.float8_e4m3fn).float().numpy().astype(np.float64)


def e4m3_bytes(values):
    """values ON the e4m3 grid -> their codes (uint8 torch tensor)"""
    t = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32))
    b = t.to(torch.float8_e4m3fn)
    assert torch.equal(b.float(), t), "not on the e4m3 grid"
    return b.view(torch.uint8)


def bytes_values(t):
    """uint8 codes (torch, CPU) -> float64 values (NaN for the NaN codes)"""
    return t.view(torch.float8_e4m3fn).float().numpy().astype(np.float64)


def f16(a):
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def f16_is_tie(v):
    v = np.asarray(v, np.float64)
    h16 = v.astype(np.float16)
    d = v - h16.astype(np.float64)
    nb = np.nextafter(h16, np.where(d > 0, np.inf, -np.inf).astype(np.float16)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (d != 0) & (np.abs(d) == np.abs(nb - v))


def is_f32(a):
    a = np.asarray(a, np.float64)
    return a.astype(np.float32).astype(np.float64) == a


def frac_bits(a):
    """per element: the smallest q >= 0 with a * 2^q an integer"""
    a = np.asarray(a, np.float64)
    m, e = np.frexp(a)
    M = np.ldexp(m, 53).astype(np.int64)
    low = (M & -M).astype(np.float64)
    _, l = np.frexp(low)                                   # low = 2^(l - 1)
    return np.where(a == 0, 0, np.maximum(53 - (l - 1) - e, 0)).astype(np.int64)


def _exponents(a):
    """(floor(log2 |a|), exponent of a's lowest set bit) per element; zeros: (-1000, +1000), so that they never decide a max / min"""
    a = np.asarray(a, np.float64)
    m, e = np.frexp(a)
    M = np.ldexp(m, 53).astype(np.int64)
    _, l = np.frexp((M & -M).astype(np.float64))
    z = a == 0
    return np.where(z, -1000, e - 1).astype(np.int64), np.where(z, 1000, e - 53 + l - 1).astype(np.int64)


ALIGN_BITS = 13
ALIGN_GROUP = 8


def misaligned(x, w):
    """What the fp8 matrix instruction does NOT add exactly, measured on an MI355X (docs/KERNEL_NOTES.md 4.12): inside one
    v_mfma_scale_f32_16x16x128_f8f6f4 the products of 8 consecutive k (channels 8 i .. 8 i + 7 of a tap) are aligned to the
    largest of them and cut off - towards zero - below 2^-13 of its leading bit; the groups' sums then enter the f32 accumulator
    with plain f32 rounding.  64 + 15 * 2^-8 - 64 in three channels of one group gives 14 * 2^-8, and a 2^-8 beside the 64
    vanishes; eight channels further on it is kept.  So the exactness of a sum needs more than mag * 2^q < 2^24: in every group
    every non-zero product must be a multiple of 2^(E - 13), E = floor(log2 |largest product of the group|).
    -> {cout: columns of w whose product breaks that at some pixel} (empty: the condition holds)."""
    Cout, K = w.shape
    P = patches(x, 3, 1, 1)
    EX, LX = _exponents(P)
    exmax, lxmin = EX.max(0), LX.min(0)
    ew, lw = _exponents(w)
    bad = {}
    for c in range(Cout):
        nz = np.flatnonzero(w[c])
        if len(nz) < 2:
            continue
        if (lxmin[nz] + lw[c, nz]).min() >= (exmax[nz] + ew[c, nz]).max() + 1 - ALIGN_BITS:      # the whole row at once: cheap, sufficient
            continue
        E, _ = _exponents(P[:, nz] * w[c, nz])
        L = LX[:, nz] + lw[c, nz]
        group = nz // ALIGN_GROUP
        first = np.flatnonzero(np.r_[True, np.diff(group) > 0])
        Emax = np.repeat(np.maximum.reduceat(E, first, axis=1), np.diff(np.r_[first, len(nz)]), axis=1)
        cols = nz[(L < Emax - ALIGN_BITS).any(0)]
        if len(cols):
            bad[c] = cols
    return bad


def class_bias(bias, bias_mode, H, Cout):
    """[H][H][Cout] (mode 1) or [1][1][Cout] / zeros: the bias of every pixel"""
    if bias is None:
        return np.zeros((1, 1, Cout))
    bias = np.asarray(bias, np.float64)
    if bias_mode == 1:
        return bias.reshape(3, 3, Cout)[border_class(H)][:, border_class(H)]
    return bias.reshape(1, 1, Cout)


def location_masks(B, H):
    """[B][H][H] masks: the last four pixels (192 .. 195) of every 196-pixel tile (14x14: the image; 28x28: seven rows), the
    other border pixels, the rest"""
    px = np.arange(H * H).reshape(H, H)
    last = np.broadcast_to((px % 196) >= 192, (B, H, H)).copy()
    edge = np.zeros((H, H), bool)
    edge[0] = edge[-1] = edge[:, 0] = edge[:, -1] = True
    border = np.broadcast_to(edge, (B, H, H)) & ~last
    return {"last": last, "border": border, "inside": ~last & ~border}


# ---------------------------------------------------------------- one conv, float64, every intermediate kept
def conv_f8_ref(x, w, oscale, bias, bias_mode, slope, residual, sub, mul):
    """One fp8 conv in float64 with every value that precedes a rounding: acc, t_scale = acc * oscale, t_bias, t_act (PReLU),
    v (+ residual), h = f16(v), z = (h - sub) * mul, code = e4m3(z); mag = oscale * sum |x||w| + |bias| + |residual| with the
    PReLU factor max(1, |slope|) on the first two."""
    B, H, _, _ = x.shape
    Cout = w.shape[0]
    acc, macc = conv_ref(x, w, None, 0, None, None, 1, 1)
    o = np.asarray(oscale, np.float64).reshape(1, 1, 1, Cout)
    b = class_bias(bias, bias_mode, H, Cout)[None]
    r = SimpleNamespace(acc=acc)
    r.t_scale = acc * o
    r.t_bias = r.t_scale + b
    mag = macc * np.abs(o) + np.abs(b)
    if slope is not None:
        s = np.asarray(slope, np.float64).reshape(1, 1, 1, Cout)
        r.t_act = np.where(r.t_bias > 0, r.t_bias, r.t_bias * s)
        mag = mag * np.maximum(1.0, np.abs(s))
        r.neg_slope = (r.t_bias < 0) & (s != 1.0)
    else:
        r.t_act = r.t_bias
        r.neg_slope = np.zeros(acc.shape, bool)
    r.v = r.t_act if residual is None else r.t_act + np.asarray(residual, np.float64)
    r.mag = mag if residual is None else mag + np.abs(residual)
    r.h = f16(r.v)
    r.sub = np.zeros(Cout) if sub is None else np.asarray(sub, np.float64)
    r.z = (r.h - r.sub.reshape(1, 1, 1, Cout)) * mul
    r.code = e4m3(r.z)
    return r


def assert_exact_f8(r, x, w, oscale, bias, slope, residual, check_code=True):
    """The conditions under which the kernel's result does not depend on its order of summation, on the reference `r`:
    per output channel all terms are multiples of 2^-q (q from the operands' own fractional bits) and mag * 2^q < 2^24;
    every value that precedes a rounding is an f32 number; nothing overflows f16; and no product falls below the window that
    the matrix instruction keeps beside the largest product of its group of 8 channels (`misaligned`)."""
    assert not misaligned(x, w), "a product below 2^-13 of its group's largest"
    Cout, K = w.shape
    Cin = x.shape[3]
    qx = frac_bits(x).reshape(-1, Cin).max(0)                                         # per input channel
    qw = np.where(w != 0, frac_bits(w) + np.tile(qx, K // Cin)[None], 0).max(1)      # per output channel: the finest product
    q = qw + frac_bits(oscale)
    if bias is not None:
        q = np.maximum(q, frac_bits(bias).reshape(-1, Cout).max(0))
    if slope is not None:
        q = q + frac_bits(slope)
    if residual is not None:
        q = np.maximum(q, frac_bits(residual).reshape(-1, Cout).max(0))
    magc = r.mag.reshape(-1, Cout).max(0)
    worst = (magc * np.ldexp(1.0, q)).max()
    assert worst < 2.0 ** 24, (worst, int(np.argmax(magc * np.ldexp(1.0, q))))
    for name in ("acc", "t_scale", "t_bias", "t_act", "v") + (("z",) if check_code else ()):
        assert is_f32(getattr(r, name)).all(), name
    assert np.isfinite(r.h).all() and np.abs(r.v).max() < 65504.0
    return float(worst)


EVENTS16 = ("f16_rounded", "f16_tie")
EVENTS8 = ("e4m3_rounded", "e4m3_tie", "sat_pos", "sat_neg", "zero_code", "subnormal_code")


def events(v, h, z=None, neg_slope=None):
    """boolean arrays, one per kind of rounding event"""
    ev = {"f16_rounded": (h != v) & ~f16_is_tie(v), "f16_tie": f16_is_tie(v)}
    if z is not None:
        c = e4m3(z)
        ev.update(e4m3_rounded=(c != z) & ~e4m3_is_tie(z) & (np.abs(z) <= E4M3_MAX), e4m3_tie=e4m3_is_tie(z) & (np.abs(z) < E4M3_MAX),
                  sat_pos=z > E4M3_MAX, sat_neg=z < -E4M3_MAX, zero_code=c == 0, subnormal_code=(c != 0) & (np.abs(c) < 2.0 ** -6))
    if neg_slope is not None:
        ev["neg_slope"] = neg_slope
    return ev


def wanted_events(want8, slope):
    return EVENTS16 + (EVENTS8 if want8 else ()) + (("neg_slope",) if slope else ())


# ---------------------------------------------------------------- planted elements
# Four output channels per conv are "planted": their weight row is a single 1 at the centre tap of an input channel that no
# other row reads, so the channel's output at a pixel is a function of that one input value (and the pixel's residual) alone and
# can be steered to each rounding event.  Their parameters span what the events need: a coarse scale for saturation, a fine one
# beside a large bias for f16 ties, a centre equal to the bias for zero and subnormal codes, a tiny scale.
PLANT = (dict(o=16.0, b=0.5, s=2.0, sub=0.25), dict(o=2.0 ** -4, b=8.0, s=0.25, sub=8.0),
         dict(o=1.0, b=0.125, s=-0.5, sub=0.125), dict(o=2.0 ** -6, b=2.0 ** -6, s=0.0, sub=0.0))


def plant_channels(C):
    return [3, 64 + 17, C - 2, C // 2 + 5]


def _plant_rows(w, Cin, cis, cos):
    w3 = w.reshape(w.shape[0], 9, Cin)
    w3[:, :, cis] = 0.0
    w3[cos] = 0.0
    for ci, co in zip(cis, cos):
        w3[co, 4, ci] = 1.0


def sparse_weights(rng, Cout, K, p):
    """P(w != 0) = p, magnitudes in {1/2, 1, 2}"""
    return rng.choice([-1.0, 1.0], (Cout, K)) * rng.choice([0.5, 1.0, 2.0], (Cout, K)) * (rng.random((Cout, K)) < p)


def _pixels(rng, masks):
    """per location, its pixels (b, y, x) in a random order"""
    out = {}
    for name, m in masks.items():
        idx = np.argwhere(m)
        out[name] = [tuple(i) for i in idx[rng.permutation(len(idx))]]
    return out


def exact_layer_operands(rng, B, H, Cin, Cout, bias_mode, slope, residual, want16, want8, sub):
    """Operands of fr_conv_nhwc_f8 on which its arithmetic is exact, with .ref (conv_f8_ref) and .want16_ / .want8_ (the outputs).
    bias_mode None = no bias; slope / residual / sub: present or not.  x multiples of 1/4 in [-2, 2], sparse weights in
    {+-1/2, +-1, +-2}, oscale in {2^-4, 1/2, 1, 2}, slopes in {1, 0, 1/2, 1/4, -1/2, -1, 2}, bias and residual multiples of 2^-7 (so that sums of a few
    tens carry more than f16's 11 bits), centre multiples of 2^-3, y8_mul a power of two; the planted channels as PLANT says."""
    o = SimpleNamespace(B=B, H=H, Cin=Cin, Cout=Cout, bias_mode=bias_mode, want16=want16, want8=want8)
    K = 9 * Cin
    o.x = rng.integers(-8, 9, (B, H, H, Cin)) / 4.0
    o.w = sparse_weights(rng, Cout, K, min(0.25, 900.0 / (K * 1.5 * 1.75)))
    o.oscale = rng.choice([2.0 ** -4, 0.5, 1.0, 2.0], Cout, p=[0.1, 0.3, 0.3, 0.3])
    nb = 9 * Cout if bias_mode == 1 else Cout
    o.bias = None if bias_mode is None else rng.integers(-1024, 1025, nb) / 128.0
    o.slope = rng.choice([1.0, 0.0, 0.5, 0.25, -0.5, -1.0, 2.0], Cout) if slope else None
    o.residual = rng.integers(-2048, 2049, (B, H, H, Cout)) / 128.0 if residual else None
    o.sub = rng.integers(-32, 33, Cout) / 8.0 if sub else None
    o.mul = float(rng.choice([0.5, 1.0, 2.0]))
    # ---- the planted channels
    cis, cos = plant_channels(Cin), plant_channels(Cout)
    _plant_rows(o.w, Cin, cis, cos)
    for k, (co, pl) in enumerate(zip(cos, PLANT)):
        o.oscale[co] = pl["o"]
        if o.bias is not None:
            o.bias.reshape(-1, Cout)[:, co] = pl["b"]
        if o.slope is not None:
            o.slope[co] = pl["s"]
        if o.sub is not None:
            o.sub[co] = pl["sub"]
    xs = e4m3_values()
    xs = xs[(xs != 0) | ~np.signbit(xs)]
    rs = np.arange(-128, 129) / 8.0 if residual else np.zeros(1)
    table = []
    for pl in PLANT:
        pre = xs[:, None] * pl["o"] + (pl["b"] if o.bias is not None else 0.0)
        act = np.where(pre > 0, pre, pre * pl["s"]) if slope else pre
        v = act + rs[None]
        h = f16(v)
        z = (h - (pl["sub"] if sub else 0.0)) * o.mul
        ok = is_f32(pre) & is_f32(act) & is_f32(v) & is_f32(z)
        ev = events(v, h, z, (pre < 0) & (pl["s"] != 1.0) & np.isfinite(v))
        table.append({name: np.argwhere(f & ok) for name, f in ev.items()})
    want = wanted_events(want8, slope)
    used = {loc: [0] * len(PLANT) for loc in ("last", "border", "inside")}
    pix = _pixels(rng, location_masks(B, H))
    for loc in used:
        for name in want:
            ks = [k for k in np.argsort(used[loc], kind="stable") if len(table[k][name])]
            assert ks, f"no planted channel reaches {name}"
            k = ks[0]
            i, j = table[k][name][rng.integers(len(table[k][name]))]
            b, y, xx = pix[loc][used[loc][k]]
            used[loc][k] += 1
            o.x[b, y, xx, cis[k]] = xs[i]
            if residual:
                o.residual[b, y, xx, cos[k]] = rs[j]
    # ---- the reference and its conditions
    o.ref = r = conv_f8_ref(o.x, o.w, o.oscale, o.bias, bias_mode, o.slope, o.residual, o.sub, o.mul)
    o.headroom = assert_exact_f8(r, o.x, o.w, o.oscale, o.bias, o.slope, o.residual, check_code=want8)
    ev = events(r.v, r.h, r.z if want8 else None, r.neg_slope if slope else None)
    o.coverage = {}
    for loc, m in location_masks(B, H).items():
        for name in want:
            n = int(ev[name][m].sum())
            assert n > 0, (loc, name)
            o.coverage[(loc, name)] = n
    o.want16_, o.want8_ = r.h.astype(np.float16), r.code
    return o


# B, H, Cin, Cout, bias_mode (None / 0 / 1), slope, residual, want16, want8, sub        (part A of tests/test_gpu_f8_pins.py)
EXACT_LAYER_CASES = [
    (1, 14, 128, 128, 1, True, False, False, True, True),       # one chunk; conv1 form: class bias + PReLU -> centred codes only
    (3, 14, 256, 256, 0, False, True, True, True, True),        # conv2 form: + residual, both outputs, y8_sub WITH a residual
    (2, 14, 384, 128, None, True, True, True, False, False),    # odd chunk count; no bias; y16 only
    (1, 14, 512, 256, 1, True, True, True, True, False),        # every epilogue operand; plain y8
    (2, 14, 256, 512, 0, True, False, True, True, True),        # four cout tiles
    (1, 28, 128, 128, None, False, True, False, True, False),   # four 7-row tiles; no bias, y8 only
    (3, 28, 128, 256, 1, True, True, True, True, True),         # every operand at 28x28, y8_sub with a residual
    (2, 28, 256, 128, 0, True, False, True, False, False),      # mode-0 bias, y16 only
]


# ---------------------------------------------------------------- float operands, interval criterion
def float_layer_operands(rng, B, H, Cin, Cout, bias_mode, slope, residual, want16, want8, sub=False):
    """Random e4m3 operands with an arbitrary f32 oscale (as test_conv_f8_layer_vs_torch draws them) and .want, .mag, .e.

    e = (9 Cin + 2) 2^-24 mag, mag = oscale sum |x||w| + |bias| + |residual| (PReLU factor max(1, |slope|) on the first two): the
    K = 9 Cin products of two e4m3 numbers are exact in f32, their sum in any order takes K - 1 additions (adding to the zero
    accumulator is exact), then the dequantising multiply, the bias and ONE of the PReLU multiply and the residual add - the forms
    measured here never have both - each rounding at most 2^-24 of a running magnitude <= mag: K - 1 + 3 = K + 2 (first order;
    the second-order term is 2e-4 of it at K = 4608)."""
    g = torch.Generator().manual_seed(int(rng.integers(1 << 31)))
    assert not (slope and residual)
    o = SimpleNamespace(B=B, H=H, Cin=Cin, Cout=Cout, bias_mode=bias_mode, want16=want16, want8=want8)
    K = 9 * Cin
    sx, o.mul = 0.037, 3.1
    f8 = lambda t: t.clamp(-448, 448).to(torch.float8_e4m3fn).float()                         # noqa: E731
    o.x = f8(torch.randn((B, H, H, Cin), generator=g) * 40).numpy().astype(np.float64)
    w = torch.randn((Cout, K), generator=g) * (2.0 / K) ** 0.5
    sw = w.abs().amax(1) / 448
    o.w = f8(w / sw[:, None]).numpy().astype(np.float64)
    o.oscale = (sw * sx).float().numpy().astype(np.float64)
    nb = 9 * Cout if bias_mode == 1 else Cout
    o.bias = None if bias_mode is None else torch.randn(nb, generator=g).numpy().astype(np.float64)
    o.slope = (torch.rand(Cout, generator=g) * 0.5).numpy().astype(np.float64) if slope else None
    o.residual = torch.randn((B, H, H, Cout), generator=g).to(torch.float16).numpy().astype(np.float64) if residual else None
    o.sub = (torch.randn(Cout, generator=g) * 0.5).numpy().astype(np.float64) if sub else None
    r = conv_f8_ref(o.x, o.w, o.oscale, o.bias, bias_mode, o.slope, o.residual, o.sub, o.mul)
    o.want, o.mag = r.v, r.mag
    o.e = (K + 2) * U32 * r.mag
    return o


def code_of_f16(h, sub, mul):
    """the kernel's f32 operations on an f16 value: e4m3(((float)h - sub) * mul), emulated in np.float32"""
    h32 = np.asarray(h, np.float32)
    s32 = np.zeros(h32.shape[-1], np.float32) if sub is None else np.asarray(sub, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return e4m3(((h32 - s32) * np.float32(mul)).astype(np.float64))


def interval_check(o, y16, y8):
    """The criterion of part B on EVERY element (RNE is monotone): y16 in [f16(want - e), f16(want + e)]; y8 = the code of the
    kernel's own y16 where y16 is produced, else a code between the codes of the interval's two ends.
    -> (passes, worst err / e or None; err = the distance from want to the nearest value that rounds to y16)."""
    lo, hi = f16(o.want - o.e), f16(o.want + o.e)
    ok, worst = True, None
    if o.want16:
        g = np.asarray(y16, np.float64)
        ok = ok and not np.isnan(g).any() and bool(((g >= lo) & (g <= hi)).all())
        g16 = np.asarray(y16, np.float16)
        nb = np.nextafter(g16, np.where(o.want > g, np.inf, -np.inf).astype(np.float16)).astype(np.float64)
        with np.errstate(invalid="ignore"):               # the least f32 error that explains y16: from want to the nearest value that rounds to it
            worst = float(np.nanmax(np.maximum(np.abs(g - o.want) - 0.5 * np.abs(nb - g), 0.0) / o.e))
    if o.want8:
        c = np.asarray(y8, np.float64)
        if o.want16:
            ok = ok and bool(np.array_equal(c, code_of_f16(np.asarray(y16, np.float16), o.sub, o.mul)))
        else:
            clo, chi = code_of_f16(lo.astype(np.float16), o.sub, o.mul), code_of_f16(hi.astype(np.float16), o.sub, o.mul)
            ok = ok and not np.isnan(c).any() and bool(((c >= clo) & (c <= chi)).all())
    return ok, worst


# the five shapes of tests/test_gpu_embed.py::test_conv_f8_layer_vs_torch + an odd chunk count           (part B)
FLOAT_LAYER_CASES = [
    (2, 14, 256, 256, 1, True, False, False, True),
    (2, 14, 256, 256, 0, False, True, True, True),
    (3, 28, 128, 128, 1, True, False, True, False),
    (1, 28, 128, 256, 0, False, True, True, True),
    (5, 14, 256, 512, 1, True, False, True, False),
    (2, 14, 384, 128, 1, True, False, True, True),
]


# ---------------------------------------------------------------- the stage kernel: a run of residual blocks
STAGE_ROWS = 14                                                        # oscale, 1 / oscale, 9 biases, slope, mu_next, 1 / sx_next
STAGE_CASES = [(nb, B) for nb in (1, 2, 3) for B in (1, 3)]           # nblocks, B                                (part C)


def _pow2_near(a):
    return float(np.ldexp(1.0, int(np.round(np.log2(a)))))


def exact_stage_run(rng, B, nblocks):
    """Operands of fr_conv_stage14_f8 (14x14x256, 2 * nblocks convs) on which the whole run is exact: .x16, .x8 =
    e4m3((x16 - mu_0) * inv_sx_0), per conv .w[j] (e4m3 values [256][2304]) and .prm[j] ([14][256], the rows as _pack_stage14_f8
    lays them out), .mu[j] / .inv_sx[j] (conv j's INPUT centre and scale), the references .conv[j] (conv_f8_ref) and .y[b] (f16
    output of block b).  Conv j + 1's centre and scale ride in conv j's rows; the last conv gets mu = 0, 1 / sx = 1.  Block b's
    residual is y[b - 1] (x16 for b = 0).  mu differs from channel to channel and conv to conv, 1 / sx from each conv to the next.
    Exactness and coverage are asserted per conv (the last conv's codes stay in the kernel: its e4m3 events are not asked for);
    the planted channels (PLANT) chain through the run, steered by their x16 values at pixels taken in turn from the last pixel
    tile, the border and the inside."""
    C, H, K = 256, 14, 2304
    nconv = 2 * nblocks
    P = plant_channels(C)
    o = SimpleNamespace(B=B, nblocks=nblocks, nconv=nconv, C=C)
    o.x16 = rng.integers(-8, 9, (B, H, H, C)) / 4.0
    o.prm = []
    for j in range(nconv):
        prm = np.zeros((STAGE_ROWS, C))
        prm[0] = rng.choice([2.0 ** -4, 0.5, 1.0, 2.0], C, p=[0.1, 0.3, 0.3, 0.3])
        prm[2:11] = rng.integers(-1024, 1025, (9, C)) / 128.0
        prm[11] = rng.choice([1.0, 0.0, 0.5, 0.25, -0.5, -1.0, 2.0], C) if j % 2 == 0 else 1.0
        for co, pl in zip(P, PLANT):
            prm[0, co], prm[2:11, co] = pl["o"], pl["b"]
            if j % 2 == 0:
                prm[11, co] = pl["s"]
        prm[1] = 1.0 / prm[0]
        o.prm.append(prm)
    o.mu = []
    for j in range(nconv):
        mu = rng.integers(-4, 5, C) / 4.0
        mu[P] = [pl["sub"] for pl in PLANT]
        o.mu.append(mu)
    o.inv_sx = [2.0]
    o.w = []

    def run(draw):
        """conv after conv; draw: choose the weights' density and the next conv's scale from the data (first pass)"""
        codes, resid, convs, ys = e4m3((o.x16 - o.mu[0]) * o.inv_sx[0]), o.x16, [], []
        for j in range(nconv):
            first, last = j % 2 == 0, j + 1 == nconv
            prm = o.prm[j]
            if draw:
                w = sparse_weights(rng, C, K, min(0.25, 100.0 / (K * max(np.abs(codes).mean(), 1e-3) * 1.17)))
                _plant_rows(w, C, P, P)
                for _ in range(8):                       # a weight whose product would fall out of the matrix instruction's window: zero
                    bad = misaligned(codes, w)
                    if not bad:
                        break
                    for c, cols in bad.items():
                        w[c, cols] = 0.0
                o.w.append(w)
            r = conv_f8_ref(codes, o.w[j], prm[0], prm[2:11].reshape(-1), 1, prm[11] if first else None, None if first else resid,
                            None, 1.0)
            if draw and not last:          # 1 / sx of the next conv: its codes some tens, and never its predecessor's scale
                s = max(_pow2_near(16.0 / max(np.sqrt(np.mean((r.h - o.mu[j + 1]) ** 2)), 1e-3)), 0.125)      # >= 1/8: the planted 7168 saturates
                o.inv_sx.append(s if s != o.inv_sx[-1] else 2 * s)
            mu_n, isx_n = (np.zeros(C), 1.0) if last else (o.mu[j + 1], o.inv_sx[j + 1])
            prm[12], prm[13, 0] = mu_n, isx_n
            r.sub, r.z = mu_n, (r.h - mu_n) * isx_n
            r.code = e4m3(r.z)
            r.x, r.resid = codes, None if first else resid
            convs.append(r)
            if not first:
                ys.append(r.h)
                resid = r.h
            codes = r.code
        return convs, ys

    run(True)
    # ---- planted chains: channel P[k]'s values through the run are a function of its own x16 value alone
    cand = np.unique(np.concatenate([np.arange(-2048, 2049) / 8.0, np.arange(-256, 257) / 64.0]))
    need = [(j, name) for j in range(nconv) for name in wanted_events(j + 1 < nconv, j % 2 == 0)]
    flags = []
    for k, pl in enumerate(PLANT):
        f, r = np.zeros((len(cand), len(need)), bool), cand
        ok = np.ones(len(cand), bool)
        code = e4m3((cand - o.mu[0][P[k]]) * o.inv_sx[0])
        for j in range(nconv):
            pre = code * pl["o"] + pl["b"]
            v = np.where(pre > 0, pre, pre * pl["s"]) if j % 2 == 0 else pre + r
            h = f16(v)
            last = j + 1 == nconv
            z = (h - (0.0 if last else o.mu[j + 1][P[k]])) * (1.0 if last else o.inv_sx[j + 1])
            qk = max(9 + int(frac_bits(pl["o"])) + int(frac_bits(pl["s"])), 7)           # as assert_exact_f8 will count it
            mag = (np.abs(code * pl["o"]) + pl["b"]) * max(1.0, abs(pl["s"])) + (0.0 if j % 2 == 0 else np.abs(r))
            ok &= is_f32(pre) & is_f32(v) & is_f32(z) & np.isfinite(h) & (mag * 2.0 ** qk < 2.0 ** 24) & (frac_bits(r) <= qk)
            ev = events(v, h, z, (pre < 0) & (pl["s"] != 1.0))
            for i, (jj, name) in enumerate(need):
                if jj == j:
                    f[:, i] = ev[name]
            if j % 2:
                r = h
            code = e4m3(z)
        flags.append(f & ok[:, None])
    pix = _pixels(rng, location_masks(B, H))
    order = [pix[loc][i] for i in range(4 * B) for loc in ("last", "border", "inside")]
    slot = [0] * len(PLANT)
    todo = np.ones(len(need), bool)
    while todo.any():
        gain = [(f[:, todo].sum(1).max(), k) for k, f in enumerate(flags) if slot[k] < len(order)]
        n, k = max(gain) if gain else (0, 0)
        if n == 0:                     # what no planted chain reaches is left to the draw; the assertions below decide
            break
        i = int(np.argmax(flags[k][:, todo].sum(1)))
        b, y, xx = order[slot[k]]
        slot[k] += 1
        o.x16[b, y, xx, P[k]] = cand[i]
        todo &= ~flags[k][i]
    # ---- the run proper, with its conditions
    o.conv, o.y = run(False)
    o.x8 = o.conv[0].x
    o.headroom, o.coverage = [], []
    for j, r in enumerate(o.conv):
        first, last = j % 2 == 0, j + 1 == nconv
        prm = o.prm[j]
        o.headroom.append(assert_exact_f8(r, r.x, o.w[j], prm[0], prm[2:11], prm[11] if first else None, r.resid, check_code=not last))
        ev = events(r.v, r.h, None if last else r.z, r.neg_slope if first else None)
        cov = {name: int(ev[name].sum()) for name in wanted_events(not last, first)}
        assert all(cov.values()), (j, cov)
        o.coverage.append(cov)
    assert len(set(zip(o.inv_sx, o.inv_sx[1:]))) and all(a != b for a, b in zip(o.inv_sx, o.inv_sx[1:]))
    return o


# ---------------------------------------------------------------- float32 emulation of the kernels, with planted faults
LAYER_FAULTS = ("drop_first", "drop_last", "bias_tile", "res_before_prelu", "y8_unrounded", "trunc", "nosat", "mu_prev_ch",
                "oscale_prev_ch", "slope_prev_ch")
STAGE_FAULTS = LAYER_FAULTS + ("mu_this", "isx_prev", "res_x16", "last_unwritten")


def _emulate_conv(x, w, oscale, bias, bias_mode, slope, residual, sub, mul, fault=None, cache=None):
    """One fp8 conv in float32 -> (h float16, codes float64).  Faults: "drop_first" / "drop_last": a tap x 128-channel step is
    skipped; "bias_tile": pixels 192 .. 195 of a 196-pixel tile take the bias class of the column to their left;
    "res_before_prelu"; "y8_unrounded": the codes come from the f32 value, not from its f16 rounding; "trunc": codes rounded
    towards zero; "nosat": no clamp, a NaN code beyond +-448; "mu_prev_ch" / "oscale_prev_ch" / "slope_prev_ch": channel c - 1's."""
    B, H, _, Cin = x.shape
    Cout, K = w.shape
    if cache is not None and fault not in ("drop_first", "drop_last") and "acc" in cache:
        acc = cache["acc"]
    else:
        p, w32 = patches(x, 3, 1, 1).astype(np.float32), w.astype(np.float32)
        if fault in ("drop_first", "drop_last"):
            s = 0 if fault == "drop_first" else K // STEP_K - 1
            keep = np.ones(K, bool)
            keep[s * STEP_K:(s + 1) * STEP_K] = False
            p, w32 = p[:, keep], w32[:, keep]
        acc = (p @ w32.T).reshape(B, H, H, Cout)
        if cache is not None and fault not in ("drop_first", "drop_last"):
            cache["acc"] = acc
    roll = lambda a, f: np.roll(a, 1) if fault == f else a                                    # noqa: E731
    v = acc * roll(np.asarray(oscale, np.float32), "oscale_prev_ch")
    if bias is not None:
        b = np.asarray(bias, np.float32)
        if bias_mode == 1:
            cc = np.broadcast_to(border_class(H)[None], (H, H)).copy()
            if fault == "bias_tile":
                px = np.arange(H * H).reshape(H, H)
                left = np.broadcast_to(border_class(H)[None], (H, H))[:, np.maximum(np.arange(H) - 1, 0)]
                cc = np.where(px % 196 >= 192, left, cc)
            b = b.reshape(3, 3, Cout)[border_class(H)[:, None], cc]
        v = v + b
    r32 = None if residual is None else np.asarray(residual, np.float32)
    if r32 is not None and fault == "res_before_prelu":
        v = v + r32
    if slope is not None:
        v = np.where(v > 0, v, v * roll(np.asarray(slope, np.float32), "slope_prev_ch")).astype(np.float32)
    if r32 is not None and fault != "res_before_prelu":
        v = v + r32
    h = v.astype(np.float16)
    s32 = np.zeros(Cout, np.float32) if sub is None else roll(np.asarray(sub, np.float32), "mu_prev_ch")
    z = (((v if fault == "y8_unrounded" else h.astype(np.float32)) - s32) * np.float32(mul)).astype(np.float64)
    c = e4m3_trunc(z) if fault == "trunc" else e4m3(z)
    if fault == "nosat":
        c = np.where(np.abs(z) > E4M3_MAX, np.nan, c)
    return h, c


def emulate_layer(o, fault=None):
    """fr_conv_nhwc_f8 on the operands `o` in float32 -> (y16 float16 or None, y8 values or None)"""
    if not hasattr(o, "_cache"):
        o._cache = {}
    h, c = _emulate_conv(o.x, o.w, o.oscale, o.bias, o.bias_mode, o.slope, o.residual, o.sub, o.mul, fault, o._cache)
    return (h if o.want16 else None), (c if o.want8 else None)


def layer_is_exact(o, y16, y8):
    ok = True
    if o.want16:
        ok = ok and np.array_equal(np.asarray(y16, np.float16), o.want16_)
    if o.want8:
        ok = ok and np.array_equal(np.asarray(y8, np.float64), o.want8_)
    return ok


def emulate_stage(run, fault=None):
    """fr_conv_stage14_f8 in float32 from the parameter rows, as the kernel reads them -> y16 (float16).  Faults: _emulate_conv's
    in every conv, and "mu_this": the codes are centred with this conv's own input centre, not the next conv's; "isx_prev": scaled
    with the 1 / sx that the previous conv's rows carry; "res_x16": every block's residual is x16; "last_unwritten": the last
    block's output of the last image is not stored (y16 keeps the block before, or its fill)."""
    codes, resid, y = run.x8, run.x16, None
    if not hasattr(run, "_cache"):
        run._cache = [dict() for _ in range(run.nconv)]
    for j in range(run.nconv):
        first = j % 2 == 0
        prm = run.prm[j]
        sub, mul = prm[12], prm[13, 0]
        if fault == "mu_this":
            sub = run.mu[j]
        if fault == "isx_prev":
            mul = run.inv_sx[j]
        cache = run._cache[j] if j == 0 else None                   # later convs' inputs depend on the fault
        h, c = _emulate_conv(codes, run.w[j], prm[0], prm[2:11].reshape(-1), 1, prm[11] if first else None,
                             None if first else resid, sub, mul, fault, cache)
        if not first:
            prev, y = y, h
            resid = run.x16 if fault == "res_x16" else h.astype(np.float64)
        codes = c
    if fault == "last_unwritten":
        y = y.copy()
        y[-1] = np.nan if prev is None else prev[-1]
    return y
