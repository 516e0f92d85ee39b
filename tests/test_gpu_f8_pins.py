"""GPU pins of the fp8 (e4m3) conv path of the embed net against tests/helpers/f8_ref.py - per element, nothing left out.

A. fr_conv_nhwc_f8 on exact operands (e4m3 inputs and weights, power-of-two scales and slopes, bias / centre / residual multiples
   of a power of two): every value before a rounding is known exactly, so y16 and the y8 codes are compared with the reference
   bit for bit although the roundings (f16 and e4m3, ties, subnormals, saturation) all occur - the helper asserts both, on border
   pixels, in the last pixel tile and inside.  One to four chunks of 128 input channels, one to four cout tiles, 14x14 and 28x28,
   bias NULL / plain / nine border classes, slope, residual, y8_sub, y16 / y8 / both.
B. The same entry on random operands with an arbitrary f32 oscale: y16 inside [f16(want - e), f16(want + e)], e = (9 Cin + 2)
   2^-24 mag; y8 = the code of the kernel's own y16 (or, without y16, between the codes of the interval's ends).
C. fr_conv_stage14_f8 over 1, 2 and 3 blocks, 1 and 3 faces, exact: the residual read back through HBM and scaled by 1 / oscale,
   the hand-over of mu / 1/sx from one conv's rows to the next, the last conv; weights through fr_conv_stage14_f8_pack; one block
   also through two fr_conv_nhwc_f8 calls, same bits.
D. The stage kernel's residual path with an oscale that is no power of two (conv2's weights all zero).
E. The two quantisers on every finite f16 value and +-inf, and the centred form across the wrap of its grid-stride loop.

Outputs are pre-filled (NaN, 0x7f bytes = the e4m3 NaN code) and carry one guard image beyond B that must stay untouched."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.helpers import f8_ref as fr

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _ids(c):
    return "-".join(str(v) for v in c)


def _f(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _codes(values):
    return fr.e4m3_bytes(values).cuda()


def _guarded(B, shape, dtype):
    """an output for B images with one guard image behind it, pre-filled"""
    if dtype == torch.float16:
        return torch.full((B + 1,) + shape, NAN, dtype=dtype, device="cuda")
    return torch.full((B + 1,) + shape, 0x7f, dtype=torch.uint8, device="cuda")


def _take(t, B):
    """the B images of a guarded output on the host, after checking the guard"""
    torch.cuda.synchronize()
    g = t[B:].cpu()
    assert bool(torch.isnan(g).all()) if t.dtype == torch.float16 else bool((g == 0x7f).all()), "the guard image was written"
    return t[:B].cpu()


def _run_layer(lib, x8, w8, oscale, bias, bias_mode, slope, residual, sub, mul, B, H, Cin, Cout, want16, want8):
    """fr_conv_nhwc_f8 -> (y16 float16 numpy or None, y8 values float64 or None); x8 / w8 / residual are device tensors"""
    from facerecognition_infrenceengine_amd import _lib
    od, bd, sd, ud = _f(oscale), _f(bias), _f(slope), _f(sub)
    y16 = _guarded(B, (H, H, Cout), torch.float16) if want16 else None
    y8 = _guarded(B, (H, H, Cout), torch.uint8) if want8 else None
    a = _lib.ConvF8Args(_lib.ptr(x8), _lib.ptr(w8), _lib.ptr(y16), _lib.ptr(y8), _lib.ptr(od), _lib.ptr(bd), _lib.ptr(sd),
                        _lib.ptr(residual), B, H, H, Cin, Cout, 1 if bias_mode == 1 else 0, float(mul), _lib.ptr(ud))
    assert lib.fr_conv_nhwc_f8(ctypes.byref(a), _lib.stream_ptr()) == 0
    return (_take(y16, B).numpy() if want16 else None), (fr.bytes_values(_take(y8, B)) if want8 else None)


def _run_operands(lib, o):
    return _run_layer(lib, _codes(o.x), _codes(o.w), o.oscale, o.bias, o.bias_mode, o.slope, _f(o.residual, torch.float16), o.sub,
                      o.mul, o.B, o.H, o.Cin, o.Cout, o.want16, o.want8)


# ---------------------------------------------------------------- A. the layer kernel, exact
@pytest.mark.parametrize("case", fr.EXACT_LAYER_CASES, ids=_ids)
def test_conv_f8_layer_exact(lib, case):
    o = fr.exact_layer_operands(np.random.default_rng(fr.seed_of(case)), *case)
    y16, y8 = _run_operands(lib, o)
    if o.want16:
        assert torch.equal(torch.from_numpy(y16), torch.from_numpy(o.want16_))
    if o.want8:
        assert torch.equal(torch.from_numpy(y8), torch.from_numpy(o.want8_))


# ---------------------------------------------------------------- B. the layer kernel, float operands
@pytest.mark.parametrize("case", fr.FLOAT_LAYER_CASES, ids=_ids)
def test_conv_f8_layer_interval(lib, case):
    o = fr.float_layer_operands(np.random.default_rng(fr.seed_of(case)), *case)
    y16, y8 = _run_operands(lib, o)
    ok, worst = fr.interval_check(o, y16, y8)
    print(f"\nfr_conv_nhwc_f8 {case}: worst err / e {worst}")
    assert ok


# ---------------------------------------------------------------- C. the stage kernel, exact
@functools.lru_cache(maxsize=None)
def _stage_run(case):
    return fr.exact_stage_run(np.random.default_rng(fr.seed_of(case)), case[1], case[0])


def _pack_stream(lib, ws):
    """the convs' e4m3 values [256][2304] -> the stage kernel's weight stream"""
    from facerecognition_infrenceengine_amd import _lib
    per = lib.fr_conv_stage14_f8_weight_bytes(1)
    assert per == 18 * 32768 and lib.fr_conv_stage14_f8_param_floats() == fr.STAGE_ROWS * 256
    stream = torch.full((len(ws) * per,), 0x7f, dtype=torch.uint8, device="cuda")
    for j, w in enumerate(ws):
        wd = _codes(w)
        assert lib.fr_conv_stage14_f8_pack(_lib.ptr(wd), _lib.ptr(stream[j * per:]), _lib.stream_ptr()) == 0
        torch.cuda.synchronize()
    return stream


def _run_stage(lib, x8d, x16d, stream, prm, B, nblocks):
    from facerecognition_infrenceengine_amd import _lib
    pd = _f(np.stack(prm))
    y = _guarded(B, (14, 14, 256), torch.float16)
    assert lib.fr_conv_stage14_f8(_lib.ptr(x8d), _lib.ptr(x16d), _lib.ptr(y), _lib.ptr(stream), _lib.ptr(pd), B, nblocks, _lib.stream_ptr()) == 0
    return _take(y, B)


@pytest.mark.parametrize("case", fr.STAGE_CASES, ids=_ids)
def test_conv_stage14_f8_exact(lib, case):
    nblocks, B = case
    run = _stage_run(case)
    x8d, x16d = _codes(run.x8), _f(run.x16, torch.float16)
    stream = _pack_stream(lib, run.w)
    y = _run_stage(lib, x8d, x16d, stream, run.prm, B, nblocks)
    assert torch.equal(y, torch.from_numpy(run.y[-1]).to(torch.float16))
    if nblocks == 1:                 # the same operands through the per-layer kernel: conv1 -> centred codes, conv2 + x16 -> f16
        p1, p2 = run.prm
        _, mid = _run_layer(lib, x8d, _codes(run.w[0]), p1[0], p1[2:11], 1, p1[11], None, p1[12], p1[13, 0], B, 14, 256, 256, False, True)
        assert torch.equal(torch.from_numpy(mid), torch.from_numpy(run.conv[0].code))
        y2, _ = _run_layer(lib, _codes(mid), _codes(run.w[1]), p2[0], p2[2:11], 1, None, x16d, None, 1.0, B, 14, 256, 256, True, False)
        assert torch.equal(torch.from_numpy(y2), y)


# ---------------------------------------------------------------- D. the stage kernel's residual path, general oscale
def test_conv_stage14_f8_residual_with_a_general_oscale(lib):
    """conv2's weights all zero codes (conv1's arbitrary), random f32 oscale: block 1 is y = f16(b2 + r (1 / o) o) with r = x16;
    the residual's product with the rounded reciprocal, the dequantising multiply and the bias add round once each and 1 / o is
    itself rounded: within 4 2^-24 (|r| + |b2|) before the f16 rounding (the zero products add nothing).  Block 2 does the same to
    block 1's ROUNDED output, read back through HBM: its interval starts from the ends of block 1's."""
    B, C, u4 = 2, 256, 4 * fr.U32
    rng = np.random.default_rng(41)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)                   # noqa: E731
    x16 = fr.f16(rng.standard_normal((B, 14, 14, C)) * 3)
    grid = fr.e4m3_values()
    grid = grid[np.abs(grid) <= 2]                                                   # conv1's map stays far inside f16
    prm, ws = [], []
    for j in range(4):
        p = np.zeros((fr.STAGE_ROWS, C))
        p[0] = f32(rng.uniform(0.01, 0.1, C))
        p[1] = f32(1.0 / p[0])
        p[2:11] = f32(rng.standard_normal((9, C)))
        p[11] = f32(rng.uniform(0, 0.5, C)) if j % 2 == 0 else 1.0
        p[12], p[13, 0] = (f32(rng.standard_normal(C)), 0.7) if j < 3 else (0.0, 1.0)
        p[13, 0] = f32(p[13, 0])
        prm.append(p)
        ws.append(rng.choice(grid, (C, 2304)) if j % 2 == 0 else np.zeros((C, 2304)))
    x8 = fr.e4m3((x16 - f32(rng.standard_normal(C))) * 0.7)
    x8d, x16d = _codes(x8), _f(x16, torch.float16)
    stream = _pack_stream(lib, ws)

    def ends(lo, hi, b9):
        b = fr.class_bias(b9.reshape(-1), 1, 14, C)[None]
        return fr.f16(lo + b - u4 * (np.abs(lo) + np.abs(b))), fr.f16(hi + b + u4 * (np.abs(hi) + np.abs(b)))
    lo1, hi1 = ends(x16, x16, prm[1][2:11])
    y1 = _run_stage(lib, x8d, x16d, stream, prm[:2], B, 1).numpy().astype(np.float64)
    assert ((y1 >= lo1) & (y1 <= hi1)).all()
    lo2, hi2 = ends(lo1, hi1, prm[3][2:11])
    y2 = _run_stage(lib, x8d, x16d, stream, prm, B, 2).numpy().astype(np.float64)
    assert ((y2 >= lo2) & (y2 <= hi2)).all()
    def least(y, t, e):                 # the least f32 error that explains y, over e (as f8_ref.interval_check reports it)
        h = y.astype(np.float16)
        nb = np.nextafter(h, np.where(t > y, np.inf, -np.inf).astype(np.float16)).astype(np.float64)
        return float((np.maximum(np.abs(y - t) - 0.5 * np.abs(nb - y), 0.0) / e).max())
    b = fr.class_bias(prm[1][2:11].reshape(-1), 1, 14, C)[None]
    t, e = x16 + b, u4 * (np.abs(x16) + np.abs(b))
    emu = ((x16.astype(np.float32) * prm[1][1].astype(np.float32)) * prm[1][0].astype(np.float32) + b.astype(np.float32)).astype(np.float16)
    print(f"\nfr_conv_stage14_f8 residual path, block 1: worst err / bound {least(y1, t, e):.4f} (float32 emulation {least(emu.astype(np.float64), t, e):.4f}); "
          f"interval ends differ in {float((lo1 != hi1).mean()):.4f} (block 1) / {float((lo2 != hi2).mean()):.4f} (block 2) of the elements")


# ---------------------------------------------------------------- E. the quantisers
def _all_f16():
    """every finite f16 value and +-inf, padded with zeros to a multiple of 8"""
    bits = np.arange(1 << 16, dtype=np.uint16)
    v = bits.view(np.float16)
    v = v[~np.isnan(v)]
    assert len(v) == 63490
    return np.concatenate([v, np.zeros(-len(v) % 8, np.float16)])


@pytest.mark.parametrize("mul", [1.0, 2.0 ** -3])
def test_quantisers_on_every_f16_value(lib, mul):
    from facerecognition_infrenceengine_amd import _lib
    v = _all_f16()
    n = len(v)
    xd = torch.from_numpy(v).cuda()
    out = torch.full((n + 64,), 0x7f, dtype=torch.uint8, device="cuda")
    assert lib.fr_quantize_f16_f8(_lib.ptr(xd), _lib.ptr(out), n, mul, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((out[n:] == 0x7f).all())
    assert np.array_equal(fr.bytes_values(out[:n].cpu()), fr.e4m3(v.astype(np.float64) * mul))
    # centred, C = 8, power-of-two centres: ((float)h - sub) * mul in f32, as the kernel computes it
    sub = np.array([1.0, -2.0, 0.5, 4.0, -0.25, 8.0, -16.0, 2.0 ** -6])
    sd = _f(sub)
    out.fill_(0x7f)
    assert lib.fr_quantize_f16_f8_centred(_lib.ptr(xd), _lib.ptr(out), n, 8, _lib.ptr(sd), mul, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((out[n:] == 0x7f).all())
    assert np.array_equal(fr.bytes_values(out[:n].cpu()), fr.code_of_f16(v.reshape(-1, 8), sub, mul).reshape(-1))


def test_quantiser_centred_across_the_grid_stride_wrap(lib):
    """n / 8 = 16384 * 256 + 128 items on a grid capped at 16384 x 256 threads: the first 128 threads take a second item, whose
    channel group is (i % C8) of the item, not of the thread."""
    from facerecognition_infrenceengine_amd import _lib
    C = 128
    n = 16384 * 256 * 8 + 8 * C
    g = torch.Generator().manual_seed(6)
    x = torch.randn(n // 64, generator=g).repeat(64)                      # 64 different phases against the channel period
    x = (x * torch.linspace(1, 60, n)).to(torch.float16)
    mu = torch.randn(C, generator=g) * 10
    xd, md = x.cuda(), mu.cuda()
    out = torch.full((n + 64,), 0x7f, dtype=torch.uint8, device="cuda")
    assert lib.fr_quantize_f16_f8_centred(_lib.ptr(xd), _lib.ptr(out), n, C, _lib.ptr(md), 0.7, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((out[n:] == 0x7f).all())
    want = ((x.float().reshape(-1, C) - mu[None]) * 0.7).clamp(-448, 448).to(torch.float8_e4m3fn).reshape(-1)
    assert torch.equal(out[:n].cpu().view(torch.float8_e4m3fn).float(), want.float())
