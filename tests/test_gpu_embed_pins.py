"""GPU pins of the embed net's conv kernels against the float64 references of tests/helpers/embed_ref.py.

A. Exact-integer operands, torch.equal against the reference cast to the output type (independent of K and of summation order;
   that the operands make the arithmetic exact is asserted on the reference by the helper).  Outputs are pre-filled with NaN
   wherever the entry does not alias them.  Kernel forms reached:
     fr_conv_nhwc_f16   conv_mfma_kernel<2, false> (128-cout tile): 3x3 / s2 at 13x13, 1x1 / s2 at 13x13, a 128-pixel tile across
                        three images with M = 135; <1, false> (64-cout tile): 1x1 / s2, 3x3 / s1 at 9x5 with border-class bias +
                        PReLU + residual, 14x14 with Cout = 64, M = 315 of 2 x 256; both with the second input (x2) at odd and
                        even H; <1, true> and <2, true> (packed stem declined by conv_stem: W = 24, H = 6, no slope + residual,
                        Cout = 128); conv_stem_kernel (H % 4 == 0, W % 16 == 0); conv_halo_kernel lean 7x7 (4 + 1 images), 14x14,
                        28x28, and the single-chunk 56x56 and 112x112 variants
     fr_conv_inblock_f16  one-, two- and four-tile forms, the ring wrap at Cin = 512, 2x2 (all corners), a tile across images
     fr_conv_walk64_f16   c1 / c2 forms, cout 64 / 128, HW 28 / 56 / 84, walks cut in 2 and 4 pieces and uncut (B = 130)
     fr_conv_stage14_f16, fr_conv_stage28_f16   one block, B = 1 and 3 (the intermediate map is an f16 integer too)
B. The split-K partials mode of fr_conv_nhwc_f16, every slice against float64 within (K_slice + 2) 2^-24 mag_slice, empty slices
   exact zeros, and the same cases on integer operands exactly: the engine's slice counts, a ragged and an empty last slice, the
   x2 form with a slice across nk_main, the FC at its real shape (one and two pixel tiles) and a short FC with 13 empty slices.
C. fr_conv_splitk_epilogue alone from random f32 partials (float64 bound) and integer partials (exact); fr_conv_sequence kind 1.
D. fr_fc_reduce_l2norm: eight-at-a-time slice loop and its tail, the keep[] registers and the read-back path, partial workgroups.

Every float64 test prints its worst err / bound; docs/KERNEL_NOTES.md records them."""
import ctypes

import numpy as np
import pytest
import torch

from tests.helpers import embed_ref as er

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _dev(a, dtype=torch.float16):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _ids(c):
    return "-".join(str(v) for v in c)


def _conv_args(_lib, o, xd, wd, yd, bd, sd, rd, part=None, splitk=1, x2d=None):
    return _lib.ConvArgs(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(yd), _lib.ptr(bd), _lib.ptr(sd), _lib.ptr(rd), _lib.ptr(part),
                         o.B, o.H, o.W, o.Cin, o.Cout, o.k, o.k, o.stride, o.pad, o.Ho, o.Wo, o.bias_mode, splitk, _lib.ptr(x2d), o.C2)


def _run_exact_conv(lib, entry, o, stem=False):
    from facerecognition_infrenceengine_amd import _lib
    w = o.w
    if stem:                                              # [Cout][16 taps][8]: taps 9 .. 15 are zero
        w = np.zeros((o.Cout, 16, 8))
        w[:, :9] = o.w.reshape(o.Cout, 9, 8)
        w = w.reshape(o.Cout, 128)
    xd, wd, x2d = _dev(o.x), _dev(w), _dev(o.x2)
    bd, sd, rd = _dev(o.bias, torch.float32), _dev(o.slope, torch.float32), _dev(o.residual)
    y = torch.full((o.B, o.Ho, o.Wo, o.Cout), NAN, dtype=torch.float16, device="cuda")
    a = _conv_args(_lib, o, xd, wd, y, bd, sd, rd, x2d=x2d)
    getattr(lib, entry)(ctypes.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), torch.from_numpy(o.want).to(torch.float16))


# ---------------------------------------------------------------- A. exact-integer pins
NHWC_CASES = [
    # B, H, W, Cin, Cout, k, stride, pad, bias_mode, bias, slope, residual, C2
    (2, 13, 13, 128, 128, 3, 2, 1, 0, True, False, True, 0),     # generic, 128-cout tile: 3x3 / s2, odd image
    (2, 13, 13, 64, 128, 1, 2, 0, 0, False, False, False, 0),    # generic: 1x1 / s2 shortcut, no epilogue operand at all
    (1, 13, 13, 64, 64, 1, 2, 0, 0, True, True, False, 0),       # generic, 64-cout tile: 1x1 / s2
    (1, 9, 5, 64, 64, 3, 1, 1, 1, True, True, True, 0),          # generic: non-square (the halo kernel declines), full epilogue
    (2, 14, 14, 128, 64, 3, 1, 1, 1, True, True, False, 0),      # 14x14 with Cout = 64: the halo kernel declines
    (3, 9, 5, 128, 128, 3, 1, 1, 1, True, True, True, 0),        # M = 135: a 128-pixel tile across three images + 7 pixels
    (7, 9, 5, 64, 64, 3, 1, 1, 1, True, True, True, 0),          # M = 315: 256-pixel tiles across images, 59-pixel tail
    (5, 7, 7, 128, 128, 3, 1, 1, 1, True, True, True, 0),        # halo, lean 7x7: 4 + 1 images
    (1, 14, 14, 128, 128, 3, 1, 1, 1, True, True, True, 0),      # halo, lean 14x14, two chunks
    (1, 28, 28, 128, 128, 3, 1, 1, 1, True, True, True, 0),      # halo, lean 28x28
    (1, 56, 56, 64, 128, 3, 1, 1, 1, True, True, True, 0),       # halo, single-chunk 56x56, two cout tiles
    (1, 112, 112, 64, 64, 3, 1, 1, 1, True, True, True, 0),      # halo, 112x112
    (2, 13, 13, 64, 128, 3, 2, 1, 0, True, False, False, 64),    # x2 form, odd H: the 1x1 tap's last position is the last pixel
    (1, 14, 14, 128, 128, 3, 2, 1, 0, True, False, False, 64),   # x2 form, even H
    (1, 13, 13, 64, 64, 3, 2, 1, 0, True, False, False, 64),     # x2 form, 64-cout tile
]


@pytest.mark.parametrize("case", NHWC_CASES, ids=_ids)
def test_conv_nhwc_exact(lib, case):
    B, H, W, Cin, Cout, k, stride, pad, bias_mode, bias, slope, residual, C2 = case
    o = er.int_operands(np.random.default_rng(er.case_seed(case)), B, H, W, Cin, Cout, k, stride, pad, bias_mode, bias, slope, residual, C2)
    _run_exact_conv(lib, "fr_conv_nhwc_f16", o)


STEM_CASES = [
    # B, H, W, Cout, slope, residual                      fr_conv_stem_try takes: Cout 64, bias + slope, no residual, W % 16 == 0, H % 4 == 0
    (2, 8, 16, 64, True, False),           # conv_stem_kernel
    (1, 20, 48, 64, True, False),          # conv_stem_kernel, three column groups
    (2, 6, 24, 64, True, False),           # W % 16 != 0 and H % 4 != 0: conv_mfma_kernel<1, true>
    (1, 8, 16, 128, True, False),          # Cout = 128: conv_mfma_kernel<2, true>
    (2, 8, 16, 64, False, True),           # no slope, a residual: conv_mfma_kernel<1, true>
]


@pytest.mark.parametrize("case", STEM_CASES, ids=_ids)
def test_conv_packed_stem_exact(lib, case):
    B, H, W, Cout, slope, residual = case
    o = er.int_operands(np.random.default_rng(er.case_seed(case)), B, H, W, 8, Cout, 3, 1, 1, 0, True, slope, residual, stem=True)
    _run_exact_conv(lib, "fr_conv_nhwc_f16", o, stem=True)


INBLOCK_CASES = [
    # B, H, W, Cin, Cout, bias_mode, slope, residual       (pixel tiles of 16) x (Cout / 32) workgroups: <= 256 one tile, else two, else four
    (1, 14, 14, 256, 256, 1, True, True),      # one-tile form, 13 x 8 workgroups, 72 K steps: waves with 5 and with 4
    (4, 14, 14, 256, 256, 1, True, True),      # two-tile form (392 -> 25 x 8)
    (8, 14, 14, 256, 256, 0, False, True),     # four-tile form (784 -> 392 -> 25 x 8)
    (1, 7, 7, 512, 512, 1, True, True),        # 144 K steps: the ring of five wraps; 49 pixels = 3 tiles + 1
    (9, 7, 7, 512, 512, 1, True, False),       # four-tile form through a ring of two
    (1, 2, 2, 128, 32, 1, True, False),        # every pixel a corner
    (3, 5, 9, 160, 96, 1, True, True),         # 45 K steps, three cout tiles, a tile across two images
]


@pytest.mark.parametrize("case", INBLOCK_CASES, ids=_ids)
def test_conv_inblock_exact(lib, case):
    B, H, W, Cin, Cout, bias_mode, slope, residual = case
    o = er.int_operands(np.random.default_rng(er.case_seed(case)), B, H, W, Cin, Cout, 3, 1, 1, bias_mode, True, slope, residual)
    _run_exact_conv(lib, "fr_conv_inblock_f16", o)


WALK64_CASES = [
    # B, HW, cout, form         pieces: doubled while B * cout / 64 * pieces * 2 <= 256 and a piece keeps >= 2 of the (HW/28) * (HW/14) regions
    (1, 28, 64, "c2"),          # 2 regions: uncut
    (130, 28, 64, "c1"),        # 130 faces: uncut by the workgroup count
    (1, 56, 64, "c1"),          # 8 regions in 4 pieces
    (1, 56, 128, "c2"),         # two cout groups, 4 pieces
    (1, 84, 64, "c2"),          # 18 regions in 2 pieces
    (1, 84, 128, "c1"),
]


@pytest.mark.parametrize("case", WALK64_CASES, ids=_ids)
def test_conv_walk64_exact(lib, case):
    from facerecognition_infrenceengine_amd import _lib
    B, HW, cout, form = case
    c1 = form == "c1"
    o = er.int_operands(np.random.default_rng(er.case_seed(case[:3]) + c1), B, HW, HW, 64, cout, 3, 1, 1, int(c1), True, c1, not c1)
    xd, wd = _dev(o.x), _dev(o.w)
    bd, sd = _dev(o.bias, torch.float32), _dev(o.slope, torch.float32)
    ws = torch.empty(lib.fr_conv_walk64_weight_bytes(cout) // 2, dtype=torch.float16, device="cuda")
    lib.fr_conv_walk64_pack(_lib.ptr(wd), _lib.ptr(ws), cout, _lib.stream_ptr())
    # the c2 form adds the residual in place (it aliases y, as in the engine); the c1 form writes a NaN-filled y
    y = torch.full((B, HW, HW, cout), NAN, dtype=torch.float16, device="cuda") if c1 else _dev(o.residual)
    lib.fr_conv_walk64_f16(_lib.ptr(xd), _lib.ptr(ws), _lib.ptr(y), _lib.ptr(bd), int(c1), _lib.ptr(sd), None if c1 else _lib.ptr(y),
                           B, HW, cout, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), torch.from_numpy(o.want).to(torch.float16))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("HW", [14, 28])
def test_conv_stage_block_exact(lib, HW, B):
    """fr_conv_stage14_f16 (x -> y) and fr_conv_stage28_f16 (in place, NaN-filled scratch): one block."""
    from facerecognition_infrenceengine_amd import _lib
    C = 256 if HW == 14 else 128
    name = f"fr_conv_stage{HW}"
    o = er.int_stage_block(np.random.default_rng(HW * 10 + B), B, HW, C)
    per = getattr(lib, name + "_weight_bytes")(1) // 2
    stream = torch.empty(2 * per, dtype=torch.float16, device="cuda")
    w1d, w2d = _dev(o.w1), _dev(o.w2)
    for j, wd in enumerate((w1d, w2d)):
        getattr(lib, name + "_pack")(_lib.ptr(wd), _lib.ptr(stream[j * per:]), _lib.stream_ptr())
    prm = np.empty((2, 10, C))
    prm[0, :9], prm[0, 9] = o.b9.reshape(9, C), o.slope
    prm[1, :9], prm[1, 9] = o.b2[None], 1.0
    pd, xd = _dev(prm, torch.float32), _dev(o.x)
    other = torch.full_like(xd, NAN)
    if HW == 14:
        lib.fr_conv_stage14_f16(_lib.ptr(xd), _lib.ptr(other), _lib.ptr(stream), _lib.ptr(pd), B, 1, _lib.stream_ptr())
        y = other
    else:
        lib.fr_conv_stage28_f16(_lib.ptr(xd), _lib.ptr(other), _lib.ptr(stream), _lib.ptr(pd), B, 1, _lib.stream_ptr())
        y = xd
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), torch.from_numpy(o.want).to(torch.float16))


# ---------------------------------------------------------------- B. split-K partials, per slice
@pytest.mark.parametrize("kind", ["float", "int"])
@pytest.mark.parametrize("case", er.PARTIAL_CASES, ids=_ids)
def test_conv_splitk_partials_per_slice(lib, case, kind):
    from facerecognition_infrenceengine_amd import _lib
    splitk = case[8]
    o = er.partial_operands(case, kind)
    refs = er.partial_refs(o, splitk, kind)
    M = o.B * o.Ho * o.Wo
    xd, wd, x2d = _dev(o.x), _dev(o.w), _dev(o.x2)
    part = torch.full((splitk, M, o.Cout), NAN, dtype=torch.float32, device="cuda")
    a = _conv_args(_lib, o, xd, wd, None, None, None, None, part=part, splitk=splitk, x2d=x2d)
    lib.fr_conv_nhwc_f16(ctypes.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    got = part.cpu().numpy().astype(np.float64)
    worst = 0.0
    for z, (want, mag, ksl) in enumerate(refs):
        if kind == "int" or ksl == 0:
            assert np.array_equal(got[z], want), z                    # empty slice: exact zeros
            continue
        err, bound = np.abs(got[z] - want), (ksl + 2) * er.U32 * mag
        worst = max(worst, er.worst_ratio(err, bound))
    if kind == "float":
        print(f"\nfr_conv_nhwc_f16 partials {case}: worst err / bound {worst:.4f}")
    assert worst <= 1.0


# ---------------------------------------------------------------- C. the split-K epilogue alone
def _run_epilogue(lib, o):
    from facerecognition_infrenceengine_amd import _lib
    pd = _dev(o.partial, torch.float32)
    bd, sd, rd = _dev(o.bias, torch.float32), _dev(o.slope, torch.float32), _dev(o.residual)
    y = torch.full((o.M, o.Cout), NAN, dtype=torch.float16, device="cuda")
    lib.fr_conv_splitk_epilogue(_lib.ptr(pd), o.splitk, o.M, o.Cout, o.Ho, o.Wo, _lib.ptr(bd), o.bias_mode, _lib.ptr(sd), _lib.ptr(rd),
                                _lib.ptr(y), _lib.stream_ptr())
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("Cout", er.EPILOGUE_COUT)
@pytest.mark.parametrize("splitk", er.EPILOGUE_SPLITK)
def test_splitk_epilogue_alone(lib, splitk, Cout):
    """Every (bias NULL / mode 0 / mode 1) x (slope) x (residual) form at B = 3, 5 x 9 pixels: float partials within
    (splitk + 3) 2^-24 mag + 2^-11 |want| + 2^-25, integer partials exactly."""
    rng = np.random.default_rng(splitk * 100 + Cout)
    worst = 0.0
    for bias_mode, slope, res in er.EPILOGUE_FORMS:
        o = er.epilogue_operands(rng, splitk, Cout, bias_mode, slope, res, "float")
        got = _run_epilogue(lib, o).numpy().astype(np.float64)
        r = er.worst_ratio(np.abs(got - o.want), er.epilogue_bound(splitk, o.mag, o.want))
        worst = max(worst, r)
        assert r <= 1.0, (bias_mode, slope, res, r)
        o = er.epilogue_operands(rng, splitk, Cout, bias_mode, slope, res, "int")
        assert torch.equal(_run_epilogue(lib, o), torch.from_numpy(o.want).to(torch.float16)), (bias_mode, slope, res)
    print(f"\nfr_conv_splitk_epilogue splitk {splitk} Cout {Cout}: worst err / bound {worst:.4f}")


def test_conv_sequence_splitk_step_equals_the_two_calls(lib):
    """fr_conv_sequence kind 1 with border-class bias + PReLU + residual: the same bits as the partials launch followed by
    fr_conv_splitk_epilogue, and exact on integer operands."""
    from facerecognition_infrenceengine_amd import _lib
    splitk = 6
    o = er.int_operands(np.random.default_rng(61), 3, 5, 9, 128, 128, 3, 1, 1, 1, True, True, True)
    of = er.float_operands(np.random.default_rng(62), 3, 5, 9, 128, 128, 3, 1, 1, 1, True, True, True)
    M = o.B * o.Ho * o.Wo
    for ops in (o, of):
        xd, wd = _dev(ops.x), _dev(ops.w)
        bd, sd, rd = _dev(ops.bias, torch.float32), _dev(ops.slope, torch.float32), _dev(ops.residual)
        ys, parts = [], []
        for _ in range(2):
            ys.append(torch.full((M, o.Cout), NAN, dtype=torch.float16, device="cuda"))
            parts.append(torch.full((splitk, M, o.Cout), NAN, dtype=torch.float32, device="cuda"))
        st = (_lib.ConvStep * 1)()
        st[0].kind = 1
        st[0].args = _conv_args(_lib, ops, xd, wd, ys[0], bd, sd, rd, part=parts[0], splitk=splitk)
        lib.fr_conv_sequence(st, 1, _lib.stream_ptr())
        a = _conv_args(_lib, ops, xd, wd, None, None, None, None, part=parts[1], splitk=splitk)
        a.bias_mode = 0
        lib.fr_conv_nhwc_f16(ctypes.byref(a), _lib.stream_ptr())
        lib.fr_conv_splitk_epilogue(_lib.ptr(parts[1]), splitk, M, o.Cout, o.Ho, o.Wo, _lib.ptr(bd), 1, _lib.ptr(sd), _lib.ptr(rd),
                                    _lib.ptr(ys[1]), _lib.stream_ptr())
        torch.cuda.synchronize()
        assert not torch.isnan(ys[0]).any() and torch.equal(ys[0], ys[1]) and torch.equal(parts[0], parts[1])
    # ops is now the float case; the integer case's sequence output against the reference:
    xd, wd = _dev(o.x), _dev(o.w)
    bd, sd, rd = _dev(o.bias, torch.float32), _dev(o.slope, torch.float32), _dev(o.residual)
    y = torch.full((M, o.Cout), NAN, dtype=torch.float16, device="cuda")
    part = torch.full((splitk, M, o.Cout), NAN, dtype=torch.float32, device="cuda")
    st = (_lib.ConvStep * 1)()
    st[0].kind = 1
    st[0].args = _conv_args(_lib, o, xd, wd, y, bd, sd, rd, part=part, splitk=splitk)
    lib.fr_conv_sequence(st, 1, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().reshape(o.want.shape), torch.from_numpy(o.want).to(torch.float16))


# ---------------------------------------------------------------- D. the FC tail
@pytest.mark.parametrize("case", er.FC_TAIL_CASES, ids=_ids)
def test_fc_reduce_l2norm(lib, case):
    """embedding within (splitk + 1) 2^-24 (|bias| + sum |partial|) of float64; normed against the kernel's OWN embedding
    normalised in float64, within ((dim + 2) / 2 + 3) 2^-24 |want| (dim squares summed in f32 in any order, a correctly rounded
    square root and division: the build sets -fno-fast-math, and hipcc's HIP default is correctly rounded sqrtf and /); rows
    past B of pre-filled outputs stay untouched; integer partials give an exact embedding."""
    from facerecognition_infrenceengine_amd import _lib
    B, splitk, dim = case
    rng = np.random.default_rng(er.case_seed(case))
    for kind in ("float", "int"):
        o = er.fc_tail_operands(rng, B, splitk, dim, kind)
        pd, bd = _dev(o.partial, torch.float32), _dev(o.bias, torch.float32)
        emb = torch.full((B + 3, dim), -7.0, dtype=torch.float32, device="cuda")
        nrm = torch.full((B + 3, dim), -7.0, dtype=torch.float32, device="cuda")
        emb[:B] = NAN
        nrm[:B] = NAN
        lib.fr_fc_reduce_l2norm(_lib.ptr(pd), splitk, B, dim, _lib.ptr(bd), _lib.ptr(emb), _lib.ptr(nrm), _lib.stream_ptr())
        torch.cuda.synchronize()
        e, n = emb.cpu().numpy().astype(np.float64), nrm.cpu().numpy().astype(np.float64)
        assert (e[B:] == -7.0).all() and (n[B:] == -7.0).all()
        e, n = e[:B], n[:B]
        if kind == "int":
            assert np.array_equal(e, o.want)
        re = er.worst_ratio(np.abs(e - o.want), er.fc_tail_bound(splitk, o.mag))
        want_n = er.normed_ref(e)
        rn = er.worst_ratio(np.abs(n - want_n), er.normed_bound(dim, want_n))
        if kind == "float":
            print(f"\nfr_fc_reduce_l2norm {case}: embedding err / bound {re:.4f}, normed err / bound {rn:.4f}")
        assert re <= 1.0 and rn <= 1.0, (kind, re, rn)
