"""CPU only: the instruments of tests/test_gpu_embed_pins.py would fail a subtly wrong kernel, and pass a right one.

The float64 references of tests/helpers/embed_ref.py are compared against a float32 emulation of the kernels (same f16 operands,
f32 products and sums) with faults planted one at a time: every plant must be caught by the exact-integer comparison and, where
the GPU test uses the float64 bound (its parts B, C and D), by the bound; the unfaulted emulation must stay inside every bound
that the GPU test uses, on the GPU test's own cases."""
import numpy as np
import pytest

from tests.helpers import embed_ref as er


def test_splitk_slices_restate_the_kernel():
    assert er.splitk_slices(18, 4) == [(0, 5), (5, 10), (10, 15), (15, 18)]
    assert er.splitk_slices(9, 4) == [(0, 3), (3, 6), (6, 9), (9, 9)]
    assert er.splitk_slices(19, 4)[-1] == (15, 19)
    s = er.splitk_slices(30, 28)
    assert s[14] == (28, 30) and all(ks >= ke for ks, ke in s[15:]) and s[27] == (54, 30)
    assert er.splitk_slices(392, 28) == [(14 * z, 14 * z + 14) for z in range(28)]
    for nk, sk in ((18, 6), (18, 2), (36, 12), (36, 4), (72, 24), (72, 8)):          # the engine's counts: whole slices of 3 / 9 steps
        assert er.splitk_slices(nk, sk) == [(z * nk // sk, (z + 1) * nk // sk) for z in range(sk)]


def test_conv_ref_against_a_direct_loop():
    """conv_ref itself (layout, border classes, operation order, x2 columns, krange) against the definition written out."""
    rng = np.random.default_rng(0)
    o = er.float_operands(rng, 2, 5, 4, 8, 4, 3, 2, 1, bias=True, slope=True, residual=True, C2=8)
    want, mag = er.conv_ref(o.x, o.w, o.bias, 0, o.slope, o.residual, 2, 1, x2=o.x2)
    ref = np.zeros_like(want)
    for b in range(2):
        for ho in range(o.Ho):
            for wo in range(o.Wo):
                col = []
                for kh in range(3):
                    for kw in range(3):
                        h, w_ = ho * 2 - 1 + kh, wo * 2 - 1 + kw
                        col.append(o.x[b, h, w_] if 0 <= h < 5 and 0 <= w_ < 4 else np.zeros(8))
                col.append(o.x2[b, ho * 2, wo * 2])
                v = o.w @ np.concatenate(col) + o.bias
                v = np.where(v > 0, v, v * o.slope)
                ref[b, ho, wo] = v + o.residual[b, ho, wo]
    assert np.abs(want - ref).max() < 1e-12 and (mag >= np.abs(want) - 1e-12).all()
    halves = [er.conv_ref(o.x, o.w, None, 0, None, None, 2, 1, x2=o.x2, krange=r)[0] for r in ((0, 40), (40, 80))]
    full = er.conv_ref(o.x, o.w, None, 0, None, None, 2, 1, x2=o.x2)[0]
    assert np.abs(halves[0] + halves[1] - full).max() < 1e-12
    o = er.float_operands(rng, 1, 4, 5, 4, 3, 3, 1, 1, bias_mode=1, bias=True)
    want, _ = er.conv_ref(o.x, o.w, o.bias, 1, None, None, 1, 1)
    base, _ = er.conv_ref(o.x, o.w, None, 0, None, None, 1, 1)
    b9 = o.bias.reshape(3, 3, 3)
    assert np.allclose((want - base)[0, 0, 0], b9[0, 0]) and np.allclose((want - base)[0, 3, 4], b9[2, 2])
    assert np.allclose((want - base)[0, 1, 4], b9[1, 2]) and np.allclose((want - base)[0, 3, 2], b9[2, 1])


def _exact_f16(got, want):
    return np.array_equal(got.astype(np.float64), want)


# ---------------------------------------------------------------- A: the fused conv, exact-integer instrument
def _emulate_conv(o, fault=None, drop=None):
    part = er.emulate_partials(o, 1, ("drop", drop) if drop is not None else None)
    res = None if o.residual is None else o.residual.reshape(-1, o.Cout)
    return er.emulate_epilogue(part, o.bias, o.bias_mode, o.slope, res, o.Ho, o.Wo, fault).reshape(o.want.shape)


@pytest.mark.parametrize("geom", [(3, 5, 9, 128, 64, 3, 1, 1), (1, 7, 7, 512, 128, 3, 1, 1), (2, 1, 1, 25088, 512, 1, 1, 0)])
def test_exact_instrument_catches_each_plant_in_the_fused_conv(geom):
    rng = np.random.default_rng(sum(geom))
    k3 = geom[5] == 3
    o = er.int_operands(rng, *geom, bias_mode=1 if k3 else 0, bias=True, slope=True, residual=True,
                        w=None if k3 else er.fc_weights("int", geom[3]))
    assert _exact_f16(_emulate_conv(o), o.want)
    nk = o.K // er.BK
    for s in (0, nk // 2, nk - 1):
        assert not _exact_f16(_emulate_conv(o, drop=s), o.want), s
    for fault in ("slope_prev", "res_neighbour") + (("bias_col",) if k3 else ()):
        assert not _exact_f16(_emulate_conv(o, fault), o.want), fault


def test_exact_stage_block_is_exact_and_catches_a_dropped_step():
    rng = np.random.default_rng(14)
    o = er.int_stage_block(rng, 1, 14, 256)
    c1 = SimpleConv(o.x, o.w1, 9 * 256, o.b9, 1, o.slope, None, o.mid)
    assert _exact_f16(_emulate_conv(c1), o.mid)
    c2 = SimpleConv(o.mid, o.w2, 9 * 256, o.b2, 0, None, o.x, o.want)
    assert _exact_f16(_emulate_conv(c2), o.want)
    assert not _exact_f16(_emulate_conv(c2, drop=17), o.want) and not _exact_f16(_emulate_conv(c1, fault="bias_col"), o.mid)
    assert np.abs(o.mid).max() > 20 and np.abs(o.want).max() > 100         # not exact by being trivial


class SimpleConv:
    def __init__(self, x, w, K, bias, bias_mode, slope, residual, want):
        self.x, self.w, self.K, self.bias, self.bias_mode, self.slope, self.residual, self.want = x, w, K, bias, bias_mode, slope, residual, want
        self.k, self.stride, self.pad, self.x2 = 3, 1, 1, None
        self.Ho, self.Wo, self.Cout = x.shape[1], x.shape[2], w.shape[0]


# ---------------------------------------------------------------- B: split-K partials, per slice
def _check_slices(got, refs, kind):
    """-> (all slices pass, worst err / bound)"""
    ok, worst = True, 0.0
    for z, (want, mag, ksl) in enumerate(refs):
        g = got[z].astype(np.float64)
        if kind == "int" or ksl == 0:
            ok = ok and np.array_equal(g, want)
            continue
        if np.isnan(g).any():
            ok = False
            continue
        err, bound = np.abs(g - want), (ksl + 2) * er.U32 * mag
        ok = ok and bool((err <= bound).all())
        worst = max(worst, er.worst_ratio(err, np.where(bound == 0, 1.0, bound)))
    return ok, worst


@pytest.mark.parametrize("case", er.PARTIAL_CASES, ids=lambda c: "-".join(map(str, c)))
def test_partials_emulation_inside_the_bound_and_plants_outside(case):
    splitk = case[8]
    if case[0] == 130:
        case = (5,) + case[1:]                   # the CPU emulation does not depend on the pixel tiling: five rows say the same
    for kind in ("float", "int"):
        o = er.partial_operands(case, kind)
        refs = er.partial_refs(o, splitk, kind)
        ok, worst = _check_slices(er.emulate_partials(o, splitk), refs, kind)
        print(f"partials {case} {kind}: f32 emulation, worst err / bound {worst:.3f}")
        assert ok
        sl = er.splitk_slices(o.K // er.BK, splitk)
        full = [s for s, (ks, ke) in enumerate(sl) if ke > ks]
        for s in (sl[full[0]][0], sl[full[-1]][1] - 1):                                       # the first and the last K step
            assert not _check_slices(er.emulate_partials(o, splitk, ("drop", s)), refs, kind)[0], (kind, s)
        assert not _check_slices(er.emulate_partials(o, splitk, "boundary"), refs, kind)[0], kind
        if len(full) < splitk:
            assert not _check_slices(er.emulate_partials(o, splitk, "unwritten"), refs, kind)[0], kind


def test_partial_refs_are_conv_ref_per_slice():
    case = er.PARTIAL_CASES[8]                   # the x2 form
    o = er.partial_operands(case, "float")
    for (ks, ke), (want, mag, _) in zip(er.splitk_slices(o.K // er.BK, case[8]), er.partial_refs(o, case[8], "float")):
        w2, m2 = er.conv_ref(o.x, o.w, None, 0, None, None, o.stride, o.pad, x2=o.x2, krange=(ks * er.BK, ke * er.BK))
        assert np.array_equal(w2.reshape(want.shape), want) and np.array_equal(m2.reshape(mag.shape), mag)


# ---------------------------------------------------------------- C: the split-K epilogue
@pytest.mark.parametrize("Cout", er.EPILOGUE_COUT)
@pytest.mark.parametrize("splitk", er.EPILOGUE_SPLITK)
def test_epilogue_emulation_inside_the_bound_and_plants_outside(splitk, Cout):
    rng = np.random.default_rng(splitk * 100 + Cout)
    worst = 0.0
    for bias_mode, slope, res in er.EPILOGUE_FORMS:
        for kind in ("float", "int"):
            o = er.epilogue_operands(rng, splitk, Cout, bias_mode, slope, res, kind)

            def passes(fault=None):
                got = er.emulate_epilogue(o.partial, o.bias, o.bias_mode, o.slope, o.residual, o.Ho, o.Wo, fault).astype(np.float64)
                if kind == "int":
                    return np.array_equal(got, o.want), 0.0
                err, bound = np.abs(got - o.want), er.epilogue_bound(splitk, o.mag, o.want)
                return bool((err <= bound).all()), er.worst_ratio(err, bound)
            ok, r = passes()
            worst = max(worst, r)
            assert ok, (bias_mode, slope, res, kind, r)
            plants = (["miss_slice"] + (["bias_col"] if bias_mode == 1 else []) + (["slope_prev"] if slope else [])
                      + (["res_neighbour"] if res else []))
            for fault in plants:
                assert not passes(fault)[0], (bias_mode, slope, res, kind, fault)
    print(f"epilogue splitk {splitk} Cout {Cout}: f32 emulation, worst err / bound {worst:.3f}")


# ---------------------------------------------------------------- D: the FC tail
@pytest.mark.parametrize("case", er.FC_TAIL_CASES, ids=lambda c: "-".join(map(str, c)))
def test_fc_tail_emulation_inside_the_bounds_and_plants_outside(case):
    B, splitk, dim = case
    rng = np.random.default_rng(er.case_seed(case))
    o = er.fc_tail_operands(rng, B, splitk, dim, "float")

    def ratios(fault=None):
        e, n = er.emulate_fc_tail(o.partial, o.bias, fault)
        want_n = er.normed_ref(e)
        return (er.worst_ratio(np.abs(e - o.want), er.fc_tail_bound(splitk, o.mag)),
                er.worst_ratio(np.abs(n - want_n), er.normed_bound(dim, want_n)))
    re, rn = ratios()
    print(f"fc tail {case}: f32 emulation, embedding err / bound {re:.3f}, normed err / bound {rn:.3f}")
    assert re <= 1 and rn <= 1
    assert ratios("miss_slice")[0] > 1 and ratios("short_norm")[1] > 1
    oi = er.fc_tail_operands(rng, B, splitk, dim, "int")
    assert np.array_equal(er.emulate_fc_tail(oi.partial, oi.bias)[0].astype(np.float64), oi.want)
    assert not np.array_equal(er.emulate_fc_tail(oi.partial, oi.bias, "miss_slice")[0].astype(np.float64), oi.want)
