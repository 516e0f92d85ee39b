"""CPU only: the instruments of tests/test_gpu_stage_pins.py would fail a subtly wrong stage kernel, and pass a right one.

A float32 emulation of a whole stage run (tests/helpers/stage_ref.py emulate_stage_run: f16 maps, f32 arithmetic, any order of
summation) runs the GPU test's own cases: unfaulted it must pass every assertion the GPU test makes - which also asserts, inside
the helper, that each reference is exact, covers every K step of every wave group and reaches the listed roundings - and with
one fault planted it must fail the exact comparison of a 3-block run and, where the fault touches the conv that the selector
shows, the per-element bound.  Two plants need a rounding to show at all (truncation, an unrounded `mid`): a 3-block run at 2 per
row has none (max |v| < 2048), so they are planted in the 4-block run at 4 per row."""
import numpy as np
import pytest

from tests.helpers import stage_ref as sr


def _equal(got16, want):
    return np.array_equal(got16.astype(np.float64), want)


def test_step_of_column_restates_the_pack_kernels():
    """stage14_pack_weights: slot q = tap * 8 + g takes columns tap * 256 + g * 32 + (0 .. 31); stage28_pack_weights: slot q =
    plane * 18 + tap * 2 + gg takes columns tap * 128 + plane * 64 + gg * 32 + (0 .. 31)."""
    s14, s28 = sr.step_of_column(14), sr.step_of_column(28)
    for q in range(72):
        tap, g = q >> 3, q & 7
        assert np.array_equal(np.flatnonzero(s14 == q), tap * 256 + g * 32 + np.arange(32))
    for q in range(36):
        plane, k = divmod(q, 18)
        assert np.array_equal(np.flatnonzero(s28 == q), (k >> 1) * 128 + plane * 64 + (k & 1) * 32 + np.arange(32))


def test_covering_weights_cover_and_a_gap_is_seen():
    for HW, per_row in ((14, 2), (28, 4)):
        w = sr.covering_weights(np.random.default_rng(HW), HW, per_row)
        assert set(np.unique(w)) == {-1.0, 0.0, 1.0} and ((w != 0).sum(1) == per_row).all()
        w[:64, sr.step_of_column(HW) == 5] = 0.0
        assert not sr.covers_every_step(w, HW)


def test_rounding_events_on_known_integers():
    v = np.array([2047.0, 2049.0, 2051.0, -2049.0, 4097.0, 4098.0, 4102.0, 4099.0, 0.0])
    ev = sr.rounding_events(v)
    assert ev["unrounded"].tolist() == [True] + [False] * 8
    assert ev["tie_down"].tolist() == [False, True, False, False, False, True, False, False, False]      # 2049 -> 2048, 4098 -> 4096
    assert ev["tie_up"].tolist() == [False, False, True, True, False, False, True, False, False]         # 2051 -> 2052, -2049 -> -2048
    assert ev["rounded_non_tie"].tolist() == [False] * 4 + [True, False, False, True, False]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("depth", sr.DEPTHS, ids=lambda d: f"{d[0]}x{d[1]}")
@pytest.mark.parametrize("HW", [14, 28])
def test_emulation_passes_the_exact_runs(HW, depth, B):
    o = sr.exact_case(HW, *depth, B)
    y, mid = sr.emulate_stage_run(o.x, o.w, o.prm, HW)
    assert _equal(y, o.want) and _equal(mid, o.mids[-1])
    print(f"\nexact run {HW}x{HW}, {depth[0]} blocks at {depth[1]} per row, {B} faces: max |v| per block {o.growth}, events {o.events}")
    assert o.rounds == (depth in ((7, 2), (4, 4)))
    if o.rounds:
        assert o.growth[-1] > 4096
    else:
        assert o.growth[-1] < 2048


@pytest.mark.parametrize("HW", [14, 28])
def test_wide_launch_gather_and_its_plant(HW):
    """256 / 257 faces from 7 distinct ones: the expectation is the same gather; the last face's output missing (14x14: y keeps its
    NaN; 28x28: x keeps the input) is seen."""
    o = sr.exact_case(HW, 3, 2, sr.WIDE_FACES)
    y, _ = sr.emulate_stage_run(o.x, o.w, o.prm, HW)
    idx = np.arange(257) % sr.WIDE_FACES
    assert all(idx[i] != idx[i + 1] for i in range(256)) and idx[256] == 4
    want = sr.gather_faces(o.want, 257)
    got = sr.gather_faces(y, 257)
    assert _equal(got, want) and _equal(got[:256], sr.gather_faces(o.want, 256))
    got[256] = np.nan if HW == 14 else sr.gather_faces(o.x, 257)[256]
    assert not _equal(got, want)


PLANTS3 = [("prm_prev", 1), ("prm_prev", 2), ("prm_prev", 4), ("res_from_x", 3), ("res_from_x", 5), ("in_from_x", 2), ("in_from_x", 4),
           ("first_slot", 1), ("first_slot", 2), ("first_slot", 5), ("drop_last", 0), ("drop_last", 3), ("drop_last", 5),
           ("slope_prev", None), ("bias_prev", None)]


@pytest.mark.parametrize("HW", [14, 28])
def test_each_plant_fails_the_exact_comparison_of_a_three_block_run(HW):
    o = sr.exact_case(HW, 3, 2, 3)
    plants = PLANTS3 + ([("border_192", None)] if HW == 14 else [("halo15", 2), ("halo15", 3), ("halo15", 5), ("half_unwritten", None)])
    for fault, at in plants:
        y, mid = sr.emulate_stage_run(o.x, o.w, o.prm, HW, fault, at)
        assert not _equal(y, o.want), (fault, at)
    # what only the 28x28 kernel's visible `mid` shows: a fault in the last block's first conv is also caught there
    if HW == 28:
        assert not _equal(sr.emulate_stage_run(o.x, o.w, o.prm, HW, "drop_last", 4)[1], o.mids[-1])


@pytest.mark.parametrize("HW", [14, 28])
def test_rounding_plants_fail_the_deep_run(HW):
    o = sr.exact_case(HW, 4, 4, 1)
    for fault in ("trunc", "mid_unrounded"):
        y, _ = sr.emulate_stage_run(o.x, o.w, o.prm, HW, fault)
        assert not _equal(y, o.want), fault
    # and neither shows in the 3-block run, which has no rounding: the reason for the deep run
    o = sr.exact_case(HW, 3, 2, 3)
    assert _equal(sr.emulate_stage_run(o.x, o.w, o.prm, HW, "trunc")[0], o.want)


# ---------------------------------------------------------------- the selector blocks
SELECTOR_PLANTS = {          # (fault, conv of the block it is planted at: 0 / 1 / None)
    "conv2": [("drop_last", 0), ("slope_prev", 0), ("bias_prev", 0), ("prm_prev", 1), ("first_slot", 1)],
    "conv1": [("drop_last", 1), ("bias_prev", 1), ("prm_prev", 1), ("first_slot", 1)],
}


@pytest.mark.parametrize("which", ["conv2", "conv1"])
@pytest.mark.parametrize("HW", [14, 28])
def test_selector_emulation_inside_the_bound_and_plants_outside(HW, which):
    for name, x, w, prm, blk, j0 in sr.selector_cases(HW, which):
        y, mid = sr.emulate_stage_run(x, w, prm, HW)
        r = sr.selector_ratio(blk, y, mid)
        zero = float((blk.x == 0).mean())
        print(f"\nselector {which} {HW}x{HW} {name}: f32 emulation, worst err / bound {r:.4f} (residual zero in {zero:.0%} of the elements)")
        assert r <= 1.0
        plants = list(SELECTOR_PLANTS[which])
        if j0:
            plants += [("res_from_x", 1), ("in_from_x", 0)]
        if HW == 14 and which == "conv2":
            plants.append(("border_192", 0))
        if HW == 28:
            plants += [("half_unwritten", None)] + ([("halo15", int(which == "conv1"))] if j0 else [])      # a stale row needs an earlier block, and a conv that reads neighbours
        for fault, at in plants:
            yf, _ = sr.emulate_stage_run(x, w, prm, HW, fault, None if at is None else j0 + at)
            assert np.isnan(yf.astype(np.float64)).any() or sr.selector_ratio(blk, yf) > 1.0, (name, fault, at)


def test_selector_conv2_shows_the_first_conv_untouched_where_the_residual_is_zero():
    rng = np.random.default_rng(5)
    x = sr.selector_input(rng, 1, 14, "odd")
    blk = sr.selector_block(rng, 14, "conv2", x)
    z = x == 0
    assert z[..., 1::2].all() and z.mean() < 0.51
    assert np.array_equal(blk.bound[z], blk.bound_mid[..., blk.perm][z]) and (blk.bound[~z] > blk.bound_mid[..., blk.perm][~z]).all()
    y, mid = sr.emulate_stage_run(x, blk.w, blk.prm, 14)
    assert np.array_equal(y.astype(np.float64)[z], (blk.sign * mid.astype(np.float64)[..., blk.perm])[z])
