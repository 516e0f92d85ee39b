"""CPU only: the instruments of tests/test_gpu_f8_pins.py would fail a subtly wrong fp8 kernel, and pass a right one.

tests/helpers/f8_ref.py's e4m3 rounding is checked on every code and every tie; its float64 references are compared against a
float32 emulation of fr_conv_nhwc_f8 and fr_conv_stage14_f8 with faults planted one at a time, on the GPU test's own cases: the
unfaulted emulation must pass the exact comparison and the interval criterion, every plant must fail one of them; and the
centring identity that IResNetHIP.enable_fp8 builds its border-class biases on is checked in float64."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import f8_ref as fr

# ---------------------------------------------------------------- e4m3
def test_e4m3_on_every_code_and_every_tie():
    from facerecognition_infrenceengine_amd.iresnet import round_e4m3
    v = fr.e4m3_values()
    assert len(v) == 254 and v.max() == 448 and v.min() == -448
    pos = np.sort(v[(v > 0)])
    assert pos[0] == 2.0 ** -9 and len(pos) == 126 and np.array_equal(np.diff(pos[:8]), np.full(7, 2.0 ** -9))
    assert np.array_equal(fr.e4m3(v), v)                                    # every code is a fixed point (and -0 stays -0)
    assert np.signbit(fr.e4m3(np.array([-0.0, -1e-9]))).all()
    grid = np.concatenate([[0.0], pos])
    mid = (grid[:-1] + grid[1:]) / 2                                       # every tie; exact: neighbours share all but one bit
    even = np.where(np.arange(len(mid)) % 2 == 0, grid[:-1], grid[1:])      # positive codes count up with the value: grid[i] is code i
    assert fr.e4m3_is_tie(mid).all() and not fr.e4m3_is_tie(grid).any()
    m32 = mid.astype(np.float32)                                            # the neighbours of a tie among the f32 numbers
    probe = np.concatenate([mid, np.nextafter(m32, np.float32(0)).astype(np.float64), np.nextafter(m32, np.float32(1e9)).astype(np.float64), [448.0, 449.0, 464.0, 480.0, 1e6, np.inf, 2.0 ** -10, 2.0 ** -11]])
    probe = np.concatenate([probe, -probe])
    got = fr.e4m3(probe)
    t = torch.from_numpy(probe)
    assert np.array_equal(got, t.float().clamp(-448, 448).to(torch.float8_e4m3fn).float().numpy().astype(np.float64))
    assert np.array_equal(got, round_e4m3(t).numpy())
    assert np.array_equal(got[:len(mid)], even)                            # ties go to the even code
    assert np.array_equal(fr.e4m3_trunc(np.nextafter(grid[1:], 0)), grid[:-1])
    rng = np.random.default_rng(0)
    r = np.concatenate([rng.standard_normal(20000) * 100, rng.standard_normal(20000) * 0.01])
    r32 = r.astype(np.float32).astype(np.float64)
    assert np.array_equal(fr.e4m3(r32), torch.from_numpy(r32).float().clamp(-448, 448).to(torch.float8_e4m3fn).float().numpy().astype(np.float64))
    assert np.array_equal(fr.bytes_values(fr.e4m3_bytes(v)), v)


def test_helpers_of_the_instrument():
    assert np.array_equal(fr.frac_bits(np.array([0.0, 1.0, 0.5, -0.375, 448.0, 2.0 ** -9, 3 * 2.0 ** -24])), [0, 0, 1, 3, 0, 9, 24])
    assert np.array_equal(fr.f16_is_tie(np.array([8 + 2.0 ** -8, 8 + 2.0 ** -9, 8.0, -(2048.0 + 1), 2.0 ** -25])), [True, False, False, True, True])
    m = fr.location_masks(2, 28)
    assert m["last"].sum() == 2 * 4 * 4 and m["last"][0, 6, 24:].all() and m["last"][1, 27, 27] and not m["last"][0, 7].any()
    m = fr.location_masks(1, 14)
    assert m["last"].sum() == 4 and m["last"][0, 13, 10:].all() and m["border"].sum() == 52 - 4 and m["inside"].sum() == 144


def test_misaligned_restates_what_the_matrix_instruction_drops():
    """the sums measured on an MI355X (KERNEL_NOTES 4.12): 256 * 1/4 + x * 1 - 256 * 1/4 in three adjacent channels returns x cut
    to a multiple of 2^-7 = 2^(6 - 13); the condition flags exactly the x that are no such multiple, blames their column, and
    looks at one group of 8 channels at a time"""
    def operands(xs, col):
        x, w = np.zeros((1, 14, 14, 256)), np.zeros((128, 9, 256))
        x[0, 5, 5, 0] = x[0, 5, 5, 2] = 256.0
        x[0, 5, 5, col] = xs
        w[7, 4, 0], w[7, 4, 2], w[7, 4, col] = 0.25, -0.25, 1.0
        return x, w.reshape(128, -1)
    assert fr.misaligned(*operands(15 * 2.0 ** -8, 1)) == {7: np.array([4 * 256 + 1])}
    assert fr.misaligned(*operands(2.0 ** -8, 1)) and fr.misaligned(*operands(2.0 ** -8, 7))
    assert not fr.misaligned(*operands(14 * 2.0 ** -8, 1)) and not fr.misaligned(*operands(2.0 ** -7, 1))
    assert not fr.misaligned(*operands(2.0 ** -9, 8)) and not fr.misaligned(*operands(2.0 ** -9, 128))      # the next group, the next K step


# ---------------------------------------------------------------- the cases of the GPU test, built once
@pytest.fixture(scope="module")
def exact_layers():
    return {c: fr.exact_layer_operands(np.random.default_rng(fr.seed_of(c)), *c) for c in fr.EXACT_LAYER_CASES}


@pytest.fixture(scope="module")
def float_layers():
    return {c: fr.float_layer_operands(np.random.default_rng(fr.seed_of(c)), *c) for c in fr.FLOAT_LAYER_CASES}


@pytest.fixture(scope="module")
def stage_runs():
    return {c: fr.exact_stage_run(np.random.default_rng(fr.seed_of(c)), c[1], c[0]) for c in fr.STAGE_CASES}


def _applies(o, fault):
    """a fault that the case's form cannot show"""
    if fault == "bias_tile":
        return o.bias_mode == 1
    if fault == "res_before_prelu":
        return o.residual is not None and o.slope is not None
    if fault == "slope_prev_ch":
        return o.slope is not None
    if fault == "mu_prev_ch":
        return o.want8 and o.sub is not None
    if fault in ("y8_unrounded", "trunc", "nosat"):
        return o.want8
    return True


def test_exact_layer_cases_cover_every_form_at_both_sizes():
    for H in (14, 28):
        cs = [c for c in fr.EXACT_LAYER_CASES if c[1] == H]
        assert {c[4] for c in cs} == {None, 0, 1}                                         # bias NULL / mode 0 / mode 1
        for col in (5, 6, 9):                                                                   # slope, residual, y8_sub: with and without
            assert {c[col] for c in cs} == {True, False}
        assert {(c[7], c[8]) for c in cs} == {(True, False), (False, True), (True, True)}     # y16 only, y8 only, both
    assert any(c[6] and c[9] and c[8] for c in fr.EXACT_LAYER_CASES)                          # y8_sub with a residual


def test_exact_layer_emulation_passes_and_every_plant_fails(exact_layers):
    caught = {f: 0 for f in fr.LAYER_FAULTS}
    for case, o in exact_layers.items():
        assert fr.layer_is_exact(o, *fr.emulate_layer(o)), case
        for fault in fr.LAYER_FAULTS:
            if _applies(o, fault):
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    assert not fr.layer_is_exact(o, *fr.emulate_layer(o, fault)), (case, fault)
                caught[fault] += 1
    assert all(caught.values()), caught
    ev = {k: min(o.coverage[k] for o in exact_layers.values() if k in o.coverage) for o in exact_layers.values() for k in o.coverage}
    print("\nexact layer cases: fewest elements per (location, event):", ev)
    print("largest mag * 2^q / 2^24:", max(o.headroom for o in exact_layers.values()) / 2.0 ** 24)


def test_float_layer_emulation_inside_the_interval_and_plants_outside(float_layers):
    for case, o in float_layers.items():
        y16, y8 = fr.emulate_layer(o)
        ok, worst = fr.interval_check(o, y16, y8)
        print(f"\nfr_conv_nhwc_f8 {case}: f32 emulation, worst err / e {worst}")
        assert ok, case
        for fault in ("drop_first", "drop_last", "bias_tile", "oscale_prev_ch", "slope_prev_ch", "trunc", "y8_unrounded"):       # no code saturates here: "nosat" is the exact cases'
            if not _applies(o, fault) or (fault == "y8_unrounded" and not o.want16):     # without y16 the interval admits it
                continue
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                y16, y8 = fr.emulate_layer(o, fault)
                assert not fr.interval_check(o, y16, y8)[0], (case, fault)


def test_stage_emulation_passes_and_every_plant_fails(stage_runs):
    for case, run in stage_runs.items():
        want = run.y[-1].astype(np.float16)
        assert np.array_equal(fr.emulate_stage(run), want), case
        for fault in fr.STAGE_FAULTS:
            if (fault == "res_x16" and run.nblocks < 2) or fault == "res_before_prelu":   # a second conv has no PReLU
                continue
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                assert not np.array_equal(fr.emulate_stage(run, fault), want), (case, fault)
    print("\nstage runs: events per conv of (3 blocks, 3 faces):", stage_runs[(3, 3)].coverage)
    print("largest mag * 2^q / 2^24 per conv:", [h / 2.0 ** 24 for h in stage_runs[(3, 3)].headroom])


def test_stage_run_layout(stage_runs):
    """the rows as _pack_stage14_f8 lays them out, and what makes a neighbour's or a predecessor's value visible"""
    run = stage_runs[(3, 1)]
    assert len(run.prm) == 6 and all(p.shape == (14, 256) for p in run.prm)
    for j, p in enumerate(run.prm):
        assert np.array_equal(p[1], 1.0 / p[0]) and np.array_equal(p[0], 2.0 ** np.round(np.log2(p[0])))
        assert (p[11] == 1.0).all() == (j % 2 == 1)
        if j < 5:
            assert np.array_equal(p[12], run.mu[j + 1]) and p[13, 0] == run.inv_sx[j + 1] and run.inv_sx[j + 1] != run.inv_sx[j]
            assert (p[12] != np.roll(p[12], 1)).mean() > 0.5 and (p[12] != run.mu[j]).mean() > 0.5
        else:
            assert not p[12].any() and p[13, 0] == 1.0
    assert np.array_equal(run.x8, fr.e4m3((run.x16 - run.mu[0]) * run.inv_sx[0]))
    assert np.array_equal(run.conv[3].resid, run.y[0]) and np.array_equal(run.conv[2].x, run.conv[1].code)


# ---------------------------------------------------------------- the centring identity of enable_fp8
@pytest.mark.parametrize("base9", [False, True])
def test_centring_identity_by_border_class(base9):
    """conv(x) + base == conv(x - mu) + border_bias9(base, tap): tap[co][kh][kw] = sum_ci w[co][ci][kh][kw] mu[ci], summed over
    the taps that fall inside the image - per border class, 6 x 7 image, 8 channels, float64."""
    from facerecognition_infrenceengine_amd.iresnet import border_bias9
    g = torch.Generator().manual_seed(5 + base9)
    Cin, Cout, H, W = 8, 8, 6, 7
    x = torch.randn((2, Cin, H, W), generator=g, dtype=torch.float64)
    w = torch.randn((Cout, Cin, 3, 3), generator=g, dtype=torch.float64)
    mu = torch.randn(Cin, generator=g, dtype=torch.float64)
    base = torch.randn((3, 3, Cout) if base9 else (Cout,), generator=g, dtype=torch.float64)
    tap = (w * mu[None, :, None, None]).sum(1)
    b9 = border_bias9(base, tap)
    rc, cc = torch.ones(H, dtype=torch.long), torch.ones(W, dtype=torch.long)
    rc[0] = cc[0] = 0
    rc[-1] = cc[-1] = 2
    per_px = lambda b: b[rc][:, cc].permute(2, 0, 1)[None]                 # noqa: E731
    want = F.conv2d(x, w, None, 1, 1) + (per_px(base) if base9 else base[None, :, None, None])
    got = F.conv2d(x - mu[None, :, None, None], w, None, 1, 1) + per_px(b9)
    assert (want - got).abs().max() < 1e-12
    assert (b9[1, 1] - b9[0, 0]).abs().min() > 1e-3                        # the classes differ: a plain bias would not do
