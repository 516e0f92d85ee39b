"""CPU only: the instruments of tests/test_gpu_coarse_pins.py pass a right coarse scan and would fail a subtly wrong one.

A. `coarse_ref` against a brute-force loop; on every shape of the GPU test an emulated scan with one planted fault changes a compared value.
B. a float32 model with sequential accumulation stays inside the bound of DESIGN.md 4.6b on every family; flushing f16 subnormals, a
   13-bit window and a truncating conversion each leave it on at least one.
C. an emulation of the lists, the spill bounds and the certificate gives every expected flag; without any one of the three spill updates,
   or with the bound read one candidate too far, it certifies a wrong list in the case built for that path."""
import numpy as np
import pytest

from tests.helpers import coarse_ref as cr


# ---------------------------------------------------------------- A
@pytest.mark.parametrize("kind", ["f16", "f8"])
def test_coarse_ref_agrees_with_a_plain_loop(kind):
    rng = np.random.default_rng(3)
    for N, F, off in ((1, 1, 0), (5, 3, 7), (67, 9, (1 << 33) + 5), (130, 4, 0)):
        G = (rng.integers(-3, 4, (N, 512)) / (8 if kind == "f16" else 256)).astype(np.float32)
        Q = (rng.integers(-3, 4, (F, 512)) / (4 if kind == "f16" else 256)).astype(np.float32)
        G[N // 2] = G[0]                                                   # an exact tie: the first group wins
        Q[0] = G[0] * 2
        a, b = cr.coarse_ref(Q, G, kind, off), cr.brute_ref(Q, G, kind, off)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
        assert a[0][0] == off                                              # group 0, although row N // 2 scores the same
    # no score above -1: (-1, -1.0); exactly -1 is not above it
    G = np.zeros((8, 512), np.float32); G[:, 0] = [1, 1, 1, 1, 0.5, 1, 1, 1]
    for q0, n, want in ((-1.0, 4, (-1, -1.0)), (-1.0, 8, (4, -0.5)), (-0.5, 4, (0, -0.5)), (-1.5, 4, (-1, -1.0))):
        Q = np.zeros((1, 512), np.float32); Q[0, 0] = q0
        idx, sc = cr.coarse_ref(Q, G[:n], kind)
        assert (int(idx[0]), float(sc[0])) == want
        assert cr.brute_ref(Q, G[:n], kind)[0][0] == want[0]
    if kind == "f8":                                                       # the stored operand: x 256, ties to even, saturation
        x = np.array([17, 19, 21, 23, 26, 512, -460.8, 1792, 3, 0]) / 256
        assert cr.stored(x, "f8").tolist() == [16, 20, 20, 24, 26, 448, -448, 448, 3, 0]
    else:
        assert cr.stored([2.0 ** -25 * 1.01, 2.0 ** -24, 65504, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11], "f16").tolist() == \
            [2.0 ** -24, 2.0 ** -24, 65504, 1, 1 + 2.0 ** -9]


def test_plan_copy_matches_the_table():
    for (N, F), want in cr.SCAN_PLANS.items():
        pl = cr.plan(F, N)
        assert (pl.nqt, pl.nranges, pl.tiles_per_range) == want
    pl = cr.plan(8, cr.TOPK_N)
    assert (pl.nranges, pl.rows_per_range) == (256, 128)
    pl = cr.plan(8, cr.TOPK_N + 3)
    assert (pl.nranges, pl.rows_per_range) == (171, 192)
    from facerecognition_infrenceengine_amd import _lib
    lib = _lib.load()                                                      # the public size needs no GPU
    for N, F in cr.SCAN_SHAPES + [(cr.TOPK_N, 6), (cr.TOPK_N + 3, 1)]:
        cr.check_plan(lib.fr_gallery_match_f16_workspace(F, N), F, N, "f16")
        cr.check_plan(lib.fr_gallery_match_f8_workspace(F, N), F, N, "f8")
        assert lib.fr_gallery_match_view_f16_workspace(F, N) == lib.fr_gallery_match_f16_workspace(F, N)


def _variants(N, F, kind):
    v = [("plain", pi) for pi in cr.launches(N, F)]
    if kind == "f8" and F == N:
        v += [("offgrid", pi) for pi in cr.launches(N, F)[1:2]]
    if (N, F) == (63, 63):
        v += [("negative", pi) for pi in cr.launches(N, F)[:2]]
    return v


@pytest.mark.parametrize("kind", ["f16", "f8"])
@pytest.mark.parametrize("N,F", cr.SCAN_SHAPES)
def test_planted_scan_faults_change_a_compared_value(N, F, kind):
    """Every launch of the GPU test: the unfaulted emulation equals the reference; each fault changes idx or score bits in every shape
    that holds something it touches - a row 16 .. 31 of a tile among the planted rows (drop_chunk), any row (swap_halves), a partial
    last tile whose zero rows would win (unmasked_tail: the all-negative launches at N = 63)."""
    changed = {f: 0 for f in cr.SCAN_FAULTS}
    every_row = np.zeros(N, bool)
    for variant, pi in _variants(N, F, kind):
        Q, G, S = cr.planted(N, kind, pi, variant)
        want = cr.pick(S, kind)
        base = S if N > 300 else None                                      # large shapes: the faults are applied to the matrix at hand
        got = cr.emulate_scan(Q, G, kind, S=base)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.int32), want[1].view(np.int32))
        if variant != "negative":
            assert np.array_equal(want[0], pi // 4 * 4)
            every_row[pi] = True
        for fault in cr.SCAN_FAULTS:
            if fault == "unmasked_tail" and variant != "negative" and N > 300:
                continue                                                   # zero rows cannot win a launch whose maxima are positive
            bad = cr.emulate_scan(Q, G, kind, fault, S=base)
            n = int(((bad[0] != want[0]) | (bad[1].view(np.int32) != want[1].view(np.int32))).sum())
            changed[fault] += n
            if fault == "swap_halves" and variant == "plain":
                assert n >= 0.9 * F, (fault, n)                            # nearly every planted row shows it (a row may be symmetric by chance)
            if fault == "drop_chunk" and variant == "plain":
                hit = int(((pi % 64 >= 16) & (pi % 64 < 32)).sum())
                assert n >= 0.9 * hit, (fault, n, hit)
            if fault == "unmasked_tail" and variant == "negative":
                assert n == F                                              # every query would answer 0.0 from a row past the end
    if F == N:
        assert every_row.all()                                             # every row is some query's winner
    assert changed["swap_halves"] > 0
    assert changed["drop_chunk"] > 0 or N < 17 or (N, F) == (4097, 1)
    assert changed["unmasked_tail"] > 0 or (N, F) != (63, 63)


# ---------------------------------------------------------------- B
def _ratios(fam, got):
    out = {}
    for p, v in zip(fam, np.asarray(got, np.float64)):
        r = abs(v - p.d) / cr.eps_bound(p.q, p.g, p.full)
        if p.exact and v != p.d:
            r = max(r, 2.0)                                                # required bit-exact
        out[p.name] = r
    return out


def test_bound_holds_for_a_float32_model_and_each_fault_breaks_a_family():
    fam = cr.eps_families()
    assert {p.family for p in fam} == {1, 2, 3, 4} and len({p.name for p in fam}) == len(fam)
    Q, G = np.stack([p.q for p in fam]), np.stack([p.g for p in fam])
    good = _ratios(fam, cr.emulate_dot(Q, G))
    assert max(good.values()) <= 1.0
    by = lambda r, k: max(v for p, v in zip(fam, r.values()) if p.family == k)         # noqa: E731
    assert by(good, 1) > 0.9                                               # the conversion term is approached, not merely respected
    assert by(good, 2) > 0.6                                               # and the subnormal term
    broke = {}
    for fault in cr.DOT_FAULTS:
        r = _ratios(fam, cr.emulate_dot(Q, G, fault))
        broke[fault] = sorted({p.family for p in fam if r[p.name] > 1.0})
    assert broke["flush"] == [2] and broke["window13"] == [3] and set(broke["trunc"]) == {1, 2}, broke
    # the 13-bit window is caught at s = 14 .. 18, at every position of the large product, with and without cancellation
    r = _ratios(fam, cr.emulate_dot(Q, G, "window13"))
    caught = sorted({p.s for p in fam if p.family == 3 and r[p.name] > 1.0})
    assert caught == [14, 15, 16, 17, 18]
    assert all(r[p.name] > 1.0 for p in fam if p.family == 3 and p.s in (14, 18))


def test_the_formula_is_the_kernels():
    """eps of the certificate >= the bound of the families at Gmax = |g|: c = 1.125 covers (2u + u^2) + 2^-14 (...) in units of 2^-10"""
    u = cr.U
    assert ((2 * u + u * u) + 2.0 ** -14 * (1 + u) ** 2 * (1 + 2.0 ** -14)) / 2.0 ** -10 < 1.125
    for nq, ng in ((1.0, 1.0), (300.0, 1.0), (1e-3, 50.0)):
        q = np.zeros(512); q[0] = nq
        g = np.zeros(512); g[0] = ng
        assert cr.eps_bound(q, g) < cr.cert_eps(nq, ng)


# ---------------------------------------------------------------- C
def test_row_constructions():
    assert float(np.float16(cr.PA)) == cr.P16 and cr.PA > cr.P16 + 2e-4                       # A ties B coarsely, beats it exactly
    assert float(np.float16(cr.QC)) > cr.QC * (1 + 0.95 * cr.U)                               # the query's second element rounds up by nearly u
    assert float(np.float16(cr.X0)) == cr.X0 and float(np.float16(cr.X1)) == cr.X1
    cx, ex = cr.X0 + float(np.float16(cr.QC)) * cr.X1, cr.X0 + cr.QC * cr.X1
    eps = cr.cert_eps(np.sqrt(1 + cr.QC ** 2), 1.0)
    assert cx > cr.P16 + 1e-4 and ex < cr.PA - 1e-4 and abs(cx - ex) < eps and cr.PA - cr.P16 < eps    # far above f32 noise, below eps
    assert cr.PC - cr.P16 > 2 * eps                                                            # the positive controls' gap


@pytest.mark.parametrize("name", cr.TOPK_GROUPS)
def test_expected_flags_and_each_mutant_certifies_a_wrong_list(name):
    grp = cr.topk_group(name)
    assert (grp.plan.nranges, grp.plan.rows_per_range) == ((171, 192) if name == "partial" else (256, 128))
    G = cr.topk_gallery(grp)
    assert np.abs(G @ grp.Q.T)[[r for r in range(0, grp.N, 97) if r not in grp.rows]].max() == 0      # the background scores exactly 0
    assert np.linalg.norm(G.astype(np.float64), axis=1).max() == 1.0                                   # Gmax
    matching = {1: "drop_door", 2: "drop_insert", 3: "drop_pushed", 4: "read_c_plus_2"}
    for f, c in enumerate(grp.cases):
        truth = cr.topk_truth(grp, f, c.K)
        flag, rows, info = cr.emulate_topk(grp, f, c.K)
        if c.control:
            assert flag == 0 and rows == truth and info.gap > 2 * cr.cert_eps(np.linalg.norm(grp.Q[f]), 1.0)
            f2, r2, _ = cr.emulate_topk(grp, f, c.K, "read_c")
            assert (f2 == 1) == (c.layout == 4)                            # the bound read one candidate early: sound, but refuses layout 4's control
            continue
        assert flag == 1 and truth[0] == c.a_row and rows != truth        # A is the true top-1 and the lists do not hold it
        for mutant in cr.TOPK_MUTANTS[:4]:
            mflag, mrows, _ = cr.emulate_topk(grp, f, c.K, mutant)
            if mutant == matching[c.layout]:
                assert mflag == 0 and mrows != truth, (c.name, mutant)     # certified, and wrong
            else:
                assert mflag == 1, (c.name, mutant)                        # each case isolates its own path
