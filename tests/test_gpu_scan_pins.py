"""Pins for the exact f32 gallery scans (csrc/match.hip, match_scan.h, match_topk.hip, topk_list.h) and the first-hit consumers, through
the C entries with raw Q (no GalleryMatcher: it renormalises).  docs/KERNEL_NOTES.md 4.15 is the long form.

A. Operands on an exact grid (multiples of 2^-3, |x| <= 2: every partial sum exact in f32 in any order): indices AND score bits with
   torch.equal against tests/helpers/scan_ref.py - every row the winner of some query at every residue of the 32-row tile, one to four
   waves, one and many blocks, the second lap of the grid-stride loop; dense ties with hundreds of tied rows per query at every K;
   tie pairs at the distance of each merge level, in both memory orders; the '> -1' rule; the first-hit scans.
B. Float operands: the scores equal an emulation of v_mfma_f32_32x32x2_f32 (scan_ref.HW) bit for bit, the listed rows are that emulation's
   own ranking; |s - q.g| <= gamma_512 sum |q_k g_k| is the one tolerance, and it is derived.
C. The VALU consumers (first-hit dot, cosine, mean, l2norm, unit row) equal their NumPy float32 replay bit for bit.
Every output is prefilled with a sentinel (NaN scores, -7 indices).  tests/test_scan_ref_host.py shows on the CPU that these instruments
fail planted faults."""
import numpy as np
import pytest
import torch

from tests.helpers import scan_ref as sr

pytestmark = pytest.mark.gpu
IDX_FILL = -7
SCORE_FILL = 0x7FC0BEEF                                                    # a NaN no kernel produces
OFFSET = (1 << 33) + 5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _outputs(*shape):
    idx = torch.full(shape, IDX_FILL, dtype=torch.int64, device="cuda")
    score = torch.full(shape, SCORE_FILL, dtype=torch.int32, device="cuda").view(torch.float32)
    return idx, score


def _same(got, want):
    """indices and score bits, both with torch.equal"""
    wi, ws = torch.from_numpy(np.ascontiguousarray(want[0])), torch.from_numpy(np.ascontiguousarray(want[1]).view(np.int32))
    gi, gs = got[0].cpu(), _bits(got[1]).cpu()
    assert gi.shape == wi.shape and gs.shape == ws.shape
    return torch.equal(gi, wi) and torch.equal(gs, ws)


def _diff(got, want):
    return (int((got[0].cpu().numpy() != want[0]).sum()), int((_bits(got[1]).cpu().numpy() != want[1].view(np.int32)).sum()))


def _match(lib, Qd, Gd, N, row_offset=0, view=None):
    from facerecognition_infrenceengine_amd import _lib
    F = Qd.shape[0]
    need = lib.fr_gallery_match_workspace(F, N)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    idx, score = _outputs(F)
    if view is None:
        lib.fr_gallery_match_f32(_lib.ptr(Qd), _lib.ptr(Gd), F, N, 512, row_offset, _lib.ptr(idx), _lib.ptr(score), _lib.ptr(ws), need,
                                 None, 0, _lib.stream_ptr())
    else:
        assert row_offset == 0
        lib.fr_gallery_match_view_f32(_lib.ptr(Qd), _lib.ptr(Gd), _lib.ptr(view), F, N, 512, _lib.ptr(idx), _lib.ptr(score),
                                      _lib.ptr(ws), need, _lib.stream_ptr())
    return idx, score


def _topk(lib, Qd, Gd, N, K, row_offset=0, view=None, mask=None):
    from facerecognition_infrenceengine_amd import _lib
    F = Qd.shape[0]
    need = lib.fr_gallery_topk_workspace(F, N, K)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    idx, score = _outputs(F, K)
    if mask is not None:
        lib.fr_gallery_topk_view_masked_f32(_lib.ptr(Qd), _lib.ptr(Gd), _lib.ptr(view), F, N, 512, K, _lib.ptr(idx), _lib.ptr(score),
                                            _lib.ptr(ws), need, _lib.ptr(mask), _lib.stream_ptr())
    elif view is not None:
        assert row_offset == 0
        lib.fr_gallery_topk_view_f32(_lib.ptr(Qd), _lib.ptr(Gd), _lib.ptr(view), F, N, 512, K, _lib.ptr(idx), _lib.ptr(score),
                                     _lib.ptr(ws), need, _lib.stream_ptr())
    else:
        lib.fr_gallery_topk_f32(_lib.ptr(Qd), _lib.ptr(Gd), F, N, 512, K, row_offset, _lib.ptr(idx), _lib.ptr(score), _lib.ptr(ws), need,
                                None, 0, _lib.stream_ptr())
    return idx, score


def _prefix(ref16, K, row_offset=0):
    """the reference list of length K is the first K entries of the reference list of length 16 (one total order, one '> -1' cut)"""
    idx = ref16[0][:, :K]
    return np.where(idx >= 0, idx + row_offset, -1), ref16[1][:, :K]


def _check_all_entries(lib, Qd, Gd, S, view=None, offset=0, tag=None):
    """top-1 and every K of the plain (view None) or view entries against the rules over S (scores in scan order)"""
    N = S.shape[1]
    ref16 = sr.topk_ref(S, 16)
    got, want = _match(lib, Qd, Gd, N, offset, view), _prefix(ref16, 1, offset)
    want = (want[0][:, 0], want[1][:, 0])
    assert _same(got, want), (tag, "match", _diff(got, want))
    for K in sr.KS:
        got, want = _topk(lib, Qd, Gd, N, K, offset, view), _prefix(ref16, K, offset)
        assert _same(got, want), (tag, "topk", K, _diff(got, want))
    return ref16


# ---------------------------------------------------------------- A.1 every row wins
@pytest.mark.parametrize("N", sr.WIN_NS)
def test_every_row_wins(lib, N):
    """F = N, query f = row pi(f) under three permutations: each row must come back as the winner with |row|^2 = 10.5, and the top-K lists
    over the same galleries (cross-scores tie densely at 0) equal the reference.  The view form reads the rows out of order from a slab
    with NaN slots and two decoys that would win; the masked form reports (-1, -1.0) for masked-out queries."""
    G, S0 = sr.win_gallery(N)
    Gd = _dev(G)
    slab, view = sr.view_slab(G, S0, N)
    slabd, viewd = _dev(slab), _dev(view)
    for p in range(3):
        Q, _, S, pi = sr.win_case(N, p)
        Qd = _dev(Q)
        ref16 = _check_all_entries(lib, Qd, Gd, S, None, OFFSET if p == 1 else 0, ("plain", p))
        assert np.array_equal(ref16[0][:, 0], pi) and (ref16[1][:, 0] == sr.SELF).all()
        _check_all_entries(lib, Qd, slabd, S, viewd, 0, ("view", p))
        mask = ((np.arange(N) + p) % 3 != 0).astype(np.int32)
        maskd = _dev(mask)
        for K in sr.KS:
            got = _topk(lib, Qd, slabd, N, K, 0, viewd, maskd)
            want = _prefix(ref16, K)
            want = (np.where(mask[:, None] > 0, want[0], -1), np.where(mask[:, None] > 0, want[1], np.float32(-1.0)))
            assert _same(got, want), ("masked", p, K, _diff(got, want))


# ---------------------------------------------------------------- A.2 the second lap
@pytest.fixture(scope="module")
def lap(lib):
    Q, G, S, view = sr.lap_case()
    return Q, _dev(Q), _dev(G), S, view


def test_second_lap_rows_win_and_tie_with_the_first_lap(lib, lap):
    """N = 131072 + 173: rows 131072 .. 131244 each win one query; 83 queries tie a first-lap row with the row one lap on (same block,
    wave, lane and register): the first-lap row is listed first.  Through the view with each tied pair exchanged in memory the list is
    still ordered by view position."""
    Q, Qd, Gd, S, view = lap
    ref16 = _check_all_entries(lib, Qd, Gd, S, None, 0, "lap")
    assert (ref16[0][:173, 0] >= sr.LAP).all() and (ref16[0][173:, 1] == ref16[0][173:, 0] + sr.LAP).all()
    _check_all_entries(lib, Qd, Gd, S, None, OFFSET, "lap+offset")
    refv = _check_all_entries(lib, Qd, Gd, S[:, view], _dev(view), 0, "lap view")
    assert np.array_equal(refv[0][173:, :2], ref16[0][173:, :2]) and (view[ref16[0][173:, 0]] == ref16[0][173:, 1]).all()


# ---------------------------------------------------------------- A.3 dense ties
@pytest.mark.parametrize("N", sr.TIE_NS)
def test_dense_ties_list_the_lowest_rows(lib, N):
    """7 row patterns with period 7: >= N / 7 rows share every query's top score, far more than K.  The list is the K lowest rows; through
    a permuted view it is the K lowest view positions."""
    Q, G, S = sr.tie_case(N)
    Qd, Gd = _dev(Q), _dev(G)
    ref16 = _check_all_entries(lib, Qd, Gd, S, None, 0, "plain")
    assert all(ref16[0][f].tolist() == list(range(f, f + 7 * 16, 7)) for f in range(7))
    view = sr.shuffled_view(N, N)
    refv = _check_all_entries(lib, Qd, Gd, S[:, view], _dev(view), 0, "view")
    assert all((view[refv[0][f]] % 7 == f).all() and (np.diff(refv[0][f]) > 0).all() for f in range(7))


def test_tie_pairs_at_every_merge_distance(lib, lap):
    """Two rows tie above all others at distance +1, +4 (other half-wave), +8 (next register group), +32 (next wave), +128 (next block),
    with the lower row in either half-wave; +131072 (next lap) is the lap gallery's.  Once as stored, once through a view that exchanges
    the two rows in memory: the lower POSITION is listed first either way."""
    Q, G, S, pairs, view = sr.pair_case()
    Qd, Gd = _dev(Q), _dev(G)
    want2 = np.array([[a, a + d] for a, d in pairs])
    ref16 = _check_all_entries(lib, Qd, Gd, S, None, 0, "stored")
    assert np.array_equal(ref16[0][:, :2], want2)
    refv = _check_all_entries(lib, Qd, Gd, S[:, view], _dev(view), 0, "exchanged")
    assert np.array_equal(refv[0][:, :2], want2) and np.array_equal(view[want2[:, 0]], want2[:, 1])
    # the next lap: queries 173 .. 255 of the lap gallery, alone (F = 83: partial query group)
    Ql, _, Gld, Sl, viewl = lap
    _check_all_entries(lib, _dev(Ql[173:]), Gld, Sl[173:], None, 0, "lap pairs")
    _check_all_entries(lib, _dev(Ql[173:]), Gld, Sl[173:][:, viewl], _dev(viewl), 0, "lap pairs exchanged")


# ---------------------------------------------------------------- A.4 the '> -1' rule
def test_rows_at_or_below_minus_one_are_never_listed(lib):
    """Query f has exactly f rows above -1 (scores -0.875, -0.5, -0.25) among rows at -1 and -1.125: f < K leaves the tail (-1, -1.0), a best
    score of exactly -1 reports (-1, -1.0), -0.875 is listed; row_offset is added to real rows only; N = 0 reports (-1, -1.0) throughout."""
    Q, G, S = sr.minus_one_case()
    Qd, Gd = _dev(Q), _dev(G)
    for off, view in ((0, None), (OFFSET, None), (0, sr.shuffled_view(len(G), 3))):
        Sv = S if view is None else S[:, view]
        ref16 = _check_all_entries(lib, Qd, Gd, Sv, None if view is None else _dev(view), off, ("minus one", off))
        assert ((ref16[0] >= 0).sum(1) == np.minimum(np.arange(len(Q)), 16)).all()
        assert ref16[0][0, 0] == -1 and ref16[1][0, 0] == -1.0 and ref16[1][1, 0] == np.float32(-0.875)
    empty = np.zeros((len(Q), 0), np.float32)
    _check_all_entries(lib, Qd, None, empty, None, OFFSET, "N = 0")
    _check_all_entries(lib, Qd, Gd, empty, _dev(np.zeros(1, np.int64)), 0, "Nview = 0")
    mask = _dev(np.ones(len(Q), np.int32))
    got = _topk(lib, Qd, Gd, 0, 5, 0, _dev(np.zeros(1, np.int64)), mask)
    assert _same(got, sr.topk_ref(empty, 5))


# ---------------------------------------------------------------- A.5 first hit
def _first_above(lib, Qd, Gd, N, thr, inclusive, row_offset=0, blocked=False, view=None, take=None):
    from facerecognition_infrenceengine_amd import _lib
    F = Qd.shape[0]
    ws = torch.empty(F * 8, dtype=torch.uint8, device="cuda")
    idx, score = _outputs(F)
    if blocked:
        lib.fr_gallery_first_above_blocked_f32(_lib.ptr(Qd), _lib.ptr(Gd), _lib.ptr(view), _lib.ptr(take), F, N, 512, float(thr),
                                               inclusive, row_offset, _lib.ptr(idx), _lib.ptr(score), _lib.ptr(ws), F * 8,
                                               _lib.stream_ptr())
    else:
        lib.fr_gallery_first_above_f32(_lib.ptr(Qd), _lib.ptr(Gd), F, N, 512, float(thr), inclusive, row_offset, _lib.ptr(idx),
                                       _lib.ptr(score), _lib.ptr(ws), F * 8, _lib.stream_ptr())
    return idx, score


def _check_first_hit(lib, Q, G, S, thrs, slab=None, view=None, tag=None):
    """both first-hit entries (plain; blocked plain / view / take) against the plain loop over the float32 scores S"""
    N, F = len(G), len(Q)
    Qd, Gd = _dev(Q), _dev(G)
    slabd, viewd = (None, None) if view is None else (_dev(slab), _dev(view))
    take = (np.arange(F) % 4 != 1).astype(np.int32)
    taked = _dev(take)
    hits = 0
    for thr in thrs:
        for inclusive in (0, 1):
            want = sr.first_above_ref(S, thr, inclusive)
            hits += int((want[0] >= 0).sum())
            got = _first_above(lib, Qd, Gd, N, thr, inclusive)
            assert _same(got, want), (tag, "plain", thr, inclusive, _diff(got, want))
            got = _first_above(lib, Qd, Gd, N, thr, inclusive, blocked=True)
            assert _same(got, want), (tag, "blocked", thr, inclusive, _diff(got, want))
            wo = sr.first_above_ref(S, thr, inclusive, OFFSET, take)
            got = _first_above(lib, Qd, Gd, N, thr, inclusive, OFFSET, blocked=True, take=taked)
            assert _same(got, wo), (tag, "blocked take", thr, inclusive, _diff(got, wo))
            got = _first_above(lib, Qd, Gd, N, thr, inclusive, OFFSET)
            wo = sr.first_above_ref(S, thr, inclusive, OFFSET)
            assert _same(got, wo), (tag, "plain offset", thr, inclusive, _diff(got, wo))
            if view is not None:
                got = _first_above(lib, Qd, slabd, N, thr, inclusive, blocked=True, view=viewd)
                assert _same(got, want), (tag, "blocked view", thr, inclusive, _diff(got, want))
    return hits


@pytest.mark.parametrize("N", sr.FIRST_NS)
def test_first_hit_on_the_grid(lib, N):
    """thr equal to a reachable score, inclusive 0 and 1: first passing position against a plain loop, score bits exact, (-1, 0.f) when
    nothing passes.  At thr = 10.5 only the target row passes, and only inclusively: targets in each wave of a block and in the last
    row.  F = 1, 15, 16, 17, 33: partial query blocks of the blocked form."""
    for F in sr.FIRST_FS:
        Q, G, S, targets, thrs = sr.first_case(N, F)
        slab, view = sr.view_slab(G, sr.win_gallery(N)[1], 50 + N)
        assert len(Q) == F and targets[0] == N - 1 and (N < 100 or len(thrs) == 4)
        want = sr.first_above_ref(S, thrs[0], 1)
        assert np.array_equal(want[0], targets) and (sr.first_above_ref(S, thrs[0], 0)[0] == -1).all()
        _check_first_hit(lib, Q, G, S, thrs, slab, view, (N, F))


# ---------------------------------------------------------------- B. the score's bits on float operands
def _probe_scores(lib, cases):
    """every (name, q, g) pair through fr_gallery_match_f32: N = 32, the pair's row at a varying position, every other row scoring -4
    (never listed); pairs that share a gallery row go in launches of up to 32 queries"""
    got = np.zeros(len(cases), np.float32)
    groups = {}
    for c, (_, q, g) in enumerate(cases):
        groups.setdefault(g.tobytes(), []).append(c)
    launch = 0
    sizes = set()
    for members in groups.values():
        for at in range(0, len(members), 32):
            chunk = members[at:at + 32]
            row = (7 * launch + 3) % 32
            launch += 1
            G = np.zeros((32, 512), np.float32)
            G[:, 511] = -4.0
            G[row] = cases[chunk[0]][2]
            Q = np.stack([cases[c][1] for c in chunk])
            idx, score = _match(lib, _dev(Q), _dev(G), 32)
            assert idx.tolist() == [row] * len(chunk)
            got[chunk] = score.cpu().numpy()
            sizes.add(len(chunk))
    return got, sizes


def test_probe_what_the_f32_matrix_instruction_computes(lib):
    """big + small - big in the two k slots of one instruction, in neighbouring instructions, 8 elements apart; half-ulp ties; subnormal
    products, operands and sums.  The hardware follows exactly one of the emulations: scan_ref.HW."""
    got, sizes = _probe_scores(lib, sr.probe_cases())
    assert {1, 32} <= sizes
    got = got.view(np.int32)
    miss = {name: int((sr.probe_expect(name).view(np.int32) != got).sum()) for name in sr.EMULATIONS}
    print("\nprobe mismatches per emulation:", miss)
    if miss[sr.HW]:
        bad = np.flatnonzero(sr.probe_expect(sr.HW).view(np.int32) != got)
        cases = sr.probe_cases()
        print([(cases[c][0], float(got.view(np.float32)[c]), float(sr.probe_expect(sr.HW)[c])) for c in bad[:12]])
    assert miss[sr.HW] == 0 and all(n > 0 for name, n in miss.items() if name != sr.HW), miss


def test_float_scores_equal_the_emulation_bit_for_bit(lib):
    """Gaussian unit rows, queries off unit length, heavy cancellation and magnitudes spread over 2^+-20, N = 300, F = 40: the scores of
    the plain, view and top-K entries equal the emulation bit for bit and the listed rows are the emulation's own ranking; every listed
    score lies within gamma_512 sum |q_k g_k| of the float64 product."""
    Q, G, S64 = sr.float_case()
    S = sr.chain(Q, G, **sr.EMULATIONS[sr.HW])
    bound = sr.gamma_bound(Q, G)
    ratio = np.abs(S.astype(np.float64) - S64) / bound
    print("\nworst |emulation - float64| / bound over all pairs: %.4f" % ratio.max())
    assert ratio.max() <= 1.0
    Qd, Gd = _dev(Q), _dev(G)
    _check_all_entries(lib, Qd, Gd, S, None, 0, "float")
    view = sr.shuffled_view(len(G), 9)
    _check_all_entries(lib, Qd, Gd, S[:, view], _dev(view), 0, "float view")
    idx, score = _topk(lib, Qd, Gd, len(G), 16)
    idx, score = idx.cpu().numpy(), score.cpu().numpy().astype(np.float64)
    f = np.arange(len(Q))[:, None]
    listed = idx >= 0
    worst = (np.abs(score - S64[f, np.maximum(idx, 0)]) / bound[f, np.maximum(idx, 0)])[listed].max()
    print("worst |score - float64| / bound over the listed scores: %.4f" % worst)
    assert worst <= 1.0 and listed.sum() > 16 * 30


def test_adversarial_pairs_equal_the_emulation_bit_for_bit(lib):
    """heavy cancellation (float64 dot below 1e-6 of sum |q g|) and element magnitudes spread over 2^+-20: each pair alone in a gallery of
    its own, so its score is the one reported - equal to the emulation bit for bit and within the derived bound of the float64 dot"""
    cases = sr.adversarial_pairs()
    got, _ = _probe_scores(lib, cases)
    Q, G = np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])
    want = sr.chain(Q, G, pairwise=True, **sr.EMULATIONS[sr.HW])
    assert (want > -1).all()
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), [cases[c][0] for c in np.flatnonzero(got != want)]
    q64, g64 = Q.astype(np.float64), G.astype(np.float64)
    ratio = np.abs(got - (q64 * g64).sum(1)) / (sr.GAMMA512 * (np.abs(q64) * np.abs(g64)).sum(1))
    print("\nworst |score - float64| / bound over the adversarial pairs: %.4f (cancellation), %.4f (spread)"
          % (ratio[:24].max(), ratio[24:].max()))
    assert ratio.max() <= 1.0


# ---------------------------------------------------------------- C. the VALU consumers
def test_first_hit_scores_equal_numpy_float32(lib):
    """eight rounded products left to right per lane, wave_sum at xor 32 .. 1: fr_gallery_first_above_f32 and the blocked form return
    those bits, and the first passing row is the first under those same float32 scores - thr between scores and exactly on one"""
    Q, G, _ = sr.float_case()
    S = sr.row_dot_wave8(Q, G)
    slab, view = sr.view_slab(G, None, 8)
    thrs = [0.05, 0.1, float(S[3, 7]), float(S[25, 101]), float(np.sort(S[30])[-1]), -0.02]
    hits = _check_first_hit(lib, Q, G, S, thrs, slab, view, "float")
    assert hits > 40 * 8


@pytest.mark.parametrize("Dx", [512, 260, 100])
def test_cosine_matrix_equals_numpy_float32(lib, Dx):
    from facerecognition_infrenceengine_amd import _lib
    rng = np.random.default_rng(Dx)
    A = (rng.standard_normal((9, Dx)) * 2.0 ** rng.integers(-3, 4, (9, 1))).astype(np.float32)
    B = rng.standard_normal((21, Dx)).astype(np.float32)
    B[0] = A[0]
    Ad, Bd = _dev(A), _dev(B)
    out = torch.full((9, 21), SCORE_FILL, dtype=torch.int32, device="cuda").view(torch.float32)
    lib.fr_cosine_matrix_f32(_lib.ptr(Ad), _lib.ptr(Bd), 9, 21, Dx, _lib.ptr(out), _lib.stream_ptr())
    want = sr.cosine_rows(A, B)
    assert torch.equal(_bits(out).cpu(), torch.from_numpy(want.view(np.int32))), int((out.cpu().numpy() != want).sum())


@pytest.mark.parametrize("K", [1, 2, 7])
def test_mean_rows_equals_numpy_float32(lib, K):
    from facerecognition_infrenceengine_amd import _lib
    X = np.random.default_rng(K).standard_normal((K, 515)).astype(np.float32)
    Xd = _dev(X)
    out = torch.full((515,), SCORE_FILL, dtype=torch.int32, device="cuda").view(torch.float32)
    lib.fr_mean_rows_f32(_lib.ptr(Xd), K, 515, _lib.ptr(out), _lib.stream_ptr())
    assert torch.equal(_bits(out).cpu(), torch.from_numpy(sr.mean_rows(X).view(np.int32)))


@pytest.mark.parametrize("Dx", [512, 260])
def test_l2norm_rows_equals_numpy_float32(lib, Dx):
    """and fr_gallery_update_rows_f32(normalise=1) at D = 512: the header says the same bits as fr_l2norm_rows_f32 - both asserted"""
    from facerecognition_infrenceengine_amd import _lib
    X = sr.l2norm_case(Dx)
    R = len(X)
    Xd = _dev(X)
    out = torch.full((R, Dx), SCORE_FILL, dtype=torch.int32, device="cuda").view(torch.float32)
    lib.fr_l2norm_rows_f32(_lib.ptr(Xd), _lib.ptr(out), R, Dx, _lib.stream_ptr())
    want = torch.from_numpy(sr.l2norm_rows(X).view(np.int32))
    assert torch.equal(_bits(out).cpu(), want)
    if Dx == 512:
        slab = torch.full((R + 5, 512), SCORE_FILL, dtype=torch.int32, device="cuda").view(torch.float32)
        slots = np.random.default_rng(1).permutation(R + 5)[:R].astype(np.int64)
        slotsd = _dev(slots)
        lib.fr_gallery_update_rows_f32(_lib.ptr(slab), _lib.ptr(slotsd), _lib.ptr(Xd), R, 512, 1, _lib.stream_ptr())
        assert torch.equal(_bits(slab[slotsd]), _bits(out)) and torch.equal(_bits(slab[slotsd]).cpu(), want)
        untouched = np.setdiff1d(np.arange(R + 5), slots)
        assert bool((_bits(slab)[_dev(untouched)] == SCORE_FILL).all())
