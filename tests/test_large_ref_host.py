"""CPU: the premises of tests/test_gpu_large_offsets.py - the background bound, the planted rows' margins, the list of edge rows - hold
for what tests/helpers/large_ref.py builds.  No device."""
import numpy as np

from tests.helpers import coarse_ref as cr
from tests.helpers import large_ref as lr
from tests.helpers import scan_ref as sr


def test_background_bound_holds_for_the_generators_range():
    """every element in [-2^-7, 2^-7]: the longest row, all elements at an end of the range, stays under 0.177; f16 and e4m3 x 256 keep
    the ends of the range exactly and round monotonically, so no stored element grows; the stored query is at most 1 + 2^-11 (f16) and
    1 + 2^-4 (e4m3) long"""
    worst = np.full((1, 512), lr.AMP, np.float32)
    assert float(np.linalg.norm(worst.astype(np.float64))) == lr.BG_NORM < 0.177
    for kind, unit, bound in (("f16", 1.0, lr.BG_BOUND), ("f8", 256.0, lr.BG_BOUND_F8)):
        assert (np.abs(cr.stored(worst, kind)) == lr.AMP * unit).all() and (np.abs(cr.stored(-worst, kind)) == lr.AMP * unit).all()
        x = np.linspace(-lr.AMP, lr.AMP, 4097, dtype=np.float32)[None, :]
        s = cr.stored(x, kind)
        assert (np.abs(s) <= lr.AMP * unit).all() and (np.diff(s[0]) >= 0).all()
        rel = 2.0 ** -11 if kind == "f16" else 2.0 ** -4
        assert lr.BG_NORM * (1 + rel) < bound
    assert lr.BG_NORM * (1 + 512 * 2.0 ** -24) < lr.BG_BOUND                      # f32: the accumulation's own rounding, gamma_512
    # the e4m3 codes the fp8-only slab is filled with: sign | 0 .. 0x40 decode to |x| <= 2 = 256 * 2^-7
    from tests.helpers import f8_ref as fr
    codes = np.arange(lr.F8_CODE_MAX + 1)
    mag = np.where(codes < 8, codes * 2.0 ** -9, (1 + (codes & 7) / 8) * 2.0 ** ((codes >> 3) - 7.0))
    assert mag.max() == 2.0 == lr.AMP * 256 and (fr.e4m3(mag) == mag).all()


def test_planted_rows_are_far_apart_and_win_by_a_wide_margin():
    pl = lr.plant()
    I = pl.identities.astype(np.float64)
    cross = np.abs(I @ I.T)
    np.fill_diagonal(cross, 0)
    assert cross.max() < 0.3, cross.max()                                          # a wrapped index reads a row that loses widely
    fam = np.zeros(len(pl.rows), bool)
    fam[pl.family] = True
    assert np.abs(pl.P[fam].astype(np.float64) @ I[:-1].T).max() < 0.3             # graded rows against every other identity
    S = pl.S.astype(np.float64)
    best = S.max(1)
    assert (best - lr.BG_BOUND >= 0.5).all()
    for f in range(lr.NQ):
        own = np.flatnonzero(pl.P @ pl.Qn[f] > 0.45)
        rest = np.delete(S[f], own)
        assert rest.max() < 0.3 + 1e-6 and len(own) == (22 if f == pl.GQ else 2 if f in (37, 38) else 1), f
        assert pl.rows[own[0]] == pl.target[f] or f == pl.GQ
    assert np.abs(np.linalg.norm(pl.Qraw.astype(np.float64), axis=1) - pl.factor).max() < 1e-6
    assert pl.factor.min() >= 0.5 and pl.factor.max() <= 2 and (np.abs(pl.factor - 1) > 1e-3).all()
    norms = np.linalg.norm(pl.P.astype(np.float64), axis=1)
    heavy = pl.where[lr.N - 13]
    assert abs(norms[heavy] - lr.HEAVY) < 1e-6 and np.abs(np.delete(norms, heavy) - 1).max() < 1e-6
    # the emulated scores stay within the derived bound of the float64 dot (scan_ref's one tolerance)
    S64 = pl.Qn.astype(np.float64) @ pl.P.astype(np.float64).T
    assert (np.abs(S - S64) <= sr.gamma_bound(pl.Qn, pl.P)).all()


def test_edge_rows_are_what_they_claim():
    assert lr.N == 2 ** 22 + 4173 and lr.N % 32 == 13 and lr.N % 64 == 13
    rows = lr.edge_rows()
    assert len(rows) == 12
    for b, what in ((2 ** 20, 2 ** 31 // 2048), (2 ** 21, 2 ** 32 // 2048), (2 ** 22, 2 ** 31 // 512)):
        assert b == what and {b - 1, b, b + 1} <= set(rows)
    assert 2 ** 22 * 512 * 2 == 2 ** 32                                           # f16: 2^32 bytes at row 2^22
    assert {0, lr.N - 13, lr.N - 1} <= set(rows) and (lr.N - 13) % 64 == 0           # the first row of the last partial tile
    pl = lr.plant()
    assert set(rows) <= set(pl.rows.tolist()) and (np.diff(pl.rows) > 0).all() and pl.rows.max() == lr.N - 1
    for lo, hi in (lr.PAIR_A, lr.PAIR_B, lr.TIE_PAIR):
        assert lo < hi and np.array_equal(pl.P[pl.where[lo]], pl.P[pl.where[hi]])
    assert lr.PAIR_A[0] < 2 ** 22 < lr.PAIR_A[1] and lr.TIE_PAIR[0] < 2 ** 22 < lr.TIE_PAIR[1] and lr.PAIR_B[1] == lr.N - 2
    g = lr.graded_rows()
    assert all(r < 2 ** 20 for r in g[0::2]) and all(r > 2 ** 22 for r in g[1::2]) and len(set(g) | set(pl.rows.tolist())) == len(pl.rows)
    chk = lr.check_rows()
    assert chk.min() == 0 and chk.max() == lr.N - 1 and set(pl.rows.tolist()) <= set(chk.tolist()) and len(chk) > len(pl.rows)
    # both 32-query groups hold queries whose rows lie past every edge
    assert (pl.target[:32] > 2 ** 22).any() and (pl.target[32:] > 2 ** 22).any()


def test_graded_list_and_the_expectations():
    pl = lr.plant()
    idx, score, n = lr.expect_topk(pl.S, pl.rows, 16)
    assert n[pl.GQ] == 16 and (np.delete(n, [37, 38, pl.GQ]) == 1).all() and n[37] == 2 and n[38] == 2
    g = score[pl.GQ].astype(np.float64)
    assert (g >= 0.5).all() and g[-1] > 0.6
    gaps = -np.diff(g)
    tie = np.flatnonzero(gaps == 0)
    assert len(tie) == 1 and (np.delete(gaps, tie) >= 1e-3).all()
    assert (idx[pl.GQ, tie[0]], idx[pl.GQ, tie[0] + 1]) == lr.TIE_PAIR              # the lower row first
    gr = lr.graded_rows()
    assert idx[pl.GQ, :4].tolist() == gr[:4] and idx[pl.GQ, 6] == gr[4]
    assert idx[37, :2].tolist() == list(lr.PAIR_A) and idx[38, :2].tolist() == list(lr.PAIR_B) and score[37, 0] == score[37, 1]
    full = sr.topk_ref(pl.S, 16)
    assert (score[pl.GQ] == full[1][pl.GQ]).all()
    mi, ms = lr.expect_match(pl.S, pl.rows, lr.OFFSET)
    assert np.array_equal(mi, pl.target + lr.OFFSET) and (ms > 0.97).all()
    for inclusive in (0, 1):
        fi, fs = lr.expect_first_above(pl.S1, pl.rows, lr.THR, inclusive)
        want = pl.target.copy()
        want[pl.GQ] = min(lr.graded_rows())                                     # the lowest row that passes, not the best
        assert np.array_equal(fi, want) and (fs > 0.6).all()
    assert not (np.abs(pl.S1 - np.float32(lr.THR)) < 0.05).any()                 # no score near thr: both settings agree


def test_view_case_straddles_slot_2_22_and_only_the_planted_pairs_are_duplicates():
    vc = lr.view_case()
    slots = lr.FIRST_SLOT + np.arange(lr.NIDS)
    assert slots[0] < 2 ** 22 <= slots[-1] and slots[-1] < lr.N
    for a, b in lr.DUPS:
        assert slots[a] < 2 ** 22 < slots[b] and np.array_equal(vc.rows[a], vc.rows[b])
    assert not set(vc.zslots.tolist()) & set(slots.tolist()) and vc.zslots.min() == 0 and vc.zslots.max() == lr.N - 1
    assert (vc.zslots < slots[0]).sum() == 349 and (vc.zslots > slots[-1]).sum() == 351
    assert sorted(map(str, vc.idsA)) == sorted(map(str, vc.ids)) and vc.idsA != vc.ids and len(vc.idsB) == 500
    assert (np.abs(vc.V).sum(1) == 0).sum() == 700
    dots = vc.V.astype(np.float64) @ vc.V.astype(np.float64).T
    above = np.argwhere(np.triu(dots > 0.3, 1))
    assert np.array_equal(above, vc.pairs) and (vc.pair_scores > 0.999).all()     # nothing else comes near thr = 0.4
    win = vc.S.argmax(1)
    assert (vc.S.max(1) > 0.999).all() and [vc.idsA[p] for p in win[4:]] == vc.sel[4:].tolist()
    for f, (a, b) in enumerate(lr.DUPS):                                         # a duplicated row: the lower VIEW position
        pa, pb = vc.idsA.index(a), vc.idsA.index(b)
        assert win[f] == win[f + 2] == min(pa, pb) and vc.S[f, pa] == vc.S[f, pb]
    top = np.sort(vc.S, axis=1)[:, -16:]
    assert (top > 0).all()                                                        # the zero rows never enter a top-16 list


def test_fp8_only_plant():
    pf = lr.plant_f8()
    b = 2 ** 23
    assert lr.N8 == b + 4173 and b * 512 == 2 ** 32
    assert (pf.rows < b).sum() >= 4 and (pf.rows >= b).sum() >= 4 and pf.rows.max() == lr.N8 - 1 and (pf.rows % 4 == 0).all()
    idx, score = lr.expect_coarse_f8(pf.S, pf.rows)
    assert np.array_equal(idx, pf.rows) and (score == np.float32(10.5 / 16)).all()
    cross = pf.S * cr.unscale("f8")
    np.fill_diagonal(cross, 0)
    # a background row as e4m3 codes is at most 2 sqrt(512) long, a planted query sqrt(10.5) * 64
    assert np.abs(cross).max() < 0.3 and 2 * np.sqrt(512) * np.sqrt(10.5) * 64 / 65536 < 0.15 < 10.5 / 16 - 0.5


def test_range_clamp_cases():
    p16 = lr.plant_f16()
    tiles = -(-lr.N16 // 64)
    assert tiles > 8 * 16384 and -(-lr.F16Q // 256) == 32 and lr.CLAMP_ROWS == 16384 * 64      # 256 / 32 = 8 ranges wanted, 9 made
    for e in range(1, 9):
        assert {(e << 20) - 4, e << 20} <= set(p16.rows.tolist())
    idx, score = lr.expect_coarse_f16(p16.S, p16.rows, lr.F16Q)
    assert np.array_equal(idx[:len(p16.rows)], p16.rows) and (score == np.float32(10.5 / 16)).all() and len(idx) == lr.F16Q
    cross = p16.S.copy()
    np.fill_diagonal(cross, 0)
    assert np.abs(cross).max() < 0.3 and np.sqrt(10.5 / 16) * lr.BG_NORM * (1 + 2.0 ** -11) < 0.15 < 10.5 / 16 - 0.5
    pp = lr.plant_pairs()
    assert -(-lr.NP // 64) > 16384 and (pp.pairs[:, 0] < lr.CLAMP_ROWS).all() and (pp.pairs[:, 1] >= lr.CLAMP_ROWS).all()
    assert (np.diff(pp.pairs[:, 0]) > 0).all() and len(set(pp.rows.tolist())) == 10 and pp.rows.max() == lr.NP - 1
    dots = pp.U.astype(np.float64) @ pp.U.astype(np.float64).T
    assert np.abs(dots - np.eye(5)).max() < 0.3 and (pp.scores > 0.999).all()                      # thr 0.4: only the copies pass
    assert lr.BG_NORM * 1.0001 < lr.THR - 0.05 and lr.BG_NORM ** 2 < 0.04
