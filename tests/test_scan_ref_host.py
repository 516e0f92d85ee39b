"""CPU checks of tests/helpers/scan_ref.py, the instruments of tests/test_gpu_scan_pins.py: the exact f32 fma against rational
arithmetic, the rules against brute force, the structural emulation of the scan passing every case of A - and each planted fault
failing at least one of the GPU test's own cases."""
from fractions import Fraction

import numpy as np
import pytest

from tests.helpers import scan_ref as sr

F32 = np.float32


# ---------------------------------------------------------------- the exact fma
def _round_f32(x):
    """Fraction -> float32, round to nearest even, subnormals kept"""
    if x == 0:
        return F32(0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    q = max(e - 23, -149)
    n = round(a / Fraction(2) ** q)                                # Python rounds a Fraction half to even
    return F32(np.copysign(float(n) * 2.0 ** q, float(x)))


def _fma_cases():
    rng = np.random.default_rng(1)
    a = (rng.standard_normal(3000) * 2.0 ** rng.integers(-20, 21, 3000)).astype(F32)
    b = (rng.standard_normal(3000) * 2.0 ** rng.integers(-20, 21, 3000)).astype(F32)
    c = (rng.standard_normal(3000) * 2.0 ** rng.integers(-20, 21, 3000)).astype(F32)
    c[:1000] = -(a[:1000] * b[:1000]).astype(F32)                  # heavy cancellation: the result is the product's rounding error
    c[1000:1500] = np.nextafter(c[:500], F32(0))
    # sums within 2^-53 (relative) of a float32 midpoint: the float64 sum lands ON the midpoint, the remainder decides
    assert 8384513 * 8392705 == 2 ** 46 + 1
    special = [
        (8384513 * 2.0 ** -35, 8392705 * 2.0 ** -35, 1.0),           # 1 + 2^-24 + 2^-70: above the midpoint -> 1 + 2^-23
        (-8384513 * 2.0 ** -35, 8392705 * 2.0 ** -35, -1.0),
        (2.0 ** -24 * (1 + 2.0 ** -23), 1 - 2.0 ** -23, 1 + 2.0 ** -23),  # 1 + 2^-23 + 2^-24 - 2^-70: below it -> 1 + 2^-23
        (2.0 ** -24 * (1 + 2.0 ** -23), 1 - 2.0 ** -23, 1.0),
        (8384513 * 2.0 ** -35, 8392705 * 2.0 ** -35, 1 + 2.0 ** -23),
        (2.0 ** -24, 1.0, 1.0), (2.0 ** -24, 1.0, 1 + 2.0 ** -23),      # exact ties: to even
        (2.0 ** -100, 2.0 ** -40, 0.0), (2.0 ** -100, 2.0 ** -40, 2.0 ** -149), (2.0 ** -75, 2.0 ** -75, 2.0 ** -149),
        (3 * 2.0 ** -60, 2.0 ** -90, 2.0 ** -149), (1.5, 2.0 ** -126, -(2.0 ** -126)),
    ]
    sp = np.array(special, np.float64).astype(F32)
    assert (sp.astype(np.float64) == np.array(special)).all()
    return np.concatenate([a, sp[:, 0]]), np.concatenate([b, sp[:, 1]]), np.concatenate([c, sp[:, 2]])


def test_fma32_equals_rational_arithmetic():
    a, b, c = _fma_cases()
    got = sr.fma32(a, b, c)
    want = np.array([_round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], F32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)    # double rounding
    assert (naive[-12:-7] != want[-12:-7]).sum() >= 3               # the special cases do tell the two apart
    assert got[-12] == F32(1 + 2.0 ** -23) and got[-10] == F32(1 + 2.0 ** -23) and got[-9] == F32(1.0)


def test_fma2_32_equals_rational_arithmetic():
    a, b, c = _fma_cases()
    rng = np.random.default_rng(2)
    a1, b1 = a[rng.permutation(len(a))], b[rng.permutation(len(b))]
    a1[:500], b1[:500] = -a[:500], b[:500]                         # the two products cancel: the result is c
    got = sr.fma2_32(a, b, a1, b1, c)
    want = np.array([_round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(u)) * Fraction(float(v)) + Fraction(float(z)))
                     for x, y, u, v, z in zip(a, b, a1, b1, c)], F32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(got[:500].view(np.int32), (c[:500] + F32(0)).view(np.int32))


def test_the_emulations_disagree_on_the_probes():
    """every pair of candidate rules differs on at least one probe, so exactly one can match the hardware"""
    E = {n: sr.probe_expect(n).view(np.int32) for n in sr.EMULATIONS}
    names = list(E)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert (E[a] != E[b]).any(), (a, b)
    assert np.array_equal(sr.mfma_order()[:10], [0, 4, 1, 5, 2, 6, 3, 7, 8, 12]) and len(set(sr.mfma_order().tolist())) == 512


def test_float_faults_leave_bit_equality_and_the_emulation_keeps_the_bound():
    Q, G, S64 = sr.float_case()
    Q, G, S64 = Q[:28], G[:120], S64[:28, :120]
    S = sr.chain(Q, G, **sr.EMULATIONS[sr.HW])
    assert (np.abs(S.astype(np.float64) - S64) <= sr.gamma_bound(Q, G)).all()
    order = sr.mfma_order().copy()
    order[300], order[301] = order[301], order[300]                # one element exchanged between neighbouring k
    kw = sr.EMULATIONS[sr.HW]
    for name, other in (("swapped", sr.chain(Q, G, **{**kw, "order": order})), ("dropped", sr.chain(Q, G, **{**kw, "drop_last": True})),
                        ("mul + add", sr.chain(Q, G, **{**kw, "rule": "muladd"}))):
        assert (other.view(np.int32) != S.view(np.int32)).mean() > (0.005 if name == "swapped" else 0.05), name
    V = sr.row_dot_wave8(Q, G)
    assert (sr.row_dot_wave8(Q, G, offsets=(1, 2, 4, 8, 16, 32)).view(np.int32) != V.view(np.int32)).mean() > 0.05
    assert (sr.row_dot_wave8(Q, G, fused=True).view(np.int32) != V.view(np.int32)).mean() > 0.05
    for Dx in (512, 260):                                          # the GPU test's own rows: the pairing shows in several of them
        X = sr.l2norm_case(Dx)
        assert (sr.l2norm_rows(X, offsets=(1, 2, 4, 8, 16, 32)) != sr.l2norm_rows(X)).any(1).sum() >= 3, Dx
    assert (np.abs(V.astype(np.float64) - S64) <= sr.gamma_bound(Q, G)).all()


def test_valu_replays_against_float64():
    rng = np.random.default_rng(4)
    A, B = rng.standard_normal((5, 260)).astype(F32), rng.standard_normal((6, 260)).astype(F32)
    c64 = (A.astype(np.float64) @ B.astype(np.float64).T) / np.outer(np.linalg.norm(A.astype(np.float64), axis=1),
                                                                     np.linalg.norm(B.astype(np.float64), axis=1))
    assert np.abs(sr.cosine_rows(A, B) - c64).max() < 1e-6
    X = rng.standard_normal((7, 260)).astype(F32)
    assert np.abs(sr.l2norm_rows(X) - X / np.linalg.norm(X.astype(np.float64), axis=1, keepdims=True)).max() < 1e-6
    assert np.abs(sr.mean_rows(X) - X.astype(np.float64).mean(0)).max() < 1e-6
    assert np.array_equal(sr.wave_sum(np.arange(64, dtype=F32)[None]), [F32(2016)])


# ---------------------------------------------------------------- the rules
def test_topk_ref_against_a_full_stable_sort():
    rng = np.random.default_rng(5)
    S = (rng.integers(-80, 40, (9, 300)) / 64).astype(F32)          # many ties, scores on both sides of -1
    for K in sr.KS:
        idx, score = sr.topk_ref(S, K, 1000)
        for f in range(9):
            order = sorted(range(300), key=lambda r: (-float(S[f, r]), r))
            order = [r for r in order[:K] if S[f, r] > -1]
            assert idx[f, :len(order)].tolist() == [r + 1000 for r in order] and (idx[f, len(order):] == -1).all()
            assert (score[f, len(order):] == -1).all() and np.array_equal(score[f, :len(order)], S[f, order])
    i, s = sr.first_above_ref(S, -0.5, 1, 7, take=np.array([1, 0] * 4 + [1]))
    assert i[1] == -1 and s[1] == 0 and i[0] == 7 + min(r for r in range(300) if S[0, r] >= -0.5)


# ---------------------------------------------------------------- the structural emulation over the cases of A
def _subset(N, pi):
    """queries of a large every-row-wins case: those whose row lies in the first or last 40 rows, and every 97th"""
    if N <= 257:
        return np.arange(N)
    rows = np.r_[0:40, N - 40:N, 0:N:97]
    return np.flatnonzero(np.isin(pi, rows))


LAP_SUB = np.array([0, 172, 173, 255])                             # queries of the lap case the emulation replays


def _agree(S, **kw):
    """emulation == rules for top-1 and every K"""
    fault = kw.get("fault")
    ref_kw = {k: v for k, v in kw.items() if k in ("row_offset", "mask")}
    bad = []
    for K in (None,) + sr.KS:
        got = sr.emulate_scan(S, K, **kw)
        want = sr.topk_ref(S, K or 1, **ref_kw)
        if K is None:
            want = (want[0][:, 0], want[1][:, 0])
        if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.int32), want[1].view(np.int32))):
            bad.append(K)
    assert fault is not None or not bad, bad
    return bad


@pytest.mark.parametrize("N", sr.WIN_NS)
def test_emulation_passes_every_row_wins(N):
    for p in range(3):
        Q, G, S, pi = sr.win_case(N, p)
        sub = _subset(N, pi)
        _agree(S[sub], row_offset=(1 << 33) + 5 if p == 1 else 0)
        _agree(S[sub], mask=((np.arange(N) + p) % 3 != 0).astype(np.int32)[sub])


def test_emulation_passes_ties_pairs_minus_one_and_the_lap():
    for N in sr.TIE_NS:
        Q, G, S = sr.tie_case(N)
        _agree(S)
        _agree(S[:, sr.shuffled_view(N, N)])
    Q, G, S, pairs, view = sr.pair_case()
    _agree(S)
    _agree(S[:, view])
    Q, G, S = sr.minus_one_case()
    _agree(S, row_offset=(1 << 33) + 5)
    _agree(np.zeros((3, 0), F32))
    Q, G, S, view = sr.lap_case()
    _agree(S[LAP_SUB])
    _agree(S[LAP_SUB][:, view])


def _fault_cases():
    """fault -> the case of the GPU test that must notice it: (S, keyword arguments)"""
    win = lambda N, p=1: sr.win_case(N, p)[2]
    tie = sr.tie_case(1000)[2]
    Qp, Gp, Sp, pairs, vp = sr.pair_case()
    Sm = sr.minus_one_case()[2]
    Ql, Gl, Sl, vl = sr.lap_case()
    return {
        "partial_tile_dropped": (win(33), {}),
        "reg_skipped": (win(64), {}),
        "h1_dropped": (win(8), {}),
        "lap_stride": (Sl[LAP_SUB], {}),
        "lane_ge": (tie, {}),
        "no_row_rule": (tie, {}),
        "insert_equal": (tie, {}),
        "merge_cut_half": (tie, {}),
        "merge_cut_wave": (tie, {}),
        "merge_cut_block": (tie, {}),
        "ge_minus_one": (Sm, {}),
        "slot_returned": (Sp[:, vp], {"slots": vp}),
        "offset_on_empty": (Sm, {"row_offset": (1 << 33) + 5}),
        "mask_ignored": (win(40), {"mask": (np.arange(40) % 3 != 0).astype(np.int32)}),
    }


@pytest.mark.parametrize("fault", sr.FAULTS)
def test_each_planted_fault_fails_a_case_of_the_gpu_test(fault):
    S, kw = _fault_cases()[fault]
    assert not _agree(S, **kw)                                     # the clean emulation passes this case ...
    bad = _agree(S, fault=fault, **kw)
    assert bad, fault                                              # ... the faulty one does not
    if fault in ("lane_ge", "no_row_rule"):
        assert bad == [None]                                       # top-1 faults
    if fault.startswith("merge_cut") or fault == "insert_equal":
        assert None not in bad


def test_pair_faults_by_distance():
    """no_row_rule shows on pairs whose lower row sits in half-wave 1; the lap pairs share a lane, where '>=' for '>' shows"""
    Q, G, S, pairs, view = sr.pair_case()
    got = sr.emulate_scan(S, None, fault="no_row_rule")[0]
    wrong = [(a, d) for f, (a, d) in enumerate(pairs) if got[f] != a]
    assert (37, 4) in wrong or (101, 4) in wrong, wrong
    Ql, Gl, Sl, vl = sr.lap_case()
    sub = np.r_[173:181]
    assert (sr.emulate_scan(Sl[sub], None, fault="lane_ge")[0] >= sr.LAP).all()
