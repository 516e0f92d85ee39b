"""The gallery audit's references (tests/helpers/pairs_ref.py) hold on their own, on the CPU: the cases are what they are named after,
the structured emulation of the audit equals the plain loop, and every planted fault changes the answer on the cases."""
import functools

import numpy as np
import pytest

from tests.helpers import pairs_ref as pr
from tests.helpers import scan_ref as sr

F32 = np.float32


@pytest.mark.parametrize("N", pr.GRID_NS)
def test_grid_cases_and_emulation(N):
    c = pr.grid_case(N)
    for thr in pr.GRID_THRS:
        for inclusive in (False, True):
            ref = pr.pairs_ref(c.G, thr, inclusive, S=c.S)
            assert pr.same(pr.emulate(c.G, thr, inclusive, S=c.S, C=c.S.astype(np.float64)), ref)
            assert (ref[0][:, 0] < ref[0][:, 1]).all() and len(ref[0]) == len(np.unique(ref[0], axis=0))
            if N <= 1:
                assert len(ref[0]) == 0
        strict, incl = pr.pairs_ref(c.G, thr, False, S=c.S), pr.pairs_ref(c.G, thr, True, S=c.S)
        on = int((c.S[np.triu_indices(N, 1)] == F32(thr)).sum())
        assert len(incl[0]) - len(strict[0]) == on
        low, high, at = pr.candidates_ref(c.G, thr, c.S.astype(np.float64))
        assert low == high == at == len(incl[0])           # eps < 2^-6: the candidates are exactly the pairs at or above thr


def test_grid_300_counts():
    """what the issue found at N = 300: thousands of exact ties on either threshold"""
    up = pr.grid_case(300).S[np.triu_indices(300, 1)]
    assert [(int((up > t).sum()), int((up == t).sum())) for t in pr.GRID_THRS] == [(3645, 2669), (841, 1318)]


def test_pairs_ref_is_the_first_hit_rule():
    """for every b, first_above over the rows before b names min(partners of b): the audit and the duplicate check agree by definition"""
    c = pr.grid_case(130)
    pairs, scores = pr.pairs_ref(c.G, 0.5, False, S=c.S)
    idx, score = sr.first_above_ref(c.S, 0.5, False)
    for b in range(c.N):
        part = [(a, s) for (a, bb), s in zip(pairs, scores) if bb == b] + [(bb, s) for (a, bb), s in zip(pairs, scores) if a == b]
        first = min([a for a, _ in part] + [b])                   # the row itself scores 10.5
        assert idx[b] == first
        if first != b:
            assert dict(part)[first] == score[b]


def test_float_case_and_emulation():
    c = pr.float_case()
    st = c.stats
    print(vars(st))
    assert c.N == 870 and st.max_err <= st.eps < 2e-3
    for inclusive in (False, True):
        ref = pr.pairs_ref(c.G, c.thr, inclusive, S=c.S)
        assert pr.same(pr.emulate(c.G, c.thr, inclusive, S=c.S, C=c.C), ref)
    assert len(pr.pairs_ref(c.G, c.thr, True, S=c.S)[0]) == st.passing + st.on_thr


def test_eps_is_the_certificates_bound():
    """eps of the audit = cert_eps of DESIGN.md 4.6b with |q| = Gmax, evaluated in f32"""
    from tests.helpers import coarse_ref as cr
    for g in (1.0, float(np.sqrt(10.5)), 300.0, 1e-3):
        g = float(F32(g))
        assert abs(float(pr.eps_of(g)) - cr.cert_eps(g, g)) <= 2.0 ** -22 * cr.cert_eps(g, g)
        assert pr.t_lo_of(0.4, g) == F32(F32(0.4) - pr.eps_of(g))


@functools.lru_cache(maxsize=None)
def _ref(case, inclusive):
    """the reference of the two cases the faults are planted on, computed once"""
    c, thr = (pr.grid_case(300), 0.5) if case == "grid" else (pr.float_case(), 0.4)
    return pr.pairs_ref(c.G, thr, inclusive, S=c.S)


@pytest.mark.parametrize("fault", pr.FAULTS)
def test_every_planted_fault_changes_the_answer(fault):
    hit = 0
    g, f = pr.grid_case(300), pr.float_case()
    for case, G, S, C, thr in (("grid", g.G, g.S, g.S.astype(np.float64), 0.5), ("float", f.G, f.S, f.C, f.thr)):
        for inclusive in (False, True):
            hit += not pr.same(pr.emulate(G, thr, inclusive, fault=fault, S=S, C=C), _ref(case, inclusive))
    assert hit > 0, fault
    if fault in ("filter_at_thr", "float64_decision"):         # the float case is what these two are for
        ref = _ref("float", False)
        got = pr.emulate(f.G, f.thr, False, fault=fault, S=f.S, C=f.C)
        lost = len(set(map(tuple, ref[0])) ^ set(map(tuple, got[0])))
        assert lost == (f.stats.pass_coarse_below if fault == "filter_at_thr" else f.stats.float64_differs)
