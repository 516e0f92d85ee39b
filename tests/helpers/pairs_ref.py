"""References for the gallery audit (csrc/pair_scan.hip), plain NumPy on the CPU, shared by tests/test_pairs_ref_host.py
(CPU) and tests/test_gpu_pairs.py (GPU).

`pairs_ref` is the contract as a plain loop over `scan_ref.row_dot_wave8(G, G)`; `candidates_ref` brackets what the coarse filter may let
through, from float64 dots of the f16-rounded rows; the case builders assert what they are named after; `emulate` replays the structure of
the audit (query tiles of 256 positions, row tiles of 64, the filter at thr - eps, b > a, the f32 re-check) with the faults
tests/test_pairs_ref_host.py plants.
"""
import functools
from types import SimpleNamespace

import numpy as np

from tests.helpers import scan_ref as sr

F32 = np.float32
D = 512
ROWS = 64                                     # X16 rows per LDS tile (PS_ROWS)
QB = 256                                      # stationary positions per block (PS_QB)
GRID_NS = (1, 2, 63, 64, 65, 130, 300)
GRID_THRS = (0.5, 1.0)
DELTAS = (1e-2, -1e-2, 2e-3, -2e-3, 5e-4, -5e-4, 1e-4, -1e-4, 2e-5, -2e-5, 3e-6, -3e-6, 3e-7, -3e-7, 3e-8, -3e-8, 0)
FAULTS = ("filter_at_thr", "float64_decision", "b_ge_a", "partial_tile_dropped", "second_query_tile_dropped")


def gmax_of(G):
    """the largest stored norm, as an f32"""
    return F32(np.sqrt((np.asarray(G, np.float64) ** 2).sum(1)).max()) if len(G) else F32(0)


def eps_of(gmax):
    """pair_t_lo's eps with its f32 operations: 1.125 2^-10 Gmax Gmax + 2^-20 (Gmax + Gmax) + 2^-40"""
    g = F32(gmax)
    return F32(F32(F32(F32(1.125 * 2.0 ** -10) * g) * g + F32(F32(2.0 ** -20) * F32(g + g))) + F32(2.0 ** -40))


def t_lo_of(thr, gmax):
    return F32(F32(thr) - eps_of(gmax))


def exact_scores(G):
    """[N][N] f32: s(a, b) = row_dot_wave8(G[a], G[b]); symmetric (asserted)"""
    S = sr.row_dot_wave8(G, G)
    assert np.array_equal(S, S.T)
    return S


def coarse_scores(G):
    """[N][N] float64 dots of the f16-rounded rows: what the matrix-core filter approximates"""
    X = np.asarray(G, F32).astype(np.float16).astype(np.float64)
    return X @ X.T


def _upper(mask):
    a, b = np.nonzero(np.triu(mask, 1))
    return np.stack([a, b], 1).astype(np.int64)


def pairs_ref(G, thr, inclusive, S=None):
    """-> (pairs int64 [P][2] sorted by (a, b), scores f32 [P]): every a < b with s(a, b) > thr (inclusive: >=) in f32.  A plain loop."""
    S = exact_scores(G) if S is None else S
    thr = F32(thr)
    pairs, scores = [], []
    for a in range(len(G)):
        for b in range(a + 1, len(G)):
            s = S[a, b]
            if (s >= thr) if inclusive else (s > thr):
                pairs.append((a, b))
                scores.append(s)
    return np.array(pairs, np.int64).reshape(-1, 2), np.array(scores, F32)


def candidates_ref(G, thr, C=None):
    """-> (low, high, at): the number of pairs a < b whose float64 coarse score is >= t_lo + w / >= t_lo - w / >= t_lo, w = 2^-14 Gmax^2
    being the coarse pass's accumulation term: whatever order the matrix cores sum in, the kernel's candidate count lies
    in [low, high]"""
    C = coarse_scores(G) if C is None else C
    gm = gmax_of(G)
    t, w = float(t_lo_of(thr, gm)), 2.0 ** -14 * float(gm) ** 2
    n = lambda x: len(_upper(C >= x))                                      # noqa: E731
    return n(t + w), n(t - w), n(t)


# ---------------------------------------------------------------- cases
@functools.lru_cache(maxsize=8)
def grid_case(N):
    """scan_ref.win_gallery(N): every score an exact multiple of 2^-6 in every arithmetic, Gmax^2 = 10.5, eps < 2^-6; at N = 300 thousands
    of pairs sit exactly on either threshold and the view crosses the 256-position query tile and five row tiles"""
    G, S0 = sr.win_gallery(N)
    S = exact_scores(G)
    assert np.array_equal(S, S0) and np.array_equal(coarse_scores(G), S0)      # the wave dot, the f16 copy and the grid agree exactly
    assert gmax_of(G) == F32(np.sqrt(10.5)) and 0.0115 < eps_of(gmax_of(G)) < 2.0 ** -6
    if N == 300:
        up = S[np.triu_indices(N, 1)]
        for thr in GRID_THRS:
            assert (up > thr).sum() > 500 and (up == thr).sum() > 1000         # strict and inclusive differ by thousands of pairs
        assert N > QB and N % QB > 32 and (N + ROWS - 1) // ROWS == 5 and N % ROWS != 0
        assert (np.argwhere(np.triu(S > 1.0, 1))[:, 0] >= QB).any()            # pairs whose FIRST row lies in the second query tile
    G.setflags(write=False)
    S.setflags(write=False)
    return SimpleNamespace(G=G, S=S, N=N)


@functools.lru_cache(maxsize=2)
def float_case(seed=5, thr=0.4):
    """40 unit base rows, 17 partners each at cosine 0.4 + delta (DELTAS, down to 3e-8 and 0), 150 unrelated rows, shuffled: 870 rows.
    Asserted: pairs on all four sides of (passes the rule?) x (coarse score above thr?), pairs exactly on f32(thr), pairs a float64 dot
    decides differently, |coarse - s| <= eps, and a candidate count no summation order of the coarse pass can move."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((40, D))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    rows = [base]
    for q in base:
        for d in DELTAS:
            a = thr + d
            u = rng.standard_normal(D)
            u -= (u @ q) * q
            u /= np.linalg.norm(u)
            rows.append((a * q + np.sqrt(1 - a * a) * u)[None])
    noise = rng.standard_normal((150, D))
    rows.append(noise / np.linalg.norm(noise, axis=1, keepdims=True))
    G = np.concatenate(rows).astype(F32)[rng.permutation(870)]
    S, C = exact_scores(G), coarse_scores(G)
    S64 = G.astype(np.float64) @ G.astype(np.float64).T
    t = F32(thr)
    iu = np.triu_indices(len(G), 1)
    s, c, s64 = S[iu], C[iu], S64[iu]
    gm = gmax_of(G)
    eps = float(eps_of(gm))
    stats = SimpleNamespace(
        passing=int((s > t).sum()), on_thr=int((s == t).sum()),
        pass_coarse_below=int(((s > t) & (c < float(t))).sum()), fail_coarse_above=int((~(s > t) & (c > float(t))).sum()),
        pass_coarse_above=int(((s > t) & (c >= float(t))).sum()),
        float64_differs=int(((s > t) != (s64 > thr)).sum()), max_err=float(np.abs(c - s.astype(np.float64)).max()), eps=eps)
    low, high, at = candidates_ref(G, thr, C)
    stats.candidates = at
    assert min(stats.passing, stats.on_thr, stats.pass_coarse_below, stats.fail_coarse_above, stats.pass_coarse_above,
               stats.float64_differs) > 0, stats
    assert stats.max_err <= eps
    assert low == high == at, (low, high, at)                              # the bracket is closed
    assert (c[s >= t] >= float(t_lo_of(thr, gm))).all()                    # the filter loses no pair, strict or inclusive
    G.setflags(write=False)
    S.setflags(write=False)
    return SimpleNamespace(G=G, S=S, C=C, N=len(G), thr=thr, stats=stats, bracket=(low, high))


def nonfinite_row(G, r=1):
    """a copy of row r with one element beyond the f16 range"""
    v = np.array(G[r], F32)
    v[7] = 1e5
    return v


# ---------------------------------------------------------------- the audit's structure, with faults
def emulate(G, thr, inclusive, fault=None, S=None, C=None):
    """pairs_ref's result from the audit's own steps: per query tile of 256 positions and row tile of 64, a pair is a candidate iff
    coarse >= t_lo and a < b < N; every candidate is decided by s alone.
      filter_at_thr              the filter compares against thr, not thr - eps
      float64_decision           the re-check decides by a float64 dot of the f32 rows
      b_ge_a                     the filter's b > a is b >= a
      partial_tile_dropped       the last, partial row tile is never scanned
      second_query_tile_dropped  positions 256 .. 511 are never stationary"""
    G = np.asarray(G, F32)
    N = len(G)
    S = exact_scores(G) if S is None else S
    C = coarse_scores(G) if C is None else C
    t = F32(thr)
    cut = float(t) if fault == "filter_at_thr" else float(t_lo_of(thr, gmax_of(G)))
    if fault == "float64_decision":                                        # float64 throughout: the dot, and thr as the caller wrote it
        S, t = G.astype(np.float64) @ G.astype(np.float64).T, float(thr)
    ntiles = (N + ROWS - 1) // ROWS
    if fault == "partial_tile_dropped" and N % ROWS:
        ntiles -= 1
    pairs, scores = [], []
    for qt in range((N + QB - 1) // QB):
        if fault == "second_query_tile_dropped" and qt == 1:
            continue
        for tile in range(ntiles):
            r0, r1 = tile * ROWS, min(N, tile * ROWS + ROWS)
            if r1 <= qt * QB + 1 and fault != "b_ge_a":
                continue
            for a in range(qt * QB, min(N, qt * QB + QB)):
                for b in range(r0, r1):
                    if not ((b >= a) if fault == "b_ge_a" else (b > a)) or not C[a, b] >= cut:
                        continue
                    s = S[a, b]
                    if (s >= t) if inclusive else (s > t):
                        pairs.append((a, b))
                        scores.append(F32(s))
    order = sorted(range(len(pairs)), key=lambda i: pairs[i])
    return (np.array([pairs[i] for i in order], np.int64).reshape(-1, 2), np.array([scores[i] for i in order], F32))


def same(x, y):
    """two (pairs, scores) results agree: the same pairs in the same order, the same score bits"""
    return np.array_equal(x[0], y[0]) and np.array_equal(np.asarray(x[1], F32).view(np.uint32), np.asarray(y[1], F32).view(np.uint32))
