"""Float64 reference of the exact top-K gallery identification and the rule a GPU result is compared by (NumPy only).

Scores are float64 dot products of the exact f32 rows (after ``oracle.match.renormalise`` of each query where the
call renormalises), ranked by a stable sort on -score: score descending, row ascending.  Only rows scoring > -1 are
listed; slots past them hold (-1, -1.0).

Two f32 summation orders may swap rows whose true scores nearly coincide, so:
* every returned slot's score must be within SCORE_TOL of the float64 score OF THE ROW THE GPU RETURNED
  (2e-6: the figure DESIGN.md section 2 states for f32 gallery scores under a different summation order; NumPy's own
  f32 product differs from float64 by at most 1.3e-7 on these inputs);
* position (f, j) is AMBIGUOUS when the reference score at rank j is within 2 * SCORE_TOL of rank j-1 or rank j+1
  (rank K included).  Elsewhere the returned row must EQUAL the reference row; on an ambiguous position it must be one
  of the reference rows within 2 * SCORE_TOL of that rank's score;
* a case whose ambiguous positions exceed AMBIGUOUS_CAP of all positions is uninformative and fails.
"""
import numpy as np

from oracle import match as omatch

SCORE_TOL = 2e-6
AMBIGUOUS_CAP = 0.02


def seeded_case(seed, N, F):
    """Gaussian rows, row-normalised gallery; queries of the same kind scaled off unit length (renormalise must run)."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((N, 512)).astype(np.float32)
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    Q = rng.standard_normal((F, 512)).astype(np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    Q *= rng.uniform(0.5, 2.0, (F, 1)).astype(np.float32)
    return G, Q


def scores64(Q, G, renormalise=True):
    """float64 [F,N] scores of f32 queries against f32 rows."""
    Q = np.asarray(Q, np.float32)
    if renormalise and len(Q):
        Q = np.stack([omatch.renormalise(q) for q in Q]).astype(np.float32)
    return Q.astype(np.float64) @ np.asarray(G, np.float32).astype(np.float64).T


def topk(S, K):
    """(idx int64[F,K], score float64[F,K]) of a score matrix: stable sort on -score, rows scoring > -1 only."""
    F, N = S.shape
    idx = np.full((F, K), -1, np.int64)
    score = np.full((F, K), -1.0, np.float64)
    for f in range(F):
        order = np.argsort(-S[f], kind="stable")
        order = order[S[f, order] > -1.0][:K]
        idx[f, :len(order)] = order
        score[f, :len(order)] = S[f, order]
    return idx, score


def ambiguous_positions(S, K):
    """bool [F,K]: rank j's reference score is within 2 * SCORE_TOL of rank j-1 or j+1 (rank K included)."""
    F, N = S.shape
    amb = np.zeros((F, K), bool)
    for f in range(F):
        rs = -np.sort(-S[f], kind="stable")[:K + 1]
        near = np.abs(np.diff(rs)) <= 2 * SCORE_TOL            # near[j]: ranks j and j+1 nearly coincide
        for j in range(min(K, len(rs))):
            amb[f, j] = (j > 0 and near[j - 1]) or (j < len(near) and near[j])
    return amb


def check(idx, score, S, K):
    """Assert a returned (idx [F,K], score f32 [F,K]) against the score matrix S; returns (#ambiguous, #positions)."""
    idx, score = np.asarray(idx), np.asarray(score)
    F, N = S.shape
    assert idx.shape == (F, K) and score.shape == (F, K) and idx.dtype == np.int64 and score.dtype == np.float32
    ridx, rscore = topk(S, K)
    amb = ambiguous_positions(S, K)
    n_amb = 0
    for f in range(F):
        filled = int((ridx[f] >= 0).sum())
        got = idx[f, :filled]
        assert (got >= 0).all() and (got < N).all(), (f, idx[f])
        assert len(set(got.tolist())) == filled, ("a row listed twice", f, idx[f])
        assert (idx[f, filled:] == -1).all() and (score[f, filled:] == np.float32(-1.0)).all(), (f, idx[f], score[f])
        err = np.abs(score[f, :filled].astype(np.float64) - S[f, got])
        assert (err <= SCORE_TOL).all(), ("score off the float64 score of the returned row", f, err.max())
        for j in range(filled):
            if not amb[f, j]:
                assert got[j] == ridx[f, j], ("row", f, j, got[j], ridx[f, j], rscore[f, max(j - 1, 0):j + 2])
            else:
                n_amb += 1
                assert abs(S[f, got[j]] - rscore[f, j]) <= 2 * SCORE_TOL, ("ambiguous row", f, j, got[j], ridx[f, j])
    total = F * K
    print(f"top-{K}: F {F} N {N}: {n_amb} ambiguous of {total} positions")
    assert n_amb <= AMBIGUOUS_CAP * total, f"{n_amb} of {total} positions ambiguous: the case shows nothing"
    return n_amb, total
