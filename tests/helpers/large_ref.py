"""Builders and expectations for the gallery and frame kernels where offsets pass 2^31 and 2^32, plain NumPy on the CPU, shared by
tests/test_large_ref_host.py (CPU) and tests/test_gpu_large_offsets.py (GPU).

No reference here ever scans a large slab.  The background of a slab is filled on the device with i.i.d. uniform values in [-AMP, AMP],
AMP = 2^-7: a background row has norm <= AMP sqrt(512) < 0.177 and by Cauchy-Schwarz scores below BG_BOUND = 0.18 against any unit
query; so do its f16 copy and its e4m3 x 256 copy against the f16 copy of the query (both roundings are monotone and keep 2^-7 / 2.0),
and below BG_BOUND_F8 against the e4m3 copy of the query (relative rounding error <= 2^-4 per element).  A few dozen planted rows at
chosen indices score about 1.0 against their own queries, so the winner, its score and the planted part of a top-K list need the planted
rows alone: `plant` builds them, `expect_*` are the rules of include/frhip.h over tests/helpers/scan_ref.py's emulated scores.
"""
import functools
from types import SimpleNamespace

import numpy as np

from tests.helpers import coarse_ref as cr
from tests.helpers import scan_ref as sr

D = 512
F32 = np.float32
AMP = 2.0 ** -7
BG_NORM = AMP * np.sqrt(512.0)                 # 0.17678: the longest a background row can be
BG_BOUND = 0.18
BG_BOUND_F8 = 0.19                             # a unit query as e4m3 codes is at most 1 + 2^-4 long
EDGES = (1 << 20, 1 << 21, 1 << 22)            # f32: 2^31 bytes, 2^32 bytes; every type: 2^31 elements (f16: 2^32 bytes)
N = (1 << 22) + 4173                           # 4173 = 130 * 32 + 13 = 65 * 64 + 13: a partial 32-row and a partial 64-row tile
N8 = (1 << 23) + 4173                          # fp8: 2^32 bytes lie at row 2^23
OFFSET = 1 << 33
HEAVY = 1.25                                   # the norm of row N - 13, the longest planted row: what gmax must come to
NQ = 40                                        # two 32-query groups
THR = 0.4
PAIR_A = ((1 << 22) - 3, (1 << 22) + 7)
PAIR_B = (5, N - 2)
TIE_PAIR = ((1 << 22) - 5, (1 << 22) + 9)      # two graded rows with the same bits, either side of row 2^22
NGRADED = 20
TIE_A = 0.91                                   # between grades 3 (0.92) and 4 (0.90)


def edge_rows(n=N, edges=EDGES):
    """b - 1, b, b + 1 around every edge, then 0, n - 13 (the first row of the last, partial, tile) and n - 1"""
    return [b + d for b in edges for d in (-1, 0, 1)] + [0, n - 13, n - 1]


def extra_rows(n=N, edges=EDGES):
    """25 more single rows: the ends of the 32- and 64-row tiles next to every edge, and a few far from any"""
    near = [b + d for b in edges for d in (-33, -32, 31, 32, 63, 64)]
    return near + [1, 31, 32, 1 << 19, 3 << 20, (1 << 22) + (1 << 11), n - 14]


def graded_rows():
    """grade j (score 0.98 - 0.02 j): even j below 2^20, odd j above 2^22 - the rank order jumps across all three edges at every step"""
    return [4096 + 129 * j if j % 2 == 0 else (1 << 22) + 100 + 67 * j for j in range(NGRADED)]


def _unit(rng, n):
    v = rng.standard_normal((n, D))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


@functools.lru_cache(maxsize=1)
def plant():
    """The planted rows of the N-row slab and their 40 queries.
      rows int64 [R] ascending, P f32 [R][512] in that order (`where[row]` -> position in P)
      Qraw f32 [40][512]: the planted vectors scaled by factors in [0.5, 2]; Qn = scan_ref.l2norm_rows(Qraw), the bits the device makes
      target[f]: the row query f must come back with (the lower row of a pair; the best graded row for the last query)
      S f32 [40][R]: the f32 scan's scores (scan_ref.chain under scan_ref.HW), S1: the first-hit dot's (scan_ref.row_dot_wave8)
    Queries 0 .. 36: the single rows of edge_rows() + extra_rows(); 37: PAIR_A; 38: PAIR_B; 39 (GQ): the vector the graded rows copy."""
    rng = np.random.default_rng(2231)
    singles = edge_rows() + extra_rows()
    assert len(singles) == 37 and len(set(singles)) == 37
    base = _unit(rng, NQ)
    placed = {}
    for j, r in enumerate(singles):
        placed[r] = base[j] * (HEAVY if r == N - 13 else 1.0)
    for r in PAIR_A:
        placed[r] = base[37]
    for r in PAIR_B:
        placed[r] = base[38]
    t = base[39]
    noise = _unit(rng, NGRADED + 1)
    noise -= (noise @ t)[:, None] * t[None, :]
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    grades = [0.98 - 0.02 * j for j in range(NGRADED)]
    for j, r in enumerate(graded_rows()):
        placed[r] = grades[j] * t + np.sqrt(1 - grades[j] ** 2) * noise[j]
    for r in TIE_PAIR:
        placed[r] = TIE_A * t + np.sqrt(1 - TIE_A ** 2) * noise[NGRADED]
    rows = np.array(sorted(placed), np.int64)
    assert len(rows) == 37 + 4 + NGRADED + 2 and rows[0] == 0 and rows[-1] == N - 1
    P = np.stack([placed[r] for r in rows]).astype(F32)
    where = {int(r): k for k, r in enumerate(rows)}
    factor = 2.0 ** rng.uniform(-1, 1, NQ)
    Qraw = (base * factor[:, None]).astype(F32)
    Qn = sr.l2norm_rows(Qraw)
    target = np.array(singles + [PAIR_A[0], PAIR_B[0], graded_rows()[0]], np.int64)
    S = sr.chain(Qn, P, **sr.EMULATIONS[sr.HW])
    S1 = sr.row_dot_wave8(Qn, P)
    return SimpleNamespace(rows=rows, P=P, where=where, Qraw=Qraw, Qn=Qn, factor=factor, target=target, S=S, S1=S1, GQ=NQ - 1,
                           identities=np.concatenate([np.stack([placed[r] for r in singles]), base[37:40]]),
                           family=np.array([where[r] for r in graded_rows() + list(TIE_PAIR)]))


def check_rows(n=N, rows=None):
    """the rows a conversion or a normalisation is read back at: every planted row and both its neighbours (background rows)"""
    rows = plant().rows if rows is None else rows
    out = np.unique(np.concatenate([rows - 1, rows, rows + 1]))
    return out[(out >= 0) & (out < n)]


def expect_topk(S, rows, K, row_offset=0):
    """The planted part of the top-K lists: (idx int64 [F][K], score f32 [F][K], n int [F]).  Entries 0 .. n[f] - 1 are the planted rows
    that score above BG_BOUND in the order of the rules (score descending, row ascending; `rows` ascending, S in that order) and must come
    back bit for bit; the K - n[f] entries behind them score below BG_BOUND, where planted rows of other queries and background rows
    mix in an order only a scan of the slab could tell (the entries of `idx` / `score` past n[f] rank the planted rows alone)."""
    idx, score = sr.topk_ref(np.asarray(S, F32), K)
    n = (score > F32(BG_BOUND)).sum(1)
    assert ((score > F32(BG_BOUND)) == (np.arange(K)[None, :] < n[:, None])).all()
    idx = np.where(idx >= 0, np.asarray(rows)[np.maximum(idx, 0)] + row_offset, -1)
    return idx, score, n


def expect_match(S, rows, row_offset=0):
    idx, score, n = expect_topk(S, rows, 1, row_offset)
    assert (n == 1).all()
    return idx[:, 0].copy(), score[:, 0].copy()


def expect_first_above(S1, rows, thr, inclusive, row_offset=0):
    """the lowest planted row whose first-hit score passes thr (no background row can: BG_BOUND < thr is asserted)"""
    assert thr > BG_BOUND
    idx, score = sr.first_above_ref(np.asarray(S1, F32), thr, inclusive)
    return np.where(idx >= 0, np.asarray(rows)[np.maximum(idx, 0)] + row_offset, -1), score


# ---------------------------------------------------------------- writes and views at high slots of a slab of N slots
FIRST_SLOT = (1 << 22) - 150                   # 300 upserted ids take slots 2^22 - 150 .. 2^22 + 149
NIDS = 300
DUPS = ((100, 200), (3, 290))                  # ids with the same row: slots 2^22 - 50 / + 50 and 2^22 - 147 / + 140


@functools.lru_cache(maxsize=1)
def view_case():
    """300 unit rows for ids 0 .. 299 (two duplicate pairs across slot 2^22), 700 never-written (zero) slots from both sides of them
    under ids ("z", k), one shuffled view of all 1000 and a second view of every other one in reverse; 40 queries: scaled copies of
    rows, the duplicated ones among them.
      V f32 [1000][512]: the rows in the order of view A;  S: the f32 scan's scores of the normalised queries over V
      posB: the positions of view B's members in view A (S[:, posB] is view B's score matrix)"""
    rng = np.random.default_rng(2232)
    rows = _unit(rng, NIDS).astype(F32)
    for a, b in DUPS:
        rows[b] = rows[a]
    lo = FIRST_SLOT - 1 - rng.choice(5000, 346, replace=False)
    hi = FIRST_SLOT + NIDS + rng.choice(N - FIRST_SLOT - NIDS - 1, 350, replace=False)
    zslots = np.concatenate([[0, 1 << 20, 1 << 21, N - 1], lo, hi]).astype(np.int64)
    assert len(set(zslots.tolist())) == 700
    ids = list(range(NIDS)) + [("z", k) for k in range(700)]
    order = rng.permutation(1000)
    idsA = [ids[k] for k in order]
    V = np.concatenate([rows, np.zeros((700, D), F32)])[order]
    posB = np.arange(1000)[::-2].copy()
    sel = np.concatenate([[a for a, _ in DUPS], [b for _, b in DUPS], rng.choice(NIDS, NQ - 4, replace=False)])
    Qraw = (rows[sel] * 2.0 ** rng.uniform(-1, 1, (NQ, 1))).astype(F32)
    Qn = sr.l2norm_rows(Qraw)
    S = sr.chain(Qn, V, **sr.EMULATIONS[sr.HW])
    pos = {i: p for p, i in enumerate(idsA)}
    pairs = sorted(tuple(sorted((pos[a], pos[b]))) for a, b in DUPS)
    pair_scores = np.array([sr.row_dot_wave8(V[a:a + 1], V[b:b + 1])[0, 0] for a, b in pairs], F32)
    return SimpleNamespace(rows=rows, zslots=zslots, ids=ids, idsA=idsA, idsB=[idsA[p] for p in posB], V=V, posB=posB, Qraw=Qraw,
                           Qn=Qn, S=S, sel=sel, pairs=np.array(pairs, np.int64), pair_scores=pair_scores)


# ---------------------------------------------------------------- the fp8-only slab: 2^32 bytes at row 2^23, no f32 rows
F8_CODE_MAX = 0x40                             # e4m3 2.0 = 256 * 2^-7: background codes are sign | 0 .. 0x40


def f8_rows():
    """multiples of 4 (the coarse maximum stands for its 4-row group, reported by its first row) on both sides of row 2^23; N8 - 13
    starts the last, partial, 64-row tile and N8 - 1 is the only row of the last group"""
    b = 1 << 23
    return np.array([0, 64, b - 64, b - 8, b - 4, b, b + 4, b + 64, b + 4096, N8 - 13, N8 - 1], np.int64)


@functools.lru_cache(maxsize=1)
def plant_f8():
    """Rows on an exact grid: 24 entries of +-1/4, +-1/8, +-1/16 (scan_ref.signatures / 4), so 256 x is an e4m3 integer, every product
    and partial sum of the code dot is exact (coarse_ref.assert_exact) and the coarse score |row|^2 = 10.5 / 16 comes back bit for bit.
    Query f = row f as it stands (the library entry does not renormalise).  -> rows, P f32, S float64 code dots [F][R]"""
    rows = f8_rows()
    assert len(set(rows.tolist())) == len(rows) and (rows % 4 == 0).all() and (np.diff(rows) >= 4).all()
    P = (sr.signatures(len(rows), 823) / 4).astype(F32)
    S = cr.scores(P, P, "f8")
    return SimpleNamespace(rows=rows, P=P, S=S)


def expect_coarse_f8(S, rows, row_offset=0):
    """fr_gallery_match_f8 with G32 == NULL over planted rows that sit alone in their 4-row groups"""
    best = S.argmax(1)
    score = (S[np.arange(len(S)), best] * cr.unscale("f8")).astype(F32)
    return np.asarray(rows)[best] + row_offset, score


# ---------------------------------------------------------------- the two range clamps
CLAMP_ROWS = 1 << 20                           # scan_gemm.hip / pair_scan.hip: at most 16384 tiles of 64 rows per range (2^30 bytes of f16)
N16 = (1 << 23) + 4173                         # more than 8 ranges of 2^20 rows
F16Q = 8192                                    # 32 query tiles: the plan wants 8 ranges, the clamp makes 9
NP = (1 << 20) + 4173                          # the pair scan with max_ranges = 1: two ranges after the clamp


@functools.lru_cache(maxsize=1)
def plant_f16():
    """Exact-grid rows (scan_ref.signatures / 4: f16 holds them, every partial sum of a dot is exact) at multiples of 4 on both sides of
    every 2^20-row range edge of the N16-row f16 slab, at row 0 and in the last group; query f = row f % R as it stands.
    -> rows, P f32, S float64 [R][R]"""
    edges = [k << 20 for k in range(1, 9)]
    rows = np.array([0] + [e + d for e in edges for d in (-4, 0)] + [N16 - 1], np.int64)
    assert (rows % 4 == 0).all() and (np.diff(rows) >= 4).all()
    P = (sr.signatures(len(rows), 824) / 4).astype(F32)
    return SimpleNamespace(rows=rows, P=P, S=cr.scores(P, P, "f16"))


def expect_coarse_f16(S, rows, F, row_offset=0):
    best = S.argmax(1)
    score = S[np.arange(len(S)), best].astype(F32)
    f = np.arange(F) % len(rows)
    return np.asarray(rows)[best][f] + row_offset, score[f]


@functools.lru_cache(maxsize=1)
def plant_pairs():
    """five duplicated unit rows, one copy below row 2^20 and one at or above it -> (rows [10] ascending, P f32 [10][512],
    pairs int64 [5][2] sorted, scores f32 [5]: the first-hit dot of a row with itself)"""
    rng = np.random.default_rng(2233)
    U = _unit(rng, 5).astype(F32)
    lo = np.array([3, CLAMP_ROWS - 4097, CLAMP_ROWS - 64, CLAMP_ROWS - 2, CLAMP_ROWS - 1], np.int64)
    hi = np.array([NP - 1, CLAMP_ROWS + 1, CLAMP_ROWS + 63, CLAMP_ROWS, CLAMP_ROWS + 4100], np.int64)
    rows = np.concatenate([lo, hi])
    order = np.argsort(rows)
    scores = np.array([sr.row_dot_wave8(U[k:k + 1], U[k:k + 1])[0, 0] for k in range(5)], F32)
    return SimpleNamespace(rows=rows[order], P=np.concatenate([U, U])[order], pairs=np.stack([lo, hi], 1), scores=scores, U=U)
