"""References for the exact f32 gallery scans (csrc/match.hip, match_scan.h, match_topk.hip, topk_list.h) and the first-hit consumers,
plain NumPy on the CPU, shared by tests/test_scan_ref_host.py (CPU) and tests/test_gpu_scan_pins.py (GPU).

A. Exact-grid operands: every element a multiple of 2^-3 with |x| <= 2, so every product is a multiple of 2^-6, sum |q g| * 2^6 < 2^24
   (`assert_grid`) and every partial sum is exact in f32 in any order, fused or not.  `topk_ref` / `match_ref` / `first_above_ref` are the
   rules of include/frhip.h as plain loops over the exact scores; the case builders assert what each case is named after.
B. `fma32` is an exact f32 fused multiply-add (float64 product, TwoSum, round-to-odd before the last rounding); `chain` replays the
   accumulation of v_mfma_f32_32x32x2_f32 over the operand order of scan_tile_f32 under the three candidate rules.
C. `row_dot_wave8`, `cosine_rows`, `l2norm_rows`, `mean_rows`: the VALU consumers of match_scan.h in NumPy float32, same order of sums.
D. `emulate_scan`: the scan's structure (tile, register, half-wave, wave, block, lap, insert, bitonic merge, reduce) over a score matrix,
   with the faults tests/test_scan_ref_host.py plants.
"""
import functools

import numpy as np

D = 512
KS = (1, 2, 3, 4, 5, 8, 16)
LAP = 131072                                  # rows per lap of the grid-stride loop: 1024 blocks x 4 waves x 32 rows
LAP_N = LAP + 173                             # five whole tiles and a partial tile of 13 rows in the second lap
WIN_NS = tuple(range(1, 41)) + (63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4097)
TIE_NS = (1000, 4097)
GAMMA512 = 512 * 2.0 ** -24 / (1 - 512 * 2.0 ** -24)
F32 = np.float32


def scan_blocks(N):
    """scan_blocks of match_scan.h"""
    return int(min(max(((N + 31) // 32 + 3) // 4, 1), 1024))


def kp_of(K):
    return 2 if K <= 2 else 4 if K <= 4 else 8 if K <= 8 else 16


# ---------------------------------------------------------------- A. the grid and the rules
def assert_grid(Q, G):
    """multiples of 2^-3, |x| <= 2, and sum |q_k g_k| * 2^6 < 2^24 for every pair (bounded through the column maxima of |G|)"""
    for X in (Q, G):
        X = np.asarray(X)
        assert X.dtype == F32 and np.isfinite(X).all() and (np.abs(X) <= 2).all() and (X * 8 == np.rint(X * 8)).all()
    if len(G) and len(Q):
        worst = float((np.abs(Q).astype(np.float64) @ np.abs(G).max(0).astype(np.float64)).max()) * 64
        assert worst < 2.0 ** 24, worst


def scores_grid(Q, G):
    """[F][N] exact scores as float32 (from the float64 product; exactness asserted)"""
    assert_grid(Q, G)
    S = Q.astype(np.float64) @ G.astype(np.float64).T
    assert (S * 64 == np.rint(S * 64)).all() and (S.astype(F32) == S).all()
    return S.astype(F32)


def topk_ref(S, K, row_offset=0, mask=None):
    """the K best rows per query under (score descending, row ascending) among rows scoring > -1; (-1, -1.0) fills the rest.
    S float32 [F][N] in scan order."""
    F, N = S.shape
    idx = np.full((F, K), -1, np.int64)
    score = np.full((F, K), -1.0, F32)
    for f in range(F):
        if N == 0 or (mask is not None and mask[f] <= 0):
            continue
        s = S[f]
        rows = np.flatnonzero(s >= np.partition(s, N - K)[N - K]) if N > K else np.arange(N)
        rows = rows[np.argsort(-s[rows].astype(np.float64), kind="stable")][:K]
        rows = rows[s[rows] > -1.0]
        idx[f, :len(rows)] = rows + row_offset
        score[f, :len(rows)] = s[rows]
    return idx, score


def match_ref(S, row_offset=0):
    idx, score = topk_ref(S, 1, row_offset)
    return idx[:, 0].copy(), score[:, 0].copy()


def first_above_ref(S, thr, inclusive, row_offset=0, take=None):
    """first row whose f32 score passes thr, its score; (-1, 0.f) when none does or the query is not taken"""
    F = len(S)
    thr = F32(thr)
    idx = np.full(F, -1, np.int64)
    score = np.zeros(F, F32)
    for f in range(F):
        if take is not None and take[f] == 0:
            continue
        hit = np.flatnonzero((S[f] >= thr) if inclusive else (S[f] > thr))
        if len(hit):
            idx[f], score[f] = hit[0] + row_offset, S[f, hit[0]]
    return idx, score


# ---------------------------------------------------------------- A. cases
MAGS = np.array([1.0] * 8 + [0.5] * 8 + [0.25] * 8, F32)          # a signature: 24 entries, |row|^2 = 10.5
SELF = F32(10.5)


def signatures(N, seed):
    """N rows, each 24 entries of +-1, +-1/2, +-1/4 at positions base + step * j (step odd: distinct mod 512)"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, D, N)
    step = rng.integers(0, D // 2, N) * 2 + 1
    pos = (base[:, None] + step[:, None] * np.arange(24)[None, :]) % D
    val = rng.permuted(np.tile(MAGS, (N, 1)), axis=1) * rng.choice(np.array([-1.0, 1.0], F32), (N, 24))
    G = np.zeros((N, D), F32)
    G[np.arange(N)[:, None], pos] = val
    return G


def perms(N):
    out = [np.arange(N), (1597 * np.arange(N)) % N, (7919 * np.arange(N) + 29) % N]
    for p in out:
        assert np.array_equal(np.sort(p), np.arange(N))
    return out


@functools.lru_cache(maxsize=4)
def win_gallery(N):
    """every row wins: G [N][512] and S0 = G G^T, with the self-score strictly above every cross-score (asserted)"""
    G = signatures(N, 1000 + N)
    S0 = scores_grid(G, G)
    cross = S0.copy()
    np.fill_diagonal(cross, -np.inf)
    assert (np.diagonal(S0) == SELF).all() and (N == 1 or (cross.max(1) < SELF).all())
    return G, S0


def win_case(N, p):
    """query f = row pi(f): (Q, G, S, pi)"""
    G, S0 = win_gallery(N)
    pi = perms(N)[p]
    return G[pi], G, S0[pi], pi


NDECOY = 5


def view_slab(G, S0, seed):
    """a slab of N + NDECOY slots holding G's rows out of order behind `view` (position -> slot); two unused slots hold decoys (twice a
    row: the best row of the slab for the query that targets it, asserted when S0 = G G^T is given), the other unused slots NaN"""
    N = len(G)
    rng = np.random.default_rng(seed)
    order = rng.permutation(N + NDECOY)
    view, unused = order[:N].astype(np.int64), order[N:]
    slab = np.full((N + NDECOY, D), np.nan, F32)
    slab[view] = G
    for j, t in enumerate((N // 2, 0)):
        slab[unused[j]] = 2 * G[t]
        assert S0 is None or 2 * S0[t, t] > S0[t].max()                          # query G[t]: the decoy beats every row the view names
    assert N <= 2 or not np.array_equal(view, np.arange(N))
    return slab, view


@functools.lru_cache(maxsize=2)
def tie_case(N):
    """7 patterns repeated with period 7 (coprime to 32): (Q [12][512], G, S); for the first 7 queries >= N // 7 rows share the top score"""
    P = signatures(7, 77)
    G = P[np.arange(N) % 7]
    Q = np.concatenate([P, np.stack([P[0] + P[1], P[2] - P[3], P[4] + P[5], -P[0], P[6] - P[0]])]).astype(F32)
    S = scores_grid(Q, G)
    for f in range(7):
        top = np.flatnonzero(S[f] == S[f].max())
        assert len(top) >= N // 7 and np.array_equal(top, np.arange(f, N, 7))
    return Q, G, S


def shuffled_view(N, seed):
    """view (position -> slot) over a slab of N slots"""
    return np.random.default_rng(seed).permutation(N).astype(np.int64)


PAIR_DISTS = (1, 4, 8, 32, 128)                                    # next row, other half-wave, next register group, next wave, next block


def pair_case(N=1000):
    """exact two-row ties inside the every-row-wins gallery: query = G[a] + G[a + d] scores |row|^2 + G[a].G[a + d] on both and less
    on every other row (asserted).  a % 8 < 4 (the lower row in half-wave 0) and a % 8 >= 4 (in half-wave 1) for every distance.
    -> (Q, G, S, [(a, d)], swap view: the two rows of each pair exchanged)"""
    G, S0 = win_gallery(N)
    pairs = [(64 * i + off, d) for i, d in enumerate(PAIR_DISTS) for off in (2, 37)]
    Q = np.stack([G[a] + G[a + d] for a, d in pairs]).astype(F32)
    S = scores_grid(Q, G)
    view = np.arange(N, dtype=np.int64)
    for f, (a, d) in enumerate(pairs):
        rest = np.delete(S[f], [a, a + d])
        assert S[f, a] == S[f, a + d] and S[f, a] > rest.max() and (a % 8 < 4) == (f % 2 == 0)
        view[a], view[a + d] = a + d, a
    return Q, G, S, pairs, view


def minus_one_case(N=200, F=18):
    """query f reads column f alone (Q[f][f] = -1): exactly f rows score above -1 (-0.875, -0.5, -0.25), every other row scores -1 or
    -1.125.  Query 0: the best score is exactly -1.  Two blocks at N = 200."""
    rng = np.random.default_rng(4)
    G = np.zeros((N, D), F32)
    Q = np.zeros((F, D), F32)
    for f in range(F):
        G[:, f] = np.where(np.arange(N) % 3 == 1, 1.125, 1.0)
        rows = rng.choice(N, f, replace=False)
        G[rows, f] = np.array([0.875, 0.5, 0.25, 0.875], F32)[np.arange(f) % 4]
        Q[f, f] = -1.0
    if F > 1:
        G[N - 1, 1] = 0.875                                        # query 1: its one listed row is the last row
        G[:N - 1, 1] = np.where(np.arange(N - 1) % 3 == 1, 1.125, 1.0)
    S = scores_grid(Q, G)
    assert S[0].max() == -1.0 and ((S > -1.0).sum(1) == np.arange(F)).all() and (S == -1.125).any()
    return Q, G, S


@functools.lru_cache(maxsize=1)
def lap_case():
    """N = 131072 + 173, F = 256.  Queries 0 .. 172: row 131072 + f, the unique maximum (asserted).  Queries 173 .. 255: G[r] + G[r + LAP],
    an exact tie between a first-lap row and the row one lap further on - same block, wave, lane and register - above every other
    row (asserted).  S: one float32 BLAS product, exact on the grid.  -> (Q, G, S, swap view)"""
    N = LAP_N
    G = signatures(N, 99)
    tie_rows = (np.arange(83) * 2 + 1) % 173
    Q = np.concatenate([G[LAP:], G[tie_rows] + G[tie_rows + LAP]]).astype(F32)
    assert_grid(Q, G)
    S = Q @ G.T
    assert (S * 64 == np.rint(S * 64)).all()
    top = S.max(1)
    first = S.argmax(1)
    assert np.array_equal(first[:173], LAP + np.arange(173)) and ((S == top[:, None]).sum(1)[:173] == 1).all()
    assert np.array_equal(first[173:], tie_rows) and ((S == top[:, None]).sum(1)[173:] == 2).all()
    assert (S[np.arange(173, 256), tie_rows + LAP] == top[173:]).all()
    view = np.arange(N, dtype=np.int64)
    view[tie_rows], view[tie_rows + LAP] = tie_rows + LAP, tie_rows.copy()
    return Q, G, S, view


FIRST_NS = tuple(range(1, 10)) + (4097,)
FIRST_FS = (1, 15, 16, 17, 33)


def first_case(N, F):
    """queries over the every-row-wins gallery whose targets include rows 0 .. 7 (every wave of the first block in both first-hit
    kernels: one row per wave and step in the plain one, two in the blocked one) and the last row;
    thresholds that are reachable scores (asserted): the self-score (only the target passes, and only when inclusive), and cross-scores"""
    G, S0 = win_gallery(N)
    targets = np.unique(np.concatenate([np.arange(min(N, 8)), [N - 1], (np.arange(F) * 131) % N]))
    targets = np.resize(np.concatenate([targets[::-1][:1], targets]), F)     # the last row first
    Q, S = G[targets], S0[targets]
    thrs = [float(SELF)] + [t for t in (0.0, 0.25, 1.0) if (S == F32(t)).any()]
    return Q, G, S, targets, thrs


# ---------------------------------------------------------------- B. the f32 matrix instruction
def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def round_odd_to_f32(s, e):
    """float32(s + e) rounded once, s float64, |e| below one ulp of s: s is moved to the float64 with an odd last bit among the two
    that bracket s + e (round to odd), which float32 conversion then rounds as it would the exact value (53 >= 24 + 2)"""
    s = np.asarray(s, np.float64).copy()
    e = np.asarray(e, np.float64)
    bits = s.view(np.int64)
    fix = (e != 0) & ((bits & 1) == 0) & np.isfinite(s)
    if fix.any():
        s[fix] = np.nextafter(s[fix], np.where(e[fix] > 0, np.inf, -np.inf))
    return s.astype(F32)


def flush32(x):
    """subnormal float32 -> signed zero"""
    x = np.asarray(x, F32)
    return np.where((np.abs(x) < F32(2.0 ** -126)), np.copysign(F32(0), x), x).astype(F32)


def fma32(a, b, c):
    """float32(a * b + c) with one rounding; a, b, c float32 arrays"""
    p = np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64)     # exact: 48 bits
    s, e = two_sum(p, np.asarray(c, F32).astype(np.float64))
    return round_odd_to_f32(s, e)


def fma2_32(a0, b0, a1, b1, c):
    """float32(c + a0 * b0 + a1 * b1) with one rounding"""
    p0 = np.asarray(a0, F32).astype(np.float64) * np.asarray(b0, F32).astype(np.float64)
    p1 = np.asarray(a1, F32).astype(np.float64) * np.asarray(b1, F32).astype(np.float64)
    s1, e1 = two_sum(p0, p1)
    s2, e2 = two_sum(s1, np.asarray(c, F32).astype(np.float64))
    t, e3 = two_sum(e1, e2)
    s3, e4 = two_sum(s2, t)
    return round_odd_to_f32(s3, e4 + e3)


def mfma_order():
    """element order of the 256 instructions of scan_tile_f32: instruction 4 kk + e takes element 8 kk + e from the h = 0 lanes (k slot 0)
    and element 8 kk + 4 + e from the h = 1 lanes (k slot 1): 0, 4, 1, 5, 2, 6, 3, 7, 8, 12, ..."""
    kk, e = np.divmod(np.arange(D // 2), 4)
    return np.stack([8 * kk + e, 8 * kk + 4 + e], 1).reshape(-1)


def chain(Q, G, rule="a", order=None, flush_in=False, flush_out=False, drop_last=False, pairwise=False):
    """[F][N] float32 scores as the accumulation rule gives them.  rule "a": two chained single-rounded fmas per instruction, in `order`;
    "b": acc + a0 b0 + a1 b1 with one rounding per instruction; "muladd": rounded product, rounded sum (a fault).  flush_in / flush_out:
    subnormal operands / results become zero.  drop_last: the last instruction is left out (a fault).  pairwise: [n] scores of (Q[i], G[i])."""
    order = mfma_order() if order is None else np.asarray(order)
    Q, G = np.asarray(Q, F32), np.asarray(G, F32)
    if flush_in:
        Q, G = flush32(Q), flush32(G)
    acc = np.zeros(len(Q) if pairwise else (len(Q), len(G)), F32)
    qi, gi = (np.s_[:], np.s_[:]) if pairwise else (np.s_[:, None], np.s_[None, :])
    out = flush32 if flush_out else (lambda x: x)
    steps = len(order) - (2 if drop_last else 0)
    with np.errstate(all="ignore"):
        for j in range(0, steps, 2):
            k0, k1 = order[j], order[j + 1]
            q0, g0, q1, g1 = Q[:, k0][qi], G[:, k0][gi], Q[:, k1][qi], G[:, k1][gi]
            if rule == "a":
                acc = out(fma32(g1, q1, out(fma32(g0, q0, acc))))
            elif rule == "b":
                acc = out(fma2_32(g0, q0, g1, q1, acc))
            else:
                acc = (acc + g0 * q0).astype(F32)
                acc = (acc + g1 * q1).astype(F32)
    return acc


def gamma_bound(Q, G):
    """gamma_512 * sum |q_k g_k|, float64 [F][N]"""
    return GAMMA512 * (np.abs(Q).astype(np.float64) @ np.abs(G).astype(np.float64).T)


def probe_cases():
    """(name, q [512], g [512]): three non-zero products big + small - big placed in the two k slots of one instruction, in neighbouring
    instructions and 8 elements apart, with exact and with inexact products; products and operands in the f32 subnormal range.
    The emulations disagree on many of them (tests/test_scan_ref_host.py asserts which)."""
    cases = []
    els = (0, 4, 1, 5, 8, 12)
    big, small = F32(1.5), F32(2.0 ** -30)
    g_exact = np.ones(D, F32)
    g_odd = (1 + np.random.default_rng(5).integers(1, 2 ** 23, D) * 2.0 ** -23).astype(F32)
    for gname, g in (("ones", g_exact), ("odd", g_odd)):
        for kb in els:
            for ks in els:
                for kn in els:
                    if len({kb, ks, kn}) == 3:
                        q = np.zeros(D, F32)
                        q[kb], q[ks], q[kn] = big, small, -big
                        cases.append((f"{gname}:big@{kb} small@{ks} -big@{kn}", q, g))
    # half-ulp ties and sticky bits: 1 + (2^-24 + 2^-47) - ..., in one instruction and across two
    for k0, k1, k2 in ((0, 4, 1), (0, 1, 5), (1, 5, 8), (0, 8, 12), (4, 0, 1)):
        q = np.zeros(D, F32)
        g = np.ones(D, F32)
        q[k0], q[k1], q[k2] = 1.0, 2.0 ** -24, 2.0 ** -24
        g[k2] = 1 + 2.0 ** -23
        cases.append((f"ties:{k0},{k1},{k2}", q, g))
    sub = []
    for k0, k1 in ((0, 4), (0, 1), (4, 8)):
        q = np.zeros(D, F32); g = np.zeros(D, F32)
        q[k0], g[k0] = 2.0 ** -100, 2.0 ** -40                     # a subnormal product of normal operands
        sub.append((f"sub-product@{k0}", q, g))
        q = np.zeros(D, F32); g = np.zeros(D, F32)
        q[k0], g[k0], q[k1], g[k1] = 2.0 ** -100, 2.0 ** -40, 2.0 ** -90, 2.0 ** -45
        sub.append((f"sub-products@{k0},{k1}", q, g))
        q = np.zeros(D, F32); g = np.zeros(D, F32)
        q[k0], g[k0] = 2.0 ** -130, 2.0 ** 20                      # a subnormal operand, a normal product
        sub.append((f"sub-operand@{k0}", q, g))
        q = np.zeros(D, F32); g = np.zeros(D, F32)
        q[k0], g[k0], q[k1], g[k1] = 2.0 ** -60, 2.0 ** -60, -(2.0 ** -60), F32(2.0 ** -60) * F32(1 - 2.0 ** -20)
        sub.append((f"sub-result@{k0},{k1}", q, g))                # normal products, a subnormal sum 2^-140
    out = []
    for name, q, g in cases + sub:                                 # element 511: the other rows of the probe gallery hold -4 there
        q, g = q.copy(), g.copy()
        q[D - 1], g[D - 1] = 1.0, 0.0
        out.append((name, q, g))
    return out


EMULATIONS = {
    "a": dict(rule="a"),
    "a, h=1 first": dict(rule="a", order=mfma_order().reshape(-1, 2)[:, ::-1].reshape(-1)),
    "a, element order": dict(rule="a", order=np.arange(D)),
    "b": dict(rule="b"),
    "a, operands flushed": dict(rule="a", flush_in=True),
    "a, results flushed": dict(rule="a", flush_out=True),
    "a, both flushed": dict(rule="a", flush_in=True, flush_out=True),
    "b, operands flushed": dict(rule="b", flush_in=True),
    "b, results flushed": dict(rule="b", flush_out=True),
    "b, both flushed": dict(rule="b", flush_in=True, flush_out=True),
}
HW = "a"                                      # what an MI355X was found to follow (docs/KERNEL_NOTES.md 4.15)


def probe_expect(name):
    """[ncases] float32: the probe scores under emulation `name` (each probe is its own (q, g) pair)"""
    cases = probe_cases()
    return chain(np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases]), pairwise=True, **EMULATIONS[name])


def float_case(seed=46, N=300, F=40):
    """Gaussian unit rows and queries, queries scaled off unit length, and adversarial pairs: heavy cancellation (rows 0 .. 9 against
    queries 0 .. 9: the query is the row with alternating signs re-balanced so the float64 dot is ~1e-7 of sum |q g|) and magnitudes
    spread over 2^+-20 (rows 10 .. 19 / queries 10 .. 19)"""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((N, D)); G /= np.linalg.norm(G, axis=1, keepdims=True)
    Q = rng.standard_normal((F, D)); Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    Q[20:24] *= np.array([1.7, 0.01, 300.0, 0.6])[:, None]
    Q[24:28] = G[100:104] * np.array([1.0, 0.999, 1.3, -1.0])[:, None]
    for j in range(10):
        g = G[j]
        sgn = np.where(np.arange(D) % 2 == 0, 1.0, -1.0)
        q = sgn / np.where(np.abs(g) < 1e-3, 1e-3, g) / D          # products +-1/D alternating
        q[D - 1] -= float(q @ g) / g[D - 1]                         # re-balance: the float64 dot is (nearly) zero
        Q[j] = q
    spread = 2.0 ** rng.integers(-20, 21, (10, D))
    G[10:20] = rng.standard_normal((10, D)) * spread
    Q[10:20] = rng.standard_normal((10, D)) / spread * 2.0 ** rng.integers(-20, 21, (10, D)) / 64
    Q, G = Q.astype(F32), G.astype(F32)
    S64 = Q.astype(np.float64) @ G.astype(np.float64).T
    mag = np.abs(Q).astype(np.float64) @ np.abs(G).astype(np.float64).T
    assert (np.abs(S64[np.arange(10), np.arange(10)]) < 1e-6 * mag[np.arange(10), np.arange(10)]).all()
    return Q, G, S64


def adversarial_pairs(seed=47):
    """(name, q, g) pairs in the layout of probe_cases (element 511 reserved): heavy cancellation - products of alternating sign and
    (nearly) equal size, re-balanced so the float64 dot is below 1e-6 of sum |q g| - at unit scale and with the sizes ramping over 2^20;
    element magnitudes spread over 2^+-20 in q, in g, and in both.  A pair whose emulated score is <= -1/2 is negated (the scan lists
    nothing at or below -1)."""
    rng = np.random.default_rng(seed)
    n = D - 1
    out = []
    for j in range(24):
        g = rng.standard_normal(n)
        g = np.where(np.abs(g) < 1e-2, 1e-2, g)
        size = 2.0 ** (np.arange(n) * (20.0 / n)) if j % 3 == 2 else np.ones(n)
        if j % 3 == 1:
            size = size[rng.permutation(n)] * 2.0 ** rng.integers(-3, 4, n)
        q = np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * size / g / n
        q, g = q.astype(F32).astype(np.float64), g.astype(F32).astype(np.float64)
        for _ in range(3):                                         # re-balance on the rounded operands
            q[n - 1 - j] -= float(q @ g) / g[n - 1 - j]
            q = q.astype(F32).astype(np.float64)
        assert abs(q @ g) < 1e-6 * (np.abs(q) @ np.abs(g)), j
        out.append((f"cancel{j}", q, g))
    for j in range(24):
        eq, eg = rng.integers(-20, 21, n), rng.integers(-20, 21, n)
        q = rng.standard_normal(n) * 2.0 ** (eq if j % 3 != 1 else 0) / 64
        g = rng.standard_normal(n) * 2.0 ** (eg if j % 3 != 0 else -eq)
        out.append((f"spread{j}", q, g))
    cases = []
    for name, q, g in out:
        q, g = np.append(q, 1.0).astype(F32), np.append(g, 0.0).astype(F32)
        if chain(q[None], g[None], **EMULATIONS[HW])[0, 0] <= -0.5:
            q[:n] = -q[:n]
        cases.append((name, q, g))
    return cases


# ---------------------------------------------------------------- C. the VALU consumers, float32
def wave_sum(v, offsets=(32, 16, 8, 4, 2, 1)):
    """[..., 64] float32 -> [...]: v += shfl_xor(v, o) for o = 32 .. 1 (every lane ends with the same bits: a + b == b + a)"""
    v = np.asarray(v, F32)
    lane = np.arange(64)
    for o in offsets:
        v = (v + v[..., lane ^ o]).astype(F32)
    return v[..., 0]


def lane_dot8(q, g, fused=False):
    """row_dot_lane8: [..., 64, 8] x [..., 64, 8] -> [..., 64], eight rounded products summed left to right"""
    if fused:                                                      # a fault: contraction to fmaf(q_k, g_k, s)
        s = (q[..., 0] * g[..., 0]).astype(F32)
        for k in range(1, 8):
            s = fma32(q[..., k], g[..., k], s)
        return s
    p = (q * g).astype(F32)
    s = p[..., 0]
    for k in range(1, 8):
        s = (s + p[..., k]).astype(F32)
    return s


def row_dot_wave8(Q, G, offsets=(32, 16, 8, 4, 2, 1), fused=False):
    """[F][N] float32: the score of gallery_first_above / first_above_blocked (lane l holds elements 8l .. 8l + 7)"""
    Q, G = np.asarray(Q, F32), np.asarray(G, F32)
    out = np.empty((len(Q), len(G)), F32)
    g = G.reshape(len(G), 64, 8)
    for f in range(len(Q)):
        out[f] = wave_sum(lane_dot8(Q[f].reshape(1, 64, 8), g, fused), offsets)
    return out


def _lane_strided_sum(x):
    """[..., D] -> [..., 64]: lane l sums x[l], x[l + 64], ... in order, starting from 0.f (zero padding adds +0: the same bits)"""
    Dx = x.shape[-1]
    pad = (-Dx) % 64
    x = np.concatenate([x, np.zeros(x.shape[:-1] + (pad,), F32)], -1).reshape(x.shape[:-1] + (-1, 64))
    s = np.zeros(x.shape[:-2] + (64,), F32)
    for i in range(x.shape[-2]):
        s = (s + x[..., i, :]).astype(F32)
    return s


def cosine_rows(A, B):
    """fr_cosine_matrix_f32: [F][N] float32"""
    A, B = np.asarray(A, F32), np.asarray(B, F32)
    ab = wave_sum(_lane_strided_sum((A[:, None, :] * B[None, :, :]).astype(F32)))
    aa = wave_sum(_lane_strided_sum((A * A).astype(F32)))
    bb = wave_sum(_lane_strided_sum((B * B).astype(F32)))
    den = (np.sqrt(aa)[:, None] * np.sqrt(bb)[None, :]).astype(F32)
    return (ab / den).astype(F32)


def l2norm_rows(X, offsets=(32, 16, 8, 4, 2, 1)):
    """fr_l2norm_rows_f32 (D % 4 == 0): lane l takes the float4s at 4l, 4l + 256, ...; ss += ((x^2 + y^2) + z^2) + w^2"""
    X = np.asarray(X, F32)
    R, Dx = X.shape
    pad = (-Dx) % 256
    x = np.concatenate([X, np.zeros((R, pad), F32)], 1).reshape(R, -1, 64, 4)
    sq = (x * x).astype(F32)
    ss = np.zeros((R, 64), F32)
    for i in range(x.shape[1]):
        t = sq[:, i, :, 0]
        for c in range(1, 4):
            t = (t + sq[:, i, :, c]).astype(F32)
        ss = (ss + t).astype(F32)
    nrm = np.sqrt(wave_sum(ss, offsets)).astype(F32)
    return (X / nrm[:, None]).astype(F32)


def l2norm_case(Dx, rows=67):
    """rows of very different lengths; 67 rows: 16 blocks of 4 waves and one of 3"""
    rng = np.random.default_rng(Dx)
    return (rng.standard_normal((rows, Dx)) * 2.0 ** rng.integers(-6, 7, (rows, 1))).astype(F32)


def mean_rows(X):
    """fr_mean_rows_f32: rows summed in order from 0.f, divided by (float) K"""
    X = np.asarray(X, F32)
    s = np.zeros(X.shape[1], F32)
    for k in range(len(X)):
        s = (s + X[k]).astype(F32)
    return (s / F32(len(X))).astype(F32)


# ---------------------------------------------------------------- D. the scan's structure, with faults to plant
FAULTS = ("partial_tile_dropped", "reg_skipped", "h1_dropped", "lap_stride", "lane_ge", "no_row_rule", "insert_equal",
          "merge_cut_half", "merge_cut_wave", "merge_cut_block", "ge_minus_one", "slot_returned", "offset_on_empty", "mask_ignored")


def _before(as_, ai, bs, bi, higher=False):
    tie = (ai > bi) if higher else (ai < bi)
    return (ai >= 0) & ((bi < 0) | (as_ > bs) | ((as_ == bs) & tie))


def _merge(s, i, os_, oi, cut_higher=False):
    """TopK::merge of topk_list.h on [..., KP] arrays: the cut c[j] = better(a[j], o[KP-1-j]), then log2(KP) compare-exchange stages"""
    KP = s.shape[-1]
    rs, ri = os_[..., ::-1], oi[..., ::-1]
    take = _before(rs, ri, s, i, cut_higher)
    s, i = np.where(take, rs, s), np.where(take, ri, i)
    d = KP // 2
    while d >= 1:
        j = np.arange(KP)
        lo = j[(j & d) == 0]
        sw = _before(s[..., lo + d], i[..., lo + d], s[..., lo], i[..., lo])
        s2, i2 = s.copy(), i.copy()
        s2[..., lo] = np.where(sw, s[..., lo + d], s[..., lo]); i2[..., lo] = np.where(sw, i[..., lo + d], i[..., lo])
        s2[..., lo + d] = np.where(sw, s[..., lo], s[..., lo + d]); i2[..., lo + d] = np.where(sw, i[..., lo], i[..., lo + d])
        s, i = s2, i2
        d //= 2
    return s, i


def _insert(s, i, v, gi, ok, equal=False):
    """TopK::insert on [..., KP]: v [...] goes behind every entry with score >= v (fault `equal`: before every entry with score <= v)"""
    KP = s.shape[-1]
    pos = ((s > v[..., None]) if equal else (s >= v[..., None])).sum(-1)
    pos = np.where(ok, pos, KP)[..., None]
    j = np.arange(KP)
    sh_s = np.concatenate([s[..., :1], s[..., :-1]], -1)
    sh_i = np.concatenate([i[..., :1], i[..., :-1]], -1)
    ns = np.where(j < pos, s, np.where(j == pos, v[..., None], sh_s))
    ni = np.where(j < pos, i, np.where(j == pos, gi[..., None], sh_i))
    return ns, ni


def emulate_scan(S, K=None, row_offset=0, mask=None, slots=None, fault=None):
    """What fr_gallery_match_f32 (K None) / fr_gallery_topk_f32 (and their view forms: S in view order, `slots` the view) return for the
    float32 score matrix S [F][N], by the kernels' own structure: grid of scan_blocks(N) x 4 waves, one 32-row tile per wave and step of
    the grid-stride loop, a lane's 16 registers in order, half-wave / wave / block merges, the '> -1' rule, row_offset, the mask.
    `fault`: one of FAULTS."""
    assert fault is None or fault in FAULTS
    S = np.asarray(S, F32)
    F, N = S.shape
    nblk = scan_blocks(N)
    ntiles = (N + 31) // 32
    stride = nblk * 4 + (1 if fault == "lap_stride" else 0)
    nlaps = max((ntiles + stride - 1) // stride, 1) if ntiles else 0
    topk = K is not None
    KP = kp_of(K) if topk else 1
    Kc = K if topk else 1
    tile0 = (np.arange(nblk)[:, None] * 4 + np.arange(4)[None, :])[:, :, None]             # [nblk][4][1]
    hh = np.arange(2)[None, None, :]                                                    # [1][1][2]
    s = np.full((F, nblk, 4, 2, KP), -np.inf, F32)
    i = np.full((F, nblk, 4, 2, KP), -1, np.int64)
    Nscan = N - N % 32 if fault == "partial_tile_dropped" else N
    for lap in range(nlaps):
        for reg in range(16):
            if fault == "reg_skipped" and reg == 5:
                continue
            gi = (tile0 + lap * stride) * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * hh     # [nblk][4][2]
            ok = (gi < Nscan) & (tile0 + lap * stride < ntiles)
            if fault == "h1_dropped":
                ok = ok & (hh == 0)
            v = np.where(ok[None], S[:, np.where(ok, gi, 0)], -np.inf).astype(F32)       # [F][nblk][4][2]
            gib = np.broadcast_to(gi[None], v.shape)
            okb = np.broadcast_to(ok[None], v.shape)
            if topk:
                s, i = _insert(s, i, v, gib, okb, equal=fault == "insert_equal")
            else:
                up = okb & ((v >= s[..., 0]) if fault == "lane_ge" else (v > s[..., 0]))
                s[..., 0] = np.where(up, v, s[..., 0]); i[..., 0] = np.where(up, gib, i[..., 0])
    norule = fault == "no_row_rule"

    def better(bs, bi, cs, ci):                                     # take_better(bs, bi, cs, ci), guarded by ci >= 0
        up = (ci >= 0) & ((cs > bs) | ((cs == bs) & (ci < bi) & (not norule)))
        return np.where(up, cs, bs), np.where(up, ci, bi)

    if topk:
        ts, ti = _merge(s[:, :, :, 0], i[:, :, :, 0], s[:, :, :, 1], i[:, :, :, 1], fault == "merge_cut_half")   # [F][nblk][4][KP]
        bs, bi = ts[:, :, 0], ti[:, :, 0]
        for w in range(1, 4):
            bs, bi = _merge(bs, bi, ts[:, :, w], ti[:, :, w], fault == "merge_cut_wave")
        bs, bi = bs.copy(), bi.copy()
        bs[..., Kc:], bi[..., Kc:] = -np.inf, -1                   # the workspace holds K entries per list
        ls = np.full((F, 64, KP), -np.inf, F32)
        li = np.full((F, 64, KP), -1, np.int64)
        for b0 in range(0, nblk, 64):
            n = min(64, nblk - b0)
            ms, mi = _merge(ls[:, :n], li[:, :n], bs[:, b0:b0 + n], bi[:, b0:b0 + n], fault == "merge_cut_block")
            ls[:, :n], li[:, :n] = ms, mi
        lane = np.arange(64)
        for m in (32, 16, 8, 4, 2, 1):
            ls, li = _merge(ls, li, ls[:, lane ^ m], li[:, lane ^ m], fault == "merge_cut_block")
        fs, fi = ls[:, 0, :Kc], li[:, 0, :Kc]
    else:
        hs, hi = s[:, :, :, 0, 0], i[:, :, :, 0, 0]
        hs, hi = better(hs, hi, s[:, :, :, 1, 0], i[:, :, :, 1, 0])
        bs, bi = hs[:, :, 0], hi[:, :, 0]
        for w in range(1, 4):
            bs, bi = better(bs, bi, hs[:, :, w], hi[:, :, w])
        fs, fi = np.full(F, -np.inf, F32), np.full(F, -1, np.int64)
        for b in range(nblk):
            fs, fi = better(fs, fi, bs[:, b], bi[:, b])
        fs, fi = fs[:, None], fi[:, None]
    has = (fi >= 0) & ((fs >= -1.0) if fault == "ge_minus_one" else (fs > -1.0))
    if mask is not None and fault != "mask_ignored":
        has = has & (np.asarray(mask)[:, None] > 0)
    if slots is not None and fault == "slot_returned":
        fi = np.where(fi >= 0, np.asarray(slots)[np.maximum(fi, 0)], fi)
    idx = np.where(has, fi + row_offset, -1 + (row_offset if fault == "offset_on_empty" else 0)).astype(np.int64)
    score = np.where(has, fs, F32(-1.0)).astype(F32)
    return (idx, score) if topk else (idx[:, 0], score[:, 0])
