"""References for the coarse gallery scan (csrc/scan_gemm.hip) and the premises of the certified coarse top-K, plain
numpy on the CPU, shared by tests/test_coarse_ref_host.py (CPU) and tests/test_gpu_coarse_pins.py (GPU).

A. `coarse_ref`: what fr_gallery_match_f16 / _f8 return with G32 == NULL - the coarse maximum per query and the first row of the first
   group of 4 rows that attains it - on operands whose every product and partial sum is exact in f32 (`assert_exact`, and for fp8 the
   13-bit window of the matrix instruction, KERNEL_NOTES 4.12), so the comparison is bit for bit; `emulate_scan` plants faults.
B. `eps_families`: operand pairs built to approach each term of the bound eps of DESIGN.md 4.6b; `eps_bound` is that bound, quoted, not
   measured; `emulate_dot` is a float32 model of the scan's arithmetic with faults to plant.
C. `topk_group`: galleries on which the coarse order and the exact order disagree by less than eps, one per path on which the scan lets a
   group go; `emulate_topk` replays the lists, the spill bounds and the certificate, with each spill update removable.
"""
import functools
from types import SimpleNamespace

import numpy as np

from tests.helpers import f8_ref as fr

D = 512
ROWS = 64                                     # gallery rows per LDS tile (SG_ROWS)
QB = 256                                      # queries per block (SG_QB)
TOPK = {"f16": 4, "f8": 8}                    # FR_TOPK / FR_TOPK8: groups a list keeps
F8_SCALE = 256.0
U = 2.0 ** -11                                # f16 unit roundoff


# ---------------------------------------------------------------- the scan plan, as the public workspace size shows it
def plan(F, N):
    """scan_plan of scan_gemm.hip: (nqt, nranges, rows per range).  Tests never trust this copy: `check_plan` holds it to the library."""
    nqt = max((F + QB - 1) // QB, 1)
    tiles = max((N + ROWS - 1) // ROWS, 1)
    want = max(256 // nqt, 8)
    nr = min(tiles, want)
    tpr = (tiles + nr - 1) // nr
    nr = (tiles + tpr - 1) // tpr
    return SimpleNamespace(nqt=nqt, nranges=nr, rows_per_range=tpr * ROWS, tiles_per_range=tpr)


def check_plan(ws_bytes, F, N, kind="f16"):
    """nranges from fr_gallery_match_f16_workspace / _f8_workspace (F * nranges * 4 * TOPK * 8 + 256), asserted equal to `plan`: a later
    change of the scan plan fails here, loudly, and not a case that silently stopped reaching its path"""
    per = max(F, 1) * 4 * TOPK[kind] * 8
    assert (ws_bytes - 256) % per == 0, (ws_bytes, F, N)
    pl = plan(F, N)
    assert (ws_bytes - 256) // per == pl.nranges, ("the scan plan changed", (ws_bytes - 256) // per, pl.nranges)
    return pl


# ---------------------------------------------------------------- A. exact coarse scores
def stored(X, kind):
    """the operand as the scan holds it, float64: f16 (RNE, subnormals kept); fp8: the e4m3 code of x * 256, saturating at +-448"""
    X = np.asarray(X, np.float32)
    if kind == "f16":
        with np.errstate(over="ignore"):
            return X.astype(np.float16).astype(np.float64)
    return fr.e4m3(X.astype(np.float64) * F8_SCALE)


def unscale(kind):
    return 1.0 if kind == "f16" else 1.0 / (F8_SCALE * F8_SCALE)


def assert_exact(Qs, Gs, kind):
    """every product and every partial sum, in any order, is exact in f32: all terms are multiples of one quantum and sum |q g| (bounded
    by Cauchy-Schwarz over the worst pair) stays below 2^24 quanta; fp8: in every group of 8 channels all non-zero products lie within
    2^13 of one another (bounded by the extreme magnitudes of the group over all rows and queries)"""
    qq, qg = int(fr.frac_bits(Qs).max()), int(fr.frac_bits(Gs).max())
    worst = np.sqrt((Qs * Qs).sum(1).max() * (Gs * Gs).sum(1).max()) * 2.0 ** (qq + qg)
    assert worst < 2.0 ** 24, worst
    if kind == "f8":
        assert qq == 0 and qg == 0
        aq, ag = np.abs(Qs).reshape(len(Qs), -1, 8), np.abs(Gs).reshape(len(Gs), -1, 8)
        big = aq.max((0, 2)) * ag.max((0, 2))
        small = np.where(aq > 0, aq, np.inf).min((0, 2)) * np.where(ag > 0, ag, np.inf).min((0, 2))
        assert (big[np.isfinite(small)] < small[np.isfinite(small)] * 2.0 ** fr.ALIGN_BITS).all()
    return float(worst)


def scores(Q, G, kind):
    """[F][N] float64 coarse scores (f16: dots of the f16 operands; fp8: integer dots of the codes), exactness asserted"""
    Qs, Gs = stored(Q, kind), stored(G, kind)
    assert_exact(Qs, Gs, kind)
    return Qs @ Gs.T


def pick(S, kind, row_offset=0):
    """per query: (first row of the first group of 4 rows attaining the maximum, + row_offset; the maximum x coarse_unscale as f32), or
    (-1, -1.0) if no score exceeds -1.  S: [F][N]"""
    F, N = S.shape
    gm = np.maximum.reduceat(S, np.arange(0, N, 4), axis=1)               # group maxima; the last group may hold fewer than 4 rows
    g = gm.argmax(1)                                                   # first maximum
    sc = (gm[np.arange(F), g] * unscale(kind))
    assert fr.is_f32(sc).all()
    ok = sc.astype(np.float32) > np.float32(-1.0)
    return np.where(ok, g * 4 + row_offset, -1).astype(np.int64), np.where(ok, sc, -1.0).astype(np.float32)


def coarse_ref(Q, G, kind, row_offset=0):
    return pick(scores(Q, G, kind), kind, row_offset)


def rerank_ref(S, kind):
    """the view forms re-rank exactly against f32 rows that hold the same integers: (first ROW attaining the maximum, the maximum)"""
    r = S.argmax(1)
    sc = S[np.arange(len(S)), r] * unscale(kind)
    ok = sc > -1
    return np.where(ok, r, -1).astype(np.int64), np.where(ok, sc, -1.0).astype(np.float32)


def brute_ref(Q, G, kind, row_offset=0):
    """coarse_ref as a plain loop, integer arithmetic: the reference's reference"""
    Qs, Gs = stored(Q, kind), stored(G, kind)
    q = 2.0 ** max(int(fr.frac_bits(Qs).max()), int(fr.frac_bits(Gs).max()))
    Qi, Gi = np.rint(Qs * q).astype(np.int64), np.rint(Gs * q).astype(np.int64)
    idx, sc = [], []
    for f in range(len(Qi)):
        best, bg = None, -1
        for r in range(len(Gi)):
            s = int((Qi[f] * Gi[r]).sum())
            if best is None or s > best:
                best, bg = s, r // 4
        val = np.float32(best / (q * q) * unscale(kind))
        idx.append(bg * 4 + row_offset if val > -1 else -1)
        sc.append(val if val > -1 else np.float32(-1))
    return np.array(idx, np.int64), np.array(sc, np.float32)


@functools.lru_cache(maxsize=4)
def exact_gallery(N, kind, variant="plain"):
    """-> (G f32 [N][512], qmul, the stored rows, the stored queries qmul * G): rows of small signed integers times a dyadic quantum; the
    queries of a launch are qmul * G[pi], so with F = N its score matrix is a row permutation of ONE matrix, computed once per gallery.
    Every row wins its own query (asserted by `planted`).
      plain     integers in [-3, 3]; f16: x 1/8 (queries x 1/4), fp8: x 1/256 (codes = the integers)
      negative  integers in [0, 3], queries -2^-13 x the row (f16: rows as integers): every score in (-1, 0), a zero row would win
      offgrid   fp8 only: 17, 19, 21, 23, 26 / 256 (rounded by the conversion, ties to even) among the integers, and channels 8 .. 15 of
                every row beyond the e4m3 range (+-2, +-1.8, +-7 -> +-448, so that group of 8 meets the window on its own)"""
    rng = np.random.default_rng(1000 + N + (0 if kind == "f16" else 7) + {"plain": 0, "negative": 100_000, "offgrid": 200_000}[variant])
    if variant == "negative":
        K = rng.integers(0, 4, (N, D)).astype(np.float64)
        G = K if kind == "f16" else K / F8_SCALE
        qmul = -2.0 ** -13 if kind == "f16" else -1.0
        if kind == "f8":                                               # codes k against -k: scores -sum k k' / 65536 in (-1, 0)
            assert (K * K).sum(1).max() < 65536
    else:
        K = rng.integers(-3, 4, (N, D)).astype(np.float64)
        if variant == "offgrid":
            assert kind == "f8"
            odd = rng.random((N, D)) < 0.03
            K[odd] = rng.choice([17.0, 19.0, 21.0, 23.0, 26.0, -17.0, -19.0, -21.0, -23.0], int(odd.sum()))
            K[:, 8:16] = rng.choice([2.0, -2.0, 1.8, -1.8, 7.0, -7.0], (N, 8)) * F8_SCALE
        G = K / 8 if kind == "f16" else K / F8_SCALE
        qmul = 2.0 if kind == "f16" else 1.0
    G = G.astype(np.float32)
    Gs = stored(G, kind)
    Qs = stored((qmul * G).astype(np.float32), kind)
    assert_exact(Qs, Gs, kind)
    for a in (G, Gs, Qs):
        a.setflags(write=False)
    return G, qmul, Gs, Qs


@functools.lru_cache(maxsize=2)
def _self_scores(N, kind, variant):
    _, _, Gs, Qs = exact_gallery(N, kind, variant)
    S = Qs @ Gs.T
    S.setflags(write=False)
    return S


def planted(N, kind, pi, variant="plain"):
    """the launch "query f = qmul * row pi[f]": (Q f32, G f32, S [F][N]); asserts that row pi[f] wins query f, alone (plain / offgrid)"""
    G, qmul, Gs, Qs = exact_gallery(N, kind, variant)
    pi = np.asarray(pi)
    Q = (qmul * G[pi]).astype(np.float32)
    S = _self_scores(N, kind, variant)[pi] if len(pi) == N else Qs[pi] @ Gs.T
    if variant != "negative":
        win = S[np.arange(len(pi)), pi].copy()
        assert (S.argmax(1) == pi).all()
        if N > 1:
            S[np.arange(len(pi)), pi] = -np.inf
            assert (S.max(1) < win).all()                                  # a unique maximum
            S[np.arange(len(pi)), pi] = win
    else:
        assert (S < 0).all() and (S * unscale(kind) > -1).all()
    return Q, G, S


def permutations(N, F=None):
    """identity, and two multiplications by an odd constant mod N (+ an offset): a row's slot (row mod 64, range) is decorrelated from
    its query's slot (query mod 256: wave, n-tile, lane)"""
    F = N if F is None else F
    f = np.arange(F)
    out = [f % N]
    for c, off in ((1597, 0), (7919, 29)):
        assert np.gcd(c, N) == 1
        out.append((c * f + off) % N)
    return out


# (N, F) of the issue's table; F < N: the first F queries of each permutation
SCAN_SHAPES = [(1, 1), (63, 63), (64, 64), (67, 67), (4097, 4097), (4097, 1), (4097, 33), (4097, 257), (4097, 300), (16448, 256)]
SCAN_PLANS = {(4097, 4097): (17, 13, 5), (4097, 257): (2, 65, 1), (4097, 33): (1, 65, 1), (16448, 256): (1, 129, 2), (67, 67): (1, 2, 1)}


def launches(N, F):
    """the row each query of each launch plants; 16 448 rows x 256 queries: the first 256 rows, the last 256 (the short last range) and a
    stride through all ranges and both tiles of a range"""
    if (N, F) == (16448, 256):
        f = np.arange(F)
        return [f, N - F + f, (1597 * f + 77) % N]
    return permutations(N, F)


SCAN_FAULTS = ("drop_chunk", "swap_halves", "unmasked_tail")


_STORED = {}


def _stored_rows(G, kind):
    """stored(G) of a gallery that exact_gallery made (read-only, kept alive by its cache): converted once"""
    if G.flags.writeable:
        return stored(G, kind)
    key = (id(G), kind)
    if key not in _STORED:
        if len(_STORED) >= 4:
            _STORED.clear()
        _STORED[key] = (G, stored(G, kind))
    return _STORED[key][1]


def emulate_scan(Q, G, kind, fault=None, row_offset=0, S=None):
    """The scan's result from a score matrix built the way the kernel builds it, with one fault:
      drop_chunk     tile rows 16 .. 31 (the second 16-row MFMA block of every tile) lose one 128-byte chunk of K (f16: 64 columns,
                     fp8: 128), chunk 1
      swap_halves    lane quarter 2 reads its lo and hi 16 bytes of chunk 0 the wrong way round on the gallery side (f16: columns
                     16 .. 23 against the query's 48 .. 55 and vice versa; fp8: 32 .. 47 against 96 .. 111)
      unmasked_tail  the rows past the end of the last tile (zeros) stay candidates
    S: the unfaulted score matrix where the caller has it already (large shapes); it is not modified"""
    Qs, Gs = stored(Q, kind), _stored_rows(G, kind)
    S = Qs @ Gs.T if S is None else S.copy()
    N = len(Gs)
    cw, hw = (64, 8) if kind == "f16" else (128, 16)
    if fault == "drop_chunk":
        rows = np.flatnonzero((np.arange(N) % ROWS >= 16) & (np.arange(N) % ROWS < 32))
        S[:, rows] -= Qs[:, cw:2 * cw] @ Gs[rows, cw:2 * cw].T
    elif fault == "swap_halves":
        lo, hi = np.arange(2 * hw, 3 * hw), cw // 2 + np.arange(2 * hw, 3 * hw)
        S += Qs[:, hi] @ Gs[:, lo].T + Qs[:, lo] @ Gs[:, hi].T - Qs[:, lo] @ Gs[:, lo].T - Qs[:, hi] @ Gs[:, hi].T
    elif fault == "unmasked_tail":
        S = np.concatenate([S, np.zeros((len(Qs), (-N) % ROWS))], axis=1)
    idx, sc = pick(S, kind, row_offset)
    return idx, sc


# ---------------------------------------------------------------- B. the bound eps of DESIGN.md 4.6b
def eps_bound(q, g, full=True):
    """|coarse - float64 dot of the f32 operands| <= [(2u + u^2) + 2^-14 (1 + u)^2 (1 + 2^-14)] |q||g| + 2^-20 (|q| + |g|) + 2^-40 with the
    row's own norm for Gmax; operands exactly representable in f16 (full=False): the accumulation term alone"""
    nq, ng = np.linalg.norm(np.asarray(q, np.float64)), np.linalg.norm(np.asarray(g, np.float64))
    acc = 2.0 ** -14 * (1 + U) ** 2 * (1 + 2.0 ** -14) * nq * ng
    if not full:
        return acc
    return (2 * U + U * U) * nq * ng + acc + 2.0 ** -20 * (nq + ng) + 2.0 ** -40


def cert_eps(qn, gmax):
    """the kernel's eps: FR_CERT_C 2^-10 |q| Gmax + FR_CERT_ABS (|q| + Gmax) + 2^-40"""
    return 1.125 * 2.0 ** -10 * qn * gmax + 2.0 ** -20 * (qn + gmax) + 2.0 ** -40


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def eps_families():
    """-> list of probes (name, family, q f32 [512], g f32 [512], full, exact, s): `full` selects the bound; `exact`: every partial sum
    of the exact f16 products, in any order, is an f32 number, so the result is asserted bit-equal as well; s: family 3's exponent"""
    rng = np.random.default_rng(46)
    out = []

    def add(name, fam, q, g, full, exact=False, s=None):
        q, g = _f32(q), _f32(g)
        d = float(q.astype(np.float64) @ g.astype(np.float64))
        assert d > 0, name                                                 # the planted row is the clear maximum over rows scoring 0
        if not full:
            assert np.array_equal(stored(q, "f16"), q) and np.array_equal(stored(g, "f16"), g), name
        if exact:
            assert fr.is_f32(d), name
        out.append(SimpleNamespace(name=name, family=fam, q=q, g=g, full=full, exact=exact, s=s, d=d))

    # 1. same-direction rounding: p = 2^e (1 + k 2^-10), k <= 8, on the f16 grid; x just below / just above the midpoint to the next
    #    grid point, and (a control that only a truncating conversion fails) just below the next grid point itself
    for sign in (1.0, -1.0):
        for tag, off in (("below", U * (1 - 2.0 ** -6)), ("above", U * (1 + 2.0 ** -6)), ("neargrid", 2 * U * (1 - 2.0 ** -5))):
            e = rng.integers(-5, -3, D)
            xy = []
            for _ in range(2):
                p = np.ldexp(1 + rng.integers(0, 9, D) * 2.0 ** -10, e)
                x = _f32(sign * p * (1 + off))
                assert np.array_equal(stored(x, "f16"), sign * (p if tag == "below" else p + np.ldexp(2.0 ** -10, e))), tag
                xy.append(x)
            add(f"round-{tag}-{'pos' if sign > 0 else 'neg'}", 1, xy[0], xy[1], True)
    # 2. f16 subnormals are kept
    add("subnormal-q", 2, np.full(D, 2.0 ** -20), np.full(D, 1024.0), False, exact=True)
    add("subnormal-g", 2, np.full(D, 1024.0), np.full(D, 2.0 ** -20), False, exact=True)
    q = np.r_[np.full(256, 512.0), np.full(256, 2.0 ** -6)]
    g = np.r_[np.full(256, 2.0 ** -18), np.full(256, 0.25)]                # half subnormal, half normal: 0.5 + 1.0
    perm = rng.permutation(D)
    add("subnormal-mixed", 2, q[perm], g[perm], False, exact=True)
    for tag, frac in (("0.49", 0.49), ("0.51", 0.51), ("0.90", 0.90)):    # between subnormal grid points k 2^-24
        add(f"subnormal-between-{tag}", 2, (rng.integers(0, 31, D) + frac) * 2.0 ** -24, np.full(D, 1024.0), True)
    # 3. the accumulation window of one v_mfma_f32_16x16x32_f16: per block of 32 columns one product 1.0 and 31 products 2^-s
    for alt in (False, True):
        for s in range(8, 24):
            a = s // 2
            for pos in range(32):
                q, g = np.full(D, 2.0 ** -a), np.full(D, 2.0 ** -(s - a))
                big = np.arange(16) * 32 + pos
                q[big] = 1.0
                g[big] = np.where(np.arange(16) % 2 == 1, -1.0, 1.0) if alt else 1.0
                add(f"window-{'alt' if alt else 'pos'}-s{s}-p{pos}", 3, q, g, False, s=s)
                assert fr.is_f32(out[-1].d)                                 # representable: bit-exactness is reported, not required
    # 4. range edges
    sg = rng.choice([-1.0, 1.0], D)
    add("edge-65504-all", 4, 65504.0 * sg, 2.0 ** -14 * sg, False, exact=True)
    flip = np.where(np.arange(D) % 4 == 3, -1.0, 1.0)                      # a quarter of the products negative
    add("edge-65504-cancel", 4, 65504.0 * sg, 2.0 ** -14 * sg * flip, False, exact=True)
    add("edge-65504-offgrid", 4, 65504.0 * sg * (1 - rng.random(D) * 2.0 ** -12), 2.0 ** -14 * sg * (1 + rng.random(D) * 2.0 ** -3), True)
    w = rng.standard_normal(D)
    w /= np.linalg.norm(w)
    v = rng.standard_normal(D)
    v = 0.7 * w + 0.3 * v / np.linalg.norm(v)
    add("edge-norm300", 4, 300.0 * w, v / np.linalg.norm(v), True)
    return out


DOT_FAULTS = ("flush", "window13", "trunc")


def _f16_trunc(x):
    h = np.asarray(x, np.float32).astype(np.float16)
    over = np.abs(h.astype(np.float64)) > np.abs(np.asarray(x, np.float64))
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float64)


def emulate_dot(q, g, fault=None):
    """The coarse scores of [P] (query, row) pairs ([P][512] each) in a float32 model: operands to f16 (RNE), exact products, 512
    sequential f32 additions.  Faults: "flush": f16 subnormal operands read as zero; "trunc": the conversion rounds towards zero;
    "window13": inside a block of 32 columns every product is cut, towards zero, to a multiple of 2^-13 of the block's largest (what the
    fp8 instruction does to 8 neighbours)"""
    q, g = np.atleast_2d(q), np.atleast_2d(g)
    qh, gh = (_f16_trunc(q), _f16_trunc(g)) if fault == "trunc" else (stored(q, "f16"), stored(g, "f16"))
    if fault == "flush":
        qh, gh = np.where(np.abs(qh) < 2.0 ** -14, 0.0, qh), np.where(np.abs(gh) < 2.0 ** -14, 0.0, gh)
    prod = qh * gh                                                         # exact: 22-bit significands
    if fault == "window13":
        pb = prod.reshape(len(prod), -1, 32)
        top = np.abs(pb).max(2, keepdims=True)
        _, e = np.frexp(np.where(top > 0, top, 1.0))
        step = np.ldexp(1.0, e - 1 - 13)
        prod = (np.trunc(pb / step) * step).reshape(prod.shape)
    p32 = prod.astype(np.float32)
    assert np.array_equal(p32.astype(np.float64), prod)
    acc = np.zeros(len(p32), np.float32)
    for k in range(D):
        acc = (acc + p32[:, k]).astype(np.float32)
    return acc


# ---------------------------------------------------------------- C. "every unseen row has a coarse score <= B"
P16 = float(np.float16(0.7))                                               # row B's element: on the f16 grid
PA = float(np.float32(P16 + 0.48 * 2.0 ** -11))                            # row A's: 0.48 of the grid's spacing at 0.7 above it, so it rounds to P16
#                                                                            and its exact score is 2.3e-4 higher (a RELATIVE 0.4 * 2^-10 would round up here)
PC = float(np.float32(P16 * (1 + 2.0 ** -7)))                              # the positive controls' seen rows: 5.5e-3 higher
QC = float(np.float32(0.5 * (1 + 1.02 * U)))                               # the query's second element: f16 rounds it UP by nearly u
TOPK_N = 32768


def _row_x():
    """row X = (x0, x1) on the f16 grid with coarse(X) > coarse(A) = P16 and exact(X) < exact(A) = PA, both by as much as the grid allows"""
    qc16 = float(np.float16(QC))
    assert qc16 == 0.5 * (1 + 2 * U) and float(np.float16(PA)) == P16
    best = None
    for x1 in np.arange(0.5, 0.8, 2.0 ** -11):
        x0 = float(np.float16(P16 + 1e-4 - QC * x1))
        for x0 in (x0, x0 + 2.0 ** -12, x0 - 2.0 ** -12):
            m = min(x0 + qc16 * x1 - P16, PA - (x0 + QC * x1))
            if x0 * x0 + x1 * x1 < 1 and (best is None or m > best[0]):
                best = (m, x0, float(x1))
    return best


X_MARGIN, X0, X1 = _row_x()


def topk_rows(kind, f):
    """a planted row for query f, whose non-zero elements are 2 f (weight 1) and 2 f + 1 (weight QC)"""
    v = np.zeros(D, np.float32)
    if kind == "X":
        v[2 * f], v[2 * f + 1] = X0, X1
    else:
        v[2 * f] = {"A": PA, "B": P16, "C": PC}[kind]
    return v


def topk_query(f):
    q = np.zeros(D, np.float32)
    q[2 * f], q[2 * f + 1] = 1.0, QC
    return q


def background(N):
    """unit rows orthogonal to every query: e_(16 + r mod 496); every candidate, bound and exact score is known in closed form"""
    G = np.zeros((N, D), np.float32)
    G[np.arange(N), 16 + np.arange(N) % 496] = 1.0
    return G


def budget(K):
    """groups the re-rank re-scores (RerankBudget): 8 / 8 / 16 / 32 for KP = 2 / 4 / 8 / 16"""
    KP = 2 if K <= 2 else 4 if K <= 4 else 8 if K <= 8 else 16
    return 8 if KP <= 4 else 2 * KP


def _case(pl, N, layout, K, where, control, R0=0):
    """-> SimpleNamespace(name, layout, K, rows {row: kind}, a_row, seen [rows the lists keep], control).  A position is (range, tile, m,
    lane quarter, reg): row = range * rows_per_range + tile * 64 + m * 16 + 4 * quarter + reg; a list is (range, quarter).
    where: "mid" or "last" (A, or layout 3's last X, in the gallery's last group; the last tile may be partial)"""
    rpr, nr = pl.rows_per_range, pl.nranges
    pos = lambda R, t, m, fq, reg: R * rpr + t * ROWS + m * 16 + 4 * fq + reg           # noqa: E731
    C = budget(K)
    rows = {}
    if where == "last":
        fq = ((N - 1) % 16) // 4
        R, lt, lm, lreg = nr - 1, ((N - 1) % rpr) // ROWS, ((N - 1) % ROWS) // 16, (N - 1) % 4
        if layout == 4:
            R -= C
    else:
        fq, R, lt, lm, lreg = layout % 4, R0, 1, 1 + layout % 3, (layout + 1) % 4
    assert lt >= 1, "a range of one tile has no second tile to refuse"
    if layout == 1:                                                        # four B groups fill the list from tile 0; A ties in a later tile
        for m in range(4):
            rows[pos(R, 0, m, fq, m)] = "B"
        a = pos(R, lt, lm, fq, lreg)
    elif layout == 2:                                                      # [B B B 0]; X enters (pushing a 0 out), then A ties the kept minimum
        for m in range(3):
            rows[pos(R, 0, m, fq, 3 - m)] = "B"
        lm = max(lm, 1)
        rows[pos(R, lt, 0, fq, 2)] = "X"
        a = pos(R, lt, lm, fq, lreg)
    elif layout == 3:                                                      # A first, then four X: the fourth pushes A off the end
        a = pos(R, 0, 0, fq, 1)
        for m in range(1, 4):
            rows[pos(R, 0, m, fq, m)] = "X"
        rows[pos(R, lt, lm, fq, lreg)] = "X"
    else:                                                                  # C groups B in C lists with lower group ids; A in one more list
        for i in range(C):
            rows[pos(R + i, 0, i % 4, fq, i % 3)] = "B"
        a = pos(R + C, lt, lm, fq, lreg)
    seen = sorted(rows)
    assert a not in rows and max(max(rows), a) < N
    if where == "last":
        assert max(max(rows), a) // 4 == (N - 1) // 4
    if control:
        rows = {r: "C" for r in rows}
    rows[a] = "A"
    return SimpleNamespace(name=f"layout{layout}-K{K}-{where}{'-control' if control else ''}", layout=layout, K=K, rows=rows, a_row=a,
                           seen=seen, control=control)


TOPK_GROUPS = ("cases", "controls", "last1", "last2", "last3", "last4", "partial")


def topk_group(name):
    """-> SimpleNamespace(N, plan, cases [one per query], Q f32 [F][512], rows {row: vector}): one gallery = background + rows.
    cases / controls: layouts 1, 2, 3 and 4 at K = 1, 4 at K = 5 and K = 16, on queries 0 .. 5; last1 .. last4: one layout with A (layout 3:
    the fourth X) in rows N - 4 .. N - 1; partial: layout 1 at N = 32 771 (171 ranges of three tiles, the last tile holds 3 rows, A = N - 1)"""
    N = TOPK_N + 3 if name == "partial" else TOPK_N
    pl = plan(8, N)
    if name in ("cases", "controls"):
        spec = [(1, 1, 20), (2, 1, 50), (3, 1, 80), (4, 1, 100), (4, 5, 120), (4, 16, 150)]          # layout, K, first range
        cases = [_case(pl, N, lay, K, "mid", name == "controls", R0) for lay, K, R0 in spec]
    elif name == "partial":
        cases = [_case(pl, N, 1, 1, "last", False)]
        assert cases[0].a_row == N - 1 and N % ROWS == 3
    else:
        cases = [_case(pl, N, int(name[-1]), 1, "last", False)]
    rows = {}
    for f, c in enumerate(cases):
        for r, kind in c.rows.items():
            assert r not in rows
            rows[r] = topk_rows(kind, f)
    assert len(cases) <= 8                                                 # elements 0 .. 15 belong to the queries, 16 .. 511 to the background
    Q = np.stack([topk_query(f) for f in range(len(cases))])
    return SimpleNamespace(name=name, N=N, plan=pl, cases=cases, Q=Q, rows=rows)


def topk_gallery(grp):
    G = background(grp.N)
    for r, v in grp.rows.items():
        G[r] = v
    return G


def topk_truth(grp, f, K):
    """the exact top-K of query f in float64 (score descending, row ascending, scores > -1): planted rows, then background rows (score 0)"""
    q = grp.Q[f].astype(np.float64)
    sc = sorted(((-float(v.astype(np.float64) @ q), r) for r, v in grp.rows.items()))
    sc = [(s, r) for s, r in sc if s < 0]                                  # the other queries' rows score 0, like the background
    assert all(b[0] - a[0] > 1e-5 or a[0] == b[0] for a, b in zip(sc, sc[1:]))      # no near ties: f32 noise cannot reorder
    assert len(sc) >= K
    return [r for _, r in sc[:K]]


TOPK_MUTANTS = ("drop_door", "drop_insert", "drop_pushed", "read_c_plus_2", "read_c")


def emulate_topk(grp, f, K, mutant=None, gmax=1.0):
    """gallery_gemm_scan<SPILL> + gallery_rerank_topk for query f: the 4-entry lists per (range, lane quarter) with strict '>', the spill
    bound fed on the three paths a group leaves by, the C best groups by (coarse score, lowest group), B = max((C+1)-th, spills), exact
    re-scoring in float64, certified iff s_K > B + eps.  -> (flag, [rows of the list it would return]).
    Mutants: drop_door / drop_insert / drop_pushed: that spill update is missing; read_c_plus_2: the bound reads one candidate too far
    (unsound); read_c: one too early (sound, but refuses what it could certify)."""
    pl, N = grp.plan, grp.N
    q = grp.Q[f]
    coarse, exact = np.zeros(N), np.zeros(N)                               # the background is orthogonal to every query: exactly 0
    for r, v in grp.rows.items():
        coarse[r] = stored(v, "f16") @ stored(q, "f16")
        exact[r] = v.astype(np.float64) @ q.astype(np.float64)
    assert fr.is_f32(coarse).all()                                         # at most two non-zero products: no order of summation matters
    ninf = -np.inf
    gmx = np.concatenate([coarse, np.full((-N) % 4, ninf)]).reshape(-1, 4).max(1)
    cands, spills = [], []
    for R in range(pl.nranges):
        r0 = R * pl.rows_per_range
        nrows = min(N, r0 + pl.rows_per_range) - r0
        for fq in range(4):
            top, spill = [(ninf, -1)] * 4, ninf
            for t in range((nrows + ROWS - 1) // ROWS):
                gs = [(r0 + t * ROWS + m * 16 + 4 * fq) // 4 for m in range(4)]
                gm = [gmx[g] if g < len(gmx) and g * 4 < r0 + nrows else ninf for g in gs]
                if max(gm) > top[3][0]:
                    for s, g in zip(gm, gs):
                        if not s > top[3][0]:
                            if mutant != "drop_insert":
                                spill = max(spill, s)
                            continue
                        if mutant != "drop_pushed":
                            spill = max(spill, top[3][0])
                        top = sorted(top[:3] + [(s, g)], key=lambda e: -e[0])       # stable: the earlier group stays ahead on ties
                elif mutant != "drop_door":
                    spill = max(spill, max(gm))
            cands += [e for e in top if e[1] >= 0]
            spills.append(spill)
    C = budget(K)
    cands.sort(key=lambda e: (-e[0], e[1]))
    nth = C + 1 if mutant == "read_c_plus_2" else C - 1 if mutant == "read_c" else C
    bound = max(cands[nth][0] if len(cands) > nth else ninf, max(spills))
    rows = [r for _, g in cands[:C] for r in range(g * 4, g * 4 + 4) if r < N and exact[r] > -1]
    rows.sort(key=lambda r: (-exact[r], r))
    sk = exact[rows[K - 1]] if len(rows) >= K else -1.0
    flag = 0 if sk > bound + cert_eps(np.linalg.norm(q.astype(np.float64)), gmax) else 1
    return flag, rows[:K], SimpleNamespace(bound=bound, sk=sk, gap=sk - bound)
