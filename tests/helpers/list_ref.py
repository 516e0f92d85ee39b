"""Plain references and case tables for the three kernels that turn head maps into detections: fr_sort_nms (nms.hip),
fr_scrfd_decode (scrfd_decode.hip) and fr_pnet_candidates (detect_ops.hip).  Written from the operations' definitions
(oracle/detect.py, tests/helpers/scrfd_ref.py), never from the .hip sources: no chunks, no ballots, no templates.

All three are "ordered compaction + exact float32 formula": the references decide them bit for bit, the only tolerances
are on expf (scores / probabilities, 1e-6).  tests/test_list_ref_host.py validates the references and every precondition
a case rests on without a GPU; tests/test_gpu_list_kernels.py runs the kernels on the same tables.

Conventions of the case tables: a slot past its segment's count holds POISON (NaN boxes, NaN aux, score +inf) - a kernel
that reads one sorts it first; aux rows carry (list, entry index, column) so that a misrouted row shows; scores are
non-negative (probabilities): the kernel orders by the score's bit pattern, which is the float order only from +0 upwards.
"""
import functools
from collections import namedtuple

import numpy as np

from tests.helpers import scrfd_ref

F32 = np.float32
SENTINEL = 0x5A5AA5A5           # int32 bit pattern the outputs are prefilled with (3.8e15 as a float, no case produces it)


def bits(a):
    """float32 array -> its int32 bit patterns"""
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


# ------------------------------------------------------------------------------------------------------------ sort + NMS
class _Metric:
    """area(boxes [n,4]) and overlap(box, area, boxes [n,4], areas [n], mode) -> [n]; over(o, thr32) -> bool [n]"""


class IntMetric(_Metric):
    """Integer-valued boxes with every area below 2^24: all terms exact in float64, the quotient rounded to float32 (53 >=
    2*24 + 2: the double rounding equals the correctly rounded float32 division of the exact float32 operands)."""

    @staticmethod
    def area(b):
        b = b.astype(np.float64)
        return (b[:, 2] - b[:, 0] + 1.0) * (b[:, 3] - b[:, 1] + 1.0)

    @staticmethod
    def overlap(bi, ai, bj, aj, mode):
        bi, bj = bi.astype(np.float64), bj.astype(np.float64)
        w = np.maximum(0.0, np.minimum(bi[2], bj[:, 2]) - np.maximum(bi[0], bj[:, 0]) + 1.0)
        h = np.maximum(0.0, np.minimum(bi[3], bj[:, 3]) - np.maximum(bi[1], bj[:, 1]) + 1.0)
        inter = w * h
        den = np.minimum(ai, aj) if mode == 1 else ai + aj - inter
        return (inter / den).astype(F32)

    @staticmethod
    def over(o, thr32):
        return o > thr32


class F32Metric(_Metric):
    """float32 operation by operation, as oracle/detect.py nms() and scrfd_ref.iou_plus1 (one IEEE rounding each)"""

    @staticmethod
    def area(b):
        b = b.astype(F32)
        return ((b[:, 2] - b[:, 0] + F32(1)) * (b[:, 3] - b[:, 1] + F32(1))).astype(F32)

    @staticmethod
    def overlap(bi, ai, bj, aj, mode):
        bi, bj = bi.astype(F32), bj.astype(F32)
        xx1 = np.maximum(bi[0], bj[:, 0]); yy1 = np.maximum(bi[1], bj[:, 1])
        xx2 = np.minimum(bi[2], bj[:, 2]); yy2 = np.minimum(bi[3], bj[:, 3])
        w = np.maximum(F32(0), xx2 - xx1 + F32(1)); h = np.maximum(F32(0), yy2 - yy1 + F32(1))
        inter = (w * h).astype(F32)
        if mode == 1:
            o = inter / np.minimum(F32(ai), aj)
        else:
            o = inter / (F32(ai) + aj - inter)
        assert o.dtype == F32
        return o

    @staticmethod
    def over(o, thr32):
        return o > thr32


class F64Metric(_Metric):
    """the float64 twin of F32Metric: same formula on the same float32 inputs, nothing rounded"""

    @staticmethod
    def area(b):
        b = b.astype(np.float64)
        return (b[:, 2] - b[:, 0] + 1.0) * (b[:, 3] - b[:, 1] + 1.0)

    @staticmethod
    def overlap(bi, ai, bj, aj, mode):
        bi, bj = bi.astype(np.float64), bj.astype(np.float64)
        w = np.maximum(0.0, np.minimum(bi[2], bj[:, 2]) - np.maximum(bi[0], bj[:, 0]) + 1.0)
        h = np.maximum(0.0, np.minimum(bi[3], bj[:, 3]) - np.maximum(bi[1], bj[:, 1]) + 1.0)
        inter = w * h
        return inter / (np.minimum(ai, aj) if mode == 1 else ai + aj - inter)

    @staticmethod
    def over(o, thr32):
        return o > np.float64(thr32)


Kept = namedtuple("Kept", "boxes scores aux count index")


def seg_index(l, s, L, nseg, seg_major):
    return s * L + l if seg_major else l * nseg + s


def sorted_valid(scores, counts, l, L, nseg, seg_cap, seg_major):
    """-> (entry index i, arena slot) of list l's valid entries, descending by the score's float32 value, ties by i"""
    i = np.arange(nseg * seg_cap)
    s, j = i // seg_cap, i % seg_cap
    seg = seg_index(l, s, L, nseg, seg_major)
    valid = j < np.asarray(counts).reshape(-1)[seg]
    idx, slot = i[valid], (seg * seg_cap + j)[valid]
    order = np.lexsort((idx, -np.asarray(scores, dtype=F32).reshape(-1)[slot].astype(np.float64)))
    return idx[order], slot[order]


def sort_nms_ref(boxes, scores, aux, counts, L, nseg, seg_cap, seg_major, thr, mode, max_keep, metric=IntMetric, pairs=None):
    """Sort + greedy NMS of L lists made of nseg segments of seg_cap slots: a box survives iff no earlier SURVIVING box
    overlaps it by more than float32(thr); stop after max_keep survivors.  -> [Kept(boxes, scores, aux, count, index)] per
    list (index: the kept entries' i).  ``pairs``: a list that receives, per list, every overlap the greedy pass evaluated."""
    boxes = np.asarray(boxes, dtype=F32).reshape(-1, 4)
    scores = np.asarray(scores, dtype=F32).reshape(-1)
    naux = 0 if aux is None else int(np.asarray(aux).shape[-1])
    auxf = None if naux == 0 else np.asarray(aux, dtype=F32).reshape(-1, naux)
    thr32 = F32(thr)
    out = []
    for l in range(L):
        idx, slot = sorted_valid(scores, counts, l, L, nseg, seg_cap, seg_major)
        b = boxes[slot]
        area = metric.area(b)
        alive = np.ones(len(idx), dtype=bool)
        keep, seen = [], []
        for p in range(len(idx)):
            if not alive[p]:
                continue
            keep.append(p)
            if len(keep) == max_keep:
                break
            q = p + 1 + np.nonzero(alive[p + 1:])[0]
            o = metric.overlap(b[p], area[p], b[q], area[q], mode)
            seen.append(np.asarray(o, dtype=np.float64))
            alive[q[metric.over(o, thr32)]] = False
        if pairs is not None:
            pairs.append(np.concatenate(seen) if seen else np.zeros(0))
        keep = np.asarray(keep, dtype=np.int64)
        ks = slot[keep]
        out.append(Kept(boxes[ks], scores[ks], np.zeros((len(keep), 0), F32) if naux == 0 else auxf[ks], len(keep), idx[keep]))
    return out


NmsCase = namedtuple("NmsCase", "id boxes scores aux counts L nseg seg_cap seg_major thr mode max_keep cap_out naux metric expect")


def _arena(L, nseg, seg_cap, seg_major, naux, lists):
    """lists[l][s] = (boxes [k,4], scores [k]), k <= seg_cap -> poisoned arena (boxes, scores, aux, counts)"""
    nsl = L * nseg * seg_cap
    boxes = np.full((nsl, 4), np.nan, dtype=F32)
    scores = np.full(nsl, np.inf, dtype=F32)
    aux = np.full((nsl, naux), np.nan, dtype=F32)
    counts = np.zeros(L * nseg, dtype=np.int32)
    for l in range(L):
        for s in range(nseg):
            b, sc = lists[l][s]
            k = len(sc)
            assert k <= seg_cap
            seg = seg_index(l, s, L, nseg, seg_major)
            counts[seg] = k
            boxes[seg * seg_cap:seg * seg_cap + k] = b
            scores[seg * seg_cap:seg * seg_cap + k] = sc
            i = s * seg_cap + np.arange(k)
            aux[seg * seg_cap:seg * seg_cap + k] = (l * 65536 + i[:, None] * 16 + np.arange(naux)[None, :]).astype(F32)
    return boxes, scores, aux, counts


def _case(cid, lists, L, nseg, seg_cap, seg_major, thr, mode, max_keep, naux, metric=IntMetric, expect=None, cap_out=None):
    boxes, scores, aux, counts = _arena(L, nseg, seg_cap, seg_major, naux, lists)
    return NmsCase(cid, boxes, scores, aux, counts, L, nseg, seg_cap, seg_major, F32(thr), mode, max_keep,
                   cap_out or max_keep + 3, naux, metric, expect or {})


def _single(cid, b, sc, cap, thr, mode, max_keep, naux, **kw):
    return _case(cid, [[(np.asarray(b, dtype=F32).reshape(-1, 4), np.asarray(sc, dtype=F32))]], 1, 1, cap, 0, thr, mode, max_keep, naux, **kw)


def int_soup(rng, n, ties=True):
    """n integer boxes: x, y in [0, 300], w, h in [10, 80]; scores in [0.6, 1), a few exact ties"""
    c = rng.integers(0, 301, (n, 2))
    wh = rng.integers(10, 81, (n, 2))
    b = np.concatenate([c, c + wh], axis=1).astype(F32)
    sc = rng.uniform(0.6, 1.0, n).astype(F32)
    if ties and n > 10:
        sc[5] = sc[9]
        sc[n - 1] = sc[0]
    return b, sc


def _grid(n, cols, pitch, size, x0=0, y0=0):
    k = np.arange(n)
    x, y = x0 + (k % cols) * pitch, y0 + (k // cols) * pitch
    return np.stack([x, y, x + size - 1, y + size - 1], axis=1).astype(F32)


def _distinct_scores(rng, n, lo=0.5):
    """n distinct float32 scores in [lo, lo + n/8192), exact on the 2^-13 grid, in random order"""
    return (lo + rng.permutation(n) / 8192.0).astype(F32)


def _seg_counts(nseg, cap, l):
    if l == 1:
        return [0] * nseg                                          # a list with nothing in it
    pat = ([cap, 0, 1, cap * 37 // 100, cap, cap - 1, 2, cap // 2, cap] if l == 0 else
           [cap * 63 // 100, cap, 0, cap - 1, 1, cap, cap // 3, 0, 5])
    return pat[:nseg]


# entries (segment, slot) of a list that share one score and sit on boxes of their own: all survive, in (segment, slot) order
TIES = {0: [(0, 3), (0, 7), (2, 0), (3, 2), (4, 0)], 2: [(0, 1), (1, 5), (1, 6), (3, 0)]}
TIE_SCORE = {0: F32(0.97), 2: F32(0.93)}


def _segment_case(nseg, cap, seg_major, naux):
    rng = np.random.default_rng(1000 + nseg * 10)                   # the same lists in both layouts
    L, lists, ties = 3, [], {}
    for l in range(L):
        segs = []
        for s, k in enumerate(_seg_counts(nseg, cap, l)):
            b, sc = int_soup(rng, k, ties=False)
            segs.append((b, sc))
        t = 0
        for (s, j) in TIES.get(l, []):
            if s < nseg:
                b, sc = segs[s]
                assert j < len(sc)
                b[j] = (1000 + 40 * t, 1200 + 100 * l, 1019 + 40 * t, 1219 + 100 * l)
                sc[j] = TIE_SCORE[l]
                ties.setdefault(l, []).append(s * cap + j)
                t += 1
        lists.append(segs)
    return _case(f"seg-{nseg}x{cap}-major{seg_major}", lists, L, nseg, cap, seg_major, 0.5, 0, 256, naux, expect={"ties": ties, "empty": [1]})


CHAIN = [(0, 0, 99, 99), (0, 30, 99, 129), (0, 60, 99, 159)]       # A-B and B-C 7000/13000 = 0.538, A-C 4000/16000 = 0.25


def _pair_cases():
    A = (0, 0, 9, 9)
    half, seven = F32(0.5), F32(0.7)
    table = [("iou-eq-0.5", A, (0, 0, 9, 4), half, 0, 2),                                  # 50/100 == thr: strict >
             ("iou-above-0.5-", A, (0, 0, 9, 4), np.nextafter(half, F32(0)), 0, 1),
             ("iou-eq-0.7", A, (0, 0, 9, 6), seven, 0, 2),                                 # RN(70/100) == float32(0.7)
             ("iou-above-0.7-", A, (0, 0, 9, 6), np.nextafter(seven, F32(0)), 0, 1),
             # 65/90 == thr where 65 * RN(1/90) lies one step above it: a reciprocal-multiply division suppresses here
             ("iou-eq-65over90", (0, 0, 14, 5), (0, 0, 12, 4), F32(np.float64(65) / np.float64(90)), 0, 2),
             ("min-eq-0.7", A, (0, 0, 6, 19), seven, 1, 2),                                # 70 / min(100, 140)
             ("min-above-0.7-", A, (0, 0, 6, 19), np.nextafter(seven, F32(0)), 1, 1),
             ("touch-w0", A, (10, 0, 19, 9), F32(0.0), 0, 2),                              # xx2 - xx1 + 1 == 0: no overlap at all
             ("touch-w1", A, (9, 0, 18, 9), F32(0.0), 0, 1)]                               # one shared column: 10/190 > 0
    out = []
    for name, a, b, thr, mode, n in table:
        for order in (0, 1):
            sc = (0.9, 0.8) if order == 0 else (0.8, 0.9)
            out.append(_single(f"pair-{name}-order{order}", [a, b], sc, 2, thr, mode, 2, 1, expect={"counts": [n]}))
    return out


FRAC_SEED = {0: 1, 1: 3}          # per mode; chosen on the CPU so that frac_margin() > 1e-5 (docs/KERNEL_NOTES.md 4.13)


def frac_case(mode, seed=None):
    """1500 boxes with fractional float32 coordinates (what fr_box_refine hands the R-/O-Net stages' NMS) in 2048 slots"""
    rng = np.random.default_rng(FRAC_SEED[mode] if seed is None else seed)
    n = 1500
    c = rng.uniform(0, 300, (n, 2))
    wh = rng.uniform(10, 80, (n, 2))
    b = np.concatenate([c, c + wh], axis=1).astype(F32)
    sc = rng.uniform(0.6, 1.0, n).astype(F32)
    sc[5] = sc[9]
    return _single(f"frac-mode{mode}", b, sc, 2048, 0.7, mode, 1024, 4, metric=F32Metric)


def frac_margin(case):
    """distance to thr of the closest overlap the float64 greedy pass evaluates"""
    pairs = []
    sort_nms_ref(*case[1:5], case.L, case.nseg, case.seg_cap, case.seg_major, case.thr, case.mode, case.max_keep, metric=F64Metric, pairs=pairs)
    return min(float(np.abs(p - np.float64(case.thr)).min()) for p in pairs if len(p))


@functools.lru_cache(maxsize=None)
def nms_cases():
    cases = []
    # a. template boundaries: one full segment at, and one past, each template's capacity
    for k, cap in enumerate((512, 513, 2048, 2049, 4096)):
        for thr, mode in ((0.5, 0), (0.7, 1)):
            rng = np.random.default_rng(100 + 2 * k + mode)
            b, sc = int_soup(rng, cap)
            cases.append(_single(f"cap{cap}-mode{mode}", b, sc, cap, thr, mode, 256, (0, 4, 10, 14, 4)[k] if mode == 0 else (14, 10, 0, 4, 10)[k]))
    # b. segments
    for nseg, cap, naux in ((5, 100, 4), (9, 256, 4), (3, 700, 10)):
        for seg_major in (0, 1):
            cases.append(_segment_case(nseg, cap, seg_major, naux))
    # c. chunk machinery
    rng = np.random.default_rng(7)
    cases.append(_single("cluster200", np.tile(np.asarray([[50, 60, 120, 140]], F32), (200, 1)), (0.9 - np.arange(200) / 1024.0).astype(F32),
                         200, 0.5, 0, 256, 4, expect={"counts": [1]}))
    gb, gs = _grid(1500, 40, 20, 10), _distinct_scores(rng, 1500)
    for mk in (1024, 100, 64, 65):
        cases.append(_single(f"grid1500-keep{mk}", gb, gs, 1500, 0.5, 0, mk, 4, expect={"counts": [mk]}))
    top = np.asarray([[100, 100, 199, 199]], F32)
    db = np.concatenate([top, np.tile(top, (1200, 1)), _grid(50, 10, 30, 20, 300, 300)])
    ds = np.concatenate([[F32(0.99)], rng.uniform(0.5, 0.9, 1200).astype(F32), _distinct_scores(rng, 50, 0.1)]).astype(F32)
    perm = rng.permutation(len(ds))                                 # slot order is not score order
    cases.append(_single("deadwindow", db[perm], ds[perm], 2048, 0.5, 0, 256, 4, expect={"counts": [51], "dead_after_first_chunk": 1024}))
    cases.append(_single("chain", CHAIN, (0.9, 0.8, 0.7), 3, 0.5, 0, 16, 4, expect={"counts": [2], "index": [[0, 2]]}))
    fill = _grid(62, 10, 30, 20, 500, 500)
    cases.append(_single("chain-edge", np.concatenate([fill, np.asarray(CHAIN, F32)]),
                         np.concatenate([(0.99 - np.arange(62) / 8192.0).astype(F32), np.asarray([0.9, 0.8, 0.7], F32)]), 65, 0.5, 0, 128, 4,
                         expect={"counts": [64], "index": [list(range(63)) + [64]]}))
    # a lone box, then 300 disjoint boxes D_k each followed by E_k = D_k shifted by 10 of 40 columns (1200/2000 = 0.6)
    D = _grid(300, 20, 100, 40)
    E = D + np.asarray([10, 0, 10, 0], F32)
    alt = np.concatenate([np.asarray([[2000, 2000, 2039, 2039]], F32), np.stack([D, E], axis=1).reshape(-1, 4)])
    asc = (0.99 - np.arange(len(alt)) / 8192.0).astype(F32)
    cases.append(_single("alternate300", alt, asc, len(alt), 0.5, 0, 512, 4, expect={"counts": [301], "index": [[0] + list(range(1, 601, 2))]}))
    # d. exact thresholds
    cases.extend(_pair_cases())
    # e. non-integer boxes
    cases.extend(frac_case(m) for m in (0, 1))
    assert len({c.id for c in cases}) == len(cases)
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def nms_want(cid):
    c = {c.id: c for c in nms_cases()}[cid]
    return sort_nms_ref(c.boxes, c.scores, c.aux if c.naux else None, c.counts, c.L, c.nseg, c.seg_cap, c.seg_major, c.thr, c.mode,
                        c.max_keep, metric=c.metric)


# ---------------------------------------------------------------------------------------------------------- SCRFD decode
def decode_level64(score, bbox, kps, hw, A, stride, logit_thr, det_scale, cap):
    """float64 twin of scrfd_ref.decode_level on the same float32 inputs -> boxes, scores, kps and, per coordinate, the
    magnitude (|c| + |d| stride) / det_scale that the three float32 roundings (product, sum, quotient) are relative to"""
    score = np.asarray(score, dtype=F32)
    idx = np.nonzero(score >= F32(logit_thr))[0][:cap]
    cell = idx // A
    cx = ((cell % hw[1]) * stride).astype(np.float64)
    cy = ((cell // hw[1]) * stride).astype(np.float64)
    s, ds = np.float64(stride), np.float64(F32(det_scale))
    d, k = np.asarray(bbox, dtype=F32)[idx].astype(np.float64), np.asarray(kps, dtype=F32)[idx].astype(np.float64)
    boxes = np.stack([(cx - d[:, 0] * s) / ds, (cy - d[:, 1] * s) / ds, (cx + d[:, 2] * s) / ds, (cy + d[:, 3] * s) / ds], axis=1)
    bmag = np.stack([(cx + np.abs(d[:, 0]) * s) / ds, (cy + np.abs(d[:, 1]) * s) / ds, (cx + np.abs(d[:, 2]) * s) / ds,
                     (cy + np.abs(d[:, 3]) * s) / ds], axis=1)
    c2 = np.stack([cx, cy] * 5, axis=1)
    pts = (c2 + k * s) / ds
    pmag = (c2 + np.abs(k) * s) / ds
    sc = 1.0 / (1.0 + np.exp(-score[idx].astype(np.float64)))
    return boxes, sc, pts, bmag, pmag


ScrfdCase = namedtuple("ScrfdCase", "id Hl Wl A stride level cap logit_thr det_scale score bbox kps plants expect")
SCRFD_FRAMES = 3
SCRFD_DET_SCALE = (1.0, 0.3333333, 1.7)
# plant kinds: a logit well above the threshold, exactly on it (passes: >=), one float32 step below it (does not)
HI, AT, BELOW = "hi", "at", "below"


def _scrfd_case(cid, Hl, Wl, A, stride, level, cap, plants, expect):
    """plants: per frame {anchor (negative: from the end): kind}; expect: per frame count"""
    na = Hl * Wl * A
    rng = np.random.default_rng(na * 10 + level)
    thr = scrfd_ref.logit_threshold(0.6)
    score = rng.uniform(-12.0, -6.0, (SCRFD_FRAMES, na)).astype(F32)
    bbox = (rng.standard_normal((SCRFD_FRAMES, na, 4)) * 3.0).astype(F32)           # negative distances included
    kps = (rng.standard_normal((SCRFD_FRAMES, na, 10)) * 2.0).astype(F32)
    norm = []
    for f, pl in enumerate(plants):
        d = {}
        for t, (a, kind) in enumerate(sorted((a % na, k) for a, k in pl.items())):
            d[a] = kind
            # well separated logits, neither sorted nor equal: the scores' order is then a property of the rows
            score[f, a] = {HI: F32(thr + 0.5 + ((t * 7) % 11) * 0.37 + (t // 11) * 0.05), AT: thr, BELOW: np.nextafter(thr, F32(-np.inf))}[kind]
        norm.append(d)
    return ScrfdCase(cid, Hl, Wl, A, stride, level, cap, thr, np.asarray(SCRFD_DET_SCALE, dtype=F32), score, bbox, kps, tuple(norm), tuple(expect))


@functools.lru_cache(maxsize=None)
def scrfd_cases():
    cases = []
    for Hl, Wl, A, stride, level in ((23, 23, 2, 8, 0), (40, 20, 2, 16, 1)):
        tag = f"{Hl}x{Wl}-lv{level}"
        cases.append(_scrfd_case(f"{tag}-generous", Hl, Wl, A, stride, level, 16,
                                 [{0: HI, 1022: AT, 1023: HI, 1024: HI, 1025: BELOW, -1: HI}, {}, {7: BELOW, 500: AT, 1023: HI, 1024: HI}], [5, 0, 3]))
        cases.append(_scrfd_case(f"{tag}-cut5", Hl, Wl, A, stride, level, 5,
                                 [{0: HI, 1022: HI, 1023: HI, 1024: HI, 1025: HI, 1030: HI, -1: HI}, {},
                                  {5: HI, 6: AT, 1024: HI, 1025: HI, 1026: HI, 1027: HI}], [5, 0, 5]))
        cases.append(_scrfd_case(f"{tag}-stop3", Hl, Wl, A, stride, level, 3,
                                 [{0: HI, 1022: HI, 1023: AT, 1024: HI, -1: HI}, {}, {1024: HI, 1025: HI}], [3, 0, 2]))
        cases.append(_scrfd_case(f"{tag}-cap1", Hl, Wl, A, stride, level, 1, [{1023: HI, 1024: HI}, {}, {-1: HI}], [1, 0, 1]))
    cases.append(_scrfd_case("1x1-lv2-generous", 1, 1, 1, 32, 2, 16, [{0: AT}, {}, {0: BELOW}], [1, 0, 0]))
    # a stride that is no power of two: d * stride rounds, so a fused multiply-add would show (it cannot at 8 / 16 / 32)
    cases.append(_scrfd_case("9x11-stride7-lv2", 9, 11, 2, 7, 2, 32, [{**{a: HI for a in range(0, 198, 9)}, 5: AT}, {}, {**{a: HI for a in range(4, 198, 11)}, 3: BELOW}], [23, 0, 18]))
    cases.append(_scrfd_case("1x1-lv2-cap1", 1, 1, 1, 32, 2, 1, [{0: HI}, {}, {0: HI}], [1, 0, 1]))
    return tuple(cases)


def scrfd_want(c, f):
    return scrfd_ref.decode_level(c.score[f], c.bbox[f], c.kps[f], (c.Hl, c.Wl), c.A, c.stride, c.logit_thr, c.det_scale[f], c.cap)


# --------------------------------------------------------------------------------------------------- P-Net candidates
def softmax_face64(head):
    """float64 e1 / (e0 + e1) with the max subtracted, from the float32 logits head[..., 0:2]"""
    a = np.asarray(head, dtype=F32)[..., :2].astype(np.float64)
    m = a.max(axis=-1)
    e0, e1 = np.exp(a[..., 0] - m), np.exp(a[..., 1] - m)
    return e1 / (e0 + e1)


def pnet_candidates_ref(head, scale, thr, cap, dl=None, dl_min=0.0):
    """One frame's head map [hc, wc, 6] = (logit0, logit1, reg0..3) -> boxes float32 [n,4], scores float64 [n], regs float32
    [n,4], cells [n]: the cells with p >= float32(thr) in raster order, the first ``cap``.  A cell is considered iff dl is
    None or dl >= dl_min or dl is not finite.  Box corners in float32 operation by operation (oracle/detect.py stage 1)."""
    head = np.asarray(head, dtype=F32)
    hc, wc = head.shape[:2]
    p = softmax_face64(head)
    ok = p >= np.float64(F32(thr))
    if dl is not None:
        d = np.asarray(dl, dtype=F32).reshape(hc, wc)
        with np.errstate(invalid="ignore"):
            ok &= (d >= F32(dl_min)) | ~np.isfinite(d)
    cells = np.nonzero(ok.reshape(-1))[0][:cap]
    ys, xs = cells // wc, cells % wc
    s32 = F32(scale)
    x1 = np.floor((F32(2) * xs.astype(F32) + F32(1)) / s32)
    y1 = np.floor((F32(2) * ys.astype(F32) + F32(1)) / s32)
    x2 = np.floor((F32(2) * xs.astype(F32) + F32(12)) / s32)
    y2 = np.floor((F32(2) * ys.astype(F32) + F32(12)) / s32)
    boxes = np.stack([x1, y1, x2, y2], axis=1).astype(F32)
    return boxes, p.reshape(-1)[cells], head.reshape(-1, 6)[cells, 2:6], cells


PnetCase = namedtuple("PnetCase", "id hc wc scale thr cap head dl dl_min prob plants expect")
PNET_FRAMES = 2
PNET_THR = F32(0.6)


def _pnet_head(rng, hc, wc, plants):
    """logit1 - logit0 = -8 everywhere, +8 at the planted cells (negative: from the end)"""
    cells = hc * wc
    head = rng.standard_normal((PNET_FRAMES, cells, 6)).astype(F32)
    head[..., 1] = head[..., 0] - F32(8)
    norm = []
    for f, pl in enumerate(plants):
        pl = sorted({c % cells for c in pl if -cells <= c < cells})
        head[f, pl, 1] = head[f, pl, 0] + F32(8)
        norm.append(tuple(pl))
    return head.reshape(PNET_FRAMES, hc, wc, 6), tuple(norm)


SMALL_PLANTS = ([0, 255, 256, 257, -1], [1, 254, 258, -2])
LARGE_PLANTS = ([0, 255, 256, 257, 65535, 65536, 257 * 256 + 3, 260 * 256 + 255, 263 * 256, 264 * 256, -1],
                [1, 300, 65537, 258 * 256 + 77, 262 * 256 + 128, -2])


def _dense_head(rng, hc, wc):
    """logit differences spread over [-10, 10], none with p within 1e-3 of the threshold: about 4 cells in 10 pass"""
    cells = hc * wc
    head = rng.standard_normal((PNET_FRAMES, cells, 6)).astype(F32)
    d = rng.uniform(-10.0, 10.0, (PNET_FRAMES, cells)).astype(F32)
    head[..., 1] = head[..., 0] + d
    near = np.abs(softmax_face64(head) - np.float64(PNET_THR)) < 1e-3
    head[..., 1] = np.where(near, head[..., 0] + F32(3), head[..., 1])
    return head.reshape(PNET_FRAMES, hc, wc, 6)


@functools.lru_cache(maxsize=None)
def pnet_cases():
    cases = []
    rng = np.random.default_rng(11)

    def add(cid, hc, wc, scale, cap, plants, thr=PNET_THR, head=None, dl=None, dl_min=0.0, prob=False, expect=None, norm=((), ())):
        if head is None:
            head, norm = _pnet_head(rng, hc, wc, plants)
        if expect is None:
            expect = [min(len(p), cap) for p in norm]
        cases.append(PnetCase(cid, hc, wc, F32(scale), F32(thr), cap, head, dl, F32(dl_min), prob, norm, expect))

    add("1x1", 1, 1, 1.0, 8, ([0], []))
    add("16x16", 16, 16, 0.6, 8, SMALL_PLANTS)
    add("16x17-s0.3546", 16, 17, 0.3546, 8, SMALL_PLANTS)
    add("16x17-s1", 16, 17, 1.0, 8, SMALL_PLANTS)
    for scale in (1.0, 0.6, 0.3546):
        add(f"260x260-s{scale}", 260, 260, scale, 64, LARGE_PLANTS)
    add("260x260-cap4", 260, 260, 0.6, 4, LARGE_PLANTS)
    add("260x260-cap1", 260, 260, 0.6, 1, LARGE_PLANTS)
    # the exact edge: logit0 == logit1 gives p = 1/2 exactly
    head, norm = _pnet_head(rng, 16, 17, SMALL_PLANTS)
    edge = ((3, 5), (15, 15), (7, 0))
    for y, x in edge:
        head[0, y, x, 1] = head[0, y, x, 0]
    on = tuple(sorted(set(norm[0]) | {y * 17 + x for y, x in edge}))
    add("16x17-edge-at", 16, 17, 0.6, 16, None, thr=0.5, head=head, expect=[len(on), len(norm[1])])
    add("16x17-edge-above", 16, 17, 0.6, 16, None, thr=np.nextafter(F32(0.5), F32(1)), head=head, expect=[len(norm[0]), len(norm[1])])
    # many passing cells: the ordered compaction at work in every block, with and without overflow; probabilities of every kind
    add("16x17-dense", 16, 17, 0.6, 272, None, head=_dense_head(rng, 16, 17), prob=True, expect=[])
    add("260x260-dense", 260, 260, 0.3546, 260 * 260, None, head=_dense_head(rng, 260, 260), prob=True, expect=[])
    add("260x260-dense-cap64", 260, 260, 0.3546, 64, None, head=_dense_head(rng, 260, 260), expect=[64, 64])
    head, norm = _pnet_head(rng, 260, 260, LARGE_PLANTS)
    add("260x260-prob", 260, 260, 1.0, 64, None, head=head, prob=True, norm=norm)
    # the fused P-Net's pre-filter: dl = the true difference, except at chosen cells
    for hc, wc, plants in ((16, 17, SMALL_PLANTS), (260, 260, LARGE_PLANTS)):
        head, norm = _pnet_head(rng, hc, wc, plants)
        dl = (head[..., 1] - head[..., 0]).astype(F32).reshape(PNET_FRAMES, -1)
        p0, p1 = norm
        dl[0, p0[1]] = F32(-1.0)                                   # a passing cell the filter rules out: dropped
        dl[0, p0[2]] = np.nan                                      # not finite: rules nothing out
        dl[0, p0[3]] = np.inf
        dl[0, p0[-1]] = -np.inf
        dl[1, p1[0]] = np.nextafter(F32(0.5), F32(0))              # one step below dl_min: dropped
        dl[1, p1[1]] = F32(0.5)                                    # exactly dl_min: considered
        dl[0, 2] = F32(9.0)                                        # considered, but its exact p fails
        dl[1, 3] = np.nan
        add(f"{hc}x{wc}-dl", hc, wc, 0.6, 64, None, head=head, dl=dl.reshape(PNET_FRAMES, hc, wc), dl_min=0.5,
            norm=norm, expect=[len(p0) - 1, len(p1) - 1])
    assert len({c.id for c in cases}) == len(cases)
    return tuple(cases)


def pnet_want(c, f):
    return pnet_candidates_ref(c.head[f], c.scale, c.thr, c.cap, None if c.dl is None else c.dl[f], c.dl_min)
