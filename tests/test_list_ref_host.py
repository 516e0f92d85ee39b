"""CPU checks of tests/helpers/list_ref.py: the references against the oracle and their float64 forms, and every
precondition the GPU cases of tests/test_gpu_list_kernels.py rest on.  A case that stops exercising its mechanism fails
here instead of passing on the GPU."""
import numpy as np
import pytest

from oracle import detect as odetect
from tests.helpers import list_ref as lr
from tests.helpers import scrfd_ref

F32 = np.float32
NMS = {c.id: c for c in lr.nms_cases()}
INT_IDS = [c.id for c in lr.nms_cases() if c.metric is lr.IntMetric]


def _ref(c, **kw):
    return lr.sort_nms_ref(c.boxes, c.scores, c.aux if c.naux else None, c.counts, c.L, c.nseg, c.seg_cap, c.seg_major, c.thr, c.mode,
                           c.max_keep, **kw)


# ---------------------------------------------------------------------------------------------------------- sort + NMS
@pytest.mark.parametrize("cid", INT_IDS)
def test_sort_nms_ref_vs_oracle(cid):
    """every integer case: valid coordinates are integers in [0, 2047] (areas < 2^24, float32 exact), valid scores are finite
    and positive, the poison is in place, and the reference keeps what oracle/detect.py nms() keeps of the stably sorted
    valid entries - same entries, same order, rows carried over bit for bit"""
    c = NMS[cid]
    want = lr.nms_want(cid)
    assert c.nseg * c.seg_cap <= 4096 and c.max_keep <= min(c.cap_out, 1024)
    for l in range(c.L):
        idx, slot = lr.sorted_valid(c.scores, c.counts, l, c.L, c.nseg, c.seg_cap, c.seg_major)
        b, sc = c.boxes[slot], c.scores[slot]
        assert np.isfinite(b).all() and (b == np.floor(b)).all() and b.min(initial=0) >= 0 and b.max(initial=0) <= 2047
        assert np.isfinite(sc).all() and (sc > 0).all()
        assert (np.diff(sc.astype(np.float64)) <= 0).all()
        keep = odetect.nms(b, sc, float(c.thr), "min" if c.mode else "union")[:c.max_keep]
        w = want[l]
        assert w.count == len(keep) and np.array_equal(w.index, idx[keep])
        assert np.array_equal(lr.bits(w.boxes), lr.bits(b[keep])) and np.array_equal(lr.bits(w.scores), lr.bits(sc[keep]))
        if c.naux:
            a = w.aux.astype(np.int64)
            assert np.array_equal(a, l * 65536 + w.index[:, None] * 16 + np.arange(c.naux)[None, :])
    used = np.zeros(len(c.scores), dtype=bool)
    for seg, k in enumerate(c.counts):
        used[seg * c.seg_cap:seg * c.seg_cap + k] = True
    assert np.isnan(c.boxes[~used]).all() and np.isposinf(c.scores[~used]).all()
    if "counts" in c.expect:
        assert [w.count for w in want] == c.expect["counts"]
    if "index" in c.expect:
        assert [w.index.tolist() for w in want] == c.expect["index"]


def test_nms_case_table_covers_the_issue():
    ids = set(NMS)
    for cap in (512, 513, 2048, 2049, 4096):
        for mode in (0, 1):
            c = NMS[f"cap{cap}-mode{mode}"]
            assert (c.L, c.nseg, c.seg_cap, c.max_keep) == (1, 1, cap, 256) and c.counts.tolist() == [cap]
            assert float(c.thr) == float(F32(0.7 if mode else 0.5))
    assert {NMS[f"cap{cap}-mode{m}"].naux for cap in (512, 513, 2048, 2049, 4096) for m in (0, 1)} == {0, 4, 10, 14}
    for nseg, cap in ((5, 100), (9, 256), (3, 700)):
        for sm in (0, 1):
            assert f"seg-{nseg}x{cap}-major{sm}" in ids
    # survivor counts the issue names: one cluster 1, dead window 51, the grid 1024 / 100 / 64 / 65
    assert lr.nms_want("cluster200")[0].count == 1
    assert lr.nms_want("deadwindow")[0].count == 51
    for mk in (1024, 100, 64, 65):
        w = lr.nms_want(f"grid1500-keep{mk}")[0]
        assert w.count == mk
        c = NMS[f"grid1500-keep{mk}"]
        idx, _ = lr.sorted_valid(c.scores, c.counts, 0, 1, 1, c.seg_cap, 0)
        assert np.array_equal(w.index, idx[:mk])                   # disjoint boxes: the first max_keep of the sorted list


@pytest.mark.parametrize("cid", [c.id for c in lr.nms_cases() if c.id.startswith("seg-")])
def test_segment_cases_preconditions(cid):
    c = NMS[cid]
    want = lr.nms_want(cid)
    assert c.L == 3
    per_list = [[int(c.counts[lr.seg_index(l, s, c.L, c.nseg, c.seg_major)]) for s in range(c.nseg)] for l in range(c.L)]
    allc = [k for row in per_list for k in row]
    assert 0 in allc and 1 in allc and c.seg_cap in allc and any(1 < k < c.seg_cap for k in allc)
    assert per_list[1] == [0] * c.nseg and want[1].count == 0      # a list with every segment empty
    assert want[0].count > 0 and want[2].count > 0 and not np.array_equal(want[0].index, want[2].index)
    for l, tie in c.expect["ties"].items():
        segs = {i // c.seg_cap for i in tie}
        assert len(segs) >= 2 and len(tie) > len(segs)             # equal scores across segments and inside one
        pos = [want[l].index.tolist().index(i) for i in tie]       # all survive ...
        assert pos == list(range(pos[0], pos[0] + len(tie)))       # ... next to each other, in (segment, slot) order
        assert len({int(v) for v in lr.bits(want[l].scores[pos])}) == 1
    # the two layouts hold the same lists at different places: a layout mistake reads another list's data
    other = NMS[cid[:-1] + str(1 - c.seg_major)]
    assert not np.array_equal(lr.bits(c.boxes), lr.bits(other.boxes))
    for l in range(3):
        assert np.array_equal(want[l].index, lr.nms_want(other.id)[l].index)


def test_dead_window_precondition():
    """after the first chunk of 64 the sweep leaves at least 1024 consecutive sorted entries dead: the kernel's next window
    (1024 threads of the 2048 template) holds nothing alive"""
    c = NMS["deadwindow"]
    assert 512 < c.seg_cap <= 2048
    idx, slot = lr.sorted_valid(c.scores, c.counts, 0, 1, 1, c.seg_cap, 0)
    b = c.boxes[slot]
    area = lr.IntMetric.area(b)
    kept_pos = np.nonzero(np.isin(idx, lr.nms_want("deadwindow")[0].index))[0]
    first = kept_pos[kept_pos < 64]
    assert len(first) >= 1 and (kept_pos[len(first):] >= 64 + c.expect["dead_after_first_chunk"]).all()
    q = np.arange(64, 64 + c.expect["dead_after_first_chunk"])
    dead = np.zeros(len(q), dtype=bool)
    for p in first:
        dead |= lr.IntMetric.overlap(b[p], area[p], b[q], area[q], 0) > c.thr
    assert dead.all()


def test_chain_and_alternate_preconditions():
    A, B, C = (np.asarray(v, F32) for v in lr.CHAIN)
    ov = lambda a, b: float(lr.IntMetric.overlap(a, lr.IntMetric.area(a[None])[0], b[None], lr.IntMetric.area(b[None]), 0)[0])
    assert ov(A, B) > 0.5 and ov(B, C) > 0.5 and ov(A, C) < 0.5
    c = NMS["chain-edge"]
    idx, _ = lr.sorted_valid(c.scores, c.counts, 0, 1, 1, c.seg_cap, 0)
    assert idx.tolist() == list(range(65))                         # B is the 64th live entry, C the 65th
    w = lr.nms_want("alternate300")[0]
    assert w.count == 301 and w.count > 4 * 64                     # several chunks of survivors, each window > 64 alive


def test_exact_threshold_pairs():
    f = lambda a, b: F32(np.float64(a) / np.float64(b))
    assert f(50, 100) == F32(0.5) and f(70, 100) == F32(0.7) and f(70, min(100, 140)) == F32(0.7)
    # 70 * RN(1/100) still equals float32(0.7); the 65/90 pair is the one a reciprocal-multiply division gets wrong
    assert F32(65) * (F32(1) / F32(90)) > f(65, 90)
    for name, n in (("iou-eq-0.5", 2), ("iou-above-0.5-", 1), ("iou-eq-0.7", 2), ("iou-above-0.7-", 1), ("iou-eq-65over90", 2), ("min-eq-0.7", 2),
                    ("min-above-0.7-", 1), ("touch-w0", 2), ("touch-w1", 1)):
        for order in (0, 1):
            cid = f"pair-{name}-order{order}"
            c, w = NMS[cid], lr.nms_want(cid)[0]
            assert w.count == n and w.index[0] == order            # the higher score comes first
            p = []
            _ref(c, pairs=p)
            o = F32(p[0][0])
            if "eq" in name:
                assert o == c.thr
            elif "above" in name:
                assert np.nextafter(o, F32(0)) == c.thr
            elif name == "touch-w0":
                assert o == 0
            else:
                assert o > 0


@pytest.mark.parametrize("mode", [0, 1])
def test_frac_soup_margin_and_twin(mode):
    """the non-integer soup: no overlap the float64 greedy pass evaluates lies within 1e-5 of thr (the float32 evaluation
    is ~3 * 2^-24 relative), and the float64 twin keeps the same list as the float32 reference"""
    c = NMS[f"frac-mode{mode}"]
    b = c.boxes[:c.counts[0]]
    assert (b != np.floor(b)).mean() > 0.99 and c.counts[0] == 1500 and c.seg_cap == 2048 and float(c.thr) == float(F32(0.7))
    margin = lr.frac_margin(c)
    print(f"frac-mode{mode}: seed {lr.FRAC_SEED[mode]}, closest evaluated overlap {margin:.3e} from thr")
    assert margin > 1e-5
    w32, w64 = lr.nms_want(c.id)[0], _ref(c, metric=lr.F64Metric)[0]
    assert w32.count == w64.count and np.array_equal(w32.index, w64.index) and w32.count > 64
    # the float32 mirror is oracle/detect.py's, bit for bit
    idx, slot = lr.sorted_valid(c.scores, c.counts, 0, 1, 1, c.seg_cap, 0)
    keep = odetect.nms(c.boxes[slot], c.scores[slot], float(c.thr), "min" if mode else "union")[:c.max_keep]
    assert np.array_equal(w32.index, idx[keep])
    # and scrfd_ref.iou_plus1's on a sample of pairs
    if mode == 0:
        bb = c.boxes[slot]
        a = lr.F32Metric.area(bb)
        o = lr.F32Metric.overlap(bb[0], a[0], bb[1:200], a[1:200], 0)
        assert np.array_equal(lr.bits(o), lr.bits(np.asarray([scrfd_ref.iou_plus1(bb[0], bb[1 + k]) for k in range(199)], F32)))


def test_sort_nms_ref_catches_plants():
    """the comparison the GPU test makes would notice: ties broken the other way, a suppressed box suppressing, the other
    segment layout"""
    c = NMS["seg-5x100-major1"]
    w = lr.nms_want(c.id)
    flipped = lr.sort_nms_ref(c.boxes, c.scores, c.aux, c.counts, c.L, c.nseg, c.seg_cap, 0, c.thr, c.mode, c.max_keep)
    assert any(not np.array_equal(lr.bits(a.boxes), lr.bits(b.boxes)) for a, b in zip(w, flipped))
    c = NMS["chain"]
    keep = lr.nms_want("chain")[0].index.tolist()
    assert keep == [0, 2]                                          # classic "compare with every earlier box" NMS gives [0]


# -------------------------------------------------------------------------------------------------------- SCRFD decode
@pytest.mark.parametrize("c", lr.scrfd_cases(), ids=lambda c: c.id)
def test_scrfd_cases_and_twin(c):
    na = c.Hl * c.Wl * c.A
    assert c.score.shape == (3, na) and c.logit_thr == scrfd_ref.logit_threshold(0.6)
    assert (c.bbox < 0).any() and (c.kps < 0).any()
    assert np.array_equal(c.det_scale, np.asarray([1.0, 0.3333333, 1.7], F32))
    for f in range(3):
        pl = c.plants[f]
        for a, kind in pl.items():
            v = c.score[f, a]
            if kind == lr.AT:
                assert v == c.logit_thr
            elif kind == lr.BELOW:
                assert v < c.logit_thr and np.nextafter(v, F32(np.inf)) == c.logit_thr
            else:
                assert v > c.logit_thr + F32(0.4)
        off = np.ones(na, dtype=bool)
        off[list(pl)] = False
        assert (c.score[f, off] < c.logit_thr - 5).all()
        on = sorted(a for a, k in pl.items() if k != lr.BELOW)
        b, s, k = lr.scrfd_want(c, f)
        assert len(s) == c.expect[f] == min(len(on), c.cap)
        b64, s64, k64, bmag, pmag = lr.decode_level64(c.score[f], c.bbox[f], c.kps[f], (c.Hl, c.Wl), c.A, c.stride, c.logit_thr,
                                                      c.det_scale[f], c.cap)
        assert len(s64) == len(s)
        # three roundings (product, sum, quotient): 3 * 2^-24 * (|c| + |d| stride) / det_scale per coordinate
        assert (np.abs(b - b64) <= 3 * 2.0 ** -24 * bmag).all() and (np.abs(k - k64) <= 3 * 2.0 ** -24 * pmag).all()
        assert (np.abs(s - s64) <= 1e-6).all()
        if len(s) > 1:
            assert np.abs(np.diff(np.sort(s64))).min() > 1e-4      # the scores' order is decided
    if na > 1024 and c.id.endswith("cut5"):
        on = sorted(a for a, k in c.plants[0].items() if k != lr.BELOW)
        assert sum(a < 1024 for a in on) == 3 and sum(a >= 1024 for a in on) == 4 and c.cap == 5
    if na > 1024 and c.id.endswith("stop3"):
        on = sorted(a for a, k in c.plants[0].items() if k != lr.BELOW)
        assert sum(a < 1024 for a in on) == 3 and any(a >= 1024 for a in on) and c.cap == 3
    if na > 1024 and c.id.endswith("generous"):
        assert {0, 1022, 1023, 1024, 1025, na - 1} == set(c.plants[0])
        assert lr.AT in c.plants[0].values() and lr.BELOW in c.plants[0].values()


def test_scrfd_case_table_covers_the_issue():
    shapes = {(c.Hl, c.Wl, c.A, c.stride, c.level) for c in lr.scrfd_cases()}
    assert shapes >= {(23, 23, 2, 8, 0), (1, 1, 1, 32, 2), (40, 20, 2, 16, 1)}
    # beyond the issue's shapes: a stride of 7, where the product d * stride is not exact - contracted to a fused multiply-add
    # (one rounding instead of two) every coordinate comes out different in some row of the case
    c = {c.id: c for c in lr.scrfd_cases()}["9x11-stride7-lv2"]
    differs = np.zeros(14, dtype=bool)
    for f in (0, 2):
        b, _, k = lr.scrfd_want(c, f)
        on = np.nonzero(c.score[f] >= c.logit_thr)[0]
        cell = on // c.A
        cc = np.stack([(cell % c.Wl) * 7.0, (cell // c.Wl) * 7.0], 1)
        d, kk = c.bbox[f][on].astype(np.float64), c.kps[f][on].astype(np.float64)
        fb = (np.concatenate([cc - d[:, :2] * 7.0, cc + d[:, 2:] * 7.0], 1).astype(F32) / c.det_scale[f]).astype(F32)
        fk = ((np.tile(cc, (1, 5)) + kk * 7.0).astype(F32) / c.det_scale[f]).astype(F32)
        differs |= np.concatenate([(lr.bits(fb) != lr.bits(b)).any(0), (lr.bits(fk) != lr.bits(k)).any(0)])
    assert differs.all(), differs                                  # in each of the 4 + 10 coordinates


# ---------------------------------------------------------------------------------------------------- P-Net candidates
@pytest.mark.parametrize("c", lr.pnet_cases(), ids=lambda c: c.id)
def test_pnet_cases_and_ref(c):
    cells = c.hc * c.wc
    p = lr.softmax_face64(c.head)
    edge = p == 0.5
    assert (edge | (np.abs(p - np.float64(c.thr)) > 1e-3)).all()   # p is nowhere near thr, except exactly on it
    if "edge" in c.id:
        assert edge.sum() == 3 and abs(float(c.thr) - 0.5) < 1e-7
    # the float32 softmax, operation by operation with numpy's exp, stays within the bound held against the device's expf
    a = c.head[..., :2]
    m = np.maximum(a[..., 0], a[..., 1])
    e0, e1 = np.exp(a[..., 0] - m), np.exp(a[..., 1] - m)
    assert e0.dtype == F32 and np.abs((e1 / (e0 + e1)).astype(np.float64) - p).max() <= 1e-6
    for f in range(lr.PNET_FRAMES):
        dl = None if c.dl is None else c.dl[f]
        boxes, sc, regs, idx = lr.pnet_want(c, f)
        if c.expect:
            assert len(idx) == c.expect[f]
        if c.plants[f]:
            on = [x for x in c.plants[f]]
            if dl is None:
                assert idx.tolist() == on[:c.cap]
            else:
                d = dl.reshape(-1)[on]
                with np.errstate(invalid="ignore"):
                    assert idx.tolist() == [x for x, v in zip(on, d) if v >= c.dl_min or not np.isfinite(v)][:c.cap]
        assert (np.diff(idx) > 0).all() and len(idx) <= c.cap
        assert np.array_equal(lr.bits(regs), lr.bits(c.head[f].reshape(-1, 6)[idx, 2:6]))
        # the oracle's stage 1 formula on the same cells
        ys, xs = idx // c.wc, idx % c.wc
        s32 = F32(c.scale)
        want = np.stack([np.floor((F32(2) * xs.astype(F32) + F32(1)) / s32), np.floor((F32(2) * ys.astype(F32) + F32(1)) / s32),
                         np.floor((F32(2) * xs.astype(F32) + F32(12)) / s32), np.floor((F32(2) * ys.astype(F32) + F32(12)) / s32)], 1)
        assert np.array_equal(boxes, want.astype(F32))
        # float64 form: the quotient is one rounding away, so the floors agree unless an integer lies within 2^-24 |q|
        q = np.stack([2.0 * xs + 1, 2.0 * ys + 1, 2.0 * xs + 12, 2.0 * ys + 12], 1) / np.float64(s32)
        clear = np.abs(q - np.rint(q)) > 2.0 ** -24 * np.abs(q)
        assert (np.abs(boxes - np.floor(q)) <= 1).all() and np.array_equal(boxes[clear], np.floor(q)[clear])
    if c.id == "260x260-s1.0":
        assert cells == 67600 and -(-cells // 256) == 265          # the cross-block prefix runs a second round
        on = c.plants[0]
        assert {0, 255, 256, 257, 65535, 65536, cells - 1} <= set(on) and sum(256 * 257 <= x for x in on) >= 4
    if c.id.endswith("-dl"):
        on = c.plants[0]
        d = c.dl[0].reshape(-1)
        assert d[on[1]] < c.dl_min and np.isnan(d[on[2]]) and np.isposinf(d[on[3]]) and np.isneginf(d[on[-1]])
        got = lr.pnet_want(c, 0)[3].tolist()
        assert on[1] not in got and {on[2], on[3], on[-1]} <= set(got)


def test_pnet_case_table_covers_the_issue():
    cs = lr.pnet_cases()
    assert {(c.hc, c.wc) for c in cs} == {(1, 1), (16, 16), (16, 17), (260, 260)}
    assert {round(float(c.scale), 4) for c in cs} == {1.0, 0.6, 0.3546}
    assert {c.cap for c in cs if (c.hc, c.wc) == (260, 260)} >= {1, 4, 64}
    assert any(c.prob and c.dl is None for c in cs) and any(c.dl is not None and not c.prob for c in cs)
    assert not any(c.dl is not None and c.prob for c in cs)
    dense = {c.id: c for c in cs}["260x260-dense"]
    n = [len(lr.pnet_want(dense, f)[3]) for f in range(2)]
    assert all(0.3 * 67600 < k < 0.5 * 67600 for k in n)
