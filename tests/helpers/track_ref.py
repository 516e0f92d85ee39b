"""NumPy definition of the face tracks (include/frhip.h fr_track_associate_f32 / fr_track_commit_f32), written from the rule in
the header and DESIGN.md 4.5d, not from the kernels.  Float32 operation by operation: the IoU is ``F32Metric`` of
tests/helpers/list_ref.py (``area`` and ``overlap`` with mode 0, the detection first), the formula nms.hip is pinned to.

``TrackRef.trace`` counts what a sequence exercised, so a test can refuse a soup that never crosses."""
import numpy as np

from tests.helpers.list_ref import F32Metric

F32 = np.float32
DIM = 512
LIVE, SINCE, MISSES, ID = range(4)
EVENTS = ("carry", "reembed_age", "reembed_guard", "retire", "reuse", "full", "new")


class TrackRef:
    def __init__(self, slots, entries, iou_thr=0.5, max_reuse=4, max_misses=1):
        assert slots >= 1 and 1 <= entries <= 64 and max_reuse >= 0 and max_misses >= 0
        self.S, self.T = int(slots), int(entries)
        self.iou_thr, self.max_reuse, self.max_misses = F32(iou_thr), int(max_reuse), int(max_misses)
        assert F32(0) < self.iou_thr <= F32(1)
        self.tbox = np.zeros((self.S, self.T, 4), F32)
        self.tstate = np.zeros((self.S, self.T, 4), np.int32)
        self.next_id = np.zeros(self.S, np.int32)
        self.bank = np.zeros((self.S, self.T, 2, DIM), F32)
        self.trace = dict.fromkeys(EVENTS, 0)
        self._ever = np.zeros((self.S, self.T), bool)            # entries that have held a track (for the "reuse" event)

    def forget(self, s):
        self.tstate[s, :, LIVE] = 0

    def overlaps(self, box, s):
        """o[t] of one detection against every entry of slot s (meaningful for the live ones)"""
        box = np.asarray(box, F32)
        with np.errstate(all="ignore"):
            return F32Metric.overlap(box, F32Metric.area(box[None])[0], self.tbox[s], F32Metric.area(self.tbox[s]), 0)

    def _frame(self, boxes, count, s):
        cap = boxes.shape[0]
        entry, need, tid = np.full(cap, -1, np.int32), np.zeros(cap, np.int32), np.full(cap, -1, np.int32)
        n = min(max(int(count), 0), cap)
        if not 0 <= s < self.S:                                  # a frame without state
            need[:n] = 1
            return entry, need, tid
        box, st = self.tbox[s], self.tstate[s]
        claimed = np.zeros(self.T, bool)
        unmatched = []
        for j in range(n):
            live = st[:, LIVE] != 0
            o = self.overlaps(boxes[j], s)
            with np.errstate(invalid="ignore"):
                cand = live & ~claimed & (o >= self.iou_thr)     # a NaN compares false
                near = live & (o > F32(0))
            if not cand.any():
                unmatched.append(j)
                continue
            best = o[cand].max()
            t = int(np.flatnonzero(cand & (o == best))[0])       # the lowest entry among equal values
            near[t] = False
            claimed[t] = True
            box[t] = boxes[j]
            st[t, MISSES] = 0
            entry[j], tid[j] = t, st[t, ID]
            if st[t, SINCE] < self.max_reuse and not near.any():
                st[t, SINCE] += 1
                self.trace["carry"] += 1
            else:
                self.trace["reembed_guard" if st[t, SINCE] < self.max_reuse else "reembed_age"] += 1
                need[j] = 1
                st[t, SINCE] = 0
        for t in range(self.T):                                  # retire
            if st[t, LIVE] != 0 and not claimed[t]:
                st[t, MISSES] += 1
                if st[t, MISSES] > self.max_misses:
                    st[t, LIVE] = 0
                    self.trace["retire"] += 1
        for j in unmatched:                                      # new tracks
            need[j] = 1
            free = np.flatnonzero(st[:, LIVE] == 0)
            if free.size == 0:
                self.trace["full"] += 1
                continue
            t = int(free[0])
            self.trace["reuse" if self._ever[s, t] else "new"] += 1
            self._ever[s, t] = True
            box[t] = boxes[j]
            st[t] = (1, 0, 0, self.next_id[s])
            entry[j], tid[j] = t, self.next_id[s]
            self.next_id[s] = np.int32((int(self.next_id[s]) + 1 + 2 ** 31) % 2 ** 32 - 2 ** 31)
        return entry, need, tid

    def associate(self, boxes, counts, slot):
        """boxes f32 [N,cap,4], counts [N], slot [N] (no slot twice) -> entry, need, tid int32 [N,cap]; the state moves"""
        boxes = np.asarray(boxes, F32)
        slot = [int(s) for s in slot]
        inside = [s for s in slot if 0 <= s < self.S]
        assert len(set(inside)) == len(inside), "a slot is named twice in one call"
        out = [self._frame(boxes[i], counts[i], slot[i]) for i in range(boxes.shape[0])]
        return tuple(np.stack([o[k] for o in out]) for k in range(3))

    def commit(self, entry, need, slot, counts, emb, normed):
        """emb / normed f32 [N*cap,512], changed in place; bank rows of the embedded, batch rows of the carried"""
        N, cap = entry.shape
        for i in range(N):
            s = int(slot[i])
            if not 0 <= s < self.S:
                continue
            for j in range(min(max(int(counts[i]), 0), cap)):
                e, q = int(entry[i, j]), i * cap + j
                if not 0 <= e < self.T:
                    continue
                if need[i, j] != 0:
                    self.bank[s, e, 0], self.bank[s, e, 1] = emb[q], normed[q]
                else:
                    emb[q], normed[q] = self.bank[s, e, 0], self.bank[s, e, 1]
