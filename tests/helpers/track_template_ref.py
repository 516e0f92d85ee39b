"""NumPy definition of track templates (include/frhip.h fr_track_fuse_f32), written from the rule in the header and DESIGN.md
4.5g, not from the kernel, and composed from the pinned arithmetic of tests/helpers/scan_ref.py: ``row_dot_wave8`` (the join
test), ``mean_rows`` and ``l2norm_rows`` (the template).  It runs behind ``TrackRef.commit`` of one turn, on the (entry, need)
pair the commit launch got, the associate launch's ``tid`` and the ``normed`` rows after the commit.

State per camera slot s < S and track entry t < T, zeroed once, depth K in 1 .. 16:
  tring f32 [S,T,K,512]   the unit embeddings of the entry's last shots
  ttmpl i32 [S,T,4]       (len, head, id, 0)
  tmean f32 [S,T,512]     the template, a unit row
Entry t HOLDS A TEMPLATE FOR TRACK id iff ``len >= 1`` and ``ttmpl.id == id``: a slot given back, dropped tracks and a retired
entry taken by a new track all end in a fresh id, so nothing zeroes this state.

Per detection slot q = (i, j), j < counts[i] (clamped to 0 .. cap), s = slot[i] inside [0, S), e = entry[q] inside [0, T),
n = row q of normed:
  need != 0:  holds a template for tid[q]:  c = row_dot_wave8(n, tmean[s, e])
                c >= join_thr:       JOINED     ring[head] = n, head = (head + 1) % K, len = min(len + 1, K)
                else (NaN included): RESTARTED  ring[0] = n, head = 1 % K, len = 1
              holds none:            STARTED    as RESTARTED, and ttmpl.id = tid[q]
              then tmean[s, e] = n's bits when len == 1, else l2norm_rows(mean_rows(ring rows oldest first)), the oldest at
              ``head`` when len == K and at 0 otherwise;  query[q] = tmean[s, e], shots[q] = len
  need == 0:  holds a template for tid[q]:  READ, query[q] = tmean[s, e], shots[q] = len, no state moves
              otherwise:                    query[q] = n, shots[q] = 0, NONE
Every other slot: query[q] = normed[q], shots[q] = 0, NONE.  ``trace`` counts the branches a sequence exercised; ``cos`` holds the
join test's ``c`` of the last call per detection slot (NaN where none was made)."""
import numpy as np

from tests.helpers.scan_ref import l2norm_rows, mean_rows, row_dot_wave8

F32 = np.float32
DIM = 512
NONE, STARTED, JOINED, RESTARTED, READ = range(5)
LEN, HEAD, TID = range(3)
EVENTS = ("started", "joined", "restarted", "read", "wrapped", "stale_id", "nan_restart", "carried_without")


class TrackTemplateRef:
    def __init__(self, S, T, K, join_thr=0.4):
        assert S >= 1 and 1 <= T <= 64 and 1 <= K <= 16 and -1.0 <= join_thr <= 1.0
        self.S, self.T, self.K, self.join_thr = int(S), int(T), int(K), F32(join_thr)
        self.tring = np.zeros((S, T, K, DIM), F32)
        self.ttmpl = np.zeros((S, T, 4), np.int32)
        self.tmean = np.zeros((S, T, DIM), F32)
        self.trace = dict.fromkeys(EVENTS, 0)
        self.cos = None

    def holds(self, s, t, id_):
        return bool(self.ttmpl[s, t, LEN] >= 1 and self.ttmpl[s, t, TID] == id_)

    def template(self, s, t):
        """the template the ring of (s, t) gives: its only row's bits, or the unit mean of its rows oldest first"""
        n, head = int(self.ttmpl[s, t, LEN]), int(self.ttmpl[s, t, HEAD])
        if n == 1:
            return self.tring[s, t, (head - 1) % self.K].copy()
        start = head if n == self.K else 0
        rows = self.tring[s, t, [(start + i) % self.K for i in range(n)]]
        return l2norm_rows(mean_rows(rows)[None])[0]

    def fuse(self, entry, need, tid, slot, counts, normed):
        """entry, need, tid i32 [N,cap]; slot, counts i32 [N]; normed f32 [N*cap,512] -> query f32 [N*cap,512], shots and event
        i32 [N,cap]; the state moves"""
        entry, need, tid = (np.asarray(a, np.int32) for a in (entry, need, tid))
        normed = np.asarray(normed, F32)
        N, cap = entry.shape
        assert normed.shape == (N * cap, DIM)
        query = normed.copy()
        shots = np.zeros((N, cap), np.int32)
        event = np.zeros((N, cap), np.int32)
        self.cos = np.full((N, cap), np.nan, F32)
        K = self.K
        for i in range(N):
            s = int(slot[i])
            for j in range(min(max(int(counts[i]), 0), cap)):
                q, e = i * cap + j, int(entry[i, j])
                if not (0 <= s < self.S and 0 <= e < self.T):
                    continue
                tt, n, id_ = self.ttmpl[s, e], normed[q], tid[i, j]
                holds = self.holds(s, e, id_)
                if tt[LEN] >= 1 and not holds:
                    self.trace["stale_id"] += 1
                if need[i, j] != 0:
                    join = False
                    if holds:
                        c = self.cos[i, j] = row_dot_wave8(n[None], self.tmean[s, e][None])[0, 0]
                        join = bool(c >= self.join_thr)                     # False for a NaN
                        if c != c:
                            self.trace["nan_restart"] += 1
                    if join:
                        assert 0 <= tt[HEAD] < K and tt[LEN] <= K
                        self.tring[s, e, tt[HEAD]] = n
                        if tt[LEN] == K:
                            self.trace["wrapped"] += 1
                        tt[:] = (min(tt[LEN] + 1, K), (tt[HEAD] + 1) % K, id_, 0)
                        event[i, j] = JOINED
                        self.trace["joined"] += 1
                    else:
                        self.tring[s, e, 0] = n
                        tt[:] = (1, 1 % K, id_, 0)
                        event[i, j] = RESTARTED if holds else STARTED
                        self.trace["restarted" if holds else "started"] += 1
                    self.tmean[s, e] = self.template(s, e)
                    query[q], shots[i, j] = self.tmean[s, e], tt[LEN]
                elif holds:
                    query[q], shots[i, j], event[i, j] = self.tmean[s, e], tt[LEN], READ
                    self.trace["read"] += 1
                else:
                    self.trace["carried_without"] += 1
        return query, shots, event
