"""NumPy definition of the judging face tracks' decision (include/frhip.h fr_track_resolve_quality_i32), written from the rule in
the header and DESIGN.md 4.5f, not from the kernel.  It runs between ``TrackRef.associate`` (tests/helpers/track_ref.py) and
``TrackRef.commit`` of one turn, on the associate launch's outputs and the quality launch's verdicts, and moves ``ref.tstate``
(``since`` only) and its own ``tqual``.

State beside ``tstate``: ``tqual`` i32 [S,T,4] = (has, age, id, 0), zeroed once.  Entry t of slot s HOLDS A FIT ROW FOR THE
CURRENT TRACK iff ``has == 1`` and ``tqual.id == tstate.id``.  The id comparison is all that ``forget``, ``reset`` and the reuse
of a retired entry need: each of them ends in a track that takes a fresh id from ``next_id``, so an entry is never taken to hold
the previous person's row, and nothing has to zero ``tqual``.

Per detection slot (i, j), j < counts[i] (clamped to 0 .. cap), s = slot[i]:
  A. entry < 0, or s outside [0, S), or entry >= T:  EMBED if verdict == 0 else REJECT; no state is touched.
  B. otherwise, valid = holds a fit row for tid:
     need == 0 and valid and age < max_age:  CARRY, age += 1 (tstate as the associate launch left it)
     else verdict == 0:                      EMBED, tqual = (1, 0, tid, 0), since = 0
     else:                                   REJECT, since = 0; valid and age < max_age: age += 1 (the row stays), else has = 0
Outputs i32 [N,cap]: action (0 no face, 1 EMBED, 2 CARRY, 3 REJECT) and (need2, entry2) for the commit launch: EMBED (1, entry),
CARRY (0, entry), REJECT and no face (0, -1).

The invariant: a face the associate launch wants embedded (need == 1) is never given a held row in the same turn - CARRY
requires need == 0, so the crossing guard stays the associate launch's.  ``trace`` counts the branches a sequence exercised."""
import numpy as np

NONE, EMBED, CARRY, REJECT = range(4)
HAS, AGE, QID = range(3)
SINCE, ID = 1, 3                                                  # columns of tstate
EVENTS = ("carry", "embed", "embed_untracked", "reject_untracked", "reject_kept", "reject_cleared", "expired",
          "no_row", "stale_id")


class TrackQualityRef:
    def __init__(self, ref, max_age=8):
        assert max_age >= 0
        self.ref, self.max_age = ref, int(max_age)
        self.tqual = np.zeros((ref.S, ref.T, 4), np.int32)
        self.trace = dict.fromkeys(EVENTS, 0)

    def holds(self, s, t):
        """entry t of slot s holds a fit row for the track tstate names"""
        return bool(self.tqual[s, t, HAS] == 1 and self.tqual[s, t, QID] == self.ref.tstate[s, t, ID])

    def resolve(self, entry, need, tid, verdict, slot, counts):
        """all int32: entry, need, tid, verdict [N,cap]; slot, counts [N] -> action, need2, entry2 [N,cap]; the state moves"""
        entry, need, tid, verdict = (np.asarray(a, np.int32) for a in (entry, need, tid, verdict))
        N, cap = entry.shape
        action = np.zeros((N, cap), np.int32)
        need2 = np.zeros((N, cap), np.int32)
        entry2 = np.full((N, cap), -1, np.int32)
        tq, ts = self.tqual, self.ref.tstate
        for i in range(N):
            s = int(slot[i])
            for j in range(min(max(int(counts[i]), 0), cap)):
                e, fit = int(entry[i, j]), verdict[i, j] == 0
                if not (0 <= s < self.ref.S and 0 <= e < self.ref.T):                  # A
                    action[i, j] = EMBED if fit else REJECT
                    self.trace["embed_untracked" if fit else "reject_untracked"] += 1
                else:                                                                   # B
                    q = tq[s, e]
                    valid = q[HAS] == 1 and q[QID] == tid[i, j]
                    if q[HAS] == 1 and not valid:
                        self.trace["stale_id"] += 1
                    young = valid and q[AGE] < self.max_age
                    if need[i, j] == 0 and young:
                        action[i, j] = CARRY
                        q[AGE] += 1
                        self.trace["carry"] += 1
                    elif fit:
                        if need[i, j] == 0:
                            self.trace["expired" if valid else "no_row"] += 1
                        action[i, j] = EMBED
                        q[:] = (1, 0, tid[i, j], 0)
                        ts[s, e, SINCE] = 0
                        self.trace["embed"] += 1
                    else:
                        if need[i, j] == 0:
                            self.trace["expired" if valid else "no_row"] += 1
                        action[i, j] = REJECT
                        ts[s, e, SINCE] = 0
                        if young:
                            q[AGE] += 1
                            self.trace["reject_kept"] += 1
                        else:
                            q[HAS] = 0
                            self.trace["reject_cleared"] += 1
                if action[i, j] == EMBED:
                    need2[i, j], entry2[i, j] = 1, e
                elif action[i, j] == CARRY:
                    entry2[i, j] = e
        return action, need2, entry2
