"""The definition of the judging face tracks (tests/helpers/track_quality_ref.py) held to the rule of include/frhip.h
fr_track_resolve_quality_i32 on 20-turn sequences: one hand-built, whose every action is written out below, and the seeded soups
of tests/helpers/track_cases.py under seeded verdict schedules.  The reference's own trace must show every branch, and the
properties are checked without the reference's help: a face the associate launch wants embedded is never carried, and a carried
row is always the row the SAME track id last embedded while fit.  No GPU needed."""
import numpy as np
import pytest

from tests.helpers import track_cases as tc
from tests.helpers.track_quality_ref import CARRY, EMBED, EVENTS, NONE, REJECT, TrackQualityRef
from tests.helpers.track_ref import DIM, TrackRef

F32 = np.float32
FIT, BLUR = 0, 16
A, B, C = (0, 0, 39, 39), (100, 0, 139, 39), (200, 0, 239, 39)      # three disjoint boxes


def turn(ref, tq, boxes, verdicts, slot=0, cap=3):
    """one frame of one camera through associate and resolve -> per-face (action, need, need2, entry2) lists"""
    b = np.zeros((1, cap, 4), F32)
    b[0, :len(boxes)] = np.asarray(boxes, F32).reshape(-1, 4)
    v = np.full((1, cap), -1, np.int32)
    v[0, :len(verdicts)] = verdicts
    counts, slots = np.array([len(boxes)], np.int32), np.array([slot], np.int32)
    entry, need, tid = ref.associate(b, counts, slots)
    action, need2, entry2 = tq.resolve(entry, need, tid, v, slots, counts)
    assert (action[0, len(boxes):] == NONE).all() and (need2[0, len(boxes):] == 0).all() and (entry2[0, len(boxes):] == -1).all()
    n = len(boxes)
    return action[0, :n].tolist(), need[0, :n].tolist(), need2[0, :n].tolist(), entry2[0, :n].tolist(), tid[0, :n].tolist()


def test_hand_built_sequence_action_by_action():
    """one face standing alone at A under max_reuse = 2, max_age = 3, max_misses = 0, T = 2: 20 turns"""
    ref = TrackRef(1, 2, iou_thr=0.5, max_reuse=2, max_misses=0)
    tq = TrackQualityRef(ref, max_age=3)
    st = lambda: (tq.tqual[0, 0, :3].tolist(), int(ref.tstate[0, 0, 1]))        # ((has, age, id), since)

    def step(verdict, action, need, state):
        got = turn(ref, tq, [A], [verdict])
        assert (got[0], got[1]) == ([action], [need]), (got, action, need)
        assert got[2] == [1 if action == EMBED else 0] and got[3] == [0 if action in (EMBED, CARRY) else -1]
        assert st() == state, (st(), state)

    step(BLUR, REJECT, 1, ([0, 0, 0], 0))          # 1  a new track, unfit at birth: nothing to hold
    step(BLUR, REJECT, 0, ([0, 0, 0], 0))          # 2  need == 0 on an entry without a row: rejected, since back to 0
    step(FIT, EMBED, 0, ([1, 0, 0], 0))            # 3  need == 0 without a row, fit: embedded
    step(BLUR, CARRY, 0, ([1, 1, 0], 1))           # 4  carried on the fit row
    step(BLUR, CARRY, 0, ([1, 2, 0], 2))           # 5
    step(BLUR, REJECT, 1, ([1, 3, 0], 0))          # 6  the re-embed is due (since == max_reuse): rejected, the row kept
    step(BLUR, REJECT, 0, ([0, 3, 0], 0))          # 7  age == max_age: expired, has cleared
    step(BLUR, REJECT, 0, ([0, 3, 0], 0))          # 8  nothing held
    step(FIT, EMBED, 0, ([1, 0, 0], 0))            # 9
    step(FIT, CARRY, 0, ([1, 1, 0], 1))            # 10 a fit face is carried as tracks without quality carry it
    step(FIT, CARRY, 0, ([1, 2, 0], 2))            # 11
    step(FIT, EMBED, 1, ([1, 0, 0], 0))            # 12 re-embed by age, fit
    step(BLUR, CARRY, 0, ([1, 1, 0], 1))           # 13
    assert turn(ref, tq, [], []) == ([], [], [], [], [])                        # 14 gone: retired at once (max_misses = 0)
    assert ref.tstate[0, 0].tolist() == [0, 1, 1, 0] and tq.tqual[0, 0, :3].tolist() == [1, 1, 0]
    # 15 somebody else at the same place takes entry 0 under id 1, unfit at birth: the previous person's row (has = 1, age 1 <
    # max_age, id 0) is NOT kept - without the id comparison this would be "reject, row kept" and turn 16 a carry on it
    step(BLUR, REJECT, 1, ([0, 1, 0], 0))
    assert ref.tstate[0, 0, 3] == 1 and tq.trace["stale_id"] == 1
    step(BLUR, REJECT, 0, ([0, 1, 0], 0))          # 16
    step(FIT, EMBED, 0, ([1, 0, 1], 0))            # 17 the new id's own row
    # 18 two more faces: B takes entry 1, C finds the table full and is untracked: judged, no state
    got = turn(ref, tq, [A, B, C], [BLUR, FIT, BLUR])
    assert got[0] == [CARRY, EMBED, REJECT] and got[3] == [0, 1, -1] and got[4] == [1, 2, -1]
    got = turn(ref, tq, [A, B, C], [BLUR, BLUR, FIT])                           # 19
    assert got[0] == [CARRY, CARRY, EMBED] and got[2] == [0, 0, 1] and got[3] == [0, 1, -1]
    ref.forget(0)                                                               # 20 forget / reset: live = 0, ids run on
    got = turn(ref, tq, [A, B], [BLUR, FIT])
    assert got[0] == [REJECT, EMBED] and got[4] == [3, 4]
    assert tq.tqual[0, :, :3].tolist() == [[0, 2, 1], [1, 0, 4]]
    assert all(tq.trace[k] for k in EVENTS), tq.trace             # every branch of the rule, in this one sequence


def test_max_age_zero_never_carries_and_stateless_frames_touch_nothing():
    ref = TrackRef(2, 2, max_reuse=4)
    tq = TrackQualityRef(ref, max_age=0)
    for v, want in ((FIT, EMBED), (FIT, EMBED), (BLUR, REJECT), (FIT, EMBED)):
        assert turn(ref, tq, [A], [v])[0] == [want]
    state = (ref.tstate.copy(), tq.tqual.copy())
    for slot in (-1, 2):                                                        # outside [0, S): case A
        got = turn(ref, tq, [A, B], [FIT, BLUR], slot=slot)
        assert got[0] == [EMBED, REJECT] and got[2] == [1, 0] and got[3] == [-1, -1]
    assert np.array_equal(ref.tstate, state[0]) and np.array_equal(tq.tqual, state[1])


def schedule(seed_, shape):
    """verdicts for a soup turn: runs of unfit turns per camera on top of a 30 % unfit noise"""
    rng = np.random.default_rng(seed_)
    return np.where(rng.random(shape) < 0.3, BLUR, FIT).astype(np.int32)


@pytest.mark.parametrize("seed_,entries,fractional", tc.SOUPS)
@pytest.mark.parametrize("max_age", [1, 8])
def test_soups_hold_the_invariants(seed_, entries, fractional, max_age):
    ref = TrackRef(8, entries, **tc.SOUP_RULE)
    tq = TrackQualityRef(ref, max_age=max_age)
    last_fit = {}                                                 # (slot, track id) -> tag of the row it last embedded
    tag = 0
    for t, (boxes, counts, slot) in enumerate(tc.soup(seed_, entries, fractional)):
        n, cap = boxes.shape[:2]
        verdict = schedule(seed_ * 1000 + t, (n, cap))
        if 8 <= t < 12:
            verdict[:] = BLUR                                     # a blurred stretch: carries, then expiry at max_age
        entry, need, tid = ref.associate(boxes, counts, slot)
        since_before = ref.tstate[:, :, 1].copy()
        held_before = tq.tqual.copy()
        action, need2, entry2 = tq.resolve(entry, need, tid, verdict, slot, counts)
        valid = np.arange(cap)[None, :] < np.clip(counts, 0, cap)[:, None]
        assert ((action != NONE) == valid).all()
        assert not ((need == 1) & (action == CARRY)).any()        # THE invariant: the guard stays the associate launch's
        assert not ((verdict != 0) & (action == EMBED)).any()     # an unfit face never enters the bank
        assert ((action == EMBED) == (need2 == 1)).all() and (entry2[(action == REJECT) | (action == NONE)] == -1).all()
        assert (entry2[(action == EMBED) | (action == CARRY)] == entry[(action == EMBED) | (action == CARRY)]).all()
        # commit with tagged rows: what a carried face reads is what ITS id last wrote while fit
        emb = np.zeros((n * cap, DIM), F32)
        for i in range(n):
            for j in range(cap):
                if action[i, j] == EMBED:
                    tag += 1
                    emb[i * cap + j] = tag
                    if entry[i, j] >= 0:
                        last_fit[(int(slot[i]), int(tid[i, j]))] = tag
        normed = emb.copy()
        ref.commit(entry2, need2, slot, counts, emb, normed)
        for i in range(n):
            for j in range(cap):
                s, e = int(slot[i]), int(entry[i, j])
                if action[i, j] == CARRY:
                    assert emb[i * cap + j, 0] == last_fit[(s, int(tid[i, j]))], (t, i, j)
                    assert held_before[s, e, 0] == 1 and held_before[s, e, 2] == tid[i, j] and held_before[s, e, 1] < max_age
                    assert ref.tstate[s, e, 1] == since_before[s, e]
                elif action[i, j] in (EMBED, REJECT) and e >= 0:
                    assert ref.tstate[s, e, 1] == 0
    for k in ("carry", "embed", "embed_untracked", "reject_untracked", "reject_kept", "reject_cleared", "expired", "no_row"):
        if k in ("embed_untracked", "reject_untracked") and entries >= 13:
            continue                                              # the table fills only with 8 entries
        assert tq.trace[k], (k, tq.trace)
    assert ref.trace["reuse"] and ref.trace["reembed_guard"]
