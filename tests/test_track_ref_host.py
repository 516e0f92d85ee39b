"""The NumPy face-track reference (tests/helpers/track_ref.py) against the rule of include/frhip.h fr_track_associate_f32, case by
case, and the premise of every input tests/test_gpu_tracks.py feeds the kernels (no GPU needed)."""
import numpy as np
import pytest

from tests.helpers import track_cases as tc
from tests.helpers.track_ref import DIM, EVENTS, ID, LIVE, MISSES, SINCE, TrackRef

F32 = np.float32


def _run(case):
    ref = case["ref"]
    entry, need, tid = ref.associate(case["boxes"], case["counts"], case["slot"])
    n = int(case["counts"][0])
    for name, want in case["expect"].items():
        if name == "since":
            got = [int(ref.tstate[tc.SUBJECT, e, SINCE]) for e in entry[0, :n]]
        else:
            got = dict(entry=entry, need=need, tid=tid)[name][0, :len(want)].tolist()
        assert got == want, (name, got, want)
    # behind a frame's count: entry -1, need 0, tid -1
    for f in range(3):
        c = int(case["counts"][f])
        assert (entry[f, c:] == -1).all() and (need[f, c:] == 0).all() and (tid[f, c:] == -1).all()
    return entry, need, tid


@pytest.mark.parametrize("name", sorted(tc.hand_cases()))
def test_hand_case(name):
    _run(tc.hand_cases()[name])


def test_every_table_also_ages_a_missed_track_and_fills_an_empty_slot():
    case = tc.hand_cases()["identical"]
    entry, need, tid = _run(case)
    ref = case["ref"]
    assert ref.tstate[0, 1].tolist() == [1, 1, 1, 101]                       # frame 1: no detection, one miss, still live
    assert entry[2].tolist() == [0, 1, 2, 3] and need[2].tolist() == [1] * 4 and tid[2].tolist() == [0, 1, 2, 3]
    assert ref.next_id.tolist() == [0, 0, 0, 4] and (ref.tstate[3, :, LIVE] == 1).all()
    assert np.array_equal(ref.tbox[3], case["boxes"][2])


def test_threshold_premise_is_exactly_one_half():
    ref = TrackRef(1, 1)
    ref.tbox[0, 0] = (0, 0, 9, 9)
    o = ref.overlaps((0, 0, 9, 4), 0)
    assert o.dtype == F32 and o[0].view(np.uint32) == F32(0.5).view(np.uint32)
    assert np.nextafter(F32(0.5), F32(1)) > o[0]


def test_equal_bits_premise_and_guard_premises():
    c = tc.hand_cases()["equal_bits_lower_entry"]
    o = c["ref"].overlaps(c["boxes"][0, 0], tc.SUBJECT)
    assert o[1].view(np.uint32) == o[3].view(np.uint32) and o[1] >= F32(0.5)
    c = tc.hand_cases()["guard_on"]
    o = c["ref"].overlaps(c["boxes"][0, 0], tc.SUBJECT)
    assert o[0] == 1 and 0 < o[1] < F32(0.5)
    c = tc.hand_cases()["guard_off_at_zero"]
    o = c["ref"].overlaps(c["boxes"][0, 0], tc.SUBJECT)
    assert o[0] == 1 and o[1] == 0
    c = tc.hand_cases()["greedy_in_detector_order"]
    o0, o1 = (c["ref"].overlaps(c["boxes"][0, j], tc.SUBJECT) for j in (0, 1))
    assert o0[2] > o0[0] >= F32(0.3) and o1[2] > o1[0] >= F32(0.3)            # both prefer B; the first in order gets it


def test_nan_never_matches_and_never_guards():
    c = tc.hand_cases()["nan_boxes"]
    ref = c["ref"]
    assert np.isnan(ref.overlaps(c["boxes"][0, 0], tc.SUBJECT)).all()        # a NaN detection: NaN against every entry
    assert np.isnan(ref.overlaps(c["boxes"][0, 1], tc.SUBJECT)[1])           # a NaN entry
    _run(c)
    assert np.isnan(ref.tbox[tc.SUBJECT, 2, 2]) and ref.tstate[tc.SUBJECT, 2].tolist() == [1, 0, 0, 0]


def test_out_of_range_slot_is_stateless():
    c = tc.hand_cases()["slot_out_of_range"]
    ref = c["ref"]
    before = (ref.tbox.copy(), ref.tstate.copy(), ref.next_id.copy())
    entry, need, tid = _run(c)
    assert need[2].tolist() == [1] * 4 and (entry[2] == -1).all() and (tid[2] == -1).all()
    after_miss = before[1].copy()
    after_miss[0, 1, MISSES] += 1                                            # frame 1 (slot 0) is the only state that moved
    assert np.array_equal(ref.tstate, after_miss) and np.array_equal(ref.next_id, before[2])
    assert np.array_equal(ref.tbox.view(np.uint32), before[0].view(np.uint32))


def test_since_walks_to_max_reuse_then_reembeds():
    ref = TrackRef(1, 4, max_reuse=3)
    box = np.array([[(20, 20, 59, 59)]], F32)
    needs, sinces = [], []
    for _ in range(9):
        e, n, t = ref.associate(box, [1], [0])
        assert e[0, 0] == 0 and t[0, 0] == 0
        needs.append(int(n[0, 0]))
        sinces.append(int(ref.tstate[0, 0, SINCE]))
    assert needs == [1, 0, 0, 0, 1, 0, 0, 0, 1] and sinces == [0, 1, 2, 3, 0, 1, 2, 3, 0]
    assert ref.trace["carry"] == 6 and ref.trace["reembed_age"] == 2 and ref.trace["new"] == 1


def test_retired_after_max_misses_plus_one_turns_and_reused_that_turn():
    for mm in (0, 1, 3):
        ref = TrackRef(1, 2, max_misses=mm)
        ref.associate(np.array([[(0, 0, 39, 39)]], F32), [1], [0])
        none = np.zeros((1, 1, 4), F32)
        for k in range(mm):
            ref.associate(none, [0], [0])
            assert ref.tstate[0, 0].tolist() == [1, 0, k + 1, 0]
        e, n, t = ref.associate(np.array([[tc.FAR]], F32), [1], [0])         # turn mm + 1 without it: gone, entry 0 taken again
        assert (e[0, 0], n[0, 0], t[0, 0]) == (0, 1, 1) and ref.tstate[0, 0].tolist() == [1, 0, 0, 1]
        assert ref.trace["retire"] == 1 and ref.trace["reuse"] == 1


def test_a_seen_track_resets_its_misses():
    ref = TrackRef(1, 2, max_misses=1)
    box = np.array([[(0, 0, 39, 39)]], F32)
    for count in (1, 0, 1, 0, 1):
        e, _, t = ref.associate(box, [count], [0])
        if count:
            assert e[0, 0] == 0 and t[0, 0] == 0 and ref.tstate[0, 0, MISSES] == 0


def test_forget_clears_a_slot_and_ids_run_on():
    ref = TrackRef(2, 4)
    boxes = np.array([[(0, 0, 39, 39), (100, 0, 139, 39)]] * 2, F32)
    ref.associate(boxes, [2, 2], [0, 1])
    ref.forget(1)
    assert (ref.tstate[1, :, LIVE] == 0).all() and (ref.tstate[0, :2, LIVE] == 1).all()
    e, n, t = ref.associate(boxes, [2, 2], [0, 1])
    assert n.tolist() == [[0, 0], [1, 1]] and t.tolist() == [[0, 1], [2, 3]] and e.tolist() == [[0, 1], [0, 1]]


def test_commit_moves_rows_in_the_stated_direction_only():
    rng = np.random.default_rng(0)
    c = tc.hand_cases()["table_full"]
    ref = c["ref"]
    entry, need, _ = ref.associate(c["boxes"], c["counts"], c["slot"])
    ref.bank[...] = rng.standard_normal(ref.bank.shape).astype(F32)
    bank0 = ref.bank.copy()
    emb = rng.standard_normal((3 * tc.CAP, DIM)).astype(F32)
    normed = rng.standard_normal((3 * tc.CAP, DIM)).astype(F32)
    emb0, normed0 = emb.copy(), normed.copy()
    ref.commit(entry, need, c["slot"], c["counts"], emb, normed)
    # frame 0: detection 1 is carried from entry 0 of slot SUBJECT, 0 and 2 are untracked; frame 2: four new rows to slot 3
    assert np.array_equal(emb[1], bank0[tc.SUBJECT, 0, 0]) and np.array_equal(normed[1], bank0[tc.SUBJECT, 0, 1])
    for j in range(4):
        assert np.array_equal(ref.bank[3, j, 0], emb0[2 * tc.CAP + j]) and np.array_equal(ref.bank[3, j, 1], normed0[2 * tc.CAP + j])
    emb0[1], normed0[1] = emb[1], normed[1]
    bank0[3] = ref.bank[3]
    assert np.array_equal(emb, emb0) and np.array_equal(normed, normed0) and np.array_equal(ref.bank, bank0)


def _soup_trace(seed_, entries, fractional):
    ref = TrackRef(8, entries, **tc.SOUP_RULE)
    counts_seen = set()
    for boxes, counts, slot in tc.soup(seed_, entries, fractional):
        assert boxes.shape == (5, 8, 4) and len(set(slot.tolist())) == 5
        entry, need, tid = ref.associate(boxes, counts, slot)
        counts_seen |= set(counts.tolist())
        live = ref.tstate[..., LIVE] != 0
        for s in range(8):                                       # live ids of a slot are distinct and below next_id
            ids = ref.tstate[s, live[s], ID]
            assert len(set(ids.tolist())) == len(ids) and (ids < ref.next_id[s]).all()
    return ref.trace, counts_seen


@pytest.mark.parametrize("seed_,entries,fractional", tc.SOUPS)
def test_soups_exercise_every_event(seed_, entries, fractional):
    """a soup that never crosses, never fills the table or never retires would let the GPU comparison pass silently"""
    trace, counts_seen = _soup_trace(seed_, entries, fractional)
    print(seed_, entries, fractional, trace, sorted(counts_seen))
    assert 0 in counts_seen and 8 in counts_seen
    must = [e for e in EVENTS if e != "full" or entries == 8]    # 64 entries cannot fill from 8 detections a turn
    for e in must:
        assert trace[e] >= (2 if e != "full" else 1), (e, trace)
    if fractional:
        assert any(np.any(b != np.floor(b)) for b, _, _ in tc.soup(seed_, entries, fractional))


def test_soups_are_reproducible():
    a, b = tc.soup(11, 8), tc.soup(11, 8)
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]) for x, y in zip(a, b))
