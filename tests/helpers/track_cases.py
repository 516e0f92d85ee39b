"""The inputs the face-track tests share: hand-built single-turn tables (N = 3 frames, cap = 4, T = 4 over S = 4 slots) and
seeded multi-turn box soups.  tests/test_track_ref_host.py checks each case's premise and outcome on the NumPy reference,
tests/test_gpu_tracks.py runs the same inputs through the kernels and compares with the reference bit for bit."""
import numpy as np

from tests.helpers.track_ref import TrackRef

F32 = np.float32
CAP, T, S = 4, 4, 4
FAR = (500, 400, 539, 439)                      # a box nothing else in the tables touches
SUBJECT = 2                                     # the slot of frame 0, the frame a case is about


def seed(ref, s, t, box, since=0, misses=0, tid=None, live=1):
    """plant a track in entry t of slot s"""
    ref.tbox[s, t] = box
    ref.tstate[s, t] = (live, since, misses, t + 100 if tid is None else tid)


def _table(ref, dets, expect, slots=(SUBJECT, 0, 3)):
    """a case: frame 0 holds ``dets`` in slot SUBJECT; frame 1 is empty in a slot with one live track (which misses a turn);
    frame 2 brings cap new faces to an empty slot.  expect: name -> per-detection list for frame 0"""
    seed(ref, 0, 1, (30, 30, 69, 69), since=1)
    boxes = np.zeros((3, CAP, 4), F32)
    boxes[0, :len(dets)] = dets
    boxes[1] = 7.0                              # rubbish behind a zero count is never read as a face
    boxes[2] = [(40 * k, 10, 40 * k + 29, 49) for k in range(CAP)]
    counts = np.array([len(dets), 0, CAP], np.int32)
    return dict(ref=ref, boxes=boxes, counts=counts, slot=np.array(slots, np.int32), expect=expect)


def hand_cases():
    """name -> case (fresh state every call)"""
    cases = {}

    r = TrackRef(S, T)
    seed(r, SUBJECT, 1, (10, 10, 50, 50))
    cases["identical"] = _table(r, [(10, 10, 50, 50)], dict(entry=[1], need=[0], tid=[101], since=[1]))

    r = TrackRef(S, T, iou_thr=0.5)
    seed(r, SUBJECT, 0, (0, 0, 9, 9))
    cases["iou_equals_thr"] = _table(r, [(0, 0, 9, 4)], dict(entry=[0], need=[0], tid=[100]))

    r = TrackRef(S, T, iou_thr=np.nextafter(F32(0.5), F32(1)))
    seed(r, SUBJECT, 0, (0, 0, 9, 9))
    cases["iou_one_below_thr"] = _table(r, [(0, 0, 9, 4)], dict(entry=[1], need=[1], tid=[0]))

    r = TrackRef(S, T)
    seed(r, SUBJECT, 1, (5, 10, 24, 29))
    seed(r, SUBJECT, 3, (15, 10, 34, 29))
    cases["equal_bits_lower_entry"] = _table(r, [(10, 10, 29, 29)], dict(entry=[1], need=[1], tid=[101]))

    r = TrackRef(S, T, iou_thr=0.3)             # boxes 20 wide shifted by d: IoU = (20 - d) / (20 + d)
    seed(r, SUBJECT, 0, (0, 0, 19, 19))         # A
    seed(r, SUBJECT, 2, (8, 0, 27, 19))         # B
    cases["greedy_in_detector_order"] = _table(r, [(6, 0, 25, 19), (8, 0, 27, 19)], dict(entry=[2, 0], need=[1, 1]))

    r = TrackRef(S, T)
    seed(r, SUBJECT, 0, (100, 100, 139, 139), since=1)
    seed(r, SUBJECT, 1, (135, 135, 174, 174))   # a corner of 5 x 5 pixels in common: far below thr, above 0
    cases["guard_on"] = _table(r, [(100, 100, 139, 139)], dict(entry=[0], need=[1], since=[0]))

    r = TrackRef(S, T)
    seed(r, SUBJECT, 0, (0, 0, 9, 9), since=1)
    seed(r, SUBJECT, 1, (10, 0, 19, 9))         # the next pixel column: w = 9 - 10 + 1 = 0
    cases["guard_off_at_zero"] = _table(r, [(0, 0, 9, 9)], dict(entry=[0], need=[0], since=[2]))

    r = TrackRef(S, T, max_reuse=3)
    seed(r, SUBJECT, 0, (0, 0, 39, 39), since=2)
    seed(r, SUBJECT, 1, (100, 0, 139, 39), since=3)
    cases["age"] = _table(r, [(0, 0, 39, 39), (100, 0, 139, 39)], dict(entry=[0, 1], need=[0, 1], since=[3, 0]))

    r = TrackRef(S, T, max_misses=1)
    seed(r, SUBJECT, 0, (0, 0, 39, 39), misses=1)
    seed(r, SUBJECT, 1, (100, 0, 139, 39), misses=0)
    r.next_id[SUBJECT] = 7
    cases["retire_and_reuse"] = _table(r, [FAR], dict(entry=[0], need=[1], tid=[7]))

    r = TrackRef(S, T)
    for t in range(T):
        seed(r, SUBJECT, t, (60 * t, 0, 60 * t + 39, 39))
    cases["table_full"] = _table(r, [FAR, (0, 0, 39, 39), (FAR[0], 300, FAR[2], 339)],
                                 dict(entry=[-1, 0, -1], need=[1, 0, 1], tid=[-1, 100, -1]))

    r = TrackRef(S, T, max_reuse=0)
    seed(r, SUBJECT, 0, (0, 0, 39, 39))
    cases["max_reuse_zero"] = _table(r, [(0, 0, 39, 39)], dict(entry=[0], need=[1], since=[0]))

    r = TrackRef(S, T)
    seed(r, SUBJECT, 0, (0, 0, 39, 39))
    seed(r, SUBJECT, 1, (100, np.nan, 139, 39))
    cases["nan_boxes"] = _table(r, [(0, 0, np.nan, 39), (100, 0, 139, 39), (0, 0, 39, 39)],
                                dict(entry=[2, 3, 0], need=[1, 1, 0]))

    r = TrackRef(S, T)
    seed(r, SUBJECT, 0, (0, 0, 39, 39))
    c = _table(r, [(0, 0, 39, 39)], dict(entry=[-1], need=[1], tid=[-1]), slots=(S, 0, -1))
    cases["slot_out_of_range"] = c              # frames 0 and 2 are stateless, slot SUBJECT is not touched
    return cases


def soup(seed_, entries, fractional=False, turns=20, n=5, slots=8, cap=8):
    """A seeded sequence: per turn (boxes f32 [n,cap,4], counts i32 [n], slot i32 [n]) with the cameras in shuffled slot order.
    People jitter by 0 .. 3 pixels a turn, are born and die, go undetected now and then, and pairs walk through each other;
    camera 1 is crowded past ``cap`` for a few turns and camera 2 goes empty for two."""
    rng = np.random.default_rng(seed_)
    slot = rng.permutation(slots)[:n].astype(np.int32)
    frac = (lambda: rng.random(2)) if fractional else (lambda: np.zeros(2))

    def person(x=None, y=None, v=(0, 0)):
        x = rng.integers(0, 560) if x is None else x
        y = rng.integers(0, 400) if y is None else y
        return dict(p=np.array([x, y], np.float64) + frac(), size=float(rng.integers(30, 61)), v=np.array(v, np.float64))

    people = [[person() for _ in range(int(rng.integers(2, 5)))] for _ in range(n)]
    for cam in (0, 3):                                           # a pair on one line, walking through each other
        y = int(rng.integers(50, 350))
        people[cam] += [person(100, y, (6, 0)), person(340, y, (-6, 0))]
    out = []
    for turn in range(turns):
        boxes, counts = np.zeros((n, cap, 4), F32), np.zeros(n, np.int32)
        for cam in range(n):
            ps = people[cam]
            for q in ps:
                q["p"] += q["v"] + rng.integers(-3, 4, 2) + (frac() - 0.5 if fractional else 0)
            ps[:] = [q for q in ps if rng.random() > 0.06]       # deaths
            if rng.random() < 0.25 and len(ps) < 7:
                ps.append(person())                              # births
            if cam == 1 and 6 <= turn < 10:
                while len(ps) < cap + 3:
                    ps.append(person())
            seen = [q for q in ps if rng.random() > 0.08]        # the detector loses a face now and then
            if cam == 2 and turn in (5, 6):
                seen = []
            order = rng.permutation(len(seen))[:cap]             # the detector's order is by score: any order to the tracks
            for j, k in enumerate(order):
                q = seen[k]
                boxes[cam, j] = (q["p"][0], q["p"][1], q["p"][0] + q["size"] - 1, q["p"][1] + q["size"] - 1)
            counts[cam] = len(order)
        out.append((boxes, counts, slot.copy()))
    return out


SOUPS = [(11, 8, False), (12, 13, False), (13, 64, False), (14, 8, True)]       # (seed, T, fractional)
SOUP_RULE = dict(iou_thr=0.5, max_reuse=3, max_misses=1)
