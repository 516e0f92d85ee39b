"""GPU: fr_track_associate_f32 and fr_track_resolve_quality_i32 together, turn by turn, against tests/helpers/track_ref.py plus
tests/helpers/track_quality_ref.py.  After every turn ``action``, ``need2``, ``entry2``, ``tstate`` and ``tqual`` are compared bit
for bit; every output and both state arrays of the resolve launch lie between guard words that must survive.  The branches the
sequences exercise are asserted on the reference's own trace (tests/test_track_quality_ref_host.py holds the reference to the
rule)."""
import ctypes

import numpy as np
import pytest

from tests.helpers import track_cases as tc
from tests.helpers.track_quality_ref import CARRY, EMBED, NONE, REJECT, TrackQualityRef
from tests.helpers.track_ref import TrackRef

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 0x5AC3C35A                              # as int32 no value the rule can write
PAD = 64                                        # guard words on either side
BLUR = 16


class Guarded:
    """an int32 device array between PAD guard words on either side"""

    def __init__(self, torch, init):
        self.torch, self.shape = torch, init.shape
        flat = np.full(init.size + 2 * PAD, GUARD, np.int32)
        flat[PAD:PAD + init.size] = init.reshape(-1)
        self.buf = torch.from_numpy(flat).to("cuda:0")
        self.view = self.buf[PAD:PAD + init.size]

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + 4 * PAD)

    def read(self, what):
        flat = self.buf.cpu().numpy()
        assert (flat[:PAD] == GUARD).all() and (flat[-PAD:] == GUARD).all(), f"{what}: a guard word was written"
        return flat[PAD:len(flat) - PAD].reshape(self.shape)


class Device:
    """the state of a TrackRef and a TrackQualityRef on the device, and the two launches over it"""

    def __init__(self, ref, tq):
        import torch
        from facerecognition_infrenceengine_amd import _lib
        self.torch, self._lib, self.lib = torch, _lib, _lib.load()
        self.S, self.T, self.max_age = ref.S, ref.T, tq.max_age
        self.rule = (float(ref.iou_thr), ref.max_reuse, ref.max_misses)
        self.tbox, self.next_id = self.up(ref.tbox), self.up(ref.next_id)
        self.tstate, self.tqual = Guarded(torch, ref.tstate), Guarded(torch, tq.tqual)

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    def turn(self, boxes, counts, slot, verdict, what):
        """associate + resolve -> (entry, need, tid, action, need2, entry2) on the host, the guards checked"""
        t, p = self.torch, self._lib.ptr
        n, cap = boxes.shape[:2]
        b, c, s = self.up(boxes.astype(F32)), self.up(np.asarray(counts, np.int32)), self.up(np.asarray(slot, np.int32))
        v = self.up(np.asarray(verdict, np.int32))
        first = [t.full((n, cap), -77, dtype=t.int32, device="cuda:0") for _ in range(3)]
        self.lib.fr_track_associate_f32(p(b), p(c), p(s), n, cap, self.S, self.T, p(self.tbox), self.tstate.ptr(), p(self.next_id),
                                        *self.rule, p(first[0]), p(first[1]), p(first[2]), self._lib.stream_ptr())
        out = [Guarded(t, np.full((n, cap), -77, np.int32)) for _ in range(3)]
        self.lib.fr_track_resolve_quality_i32(p(first[0]), p(first[1]), p(first[2]), p(v), p(s), p(c), n, cap, self.S, self.T,
                                              self.tstate.ptr(), self.tqual.ptr(), self.max_age, out[0].ptr(), out[1].ptr(),
                                              out[2].ptr(), self._lib.stream_ptr())
        t.cuda.synchronize()
        return tuple(o.cpu().numpy() for o in first) + tuple(o.read((what, k)) for k, o in zip(("action", "need2", "entry2"), out))

    def same_state(self, ref, tq, what):
        assert np.array_equal(self.tstate.read((what, "tstate")), ref.tstate), (what, "tstate")
        assert np.array_equal(self.tqual.read((what, "tqual")), tq.tqual), (what, "tqual")
        assert np.array_equal(self.tbox.cpu().numpy().view(np.uint32), ref.tbox.view(np.uint32)), (what, "tbox")
        assert np.array_equal(self.next_id.cpu().numpy(), ref.next_id), (what, "next_id")


def _both(dev, ref, tq, boxes, counts, slot, verdict, what):
    got = dev.turn(boxes, counts, slot, verdict, what)
    entry, need, tid = ref.associate(boxes, counts, slot)
    want = (entry, need, tid) + tq.resolve(entry, need, tid, verdict, slot, counts)
    for name, g, w in zip(("entry", "need", "tid", "action", "need2", "entry2"), got, want):
        assert g.dtype == np.int32 and np.array_equal(g, w), (what, name, g.tolist(), w.tolist())
    dev.same_state(ref, tq, what)
    return want


def _verdicts(rng, shape, turn):
    v = np.where(rng.random(shape) < 0.3, BLUR, 0).astype(np.int32)
    if 6 <= turn < 16:
        v[np.arange(shape[0]) != 1] = BLUR | 1                    # a blurred stretch past max_age = 8 (any non-zero value is
                                                                  # "unfit"); camera 1, crowded past the table then, keeps its mix
    if turn == 13:
        v[:] = -1                                                 # the quality launch's "no face": unfit too where a face is
    return v


@pytest.mark.parametrize("max_age", [0, 1, 8])
@pytest.mark.parametrize("seed_,entries,fractional", tc.SOUPS)
def test_soups_match_the_reference_turn_by_turn(seed_, entries, fractional, max_age):
    """N = 5 frames, cap = 8, S = 8, T = 8 / 13 / 64 over 20 turns"""
    ref = TrackRef(8, entries, **tc.SOUP_RULE)
    tq = TrackQualityRef(ref, max_age=max_age)
    dev = Device(ref, tq)
    rng = np.random.default_rng(seed_ + 7)
    for turn, (boxes, counts, slot) in enumerate(tc.soup(seed_, entries, fractional)):
        want = _both(dev, ref, tq, boxes, counts, slot, _verdicts(rng, boxes.shape[:2], turn), (seed_, turn))
        assert not ((want[1] == 1) & (want[3] == CARRY)).any()    # need == 1 is never given a held row
    assert tq.trace["embed"] and tq.trace["reject_cleared"] and tq.trace["no_row"]
    if max_age:
        assert tq.trace["carry"] > 20 and tq.trace["reject_kept"] and tq.trace["expired"]
    else:
        assert tq.trace["carry"] == 0 and tq.trace["reject_kept"] == 0
    if entries == 8:
        assert tq.trace["embed_untracked"] and tq.trace["reject_untracked"] and ref.trace["full"]


def _people(rng, n, cap, per_frame):
    """n frames of disjoint boxes on a grid (they jitter by a pixel a turn, so they match and are never guarded)"""
    boxes = np.zeros((n, cap, 4), F32)
    for i in range(n):
        for j in range(per_frame[i]):
            x, y = 50 * (j % 8), 50 * (j // 8)
            boxes[i, j] = (x, y, x + 39, y + 39)
    return boxes


@pytest.mark.parametrize("N,cap,T,S", [(1, 1, 1, 1), (3, 4, 2, 5), (37, 64, 64, 5), (37, 4, 1, 1), (3, 64, 2, 1), (1, 4, 64, 5)])
def test_shapes_counts_and_slots_outside_their_ranges(N, cap, T, S):
    """counts above cap and negative, slots outside [0, S) (several frames may share such a slot: they have no state), more than
    one block of threads (37 x 64 slots); six turns so that carries, rejects with a kept row and expiry all occur"""
    rng = np.random.default_rng(N * 1000 + cap * 10 + T)
    ref = TrackRef(S, T, iou_thr=0.5, max_reuse=2, max_misses=1)
    tq = TrackQualityRef(ref, max_age=2)
    dev = Device(ref, tq)
    slot = np.full(N, S, np.int32)                                # stateless unless given a slot of its own
    inside = rng.permutation(N)[:S]
    slot[inside] = rng.permutation(S)[:len(inside)]
    if N > S:
        slot[[i for i in range(N) if i not in set(inside.tolist())][0]] = -1
    per_frame = rng.integers(0, cap + 1, N)
    per_frame[inside[0]] = cap
    counts = per_frame.astype(np.int32)
    if N >= 3:
        outside = [i for i in range(N) if i not in set(inside.tolist())]
        counts[inside[-1]] = -3 if len(inside) > 1 else counts[inside[-1]]     # negative: no face
        per_frame[inside[-1]] = 0 if len(inside) > 1 else per_frame[inside[-1]]
        if outside:
            counts[outside[-1]] = cap + 5                         # above cap: clamped
            per_frame[outside[-1]] = cap
    boxes = _people(rng, N, cap, per_frame)
    for turn in range(6):
        verdict = np.where(rng.random((N, cap)) < (0.2 if turn < 2 else 0.8), BLUR, 0).astype(np.int32)
        jitter = boxes + F32(turn % 2)
        want = _both(dev, ref, tq, jitter, counts, slot, verdict, (N, cap, T, S, turn))
        held = np.arange(cap)[None, :] < np.clip(counts, 0, cap)[:, None]
        assert ((want[3] != NONE) == held).all()
        stateless = ~np.isin(np.arange(N), inside)
        assert (want[5][stateless] == -1).all() and not (want[3][stateless] == CARRY).any()
    if T * len(inside) >= 2:
        assert tq.trace["carry"] and tq.trace["embed"]
    assert tq.trace["embed_untracked"] + tq.trace["reject_untracked"] > 0 or (N == 1 and T >= cap)


def test_launch_shape_does_not_change_the_result():
    """the five cameras of a turn in one launch pair, or one launch pair each: the same bits"""
    refs = [TrackRef(8, 13, **tc.SOUP_RULE) for _ in range(2)]
    tqs = [TrackQualityRef(r, max_age=3) for r in refs]
    da, db = (Device(r, q) for r, q in zip(refs, tqs))
    rng = np.random.default_rng(3)
    for turn, (boxes, counts, slot) in enumerate(tc.soup(12, 13)[:10]):
        verdict = _verdicts(rng, boxes.shape[:2], turn + 4)
        together = da.turn(boxes, counts, slot, verdict, turn)
        apart = [db.turn(boxes[i:i + 1], counts[i:i + 1], slot[i:i + 1], verdict[i:i + 1], (turn, i)) for i in range(5)]
        for k in range(6):
            assert np.array_equal(together[k], np.concatenate([x[k] for x in apart])), (turn, k)
        assert np.array_equal(da.tstate.read("a"), db.tstate.read("b")) and np.array_equal(da.tqual.read("a"), db.tqual.read("b"))
    assert (da.tqual.read("a")[:, :, 0] == 1).any()


def test_an_entry_index_outside_the_table_is_case_a():
    """entry >= T or a negative entry other than -1 (never written by the associate launch): judged, no state touched"""
    ref = TrackRef(2, 4)
    tq = TrackQualityRef(ref, max_age=8)
    dev = Device(ref, tq)
    t, p = dev.torch, dev._lib.ptr
    entry = np.array([[4, -5, 1000, 3]], np.int32)
    need = np.array([[0, 0, 1, 0]], np.int32)
    tid = np.array([[7, 7, 7, 9]], np.int32)
    verdict = np.array([[0, BLUR, BLUR, 0]], np.int32)
    slot, counts = np.array([1], np.int32), np.array([4], np.int32)
    want = tq.resolve(entry, need, tid, verdict, slot, counts)
    assert want[0].tolist() == [[EMBED, REJECT, REJECT, EMBED]] and want[2].tolist() == [[4, -1, -1, 3]]
    ins = [dev.up(a) for a in (entry, need, tid, verdict, slot, counts)]
    out = [Guarded(t, np.full((1, 4), -77, np.int32)) for _ in range(3)]
    dev.lib.fr_track_resolve_quality_i32(*(p(a) for a in ins), 1, 4, 2, 4, dev.tstate.ptr(), dev.tqual.ptr(), 8,
                                         out[0].ptr(), out[1].ptr(), out[2].ptr(), dev._lib.stream_ptr())
    t.cuda.synchronize()
    for k, (o, w) in enumerate(zip(out, want)):
        assert np.array_equal(o.read(k), w), k
    dev.same_state(ref, tq, "outside")
    assert tq.tqual[1, 3, :3].tolist() == [1, 0, 9] and int(np.abs(tq.tqual).sum()) == 10


def test_refusals_and_the_empty_call_leave_everything_alone():
    from facerecognition_infrenceengine_amd import _lib
    ref = TrackRef(2, 4)
    tq = TrackQualityRef(ref, max_age=8)
    tq.tqual[...] = 5
    dev = Device(ref, tq)
    t, p = dev.torch, dev._lib.ptr
    ins = [dev.up(np.zeros((2, 4), np.int32)) for _ in range(4)] + [dev.up(np.zeros(2, np.int32)), dev.up(np.full(2, 4, np.int32))]
    out = [Guarded(t, np.full((2, 4), -77, np.int32)) for _ in range(3)]

    def call(N=2, cap=4, S=2, T=4, max_age=8, drop=None):
        a = [p(x) for x in ins] + [dev.tstate.ptr(), dev.tqual.ptr()] + [o.ptr() for o in out]
        if drop is not None:
            a[drop] = None
        return dev.lib.fr_track_resolve_quality_i32(*a[:6], N, cap, S, T, a[6], a[7], max_age, a[8], a[9], a[10],
                                                    dev._lib.stream_ptr())
    for kw in (dict(T=0), dict(T=65), dict(cap=0), dict(cap=65), dict(S=0), dict(N=-1), dict(N=65536), dict(max_age=-1)):
        with pytest.raises(_lib.FrError):
            call(**kw)
    for drop in range(11):
        with pytest.raises(_lib.FrError, match="null pointer"):
            call(drop=drop)
    assert call(N=0) == 0
    t.cuda.synchronize()
    for o in out:
        assert (o.read("refused") == -77).all()
    dev.same_state(ref, tq, "refused")
