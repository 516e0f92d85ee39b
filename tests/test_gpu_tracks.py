"""GPU: fr_track_associate_f32 / fr_track_commit_f32 against the NumPy reference (tests/helpers/track_ref.py), bit for bit.  After
every turn all outputs and the whole state are compared: tbox bits, tstate, next_id, bank.  The inputs are those of
tests/test_track_ref_host.py, which checks each case's premise and that the soups exercise carry, re-embed by age and by
guard, retire, reuse of an entry and a full table."""
import copy

import numpy as np
import pytest

from tests.helpers import track_cases as tc
from tests.helpers.track_ref import DIM, TrackRef

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL = 0x7FC5A5A5                           # a NaN with a payload: any arithmetic on it, or a 0 / 1 fill, would show


class Device:
    """the state of a TrackRef on the device, and the two entries over it"""

    def __init__(self, ref):
        import torch
        from facerecognition_infrenceengine_amd import _lib
        self.torch, self._lib, self.lib = torch, _lib, _lib.load()
        self.S, self.T = ref.S, ref.T
        self.rule = (float(ref.iou_thr), ref.max_reuse, ref.max_misses)
        self.tbox, self.tstate, self.next_id, self.bank = (self.up(a) for a in (ref.tbox, ref.tstate, ref.next_id, ref.bank))

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    def associate(self, boxes, counts, slot):
        t, p = self.torch, self._lib.ptr
        n, cap = boxes.shape[:2]
        b, c, s = self.up(boxes.astype(F32)), self.up(np.asarray(counts, np.int32)), self.up(np.asarray(slot, np.int32))
        out = [t.full((n, cap), -77, dtype=t.int32, device="cuda:0") for _ in range(3)]
        self.lib.fr_track_associate_f32(p(b), p(c), p(s), n, cap, self.S, self.T, p(self.tbox), p(self.tstate), p(self.next_id),
                                        *self.rule, p(out[0]), p(out[1]), p(out[2]), self._lib.stream_ptr())
        t.cuda.synchronize()
        return tuple(o.cpu().numpy() for o in out)

    def commit(self, entry, need, slot, counts, emb, normed):
        p = self._lib.ptr
        n, cap = entry.shape
        e, nd, s, c = (self.up(np.asarray(a, np.int32)) for a in (entry, need, slot, counts))
        em, nm = self.up(emb), self.up(normed)
        self.lib.fr_track_commit_f32(p(e), p(nd), p(s), p(c), n, cap, self.S, self.T, p(self.bank), p(em), p(nm),
                                     self._lib.stream_ptr())
        self.torch.cuda.synchronize()
        return em.cpu().numpy(), nm.cpu().numpy()

    def same_state(self, ref, what):
        for name in ("tbox", "tstate", "next_id", "bank"):
            got, want = getattr(self, name).cpu().numpy(), getattr(ref, name)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (what, name)


def _sentinel(shape):
    return np.full(shape, SENTINEL, np.uint32).view(F32)


def _turn(dev, ref, boxes, counts, slot, rng, what):
    """one associate + commit on both sides, everything compared"""
    got = dev.associate(boxes, counts, slot)
    want = ref.associate(boxes, counts, slot)
    for name, g, w in zip(("entry", "need", "tid"), got, want):
        assert np.array_equal(g, w), (what, name, g.tolist(), w.tolist())
    dev.same_state(ref, what)
    entry, need, _ = want
    n, cap = entry.shape
    emb, normed = _sentinel((n * cap, DIM)), _sentinel((n * cap, DIM))
    fresh = (need.reshape(-1) != 0).nonzero()[0]                 # the rows the embed net would have written
    emb[fresh] = rng.standard_normal((len(fresh), DIM)).astype(F32)
    normed[fresh] = rng.standard_normal((len(fresh), DIM)).astype(F32)
    g_emb, g_normed = dev.commit(entry, need, slot, counts, emb.copy(), normed.copy())
    ref.commit(entry, need, slot, counts, emb, normed)
    assert np.array_equal(g_emb.view(np.uint32), emb.view(np.uint32)), (what, "emb")
    assert np.array_equal(g_normed.view(np.uint32), normed.view(np.uint32)), (what, "normed")
    dev.same_state(ref, what)
    return entry, need, emb, normed


@pytest.mark.parametrize("name", sorted(tc.hand_cases()))
def test_hand_tables_match_the_reference(name):
    case = tc.hand_cases()[name]
    ref = case["ref"]
    ref.bank[...] = _sentinel(ref.bank.shape)
    dev = Device(ref)
    _turn(dev, ref, case["boxes"], case["counts"], case["slot"], np.random.default_rng(1), name)


@pytest.mark.parametrize("seed_,entries,fractional", tc.SOUPS)
def test_soups_match_the_reference_turn_by_turn(seed_, entries, fractional):
    ref = TrackRef(8, entries, **tc.SOUP_RULE)
    ref.bank[...] = _sentinel(ref.bank.shape)
    dev = Device(ref)
    rng = np.random.default_rng(seed_)
    carried = 0
    for turn, (boxes, counts, slot) in enumerate(tc.soup(seed_, entries, fractional)):
        entry, need, emb, _ = _turn(dev, ref, boxes, counts, slot, rng, (seed_, turn))
        valid = np.arange(8)[None, :] < counts[:, None]
        c = valid & (need == 0)
        carried += int(c.sum())
        # a carried row never holds the sentinel: its entry was embedded in an earlier turn
        assert not (emb.view(np.uint32)[c.reshape(-1)] == SENTINEL).any()
    assert carried > 100 and ref.trace["reembed_guard"] and ref.trace["retire"] and ref.trace["reuse"]


def test_commit_moves_rows_in_the_stated_direction_only():
    """every row of emb / normed and of bank that the rule does not name keeps the sentinel"""
    case = tc.hand_cases()["table_full"]
    ref = case["ref"]
    ref.bank[...] = _sentinel(ref.bank.shape)
    ref.bank[tc.SUBJECT, 0] = np.random.default_rng(5).standard_normal((2, DIM)).astype(F32)
    dev = Device(ref)
    entry, need, emb, normed = _turn(dev, ref, case["boxes"], case["counts"], case["slot"], np.random.default_rng(6), "commit")
    bank = dev.bank.cpu().numpy().view(np.uint32)
    for s in range(tc.S):
        for t in range(tc.T):
            if s == 3:                                           # frame 2: four new tracks in slot 3
                assert not (bank[s, t] == SENTINEL).any(), (s, t)
            elif (s, t) != (tc.SUBJECT, 0):                      # the carried entry keeps the rows planted above
                assert (bank[s, t] == SENTINEL).all(), (s, t)
    rows = emb.view(np.uint32)
    assert np.array_equal(emb[1], ref.bank[tc.SUBJECT, 0, 0]) and np.array_equal(normed[1], ref.bank[tc.SUBJECT, 0, 1])
    untouched = [q for q in range(3 * tc.CAP) if q not in (0, 1, 2, 8, 9, 10, 11)]      # padding slots and the empty frame
    assert (rows[untouched] == SENTINEL).all()


def test_out_of_range_slot_is_stateless_on_the_device():
    case = tc.hand_cases()["slot_out_of_range"]
    ref = case["ref"]
    ref.bank[...] = _sentinel(ref.bank.shape)
    before = copy.deepcopy((ref.tbox, ref.tstate, ref.next_id))
    dev = Device(ref)
    entry, need, emb, _ = _turn(dev, ref, case["boxes"], case["counts"], case["slot"], np.random.default_rng(2), "stateless")
    assert (entry == -1).all() and need[0].tolist() == [1, 0, 0, 0] and need[2].tolist() == [1] * 4
    got = dev.tstate.cpu().numpy()
    assert np.array_equal(got[1:], before[1][1:]) and np.array_equal(dev.next_id.cpu().numpy(), before[2])
    assert (dev.bank.cpu().numpy().view(np.uint32) == SENTINEL).all()


def test_launch_shape_does_not_change_the_result():
    """the five cameras of a turn in one launch, or one launch each: the same state"""
    a, b = TrackRef(8, 13, **tc.SOUP_RULE), TrackRef(8, 13, **tc.SOUP_RULE)
    da, db = Device(a), Device(b)
    for boxes, counts, slot in tc.soup(12, 13)[:8]:
        together = da.associate(boxes, counts, slot)
        apart = [db.associate(boxes[i:i + 1], counts[i:i + 1], slot[i:i + 1]) for i in range(5)]
        for k in range(3):
            assert np.array_equal(together[k], np.concatenate([x[k] for x in apart]))
    for name in ("tbox", "tstate", "next_id"):
        assert np.array_equal(getattr(da, name).cpu().numpy().view(np.uint32), getattr(db, name).cpu().numpy().view(np.uint32))
