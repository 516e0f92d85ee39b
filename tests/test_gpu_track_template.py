"""GPU: fr_track_fuse_f32 against tests/helpers/track_template_ref.py, turn by turn over scripted sequences: ``query``, ``shots``,
``event`` and the whole state (``tring``, ``ttmpl``, ``tmean``) bit for bit after every turn.  Every array the launch writes lies
between guard words that must survive, every output is filled with a sentinel beforehand (every row has to be written), and every
state row the script never names holds a NaN-payload sentinel that must still be there.  The branches the script exercises are
asserted on the reference's own events (tests/test_track_template_ref_host.py holds the reference to the rule)."""
import ctypes

import numpy as np
import pytest

from tests.helpers.scan_ref import l2norm_rows, row_dot_wave8
from tests.helpers.track_template_ref import JOINED, NONE, READ, RESTARTED, STARTED, TrackTemplateRef

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 0x5AC3C35A                              # as int32 no value the rule can write, as float32 about 2.8e16
SENTINEL = 0x7FC0BEEF                           # a quiet NaN with a payload
PAD = 64                                        # guard words on either side


class Guarded:
    """a 4-byte device array (float32 or int32, held as int32 words) between PAD guard words on either side"""

    def __init__(self, torch, init):
        self.torch, self.shape, self.dtype = torch, init.shape, init.dtype
        flat = np.full(init.size + 2 * PAD, GUARD, np.int32)
        flat[PAD:PAD + init.size] = np.ascontiguousarray(init).reshape(-1).view(np.int32)
        self.buf = torch.from_numpy(flat).to("cuda:0")

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + 4 * PAD)

    def read(self, what):
        flat = self.buf.cpu().numpy()
        assert (flat[:PAD] == GUARD).all() and (flat[-PAD:] == GUARD).all(), f"{what}: a guard word was written"
        return flat[PAD:len(flat) - PAD].view(self.dtype).reshape(self.shape)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Device:
    """the state of a TrackTemplateRef on the device, and the launch over it"""

    def __init__(self, ref):
        import torch
        from facerecognition_infrenceengine_amd import _lib
        self.torch, self._lib, self.lib, self.ref = torch, _lib, _lib.load(), ref
        self.state = [Guarded(torch, a) for a in (ref.tring, ref.ttmpl, ref.tmean)]

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    def turn(self, entry, need, tid, slot, counts, normed, what):
        """the launch -> (query, shots, event) on the host, guards and state checked against the reference after ITS turn"""
        t, p, ref = self.torch, self._lib.ptr, self.ref
        n, cap = entry.shape
        ins = [self.up(np.asarray(a, np.int32)) for a in (entry, need, tid, slot, counts)] + [self.up(normed.astype(F32))]
        out = [Guarded(t, np.full((n * cap, 512), SENTINEL, np.int32).view(F32)), Guarded(t, np.full((n, cap), -77, np.int32)),
               Guarded(t, np.full((n, cap), -77, np.int32))]
        rc = self.lib.fr_track_fuse_f32(*(p(a) for a in ins), n, cap, ref.S, ref.T, ref.K, float(ref.join_thr),
                                        *(s.ptr() for s in self.state), *(o.ptr() for o in out), self._lib.stream_ptr())
        assert rc == 0
        t.cuda.synchronize()
        return tuple(o.read((what, k)) for k, o in zip(("query", "shots", "event"), out))

    def same_state(self, what):
        for name, dev, want in zip(("tring", "ttmpl", "tmean"), self.state, (self.ref.tring, self.ref.ttmpl, self.ref.tmean)):
            assert same_bits(dev.read((what, name)), want), (what, name)


def _both(dev, turn, what):
    got = dev.turn(*turn, what)
    want = dev.ref.fuse(*turn)
    for name, g, w in zip(("query", "shots", "event"), got, want):
        assert same_bits(g, w), (what, name, np.argwhere(g.view(np.uint32) != w.view(np.uint32))[:4].tolist())
    dev.same_state(what)
    return want


def unit(rng, rows=1):
    return l2norm_rows(rng.standard_normal((rows, 512)).astype(F32))


def near(rng, row, sigma):
    noise = rng.standard_normal(512).astype(F32) * F32(sigma / np.sqrt(512.0))
    return l2norm_rows((row + noise)[None])[0]


# ---------------------------------------------------------------- the script: S = 3, T = 4, cap = 4, N = 3, eight turns
S, T, CAP, N, TURNS = 3, 4, 4, 3, 8
TOUCHED = {(2, 1), (2, 3), (0, 0), (0, 1), (0, 2), (0, 3)}        # the (slot, entry) rows the script names


class Actor:
    """a track: its person's row and the last row embedded for it (what the commit launch hands a carried face)"""

    def __init__(self, rng):
        self.person, self.last = unit(rng)[0], None

    def shot(self, rng, sigma=0.3, row=None):
        self.last = near(rng, self.person, sigma) if row is None else row
        return self.last


def script():
    """-> (join_thr, turns, expected events): turn = (entry, need, tid, slot, counts, normed); expected[turn] = {(frame, j): event}.
    Even turns name the slots (2, 0, 3), odd turns (0, -1, 2): frames go to slots out of order, and slot 3 / -1 is outside [0, S).
      A  slot 2 entry 1 id 7: started, joined, read, joined (3 shots), joined (wrap), NaN row (restart), restart, joined
      B  slot 2 entry 3 id 8: started, read, a foreign row (restart); id 9 on the same entry: started, read, joined; entry -1; joined
      C  slot 0 entry 0 id 3: started, joined AT the threshold, a turn with count 0, read, joined beside three more entries under a
         count above cap, joined (wrap), joined, entry == T
      D  the stateless frame: entry 2, need 1 each turn; count -2 on turn 3"""
    rng = np.random.default_rng(2026)
    A, B, B2, C, D, X = (Actor(rng) for _ in range(6))
    extra = {e: Actor(rng) for e in (1, 2, 3)}                     # slot 0's other entries
    foreign = unit(rng)[0]
    c0, c1 = C.shot(rng, 1.0), near(rng, C.person, 1.0)
    join_thr = float(row_dot_wave8(c1[None], c0[None])[0, 0])     # C's second shot meets its first at exactly this value
    assert 0.3 < join_thr < 0.7
    turns, expected = [], []
    for t in range(TURNS):
        even = t % 2 == 0
        fa, fc, fd = (0, 1, 2) if even else (2, 0, 1)
        slot = np.zeros(N, np.int32)
        slot[fa], slot[fc], slot[fd] = 2, 0, (3 if even else -1)
        entry = np.full((N, CAP), -1, np.int32)
        need = np.zeros((N, CAP), np.int32)
        tid = np.full((N, CAP), -1, np.int32)
        counts = np.zeros(N, np.int32)
        normed = unit(rng, N * CAP)                                # the rows of slots without a face: anything
        want = {}

        def put(f, j, e, nd, id_, row, ev):
            entry[f, j], need[f, j], tid[f, j], normed[f * CAP + j] = e, nd, id_, row
            want[(f, j)] = ev
        ja, jb = (0, 1) if even else (1, 0)                         # two detections of one frame, on different entries
        counts[fa] = 2
        if t == 5:
            bad = near(rng, A.person, 0.3)
            bad[300] = np.nan
            put(fa, ja, 1, 1, 7, A.shot(rng, row=bad), RESTARTED)
        elif t == 2:
            put(fa, ja, 1, 0, 7, A.last, READ)
        else:
            put(fa, ja, 1, 1, 7, A.shot(rng), {0: STARTED, 6: RESTARTED}.get(t, JOINED))
        if t == 0:
            put(fa, jb, 3, 1, 8, B.shot(rng), STARTED)
        elif t == 1:
            put(fa, jb, 3, 0, 8, B.last, READ)
        elif t == 2:
            put(fa, jb, 3, 1, 8, B.shot(rng, row=foreign), RESTARTED)
        elif t == 3:
            put(fa, jb, 3, 1, 9, B2.shot(rng), STARTED)             # the entry under a new id: the held template is not its
        elif t == 4:
            put(fa, jb, 3, 0, 9, B2.last, READ)
        elif t == 6:
            put(fa, jb, -1, 1, -1, X.shot(rng), NONE)               # untracked
        else:
            put(fa, jb, 3, 1, 9, B2.shot(rng), JOINED)
        counts[fc] = 1
        if t == 0:
            put(fc, 0, 0, 1, 3, c0, STARTED)
        elif t == 1:
            put(fc, 0, 0, 1, 3, C.shot(rng, row=c1), JOINED)
        elif t == 2:
            counts[fc] = 0
            put(fc, 0, 0, 1, 3, near(rng, C.person, 0.3), NONE)     # behind the count: not a face
        elif t == 3:
            put(fc, 0, 0, 0, 3, C.last, READ)
        elif t == 4:
            counts[fc] = CAP + 3                                    # clamped to cap
            put(fc, 0, 0, 1, 3, C.shot(rng), JOINED)
            put(fc, 1, 1, 0, 4, extra[1].shot(rng), NONE)           # carried, and the entry holds no template
            put(fc, 2, 2, 1, 5, extra[2].shot(rng), STARTED)
            put(fc, 3, 3, 1, 6, extra[3].shot(rng), STARTED)
        elif t == 5:
            counts[fc] = 2
            put(fc, 0, 0, 1, 3, C.shot(rng), JOINED)
            put(fc, 1, 1, 1, 4, extra[1].shot(rng), STARTED)
        elif t == 6:
            put(fc, 0, 0, 1, 3, C.shot(rng), JOINED)
        else:
            put(fc, 0, T, 1, 3, C.shot(rng), NONE)                  # an entry index outside the table
        counts[fd] = -2 if t == 3 else 1
        put(fd, 0, 2, 1, 1, D.shot(rng), NONE)                      # a frame without state
        turns.append((entry, need, tid, slot, counts, normed))
        expected.append(want)
    return join_thr, turns, expected


def _planted(K, join_thr):
    """the reference with the sentinel in every state row the script never names"""
    ref = TrackTemplateRef(S, T, K, join_thr)
    for s in range(S):
        for e in range(T):
            if (s, e) not in TOUCHED:
                ref.tring[s, e].view(np.uint32)[...] = SENTINEL
                ref.ttmpl[s, e] = SENTINEL
                ref.tmean[s, e].view(np.uint32)[...] = SENTINEL
    return ref


def _untouched_rows_hold_the_sentinel(ref):
    for s in range(S):
        for e in range(T):
            if (s, e) not in TOUCHED:
                assert (ref.tring[s, e].view(np.uint32) == SENTINEL).all() and (ref.ttmpl[s, e] == SENTINEL).all()
                assert (ref.tmean[s, e].view(np.uint32) == SENTINEL).all()


def test_the_script_matches_the_reference_turn_by_turn():
    join_thr, turns, expected = script()
    ref = _planted(3, join_thr)
    dev = Device(ref)
    at_threshold = False
    for t, (turn, want_ev) in enumerate(zip(turns, expected)):
        query, shots, event = _both(dev, turn, t)
        for (f, j), ev in want_ev.items():
            assert event[f, j] == ev, (t, f, j, int(event[f, j]), ev)
        assert int((event != NONE).sum()) == sum(ev != NONE for ev in want_ev.values())
        c = ref.cos[~np.isnan(ref.cos)]
        at_threshold |= bool((c == ref.join_thr).any())
        assert (np.abs(c[c != ref.join_thr] - ref.join_thr) > 0.05).all()    # every other join test is far from the threshold
        plain = (event == NONE).reshape(-1)
        assert same_bits(query[plain], turn[5][plain]) and (shots.reshape(-1)[plain] == 0).all()
    assert at_threshold
    tr = ref.trace
    assert tr["wrapped"] >= 2 and tr["stale_id"] == 1 and tr["nan_restart"] == 2 and tr["carried_without"] == 1
    assert tr["started"] == 7 and tr["restarted"] == 3 and tr["read"] == 4 and tr["joined"] >= 10
    _untouched_rows_hold_the_sentinel(ref)
    dev.same_state("end")


def test_depth_one_answers_with_the_normed_rows():
    join_thr, turns, _ = script()
    ref = _planted(1, join_thr)
    dev = Device(ref)
    for t, turn in enumerate(turns):
        query, shots, event = _both(dev, turn, t)
        assert same_bits(query, turn[5]), t                           # K = 1: query == normed, bit for bit, on every turn
        assert ((shots == 1) == (event != NONE)).all()
    assert ref.trace["joined"] and ref.trace["restarted"] and ref.trace["read"]
    _untouched_rows_hold_the_sentinel(ref)


def test_the_limits_k16_t64_cap64():
    """S = 1, N = 1: 64 detections on 64 entries in a scrambled order, 18 turns so that every 16-deep ring wraps; every fourth
    track meets a foreign row on turn 9 and the odd tracks are carried on turn 5"""
    rng = np.random.default_rng(64)
    K, T_, cap = 16, 64, 64
    ref = TrackTemplateRef(1, T_, K, 0.4)
    dev = Device(ref)
    people, last = unit(rng, T_), np.zeros((T_, 512), F32)
    for t in range(18):
        order = rng.permutation(T_).astype(np.int32)
        entry, tid = order[None, :].copy(), (order[None, :] + 100).astype(np.int32)
        need = np.ones((1, cap), np.int32)
        normed = np.empty((cap, 512), F32)
        for j, e in enumerate(order):
            if t == 5 and e % 2:
                need[0, j], normed[j] = 0, last[e]
                continue
            normed[j] = unit(rng)[0] if (t == 9 and e % 4 == 0) else near(rng, people[e], 0.3)
            last[e] = normed[j]
        query, shots, event = _both(dev, (entry, need, tid, np.zeros(1, np.int32), np.array([cap], np.int32), normed), t)
        if t == 5:
            assert (event[0][order % 2 == 1] == READ).all()
        if t == 9:
            assert (event[0][order % 4 == 0] == RESTARTED).all()
    assert ref.trace["wrapped"] >= 64 and (ref.ttmpl[0, 1::2, 0] == K).all() and ref.trace["restarted"] == 32
    assert ref.trace["joined"] == 64 * 18 - 32 - 64 - 32    # all but the carried, the first and the restarted shots


def test_launch_shape_does_not_change_the_result():
    """the three frames of a turn in one launch, or one launch each: the same bits"""
    join_thr, turns, _ = script()
    da, db = Device(_planted(3, join_thr)), Device(_planted(3, join_thr))
    for t, (entry, need, tid, slot, counts, normed) in enumerate(turns):
        together = da.turn(entry, need, tid, slot, counts, normed, t)
        apart = [db.turn(entry[i:i + 1], need[i:i + 1], tid[i:i + 1], slot[i:i + 1], counts[i:i + 1],
                         normed[i * CAP:(i + 1) * CAP], (t, i)) for i in range(N)]
        for k in range(3):
            assert same_bits(together[k], np.concatenate([x[k] for x in apart])), (t, k)
        for a, b in zip(da.state, db.state):
            assert same_bits(a.read("a"), b.read("b")), t


def test_refusals_and_the_empty_call_leave_everything_alone():
    from facerecognition_infrenceengine_amd import _lib
    ref = _planted(3, 0.4)
    dev = Device(ref)
    t, p = dev.torch, dev._lib.ptr
    ins = [dev.up(np.zeros((2, 4), np.int32)) for _ in range(3)] + [dev.up(np.zeros(2, np.int32)), dev.up(np.full(2, 4, np.int32)),
                                                                    dev.up(np.zeros((8, 512), F32))]
    out = [Guarded(t, np.full((8, 512), SENTINEL, np.int32).view(F32)), Guarded(t, np.full((2, 4), -77, np.int32)),
           Guarded(t, np.full((2, 4), -77, np.int32))]

    def call(N=2, cap=4, S_=S, T_=T, K=3, join_thr=0.4, drop=None):
        a = [p(x) for x in ins] + [s.ptr() for s in dev.state] + [o.ptr() for o in out]
        if drop is not None:
            a[drop] = None
        return dev.lib.fr_track_fuse_f32(*a[:6], N, cap, S_, T_, K, join_thr, *a[6:], dev._lib.stream_ptr())
    for kw in (dict(T_=0), dict(T_=65), dict(cap=0), dict(cap=65), dict(S_=0), dict(N=-1), dict(N=65536), dict(K=0), dict(K=17),
               dict(join_thr=1.5), dict(join_thr=-1.5), dict(join_thr=float("nan"))):
        with pytest.raises(_lib.FrError):
            call(**kw)
    for drop in range(12):
        with pytest.raises(_lib.FrError, match="null pointer"):
            call(drop=drop)
    assert call(N=0) == 0
    t.cuda.synchronize()
    assert (out[0].read("refused").view(np.uint32) == SENTINEL).all()
    for o in out[1:]:
        assert (o.read("refused") == -77).all()
    dev.same_state("refused")
