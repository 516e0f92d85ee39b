"""CPU: tests/helpers/track_template_ref.py, the definition of track templates (include/frhip.h fr_track_fuse_f32), held to the
rule on hand-built sequences - depth 1, hand-computed means, the order of a wrapped ring, a join exactly at the threshold, a
NaN row, a stale id - and to the planted sequence DESIGN.md 4.5g quotes: noisy shots of one person, a foreign row on turn 8."""
import numpy as np

from tests.helpers.scan_ref import l2norm_rows, mean_rows, row_dot_wave8
from tests.helpers.track_template_ref import JOINED, NONE, READ, RESTARTED, STARTED, TrackTemplateRef

F32 = np.float32


def unit(rng, rows=1):
    return l2norm_rows(rng.standard_normal((rows, 512)).astype(F32))


def near(rng, row, sigma):
    """a unit row at cosine about 1 / sqrt(1 + sigma^2) to the unit row ``row``"""
    noise = rng.standard_normal(512).astype(F32) * F32(sigma / np.sqrt(512.0))
    return l2norm_rows((row + noise)[None])[0]


def one(ref, n, need=1, tid=5, entry=0, slot=0, count=1):
    """one frame with one detection slot -> (query row, shots, event)"""
    q, s, e = ref.fuse([[entry]], [[need]], [[tid]], [slot], [count], np.asarray(n, F32)[None])
    return q[0], int(s[0, 0]), int(e[0, 0])


def bits(a):
    return np.asarray(a, F32).view(np.uint32)


def test_depth_one_answers_with_the_row_itself():
    rng = np.random.default_rng(1)
    ref = TrackTemplateRef(2, 3, 1, join_thr=0.4)
    person = unit(rng)[0]
    events = []
    for turn in range(6):
        n = near(rng, person, 0.5) if turn != 3 else unit(rng)[0]
        need = 0 if turn == 5 else 1
        q, shots, ev = one(ref, n, need=need)
        events.append(ev)
        assert np.array_equal(bits(q), bits(n)) or need == 0
        assert shots == 1 and ref.ttmpl[0, 0].tolist() == [1, 0, 5, 0]
        if need == 0:                                              # a carried face: its normed row IS the bank's last embedded row
            assert np.array_equal(bits(q), bits(ref.tring[0, 0, 0]))
    assert events == [STARTED, JOINED, JOINED, RESTARTED, RESTARTED, READ]


def test_two_and_three_shot_means_by_hand():
    ref = TrackTemplateRef(1, 1, 4, join_thr=0.0)
    a, b, c = np.zeros(512, F32), np.zeros(512, F32), np.zeros(512, F32)
    a[0] = 1
    b[0], b[1] = F32(0.6), F32(0.8)
    c[0], c[2] = F32(0.8), F32(0.6)
    q, shots, ev = one(ref, a)
    assert (ev, shots) == (STARTED, 1) and np.array_equal(bits(q), bits(a))
    q, shots, ev = one(ref, b)
    assert (ev, shots) == (JOINED, 2) and ref.cos[0, 0] == F32(0.6)
    m = np.zeros(512, F32)
    m[0], m[1] = (F32(1) + F32(0.6)) / F32(2), F32(0.8) / F32(2)
    nrm = np.sqrt(m[0] * m[0] + m[1] * m[1], dtype=F32)
    want = np.zeros(512, F32)
    want[0], want[1] = m[0] / nrm, m[1] / nrm
    assert np.array_equal(bits(q), bits(want))
    q, shots, ev = one(ref, c)
    assert (ev, shots) == (JOINED, 3)
    m = np.zeros(512, F32)
    m[0], m[1], m[2] = ((F32(1) + F32(0.6)) + F32(0.8)) / F32(3), F32(0.8) / F32(3), F32(0.6) / F32(3)
    nrm = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2], dtype=F32)
    want = np.zeros(512, F32)
    want[:3] = m[:3] / nrm
    assert np.array_equal(bits(q), bits(want)) and np.array_equal(bits(ref.tmean[0, 0]), bits(want))
    assert ref.ttmpl[0, 0].tolist() == [3, 3, 5, 0]


def test_a_wrapped_ring_is_summed_oldest_first():
    """K = 3, five shots: after the wrap the sum starts at ``head``, and the ring's own order would give other bits"""
    rng = np.random.default_rng(3)
    ref = TrackTemplateRef(1, 2, 3, join_thr=-1.0)
    person = unit(rng)[0]
    rows = [near(rng, person, 0.8) for _ in range(5)]
    got = [one(ref, r, entry=1) for r in rows]
    assert [g[2] for g in got] == [STARTED, JOINED, JOINED, JOINED, JOINED] and [g[1] for g in got] == [1, 2, 3, 3, 3]
    assert ref.ttmpl[0, 1].tolist() == [3, 2, 5, 0] and ref.trace["wrapped"] == 2
    for turn, want_rows in ((3, (1, 2, 3)), (4, (2, 3, 4))):
        want = l2norm_rows(mean_rows(np.stack([rows[k] for k in want_rows]))[None])[0]
        assert np.array_equal(bits(got[turn][0]), bits(want)), turn
    # the ring's own order (3, 4, 2 after five shots) gives other bits: the test can tell the orders apart
    other = l2norm_rows(mean_rows(np.stack([rows[k] for k in (3, 4, 2)]))[None])[0]
    assert not np.array_equal(bits(other), bits(got[4][0]))
    assert np.array_equal(bits(ref.tring[0, 1]), bits(np.stack([rows[3], rows[4], rows[2]])))
    assert not ref.ttmpl[0, 0].any() and not ref.tring[0, 0].any()


def test_a_join_exactly_at_the_threshold_and_one_bit_above_it():
    rng = np.random.default_rng(4)
    person = unit(rng)[0]
    a, b = near(rng, person, 1.0), near(rng, person, 1.0)
    c = row_dot_wave8(b[None], a[None])[0, 0]
    assert 0.3 < c < 0.7
    ref = TrackTemplateRef(1, 1, 4, join_thr=float(c))
    assert one(ref, a)[2] == STARTED and one(ref, b)[2] == JOINED and ref.cos[0, 0] == c
    above = TrackTemplateRef(1, 1, 4, join_thr=float(np.nextafter(c, F32(1))))
    assert one(above, a)[2] == STARTED
    q, shots, ev = one(above, b)
    assert (ev, shots) == (RESTARTED, 1) and np.array_equal(bits(q), bits(b))


def test_a_nan_row_restarts_and_is_returned_as_it_is():
    rng = np.random.default_rng(5)
    ref = TrackTemplateRef(1, 1, 4, join_thr=-1.0)
    person = unit(rng)[0]
    assert one(ref, person)[2] == STARTED and one(ref, near(rng, person, 0.3))[2] == JOINED
    bad = near(rng, person, 0.3)
    bad[77] = np.float32(np.nan)
    q, shots, ev = one(ref, bad)
    assert (ev, shots) == (RESTARTED, 1) and np.array_equal(bits(q), bits(bad)) and ref.trace["nan_restart"] == 1
    q, shots, ev = one(ref, person)                                   # the template is the NaN row: the next shot restarts too
    assert (ev, shots) == (RESTARTED, 1) and np.array_equal(bits(q), bits(person))
    assert one(ref, near(rng, person, 0.3))[2] == JOINED


def test_a_stale_id_is_ignored():
    rng = np.random.default_rng(6)
    ref = TrackTemplateRef(2, 2, 4, join_thr=-1.0)
    a, b = unit(rng, 2)
    assert one(ref, a, tid=5, slot=1)[2] == STARTED and one(ref, a, tid=5, slot=1)[1] == 2
    q, shots, ev = one(ref, b, need=0, tid=6, slot=1)                 # carried under another id: the held template is not this track's
    assert (ev, shots) == (NONE, 0) and np.array_equal(bits(q), bits(b)) and ref.ttmpl[1, 0].tolist() == [2, 2, 5, 0]
    q, shots, ev = one(ref, b, need=1, tid=6, slot=1)                 # embedded under another id: a new template, never a join
    assert (ev, shots) == (STARTED, 1) and np.array_equal(bits(q), bits(b)) and ref.ttmpl[1, 0].tolist() == [1, 1, 6, 0]
    assert ref.trace["stale_id"] == 2
    q, shots, ev = one(ref, a, need=0, tid=6, slot=1)
    assert (ev, shots) == (READ, 1) and np.array_equal(bits(q), bits(b))
    # untracked, stateless and past the count: the row itself, nothing moves
    before = [x.copy() for x in (ref.tring, ref.ttmpl, ref.tmean)]
    for kw in (dict(entry=-1), dict(entry=2), dict(slot=2), dict(slot=-1), dict(count=0)):
        q, shots, ev = one(ref, a, tid=6, **kw)
        assert (ev, shots) == (NONE, 0) and np.array_equal(bits(q), bits(a)), kw
    for x, y in zip(before, (ref.tring, ref.ttmpl, ref.tmean)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_the_planted_sequence():
    """unit rows, K = 4, per-shot noise sigma = 1.0 (single-shot cosine to the person's row about 0.7), another person's row on
    turn 8: every same-person turn after the first JOINS except the return turn 9, which RESTARTS as the foreign turn does; the
    foreign shot comes back as its own bits; and on every JOINED turn the template is nearer the person's row than the shot."""
    rng = np.random.default_rng(20)
    person, foreign = unit(rng, 2)
    ref = TrackTemplateRef(1, 1, 4, join_thr=0.4)
    want = {0: STARTED, 8: RESTARTED, 9: RESTARTED}
    fused = []
    for turn in range(14):
        n = foreign if turn == 8 else near(rng, person, 1.0)
        q, shots, ev = one(ref, n)
        assert ev == want.get(turn, JOINED), (turn, ev, float(ref.cos[0, 0]))
        single, both = float(n @ person), float(q @ person)
        if turn == 8:
            assert np.array_equal(bits(q), bits(foreign)) and shots == 1
        if ev == JOINED:
            assert both > single, (turn, single, both)
            fused.append(both)
        else:
            assert np.array_equal(bits(q), bits(n))
    assert fused[0] > 0.75 and fused[2] > 0.85 and ref.trace["wrapped"]
