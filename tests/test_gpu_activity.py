"""The activity gate on the MI355X: both entry points (csrc/frame_activity.hip) against the NumPy definition of
tests/helpers/activity_ref.py, byte for byte - the cell means, the verdicts and every state array, with guard bytes round all of
them - and ``ActivityGate`` above them."""
import ctypes

import numpy as np
import pytest
import torch

from tests.helpers import activity_ref as ar

pytestmark = pytest.mark.gpu

GUARD, PATTERN = 64, 0xA5
SHAPES = [(16, 16), (32, 48), (40, 72), (56, 100), (17, 31)]


class Dev:
    """The arrays of one call on the device, each between two runs of GUARD pattern bytes; ``lead`` shifts the byte arrays off
    every alignment.  The state starts as zeros (what ``ActivityGate`` allocates), cur / changed / active as the pattern."""

    def __init__(self, S, C, N, lead=0):
        self.S, self.C, self.N = S, C, N
        self.sizes = {"grid": S * C, "geom": S * 8, "idle": S * 4, "cur": N * C, "changed": N * 4, "active": N * 4}
        self.buf, self.off = {}, {}
        for name, nbytes in self.sizes.items():
            shift = lead if name in ("grid", "cur") else 0
            b = torch.full((GUARD + shift + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
            if name in ("grid", "geom", "idle"):
                b[GUARD + shift:GUARD + shift + nbytes] = 0
            self.buf[name], self.off[name] = b, GUARD + shift

    def ptr(self, name):
        return ctypes.c_void_p(self.buf[name].data_ptr() + self.off[name])

    def state_args(self):
        return (self.ptr("grid"), self.ptr("geom"), self.ptr("idle"), self.C, self.ptr("cur"), self.ptr("changed"),
                self.ptr("active"))

    def host(self, name):
        raw = self.buf[name].cpu().numpy()
        o, n = self.off[name], self.sizes[name]
        assert (raw[:o] == PATTERN).all() and (raw[o + n:] == PATTERN).all(), f"guard bytes of {name} were written"
        body = raw[o:o + n]
        return body.view(np.int32) if name in ("geom", "idle", "changed", "active") else body

    def load(self, ref):
        """take the reference's state"""
        for name, a in (("grid", ref.grid), ("geom", ref.geom), ("idle", ref.idle)):
            o = self.off[name]
            self.buf[name][o:o + self.sizes[name]] = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def _uniform(lib, dev, frames, slots, rule):
    from facerecognition_infrenceengine_amd import _lib
    N, H, W, _ = frames.shape
    f = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    s = torch.tensor(list(slots), dtype=torch.int32).cuda()
    lib.fr_frame_activity_u8(_lib.ptr(f), N, H, W, _lib.ptr(s), dev.S, *dev.state_args(), *rule, _lib.stream_ptr())
    torch.cuda.synchronize()


def _check(dev, ref, frames, slots, rows=None):
    """Judge ``frames`` with the reference (moving its state) and compare every array of ``dev``; ``rows``: the rows of cur /
    changed / active the frames occupy (default: 0 ..)."""
    changed, active, cur = ref.judge(frames, slots)
    rows = range(len(frames)) if rows is None else rows
    got_cur = dev.host("cur").reshape(dev.N, dev.C)
    for r, c in zip(rows, cur):
        k = 0 if c is None else len(c)
        if k:
            assert np.array_equal(got_cur[r, :k], c), f"cell means of frame {r}"
        assert (got_cur[r, k:] == PATTERN).all(), f"cur row {r} past the frame's cells"
    assert np.array_equal(dev.host("changed")[list(rows)], changed)
    assert np.array_equal(dev.host("active")[list(rows)], active)
    assert np.array_equal(dev.host("grid").reshape(ref.S, ref.C), ref.grid)
    assert np.array_equal(dev.host("geom").reshape(ref.S, 2), ref.geom)
    assert np.array_equal(dev.host("idle"), ref.idle)
    return changed, active


# ------------------------------------------------------------------------------------------------------ 1. the means
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("N", [1, 3, 5])
def test_cell_means_of_random_frames(lib, H, W, N):
    """(56, 100): 3 W = 300 is no multiple of 16, so the rows start at every 4-byte phase; (17, 31): one cell and remainders
    on both sides; the byte arrays start at odd addresses (lead = 3)."""
    rng = np.random.default_rng([H, W, N])
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    S, C = 7, 24 + 5                                                       # (56, 100) has 18 cells; an odd row stride
    dev, ref = Dev(S, C, N, lead=3), ar.GateRef(S, C)
    slots = rng.permutation(S)[:N]
    _uniform(lib, dev, frames, slots, (4, 2, 0))
    changed, active = _check(dev, ref, frames, slots)
    assert (changed == -1).all() and (active == 1).all()
    _uniform(lib, dev, frames, slots, (4, 2, 0))                           # the same frames again: counted, and unchanged
    changed, active = _check(dev, ref, frames, slots)
    assert (changed == 0).all() and (active == 0).all()


@pytest.mark.parametrize("value", [0, 255])
def test_cell_means_of_flat_frames(lib, value):
    frames = np.full((2, 40, 72, 3), value, np.uint8)
    dev, ref = Dev(2, 8, 2), ar.GateRef(2, 8)
    _uniform(lib, dev, frames, [1, 0], (4, 2, 0))
    _check(dev, ref, frames, [1, 0])
    assert (dev.host("cur") == value).all()


# ------------------------------------------------------------------------------------------------------ 2. sequences
def _grey(values, h=40, w=72):
    f = np.zeros((h, w, 3), np.uint8)
    for i, row in enumerate(values):
        for j, v in enumerate(row):
            f[16 * i:16 * i + 16, 16 * j:16 * j + 16] = v
    f[32:], f[:, 64:] = 7, 9                                               # remainder rows and columns: ignored
    return f


def test_six_turns_on_four_slots(lib):
    """thr = 2, min_cells = 2, max_idle = 3 at 40 x 72 (2 x 4 cells).  Camera a: identical frames (inactive until max_idle lets
    the fifth through).  Camera b: one cell by thr, by thr + 1 (one cell: below min_cells), then a second cell (active).
    Camera c: a ramp of +1 per turn on two cells (inactive, inactive, active, and again from the refreshed grid).  Camera d:
    absent from turns 2 and 4 - its state bytes stay.  The batch order is shuffled every turn."""
    S, C, rule = 4, 8, (2, 2, 3)
    base = [[100, 100, 100, 100], [100, 100, 100, 100]]

    def cam_b(t):
        v = [list(r) for r in base]
        if t >= 1:
            v[0][1] = 102                                                  # by thr
        if t >= 2:
            v[0][1] = 103                                                  # by thr + 1
        if t >= 3:
            v[1][3] = 97                                                   # the second cell
        return v

    def cam_c(t):
        v = [list(r) for r in base]
        v[0][0] = v[1][2] = 100 + t
        return v
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, (40, 72, 3), dtype=np.uint8)
    ref = ar.GateRef(S, C, *rule)
    dev = Dev(S, C, 4)
    slot_of = {"a": 2, "b": 0, "c": 3, "d": 1}
    seen = {k: [] for k in slot_of}
    for t in range(6):
        cams = {"a": _grey(base), "b": _grey(cam_b(t)), "c": _grey(cam_c(t))}
        if t not in (2, 4):
            cams["d"] = noise if t < 5 else noise // 2
        order = [k for k in rng.permutation(sorted(cams))]
        frames = np.stack([cams[k] for k in order])
        n = len(order)
        d_state = (ref.grid[1].copy(), ref.geom[1].copy(), ref.idle[1].copy())
        _uniform(lib, dev, frames, [slot_of[k] for k in order], rule)
        changed, active = _check(dev, ref, frames, [slot_of[k] for k in order], rows=range(n))
        if "d" not in cams:
            assert all(np.array_equal(a, b) for a, b in zip(d_state, (ref.grid[1], ref.geom[1], ref.idle[1])))
        for k, c, a in zip(order, changed, active):
            seen[k].append((int(c), int(a)))
    assert seen["a"] == [(-1, 1), (0, 0), (0, 0), (0, 0), (0, 1), (0, 0)]
    assert seen["b"] == [(-1, 1), (0, 0), (1, 0), (2, 1), (0, 0), (0, 0)]
    assert seen["c"] == [(-1, 1), (0, 0), (0, 0), (2, 1), (0, 0), (0, 0)]
    assert seen["d"] == [(-1, 1), (0, 0), (0, 0), (8, 1)]


def test_ramp_on_one_cell_adds_up_against_the_last_processed_frame(lib):
    """+1 per turn on one cell, thr = 2, min_cells = 1: inactive, inactive, active - and again from the refreshed grid."""
    S, C, rule = 2, 8, (2, 1, 0)
    dev, ref = Dev(S, C, 1), ar.GateRef(S, C, *rule)
    seen = []
    for t in range(7):
        frame = _grey([[100 + t, 40, 40, 40], [40, 40, 40, 40]])[None]
        _uniform(lib, dev, frame, [1], rule)
        changed, active = _check(dev, ref, frame, [1])
        seen.append((int(changed[0]), int(active[0])))
    assert seen == [(-1, 1), (0, 0), (0, 0), (1, 1), (0, 0), (0, 0), (1, 1)]
    assert ref.grid[1, 0] == 106 and ref.idle.tolist() == [0, 0]


def test_two_gates_on_one_device_do_not_see_each_other():
    from facerecognition_infrenceengine_amd import ActivityGate
    rng = np.random.default_rng(11)
    f = torch.from_numpy(rng.integers(0, 256, (2, 40, 72, 3), dtype=np.uint8)).cuda()
    g1 = ActivityGate(slots=4, max_hw=(48, 80))
    g2 = ActivityGate(slots=4, max_hw=(48, 80), thr=0, min_cells=1)
    assert g1.cells == 16 and g1.grid.shape == (4, 16)
    a, c = g1.judge(f, ["x", "y"])
    assert a.tolist() == [True, True] and c.tolist() == [-1, -1] and a.dtype == np.bool_ and c.dtype == np.int32
    a, c = g1.judge(f, ["x", "y"])
    assert a.tolist() == [False, False] and c.tolist() == [0, 0]
    a, c = g2.judge(f, ["x", "y"])                                        # the other gate has seen nothing yet
    assert a.tolist() == [True, True] and c.tolist() == [-1, -1]
    assert g1.idle.cpu().tolist()[:2] == [1, 1] and g2.idle.cpu().tolist()[:2] == [0, 0]
    assert np.array_equal(g1.grid.cpu().numpy()[0, :8], ar.cell_means(f[0].cpu().numpy()))


def test_gate_host_layer_slots_cache_and_errors():
    from facerecognition_infrenceengine_amd import ActivityGate
    g = ActivityGate(slots=3, max_hw=(48, 80), max_idle=0)
    f = torch.zeros((2, 40, 72, 3), dtype=torch.uint8, device="cuda")
    act, chg = g.judge_device(f, ("a", "b"))
    assert act.is_cuda and chg.is_cuda and act.dtype == torch.int32 and act.tolist() == [1, 1] and chg.tolist() == [-1, -1]
    first = g._slot_arrays[("a", "b")]
    g.judge_device(f, ["a", "b"])
    assert g._slot_arrays[("a", "b")] is first                            # uploaded once
    assert g.judge(f, ["b", "a"])[0].tolist() == [False, False]           # the ids, not the positions, own the state
    with pytest.raises(ValueError, match="repeated"):
        g.judge(f, ["a", "a"])
    with pytest.raises(ValueError, match="one camera id per frame"):
        g.judge(f, ["a"])
    assert g.judge(f[:1], ["c"])[0].tolist() == [True] and len(g) == 3
    with pytest.raises(ValueError, match="slots"):
        g.judge(f[:1], ["d"])
    s = g.slot_of("b")
    g.forget("b")
    g.forget("nobody")                                                     # ignored
    assert g.slot_of("b") is None and len(g) == 2 and g.geom.cpu().tolist()[s] == [0, 0]
    act, chg = g.judge(f, ["d", "a"])                                      # the freed slot, as new: active
    assert g.slot_of("d") == s and act.tolist() == [True, False] and chg.tolist() == [-1, 0]
    bigger = torch.zeros((1, 64, 96, 3), dtype=torch.uint8, device="cuda")  # 24 cells > 16: not judged, always active
    assert [g.judge(bigger, ["a"])[1].tolist() for _ in range(2)] == [[-1], [-1]]
    assert g.judge(f[:1], ["a"])[0].tolist() == [False]                    # and a's state did not move


def test_gate_keeps_the_slot_arrays_of_the_last_64_tuples():
    from facerecognition_infrenceengine_amd import ActivityGate
    g = ActivityGate(slots=70, max_hw=(16, 16))
    f = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device="cuda")
    for i in range(70):
        g.judge_device(f, [i])
    assert len(g._slot_arrays) == 64 and (0,) not in g._slot_arrays and (69,) in g._slot_arrays
    assert g.judge(f, [0])[0].tolist() == [False]                          # uploaded again; camera 0 kept its slot and state
    assert sorted(g.idle.cpu().tolist()) == [0] * 69 + [1]


# ------------------------------------------------------------------------------------------------------ 3. the table form
def test_table_form_matches_the_uniform_form_frame_by_frame(lib):
    """Five frames of five sizes in one arena, the second at an odd byte offset; slots 0 .. 3 and, for the fourth frame, one
    outside the state.  Turn 1: all new.  Turn 2: the same bytes again.  (8, 64) holds no cell; it and the out-of-range slot
    are active with changed = -1 both turns, and write no state."""
    from facerecognition_infrenceengine_amd import _lib
    from facerecognition_infrenceengine_amd.letterbox import frame_table
    shapes = [(24, 40), (56, 100), (16, 16), (33, 47), (8, 64)]
    slots = [2, 0, 3, 9, 1]
    S, C, rule = 4, 18 + 3, (4, 2, 0)
    rng = np.random.default_rng(21)
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    offs, o = [], 0
    for i, (h, w) in enumerate(shapes):
        o = (o + 15) // 16 * 16 + (5 if i == 1 else 0)
        offs.append(o)
        o += h * w * 3
    arena = torch.full((GUARD + o + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    for f, at in zip(frames, offs):
        arena[GUARD + at:GUARD + at + f.size] = torch.from_numpy(f.reshape(-1)).cuda()
    assert (arena.data_ptr() + GUARD + offs[1]) % 2 == 1
    tab, _ = frame_table([arena.data_ptr() + GUARD + at for at in offs], shapes)
    table = torch.from_numpy(tab).cuda()
    slot = torch.tensor(slots, dtype=torch.int32).cuda()
    dev, ref = Dev(S, C, 5, lead=1), ar.GateRef(S, C, *rule)
    for turn in range(2):
        lib.fr_frame_activity_refs_u8(_lib.ptr(table), 5, _lib.ptr(slot), S, *dev.state_args(), *rule, _lib.stream_ptr())
        torch.cuda.synchronize()
        changed, active = _check(dev, ref, frames, slots)
        want = [-1] * 5 if turn == 0 else [0, 0, 0, -1, -1]
        assert changed.tolist() == want and active.tolist() == [int(c < 0) for c in want]
    assert ref.geom.tolist() == [[56, 100], [0, 0], [24, 40], [16, 16]]   # slot 1 ((8, 64)) never took a grid
    # each frame alone through the uniform entry: the same cell means and verdicts
    for i, (f, s) in enumerate(zip(frames, slots)):
        one, ref1 = Dev(S, C, 1), ar.GateRef(S, C, *rule)
        _uniform(lib, one, f[None], [s], rule)
        _check(one, ref1, [f], [s])
        k = (shapes[i][0] // 16) * (shapes[i][1] // 16) if shapes[i][0] >= 16 else 0
        assert np.array_equal(one.host("cur")[:k], dev.host("cur").reshape(5, C)[i, :k])


# ------------------------------------------------------------------------------------------------------ 4. bounds, launch shape
def test_rows_of_unnamed_slots_and_every_guard_byte_stay(lib):
    """Slots 1 and 4 of 6 are named; the rows of the others hold a pattern of their own and keep it, whether the named frames
    are active (turn 1) or not (turn 2)."""
    rng = np.random.default_rng(31)
    frames = rng.integers(0, 256, (2, 56, 100, 3), dtype=np.uint8)
    S, C = 6, 18
    dev, ref = Dev(S, C, 2, lead=7), ar.GateRef(S, C)
    ref.grid[:] = rng.integers(0, 256, (S, C), dtype=np.uint8)
    ref.geom[:] = [[56, 100], [0, 0], [56, 100], [40, 72], [56, 100], [16, 16]]
    ref.idle[:] = [3, 0, 9, 1, 5, 2]
    dev.load(ref)
    for _ in range(2):
        _uniform(lib, dev, frames, [1, 4], (4, 2, 0))
        _check(dev, ref, frames, [1, 4])                                   # every row of every array, and the guards


def test_one_launch_of_five_equals_five_launches_of_one(lib):
    from facerecognition_infrenceengine_amd import _lib
    rng = np.random.default_rng(41)
    S, C, rule = 5, 18, (3, 1, 2)
    turns = [rng.integers(0, 256, (5, 56, 100, 3), dtype=np.uint8)]
    nxt = turns[0].copy()
    nxt[1, :16, :16] = 0                                                   # frame 1: one cell moves; the others repeat
    nxt[3] = nxt[3] // 2
    turns += [nxt, nxt, nxt]                                               # then idle runs to max_idle
    a, b, ref = Dev(S, C, 5), Dev(S, C, 5), ar.GateRef(S, C, *rule)
    slots = [4, 2, 0, 1, 3]
    for frames in turns:
        _uniform(lib, a, frames, slots, rule)
        _check(a, ref, frames, slots)
        f = torch.from_numpy(frames).cuda()
        sl = torch.tensor(slots, dtype=torch.int32).cuda()
        for i in range(5):                                                 # frame i alone, its outputs at row i
            fi, si = f[i:i + 1].contiguous(), sl[i:i + 1].contiguous()
            at = lambda name, stride: ctypes.c_void_p(b.ptr(name).value + i * stride)
            lib.fr_frame_activity_u8(_lib.ptr(fi), 1, 56, 100, _lib.ptr(si), S, b.ptr("grid"), b.ptr("geom"), b.ptr("idle"), C,
                                     at("cur", C), at("changed", 4), at("active", 4), *rule, _lib.stream_ptr())
        torch.cuda.synchronize()
        for name in ("cur", "changed", "active", "grid", "geom", "idle"):
            assert np.array_equal(a.host(name), b.host(name)), name
