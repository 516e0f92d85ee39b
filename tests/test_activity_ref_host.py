"""The activity gate's NumPy definition (tests/helpers/activity_ref.py) against hand-computed values: the luma weights, the cell
means, the remainder rows and columns, and the rule - strictness of ``thr``, ``min_cells``, first frames, size changes,
``max_idle``, and the grid that moves only when a frame is processed (no GPU)."""
import numpy as np

from tests.helpers import activity_ref as ar


def _flat(h, w, value):
    return np.full((h, w, 3), value, np.uint8)


def _cells(h, w, values):
    """a frame whose cell (i, j) is the constant values[i][j] (grey), remainder rows / columns 0"""
    f = np.zeros((h, w, 3), np.uint8)
    for i, row in enumerate(values):
        for j, v in enumerate(row):
            f[16 * i:16 * i + 16, 16 * j:16 * j + 16] = v
    return f


def test_weights_sum_to_256_and_constant_frames_keep_their_value():
    assert sum(ar.WEIGHTS) == 256 and ar.CELL == 16
    for c in (0, 1, 127, 255):
        m = ar.cell_means(_flat(32, 48, c))
        assert m.dtype == np.uint8 and m.shape == (6,) and (m == c).all()
    # the largest per-pixel term and the largest cell sum the specification names
    assert 255 * 256 + 128 == 65408 and 255 * 256 == 65280


def test_one_cell_by_hand():
    f = np.zeros((16, 16, 3), np.uint8)
    f[..., 0], f[..., 1], f[..., 2] = 10, 20, 30              # B, G, R: (290 + 3000 + 2310 + 128) >> 8 = 5728 >> 8 = 22
    assert int(ar.luma(f)[0, 0]) == 22 and ar.cell_means(f).tolist() == [22]
    f[0, :8] = (255, 255, 255)                                # 8 pixels of 255, 248 of 22: 2040 + 5456 = 7496; + 128 >> 8 = 29
    assert ar.cell_means(f).tolist() == [(8 * 255 + 248 * 22 + 128) >> 8] == [29]
    g = np.zeros((16, 16, 3), np.uint8)
    g[..., 0] = 255                                           # pure blue: (29 * 255 + 128) >> 8 = 7523 >> 8 = 29
    g[..., 1] = 0
    assert ar.cell_means(g).tolist() == [29]
    g[..., 0], g[..., 1] = 0, 255                             # pure green: (38250 + 128) >> 8 = 149
    assert ar.cell_means(g).tolist() == [149]
    g[..., 1], g[..., 2] = 0, 255                             # pure red: (19635 + 128) >> 8 = 77
    assert ar.cell_means(g).tolist() == [77]


def test_remainder_rows_and_columns_belong_to_no_cell():
    rng = np.random.default_rng(1)
    f = rng.integers(0, 256, (40, 72, 3), dtype=np.uint8)     # gh = 2 (8 rows over), gw = 4 (8 columns over)
    base = ar.cell_means(f)
    assert base.shape == (8,)
    g = f.copy()
    g[32:] = 255 - g[32:]
    g[:, 64:] = 255 - g[:, 64:]
    assert np.array_equal(ar.cell_means(g), base)
    assert np.array_equal(ar.cell_means(f[:32, :64]), base)
    assert ar.cell_means(np.zeros((15, 200, 3), np.uint8)).shape == (0,)
    # row-major: cell (1, 2) of a 2 x 4 grid is entry 6
    h = _cells(40, 72, [[0, 0, 0, 0], [0, 0, 200, 0]])
    assert ar.cell_means(h).tolist() == [0, 0, 0, 0, 0, 0, 200, 0]


def test_thr_is_strict_and_min_cells_counts_cells():
    gate = ar.GateRef(slots=2, cells=8, thr=4, min_cells=2)
    base = [[100, 100, 100, 100], [100, 100, 100, 100]]
    assert gate.judge_one(_cells(32, 64, base), 0)[:2] == (-1, 1)
    by_thr = [[104, 100, 100, 100], [100, 96, 100, 100]]      # two cells off by exactly thr: unchanged
    assert gate.judge_one(_cells(32, 64, by_thr), 0)[:2] == (0, 0)
    one = [[105, 100, 100, 100], [100, 96, 100, 100]]         # one cell by thr + 1: counted, below min_cells
    assert gate.judge_one(_cells(32, 64, one), 0)[:2] == (1, 0)
    two = [[105, 100, 100, 100], [100, 95, 100, 100]]         # two cells: min_cells reached
    assert gate.judge_one(_cells(32, 64, two), 0)[:2] == (2, 1)
    assert gate.idle.tolist() == [0, 0] and gate.grid[0].tolist() == [105, 100, 100, 100, 100, 95, 100, 100]
    assert gate.grid[1].tolist() == [0] * 8 and gate.geom.tolist() == [[32, 64], [0, 0]]


def test_first_frame_and_size_change_are_active():
    gate = ar.GateRef(slots=3, cells=12)
    f = _flat(32, 48, 50)
    assert gate.judge_one(f, 1)[:2] == (-1, 1) and gate.geom[1].tolist() == [32, 48]
    assert gate.judge_one(f, 1)[:2] == (0, 0) and gate.idle[1] == 1
    assert gate.judge_one(_flat(48, 32, 50), 1)[:2] == (-1, 1)            # the same cell count, another size
    assert gate.geom[1].tolist() == [48, 32] and gate.idle[1] == 0
    # a frame without a whole cell, with more cells than a grid row, or for a slot outside the state: active, nothing moves
    before = (gate.grid.copy(), gate.geom.copy(), gate.idle.copy())
    assert gate.judge_one(_flat(8, 64, 50), 1)[:2] == (-1, 1)
    assert gate.judge_one(_flat(64, 64, 50), 1)[:2] == (-1, 1)            # 16 cells > 12
    assert gate.judge_one(f, 3)[:2] == (-1, 1) and gate.judge_one(f, -1)[:2] == (-1, 1)
    assert all(np.array_equal(a, b) for a, b in zip(before, (gate.grid, gate.geom, gate.idle)))


def test_max_idle_lets_the_fourth_identical_frame_through():
    gate = ar.GateRef(slots=1, cells=6, max_idle=3)
    f = _flat(32, 48, 9)
    assert gate.judge_one(f, 0)[:2] == (-1, 1)
    for turn in (1, 2, 3):
        assert gate.judge_one(f, 0)[:2] == (0, 0) and gate.idle[0] == turn
    assert gate.judge_one(f, 0)[:2] == (0, 1) and gate.idle[0] == 0       # active though nothing changed
    assert gate.judge_one(f, 0)[:2] == (0, 0) and gate.idle[0] == 1
    off = ar.GateRef(slots=1, cells=6, max_idle=0)                        # 0: never
    off.judge_one(f, 0)
    assert all(off.judge_one(f, 0)[1] == 0 for _ in range(8)) and off.idle[0] == 8


def test_grid_moves_only_when_a_frame_is_processed():
    """+1 per turn on one cell, thr = 2, min_cells = 1: the comparison is against the last PROCESSED frame, so the drift adds up
    to inactive, inactive, active - and starts again from the refreshed grid."""
    gate = ar.GateRef(slots=1, cells=4, thr=2, min_cells=1)
    ramp = lambda v: _cells(32, 32, [[v, 40], [40, 40]])
    assert gate.judge_one(ramp(100), 0)[:2] == (-1, 1)
    verdicts = [gate.judge_one(ramp(100 + t), 0)[:2] for t in range(1, 7)]
    assert verdicts == [(0, 0), (0, 0), (1, 1), (0, 0), (0, 0), (1, 1)]
    assert gate.grid[0].tolist() == [106, 40, 40, 40]


def test_batches_judge_frame_by_frame_and_refuse_a_repeated_slot():
    import pytest
    gate = ar.GateRef(slots=4, cells=4)
    frames = [_flat(32, 32, v) for v in (10, 20, 30)]
    changed, active, cur = gate.judge(frames, [2, 0, 3])
    assert changed.tolist() == [-1, -1, -1] and active.tolist() == [1, 1, 1] and changed.dtype == active.dtype == np.int32
    assert [c.tolist() for c in cur] == [[10] * 4, [20] * 4, [30] * 4]
    assert gate.grid[:, 0].tolist() == [20, 0, 10, 30]
    with pytest.raises(AssertionError):
        gate.judge(frames[:2], [1, 1])
