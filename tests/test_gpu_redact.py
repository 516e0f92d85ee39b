"""csrc/redact.hip against its definition, tests/helpers/redact_ref.py: ``array_equal``, no tolerance - the arithmetic is integer.
Pictures below, at and across a tile; blocks that divide 64 and blocks that do not; both modes; regions of every awkward shape;
overlapping regions that share cells across a tile edge, on noise, so that a read of bytes already written would show; counts of
0, partial (garbage behind) and cap = 64; rounding ties; a ragged table at odd byte offsets between guard bytes; bad table
entries; a seeded fuzz."""
import numpy as np
import pytest
import torch

from facerecognition_infrenceengine_amd import _lib
from facerecognition_infrenceengine_amd.letterbox import frame_table
from tests.helpers import redact_cases, redact_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COLOUR = (7, 200, 255)


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def redact_dense(lib, frames, counts, regions, block, mode=0, colour=(0, 0, 0)):
    """fr_redact_u8 on a uint8 [n,H,W,3] batch -> the redacted batch (NumPy)"""
    d, c, r = _dev(frames, counts, regions)
    n, H, W, _ = frames.shape
    lib.fr_redact_u8(_lib.ptr(d), n, H, W, _lib.ptr(c), regions.shape[1], _lib.ptr(r), block, mode, redact_cases.bgr_word(colour),
                     _lib.stream_ptr())
    torch.cuda.synchronize()
    return d.cpu().numpy()


def redact_table(lib, frames, counts, regions, block, mode=0, colour=(0, 0, 0), first=1, guard=5):
    """fr_redact_refs_u8 on frames packed into one arena, frame i behind ``guard + i`` guard bytes and the first at byte
    ``first`` -> (the redacted frames, True when every guard byte is what it was)"""
    offs, at = [], first
    for i, fr in enumerate(frames):
        at += guard + i
        offs.append(at)
        at += fr.nbytes
    host = np.full(at + guard, 0xA5, np.uint8)
    for o, fr in zip(offs, frames):
        host[o:o + fr.nbytes] = fr.reshape(-1)
    arena = torch.from_numpy(host).to(DEV)
    tab, _ = frame_table([arena.data_ptr() + o for o in offs], [fr.shape[:2] for fr in frames])
    table, c, r = _dev(tab, counts, regions)
    lib.fr_redact_refs_u8(_lib.ptr(table), len(frames), _lib.ptr(c), regions.shape[1], _lib.ptr(r), block, mode,
                          redact_cases.bgr_word(colour), _lib.stream_ptr())
    torch.cuda.synchronize()
    out = arena.cpu().numpy()
    inside = np.zeros(len(out), bool)
    for o, fr in zip(offs, frames):
        inside[o:o + fr.nbytes] = True
    return [out[o:o + fr.nbytes].reshape(fr.shape) for o, fr in zip(offs, frames)], bool((out[~inside] == 0xA5).all())


@pytest.mark.parametrize("block", redact_cases.BLOCKS)
@pytest.mark.parametrize("hw", redact_cases.SIZES, ids=lambda s: "%dx%d" % s)
def test_region_shapes_on_every_size_block_and_mode(lib, hw, block):
    """one frame per region shape (1 x 1, cutting cells on four sides, the whole picture, partly and wholly outside, +-2^20,
    overlapping, listed twice), both modes"""
    H, W = hw
    per_frame = redact_cases.shapes_of_regions(H, W)
    rng = np.random.default_rng(1000 * H + block)
    frames = redact_cases.noise(rng, len(per_frame), H, W)
    cnt, regions = redact_cases.pack(per_frame, cap=3, seed=H + block)
    for mode in (0, 1):
        want = redact_cases.expected(frames, cnt, regions, block, mode, COLOUR)
        got = redact_dense(lib, frames.copy(), cnt, regions, block, mode, COLOUR)
        for k in range(len(per_frame)):
            assert np.array_equal(got[k], want[k]), (mode, k, per_frame[k])
    for k in (8, 9, 10, 11):                                 # wholly outside: the frame as it went in
        assert np.array_equal(got[k], frames[k]), k
    assert (got[2] == COLOUR).all() and (got[5] == COLOUR).all()     # the whole picture, filled


@pytest.mark.parametrize("block", [3, 16])
def test_overlapping_regions_sharing_cells_across_tile_edges_on_noise(lib, block):
    """Two regions that overlap around the tile edges (x = 63 | 64 at block 16, 63 at block 3; y at every multiple of the block)
    and cut the cells they share: a kernel that worked region by region, or that read a neighbour's stored bytes, would average
    bytes already averaged.  Both orders and the chained application are told apart."""
    H, W = 70, 133
    rng = np.random.default_rng(21 + block)
    frames = redact_cases.noise(rng, 1, H, W).repeat(3, axis=0)
    a, b = (50, 9, 70, 40), (58, 27, 130, 61)
    cnt, regions = redact_cases.pack([[a, b], [b, a], [a, b, a]], cap=4, seed=5)
    want = redact_cases.expected(frames, cnt, regions, block)
    got = redact_dense(lib, frames.copy(), cnt, regions, block)
    for k in range(3):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])           # order and repeats do not matter
    chained = redact_ref.redact(redact_ref.redact(frames[0], [a], block), [b], block)
    assert not np.array_equal(got[0], chained)               # the case can tell a read of written bytes
    # a second launch on the first one's output is NOT idempotent on cut cells in general, but on whole cells it is
    inner = (64, 32, 111, 47)                                # whole cells at block 16, cut ones at block 3
    once = redact_dense(lib, frames[:1].copy(), np.array([1], np.int32), np.array([[inner]], np.int32), 16)
    twice = redact_dense(lib, once.copy(), np.array([1], np.int32), np.array([[inner]], np.int32), 16)
    assert np.array_equal(once, twice) and not np.array_equal(once[0], frames[0])


def test_counts_zero_partial_full_cap_64_and_out_of_range(lib):
    H, W, cap = 37, 51, 64
    rng = np.random.default_rng(31)
    frames = redact_cases.noise(rng, 5, H, W)
    made = [redact_cases.random_regions(rng, cap, H, W, spread=10) for _ in range(5)]
    made = [[(x1, y1, min(x2, x1 + 9), min(y2, y1 + 7)) for x1, y1, x2, y2 in m] for m in made]       # small: most pixels stay
    counts = [0, 5, cap, -3, cap + 9]                        # the last two are clamped to 0 and cap
    cnt, regions = redact_cases.pack(made, cap, seed=32, counts=counts)
    for f, c in enumerate(counts):                           # behind a frame's count: garbage
        k = max(0, min(c, cap))
        regions[f, k:] = rng.integers(-2 ** 31, 2 ** 31 - 1, regions[f, k:].shape)
    for block, mode in ((5, 0), (16, 0), (2, 1)):
        want = redact_cases.expected(frames, cnt, regions, block, mode, COLOUR)
        got = redact_dense(lib, frames.copy(), cnt, regions, block, mode, COLOUR)
        for k in range(5):
            assert np.array_equal(got[k], want[k]), (block, mode, k)
        assert np.array_equal(got[0], frames[0]) and np.array_equal(got[3], frames[3])
        assert not np.array_equal(got[1], frames[1]) and not np.array_equal(got[2], frames[2])
        assert (got[2] == frames[2]).all(axis=2).any()       # and pixels of the full frame that no region holds


def test_rounding_ties_with_even_and_odd_n(lib):
    """Cells whose sum sits at the tie: block 2 (n = 4, S = 2 -> 1 and S = 1 -> 0), cut cells of n = 2 and n = 1 at the
    picture's edge (S = 1, n = 2 -> 1), block 3 (n = 9: S = 4 -> 0, S = 5 -> 1) and the largest cell, 4096 pixels of 255."""
    f = np.zeros((1, 3, 3, 3), np.uint8)
    f[0, 0, 0] = (1, 1, 0)
    f[0, 0, 1] = (1, 0, 0)
    f[0, 0, 2] = (1, 0, 3)                                    # the cut cell (x = 2; y = 0 .. 1): n = 2
    f[0, 2, 2] = (255, 1, 0)                                  # n = 1
    whole = np.array([[(0, 0, 2, 2)]], np.int32)
    got = redact_dense(lib, f.copy(), np.array([1], np.int32), whole, 2)
    assert got[0, 0, 0].tolist() == [1, 0, 0] and got[0, 1, 2].tolist() == [1, 0, 2] and got[0, 2, 2].tolist() == [255, 1, 0]
    assert np.array_equal(got[0], redact_ref.redact(f[0], whole[0], 2))
    g = np.zeros((1, 3, 3, 3), np.uint8)
    g[0, 0, 0] = (4, 5, 13)
    got = redact_dense(lib, g.copy(), np.array([1], np.int32), whole, 3)
    assert (got[0] == (0, 1, 1)).all()
    big = np.full((1, 64, 64, 3), 255, np.uint8)
    got = redact_dense(lib, big.copy(), np.array([1], np.int32), np.array([[(0, 0, 63, 63)]], np.int32), 64)
    assert (got == 255).all()
    big[0, ::2] = 254                                         # S = 4096 * 254.5: the tie at n = 4096 goes up
    got = redact_dense(lib, big.copy(), np.array([1], np.int32), np.array([[(5, 4, 5, 4)]], np.int32), 64)
    assert got[0, 4, 5].tolist() == [255] * 3 and int((got != big).sum()) == 3        # one pixel, 254 -> 255, and no other byte
    assert np.array_equal(got[0], redact_ref.redact(big[0], [(5, 4, 5, 4)], 64))


def test_ragged_table_at_odd_offsets_leaves_the_guards_alone(lib):
    rng = np.random.default_rng(41)
    shapes = [(33, 47), (70, 133), (16, 64), (1, 1)]
    frames = [redact_cases.noise(rng, 1, h, w)[0] for h, w in shapes]
    made = [redact_cases.random_regions(rng, 3, h, w) + [(0, 0, w - 1, h - 1)] * (i == 2) for i, (h, w) in enumerate(shapes)]
    cnt, regions = redact_cases.pack(made, cap=4, seed=42)
    for block, mode in ((7, 0), (16, 0), (64, 0), (16, 1)):
        want = redact_cases.expected(frames, cnt, regions, block, mode, COLOUR)
        got, guards_intact = redact_table(lib, frames, cnt, regions, block, mode, COLOUR)
        assert guards_intact, (block, mode)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), (block, mode)
        one = redact_dense(lib, frames[1][None].copy(), cnt[1:2], regions[1:2], block, mode, COLOUR)
        assert np.array_equal(one[0], got[1])                # the dense entry gives the bytes of the table entry


def test_dense_and_table_entries_agree_and_bad_entries_are_skipped(lib):
    rng = np.random.default_rng(51)
    frames = redact_cases.noise(rng, 3, 40, 72)
    made = [redact_cases.random_regions(rng, 2, 40, 72) + [(10, 10, 30, 30)] for _ in range(3)]
    cnt, regions = redact_cases.pack(made, cap=3, seed=52)
    dense = redact_dense(lib, frames.copy(), cnt, regions, 5)
    table, guards_intact = redact_table(lib, list(frames), cnt, regions, 5, first=3, guard=1)
    assert guards_intact and all(np.array_equal(a, b) for a, b in zip(dense, table))
    # entries 0 and 2 made unusable on the device: their frames stay, entry 1 is redacted
    arena = torch.from_numpy(frames.copy()).to(DEV)
    tab, _ = frame_table([arena.data_ptr() + i * frames[0].nbytes for i in range(3)], [(40, 72)] * 3)
    rows = tab.view(np.int32).reshape(3, 8)
    rows[0, 2] = 0                                           # H = 0
    rows[2, 0:2] = 0                                         # a null pointer
    dev_tab, c, r = _dev(tab, cnt, regions)
    lib.fr_redact_refs_u8(_lib.ptr(dev_tab), 3, _lib.ptr(c), 3, _lib.ptr(r), 5, 0, 0, _lib.stream_ptr())
    torch.cuda.synchronize()
    out = arena.cpu().numpy()
    assert np.array_equal(out[0], frames[0]) and np.array_equal(out[2], frames[2]) and np.array_equal(out[1], dense[1])
    assert not np.array_equal(out[1], frames[1])


def test_seeded_fuzz_is_exact_and_repeats(lib):
    rng = np.random.default_rng(2025)
    frames = redact_cases.noise(rng, 48, 70, 133)
    made = [redact_cases.random_regions(rng, int(rng.integers(0, 9)), 70, 133, spread=40) for _ in range(48)]
    cnt, regions = redact_cases.pack(made, cap=8, seed=77)
    for block, mode in ((2, 0), (7, 0), (16, 0), (64, 0), (5, 1)):
        want = redact_cases.expected(frames, cnt, regions, block, mode, COLOUR)
        got = redact_dense(lib, frames.copy(), cnt, regions, block, mode, COLOUR)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), (block, mode)
        assert np.array_equal(redact_dense(lib, frames.copy(), cnt, regions, block, mode, COLOUR), got)
    untouched = int(sum((w == f).all(axis=2).sum() for w, f in zip(want, frames)))
    assert 0 < untouched < 48 * 70 * 133                      # the case has pixels no region holds, and pixels that are held
