"""csrc/face_chips.hip against its definition, tests/helpers/chip_ref.py: ``array_equal``, no tolerance - the arithmetic is integer.
Frames of 64 x 97 and 33 x 50 (odd widths: rows are not dword-aligned) of noise; every size's sides below, at and above S, in both
regimes; squares inside the frame, cut by each side, by a corner, wholly outside and at +-2^20; the largest sum the definition
allows; records no picture is defined for; guard bytes behind ``out`` and around the frames of a table; a seeded fuzz."""
import numpy as np
import pytest
import torch

from facerecognition_infrenceengine_amd import _lib
from facerecognition_infrenceengine_amd.letterbox import frame_table
from tests.helpers import chip_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = (7, 200, 255)
SIZES = (16, 48, 112, 256)
LIMIT = 1 << 20


def bgr_word(c):
    return int(c[0]) | (int(c[1]) << 8) | (int(c[2]) << 16)


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def noise(seed, n, H, W):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def cut_dense(lib, frames, records, S, fill=FILL, guard=64):
    """fr_face_chips_u8 on a uint8 [n,H,W,3] batch -> (uint8 [F,S,S,3], True when the guard bytes behind out are what they were)"""
    records = np.ascontiguousarray(records, np.int32).reshape(-1, 4)
    d, r = _dev(frames, records)
    F = len(records)
    out = torch.full((F * S * S * 3 + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    n, H, W, _ = frames.shape
    lib.fr_face_chips_u8(_lib.ptr(d), n, H, W, _lib.ptr(r), F, S, bgr_word(fill), _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    return host[:F * S * S * 3].reshape(F, S, S, 3), bool((host[F * S * S * 3:] == 0xA5).all())


def pack_arena(frames, first=1, guard=5):
    """frames packed into one host arena, frame i behind ``guard + i`` guard bytes, the first at byte ``first`` -> (host, offsets)"""
    offs, at = [], first
    for i, fr in enumerate(frames):
        at += guard + i
        offs.append(at)
        at += fr.nbytes
    host = np.full(at + guard, 0xA5, np.uint8)
    for o, fr in zip(offs, frames):
        host[o:o + fr.nbytes] = fr.reshape(-1)
    return host, offs


def cut_table(lib, frames, records, S, fill=FILL, spoil=None, guard=64):
    """fr_face_chips_refs_u8 on frames packed at odd offsets between guard bytes -> (chips, guards behind out intact, arena as
    it was).  ``spoil(rows)``: edits the table's int32 [n, 8] rows before the upload."""
    records = np.ascontiguousarray(records, np.int32).reshape(-1, 4)
    host, offs = pack_arena(frames)
    arena = torch.from_numpy(host).to(DEV)
    tab, _ = frame_table([arena.data_ptr() + o for o in offs], [fr.shape[:2] for fr in frames])
    if spoil is not None:
        spoil(tab.view(np.int32).reshape(len(frames), 8))
    table, r = _dev(tab, records)
    F = len(records)
    out = torch.full((F * S * S * 3 + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    lib.fr_face_chips_refs_u8(_lib.ptr(table), len(frames), _lib.ptr(r), F, S, bgr_word(fill), _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    return (got[:F * S * S * 3].reshape(F, S, S, 3), bool((got[F * S * S * 3:] == 0xA5).all()),
            bool(np.array_equal(arena.cpu().numpy(), host)))


def sides(S):
    return [L for L in (1, 7, S - 1, S, S + 1, 2 * S, 3 * S + 7) if 1 <= L <= chip_ref.MAX_SIDE]


def placements(H, W, L):
    """squares of side L: inside (or as far inside as L allows), cut by the left, right, top and bottom side, by a corner, wholly
    outside on two sides, and at +-2^20"""
    mid = (max((W - L) // 2, 0), max((H - L) // 2, 0))
    return [mid, (2, 3), (-(L // 2) - 1, mid[1]), (W - L // 2 - 1, mid[1]), (mid[0], -(L // 2) - 1), (mid[0], H - L // 2 - 1),
            (W - (L + 1) // 2, H - (L + 1) // 2), (-L // 3 - 1, -L // 2 - 1), (-L - 3, 5), (4, H + 2), (W, 0), (0, -L),
            (LIMIT, 3), (-LIMIT, -LIMIT), (3, LIMIT)]


def assert_chips(got, frames, records, S, fill=FILL):
    for k, rec in enumerate(np.asarray(records).reshape(-1, 4)):
        want = chip_ref.chip(frames, rec, S, fill)
        assert np.array_equal(got[k], want), (S, rec.tolist(), int((got[k] != want).sum()))


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("hw", [(64, 97), (33, 50)], ids=lambda s: "%dx%d" % s)
def test_every_side_and_placement_matches_the_definition(lib, hw, S):
    H, W = hw
    frames = noise(100 * H + S, 2, H, W)
    records = [(k % 2, x0, y0, L) for k, L in enumerate(sides(S)) for x0, y0 in placements(H, W, L)]
    got, intact = cut_dense(lib, frames, records, S)
    assert intact
    assert_chips(got, list(frames), records, S)
    fill = np.asarray(FILL, np.uint8)
    for k, (_, x0, y0, L) in enumerate(records):
        box_outside = x0 >= W or y0 >= H or x0 + L <= 0 or y0 + L <= 0
        if L >= S and box_outside:                            # wholly outside: all fill (the bilinear taps reach one pixel further)
            assert (got[k] == fill).all(), records[k]


def test_identity_at_side_equal_size(lib):
    frames = noise(3, 1, 64, 97)
    for S in (16, 48):
        got, _ = cut_dense(lib, frames, [(0, 11, 9, S)], S)
        assert np.array_equal(got[0], frames[0, 9:9 + S, 11:11 + S])


@pytest.mark.parametrize("S", [16, 256])
def test_the_largest_sum_fits_an_unsigned_accumulator(lib, S):
    """one 4096 x 4096 frame of 255s, the whole frame as the square: 255 * 2^24 + 2^23 per byte, past a signed 32-bit sum"""
    frames = torch.full((1, 4096, 4096, 3), 255, dtype=torch.uint8, device=DEV)
    r, = _dev(np.array([[0, 0, 0, 4096]], np.int32))
    out = torch.zeros((1, S, S, 3), dtype=torch.uint8, device=DEV)
    lib.fr_face_chips_u8(_lib.ptr(frames), 1, 4096, 4096, _lib.ptr(r), 1, S, 0, _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool((out == 255).all())


def test_a_4096_square_over_a_small_frame(lib):
    frames = noise(5, 1, 64, 97)
    records = [(0, -2000, -2011, 4096), (0, 0, 0, 4096), (0, 97 - 4096, 64 - 4096, 4096), (0, -4000, -10, 4096)]
    for S in (16, 112, 256):
        got, intact = cut_dense(lib, frames, records, S)
        assert intact
        assert_chips(got, list(frames), records, S)
        assert not (got[1] == np.asarray(FILL, np.uint8)).all()           # the frame shows in it


def test_records_no_picture_is_defined_for_come_back_as_fill(lib):
    frames = noise(6, 3, 33, 50)
    bad = [(-1, 0, 0, 20), (3, 0, 0, 20), (2 ** 31 - 1, 0, 0, 20), (-2 ** 31, 0, 0, 20), (0, 0, 0, 0), (0, 0, 0, -5),
           (0, 0, 0, 4097), (0, 0, 0, 2 ** 31 - 1), (1, LIMIT + 1, 0, 20), (1, 0, -LIMIT - 1, 20), (1, 2 ** 31 - 1, -2 ** 31, 20),
           (2, 5, 5, 20)]
    for S in (16, 112):
        got, intact = cut_dense(lib, frames, bad, S)
        assert intact
        assert (got[:-1] == np.asarray(FILL, np.uint8)).all()
        assert_chips(got, list(frames), bad, S)                               # the last record is a real one, behind the bad ones
        assert not (got[-1] == np.asarray(FILL, np.uint8)).all()
    # no frames at all: every record names none
    r, = _dev(np.array([[0, 0, 0, 20]], np.int32))
    out = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=DEV)
    lib.fr_face_chips_u8(None, 0, 33, 50, _lib.ptr(r), 1, 16, bgr_word(FILL), _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == np.asarray(FILL, np.uint8)).all()


@pytest.mark.parametrize("F", [1, 37])
def test_chip_counts_and_the_guard_bytes_behind_out(lib, F):
    H, W = 64, 97
    frames = noise(7 + F, 2, H, W)
    rng = np.random.default_rng(70 + F)
    records = [(int(rng.integers(0, 2)), int(rng.integers(-20, W)), int(rng.integers(-20, H)), int(rng.integers(1, 150)))
               for _ in range(F)]
    for S in (16, 48):
        got, intact = cut_dense(lib, frames, records, S, fill=(0, 0, 0))
        assert intact
        assert_chips(got, list(frames), records, S, fill=(0, 0, 0))


def test_a_table_of_differing_sizes_at_odd_offsets(lib):
    shapes = [(64, 97), (33, 50), (1, 1), (16, 64)]
    frames = [noise(80 + i, 1, h, w)[0] for i, (h, w) in enumerate(shapes)]
    records = []
    for f, (h, w) in enumerate(shapes):
        for L in (1, 7, 15, 16, 17, 40, 111, 112, 113, 300):
            records += [(f, 0, 0, L), (f, -3, -2, L), (f, w - L + 2, h - L + 1, L), (f, (w - L) // 2, (h - L) // 2, L)]
    for S in (16, 112):
        got, out_intact, arena_intact = cut_table(lib, frames, records, S)
        assert out_intact and arena_intact
        assert_chips(got, frames, records, S)
    # the uniform entry gives the bytes of the table entry
    mine = [r for r in records if r[0] == 1]
    dense, _ = cut_dense(lib, frames[1][None], [(0,) + r[1:] for r in mine], 16)
    table, _, _ = cut_table(lib, frames, mine, 16)
    assert np.array_equal(dense, table)


def test_null_and_non_positive_table_entries_give_fill(lib):
    shapes = [(33, 50), (33, 50), (64, 97), (33, 50), (33, 50)]
    frames = [noise(90 + i, 1, h, w)[0] for i, (h, w) in enumerate(shapes)]

    def spoil(rows):
        rows[0, 2] = 0                                        # H = 0
        rows[1, 0:2] = 0                                      # a null pointer
        rows[3, 3] = -50                                      # W < 0
    records = [(f, 2, 3, L) for f in range(5) for L in (9, 30, 200)] + [(5, 0, 0, 30), (-1, 0, 0, 30)]
    seen = [None, None, frames[2], None, frames[4]]
    for S in (16, 48):
        got, out_intact, arena_intact = cut_table(lib, frames, records, S, spoil=spoil)
        assert out_intact and arena_intact
        assert_chips(got, seen, records, S)
        fill = np.asarray(FILL, np.uint8)
        assert all((got[k] == fill).all() == (rec[0] not in (2, 4)) for k, rec in enumerate(records))


@pytest.mark.parametrize("S", [16, 112])
def test_seeded_fuzz_is_exact_and_repeats(lib, S):
    rng = np.random.default_rng(2026 + S)
    shapes = [(64, 97), (33, 50), (64, 97)]
    frames = [noise(int(rng.integers(1 << 30)), 1, h, w)[0] for h, w in shapes]
    records = []
    for _ in range(200):
        L = int(rng.choice([rng.integers(1, 20), rng.integers(1, 3 * S + 8), rng.integers(1, 600), S + rng.integers(-1, 2)]))
        records.append((int(rng.integers(-1, 4)), int(rng.integers(-L - 4, 101)), int(rng.integers(-L - 4, 68)), max(L, 0)))
    got, out_intact, arena_intact = cut_table(lib, frames, records, S)
    assert out_intact and arena_intact
    assert_chips(got, frames, records, S)
    again, _, _ = cut_table(lib, frames, records, S)
    assert np.array_equal(got, again)
    # frames 0 and 2 have one size: the uniform entry over them gives the same chips
    pick = [r for r in records if r[0] in (0, 2)]
    dense, intact = cut_dense(lib, np.stack([frames[0], frames[2]]), [(r[0] // 2,) + r[1:] for r in pick], S)
    assert intact
    assert_chips(dense, frames, pick, S)
