"""csrc/hud_draw.hip against its definition, tests/helpers/hud_ref.py: ``array_equal``, no tolerance - the arithmetic is integer.
Frame sizes below, at and across the 16 x 64 tile; counts of 0, partial (garbage records behind) and full; boxes partly and
wholly outside the frame; overlapping HUDs in both orders; a probe font; a ragged table at odd byte offsets; a seeded fuzz."""
import numpy as np
import pytest
import torch

from facerecognition_infrenceengine_amd import _lib
from facerecognition_infrenceengine_amd.hud_font import FONT, probe_font
from facerecognition_infrenceengine_amd.letterbox import frame_table
from tests.helpers import hud_cases, hud_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(8, 8), (16, 64), (96, 128), (75, 133)]


def _records(counts, faces, text, font):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (counts, faces, text, np.array(FONT if font is None else font))]


def draw_dense(lib, frames, counts, faces, text, scale=1, font=None):
    """fr_hud_draw_u8 on a uint8 [n,H,W,3] batch -> the drawn batch (NumPy)"""
    d = torch.from_numpy(frames).to(DEV)
    c, f, t, fn = _records(counts, faces, text, font)
    n, H, W, _ = frames.shape
    lib.fr_hud_draw_u8(_lib.ptr(d), n, H, W, _lib.ptr(c), faces.shape[1], _lib.ptr(f), _lib.ptr(t), text.shape[3], _lib.ptr(fn),
                       scale, _lib.stream_ptr())
    torch.cuda.synchronize()
    return d.cpu().numpy()


def draw_table(lib, frames, counts, faces, text, scale=1, font=None, first=1, guard=5):
    """fr_hud_draw_refs_u8 on frames packed back to back into one arena, frame i behind ``guard + i`` guard bytes and the first
    at byte ``first`` -> (the drawn frames, True when every guard byte is what it was)"""
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
    table = torch.from_numpy(tab).to(DEV)
    c, f, t, fn = _records(counts, faces, text, font)
    lib.fr_hud_draw_refs_u8(_lib.ptr(table), len(frames), _lib.ptr(c), faces.shape[1], _lib.ptr(f), _lib.ptr(t), text.shape[3],
                            _lib.ptr(fn), scale, _lib.stream_ptr())
    torch.cuda.synchronize()
    out = arena.cpu().numpy()
    inside = np.zeros(len(out), bool)
    for o, fr in zip(offs, frames):
        inside[o:o + fr.nbytes] = True
    return [out[o:o + fr.nbytes].reshape(fr.shape) for o, fr in zip(offs, frames)], bool((out[~inside] == 0xA5).all())


@pytest.mark.parametrize("cap", [1, 16])
@pytest.mark.parametrize("scale", [1, 2, 3])
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: "%dx%d" % s)
def test_counts_zero_partial_and_full(lib, hw, scale, cap):
    """Four frames: count 0 (the frame must come back as it went in), a partial count with garbage records behind it - for
    cap 1 a count beyond cap, which is clamped -, a full count, and a negative count."""
    H, W = hw
    rng = np.random.default_rng(1000 * H + 10 * scale + cap)
    frames = hud_cases.noise(rng, 4, H, W)
    made = [hud_cases.random_faces(rng, cap, -20, max(H, W) + 20) for _ in range(4)]
    counts = [0, cap // 2 if cap > 1 else 7, cap, -3]
    cnt, faces, text = hud_cases.pack(made, cap, seed=int(rng.integers(1 << 30)), counts=counts)
    for f, c in enumerate(counts):                       # behind a frame's count: garbage
        faces[f, max(0, min(c, cap)):] = rng.integers(-2 ** 31, 2 ** 31 - 1, faces[f, max(0, min(c, cap)):].shape)
    want = hud_cases.expected(frames, cnt, faces, text, scale)
    got = draw_dense(lib, frames.copy(), cnt, faces, text, scale)
    assert np.array_equal(got, want)
    assert np.array_equal(got[0], frames[0]) and np.array_equal(got[3], frames[3])
    assert not np.array_equal(got[2], frames[2])


def _one_face_frames(H, W, boxes, **kw):
    return [[hud_cases.face(b, rh=5, dh=3, lines=(b"ab",), **kw)] for b in boxes]


@pytest.mark.parametrize("scale", [1, 2])
def test_boxes_partly_and_wholly_outside_zero_size_and_whole_frame(lib, scale):
    H, W = 75, 133
    boxes = [(-15, 20, 30, 50), (110, 20, 150, 50), (40, -12, 80, 25), (40, 55, 80, 90),               # partly outside, each side
             (-90, 20, -50, 50), (200, 20, 240, 50), (40, -80, 80, -45), (40, 140, 80, 170),            # wholly outside
             (-400, -400, -300, -300), (1 << 22, 5, (1 << 22) + 9, 30),                                 # nowhere near; beyond the clamp
             (60, 30, 60, 30), (0, 0, W - 1, H - 1), (-5, -5, W + 4, H + 4)]                            # zero size; the frame; around it
    rng = np.random.default_rng(4)
    frames = hud_cases.noise(rng, len(boxes), H, W)
    cnt, faces, text = hud_cases.pack(_one_face_frames(H, W, boxes, colour=(10, 200, 250)), cap=2, seed=8)
    want = hud_cases.expected(frames, cnt, faces, text, scale)
    got = draw_dense(lib, frames.copy(), cnt, faces, text, scale)
    assert np.array_equal(got, want)
    # px is clamped into the frame and py to its top, so even a box far outside leaves its panel - except below the frame,
    # where the flipped panel (y1 - ph - 10 s) is still outside at scale 1: that frame comes back untouched
    for k in range(len(boxes)):
        assert np.array_equal(got[k], frames[k]) == (k == 7 and scale == 1), k
    # a box wholly outside shows its panel alone: outside the panel's rectangle the frame is as it was
    px, py, pw, ph = hud_ref.panel_rect(-400, -400, -300, -300, [2], H, W, scale)
    rest = np.ones((H, W), bool)
    rest[py:py + ph + 1, px:px + pw + 1] = False
    assert np.array_equal(got[8][rest], frames[8][rest]) and rest.any()


def test_overlapping_huds_are_folded_in_slot_order(lib):
    H, W = 96, 128
    a = hud_cases.face((20, 10, 70, 50), (0, 255, 0), 20, 30, (b"Name: A", b"Type: Visitor", b"Score: 0.71"))
    b = hud_cases.face((35, 20, 85, 56), (0, 0, 255), 10, 0, (b"Unknown Person", b"Detection: 0.55"))
    frames = hud_cases.noise(np.random.default_rng(5), 2, H, W)
    frames[1] = frames[0]
    cnt, faces, text = hud_cases.pack([[a, b], [b, a]], cap=3, seed=2)
    want = hud_cases.expected(frames, cnt, faces, text)
    got = draw_dense(lib, frames.copy(), cnt, faces, text)
    assert np.array_equal(got, want)
    assert not np.array_equal(got[0], got[1])            # the order of the fold shows


def test_probe_font_pins_bit_and_row_order(lib):
    """One lit pixel per glyph, in row k % 7 and column (k // 7) % 5 of glyph k: a transposed table, a reversed bit order or a
    wrong row stride moves it."""
    H, W = 96, 128
    rows = [bytes(range(0x20 + 24 * i, min(0x20 + 24 * (i + 1), 0x7F))) for i in range(4)]
    frames = hud_cases.noise(np.random.default_rng(6), 3, H, W)
    per_frame = [[hud_cases.face((10, 12, 60, 40), (255, 0, 255), 9, 9, rows)],
                 [hud_cases.face((10, 12, 60, 40), (255, 0, 255), 9, 9, [bytes([0x00, 0x1F, 0x7F, 0xFF, 0x41])])],    # -> '?' x 4, 'A'
                 [hud_cases.face((40, 30, 50, 40), (255, 0, 255), 9, 9, rows[:2])]]
    cnt, faces, text = hud_cases.pack(per_frame, cap=1, max_chars=24, seed=7)
    for font, scale in ((probe_font(), 1), (probe_font(), 2), (FONT, 1)):
        want = hud_cases.expected(frames, cnt, faces, text, scale, font)
        got = draw_dense(lib, frames.copy(), cnt, faces, text, scale, font)
        assert np.array_equal(got, want), scale
    assert not np.array_equal(hud_cases.expected(frames, cnt, faces, text, 1, probe_font()), want)


def test_ragged_table_at_odd_offsets_leaves_the_guards_alone(lib):
    rng = np.random.default_rng(11)
    shapes = [(33, 47), (75, 133), (16, 64)]
    frames = [hud_cases.noise(rng, 1, h, w)[0] for h, w in shapes]
    made = [hud_cases.random_faces(rng, 3, -20, 120) for _ in shapes]
    cnt, faces, text = hud_cases.pack(made, cap=4, seed=12)
    want = [hud_ref.draw_records(fr, cnt[i], faces[i], text[i], 2) for i, fr in enumerate(frames)]
    got, guards_intact = draw_table(lib, frames, cnt, faces, text, 2)
    assert guards_intact
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    one = draw_dense(lib, frames[1][None].copy(), cnt[1:2], faces[1:2], text[1:2], 2)
    assert np.array_equal(one[0], got[1])                # the dense entry gives the bytes of the table entry


def test_dense_and_table_entries_agree_and_bad_entries_are_skipped(lib):
    rng = np.random.default_rng(13)
    frames = hud_cases.noise(rng, 3, 40, 72)
    made = [hud_cases.random_faces(rng, 2, -10, 80) for _ in range(3)]
    cnt, faces, text = hud_cases.pack(made, cap=2, seed=14)
    dense = draw_dense(lib, frames.copy(), cnt, faces, text)
    table, guards_intact = draw_table(lib, list(frames), cnt, faces, text, first=3, guard=1)
    assert guards_intact and all(np.array_equal(a, b) for a, b in zip(dense, table))
    # entries 0 and 2 made unusable on the device: their frames stay, entry 1 is drawn
    arena = torch.from_numpy(frames.copy()).to(DEV)
    tab, _ = frame_table([arena.data_ptr() + i * frames[0].nbytes for i in range(3)], [(40, 72)] * 3)
    rows = tab.view(np.int32).reshape(3, 8)
    rows[0, 2] = 0                                       # H = 0
    rows[2, 0:2] = 0                                     # a null pointer
    c, f, t, fn = _records(cnt, faces, text, None)
    dev_tab = torch.from_numpy(tab).to(DEV)
    lib.fr_hud_draw_refs_u8(_lib.ptr(dev_tab), 3, _lib.ptr(c), 2, _lib.ptr(f), _lib.ptr(t), 40, _lib.ptr(fn), 1, _lib.stream_ptr())
    torch.cuda.synchronize()
    out = arena.cpu().numpy()
    assert np.array_equal(out[0], frames[0]) and np.array_equal(out[2], frames[2]) and np.array_equal(out[1], dense[1])


def test_seeded_fuzz_is_exact_and_repeats(lib):
    rng = np.random.default_rng(2024)
    frames = hud_cases.noise(rng, 64, 64, 96)
    made = [hud_cases.random_faces(rng, int(rng.integers(0, 9)), -40, 140) for _ in range(64)]
    cnt, faces, text = hud_cases.pack(made, cap=8, seed=99)
    want = hud_cases.expected(frames, cnt, faces, text)
    got = draw_dense(lib, frames.copy(), cnt, faces, text)
    assert np.array_equal(got, want)
    assert np.array_equal(draw_dense(lib, frames.copy(), cnt, faces, text), got)
    untouched = int((want == frames).all(axis=3).sum())
    assert 0 < untouched < frames.shape[0] * 64 * 96      # the case has pixels no layer reaches, and pixels that are drawn
