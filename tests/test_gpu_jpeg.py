"""csrc/jpeg_encode.hip against its definition, tests/helpers/jpeg_ref.py: ``==`` on bytes, no tolerance - the arithmetic is
integer.  Sizes below, at and across the 16 x 16 MCU, one to nine MCU rows, qualities at both branches of the scaling rule; noise,
ramps, flat and checkerboard pictures; a ragged table at odd byte offsets; guard bytes behind the stream and the workspace; a
seeded fuzz; a row budget just too small for one frame; table entries no encoding exists for."""
import numpy as np
import pytest
import torch

from facerecognition_infrenceengine_amd import _lib, jpeg
from facerecognition_infrenceengine_amd.letterbox import frame_table
from tests.helpers import jpeg_cases, jpeg_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64


def _consts(quality):
    enc = jpeg.JpegEncoder(quality)
    return enc, enc._consts_on(torch.device(DEV))


def _run(lib, quality, shapes, launch, row_budget=None, capacity=None):
    """Calls one of the two entries with a stream and a workspace that end in 0xA5 guard bytes.  ``launch(max_h, max_w, tail)``
    makes the call.  Returns (files - one ``bytes`` per frame -, offsets, status, True when every guard byte is what it was)."""
    n = len(shapes)
    enc, (head, codes, qt) = _consts(quality)
    h, w = max(s[0] for s in shapes), max(s[1] for s in shapes)
    budget = row_budget or jpeg.default_row_budget(w)
    if capacity is None:
        capacity = sum(enc.frame_bound(fh, fw, budget) for fh, fw in shapes)
    ws_bytes = int(lib.fr_jpeg_workspace(n, h, w, budget))
    assert ws_bytes >= n * ((h + 15) // 16) * (budget + 4)
    ws = torch.full((ws_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.full((capacity + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    offsets = torch.full((n + 2,), -7, dtype=torch.int64, device=DEV)
    status = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
    launch(h, w, (_lib.ptr(head), jpeg.HEADER_BYTES, _lib.ptr(codes), _lib.ptr(qt), budget, _lib.ptr(out), capacity,
                  _lib.ptr(offsets), _lib.ptr(status), _lib.ptr(ws), ws_bytes, _lib.stream_ptr()))
    torch.cuda.synchronize()
    off, st, host = offsets.cpu().numpy(), status.cpu().numpy(), out.cpu().numpy()
    assert off[0] == 0 and (np.diff(off[:n + 1]) >= 0).all() and off[n] <= capacity
    intact = bool((host[off[n]:] == 0xA5).all()) and bool((ws[ws_bytes:] == 0xA5).all()) and off[n + 1] == -7 and st[n] == -7
    return [host[off[f]:off[f + 1]].tobytes() for f in range(n)], off[:n + 1], st[:n], intact


def encode_dense(lib, frames, quality, **kw):
    d = torch.from_numpy(np.ascontiguousarray(frames)).to(DEV)
    n, H, W, _ = frames.shape
    return _run(lib, quality, [(H, W)] * n, lambda h, w, tail: lib.fr_jpeg_encode_u8(_lib.ptr(d), n, H, W, *tail), **kw)


def encode_table(lib, frames, quality, first=1, guard=5, spoil=None, **kw):
    """fr_jpeg_encode_refs_u8 on frames packed into one arena, frame i behind ``guard + i`` guard bytes and the first at byte
    ``first``; ``spoil(refs)`` may edit the table.  The arena must come back as it went in."""
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
    if spoil is not None:
        refs = (_lib.FrameRef * len(frames)).from_buffer(tab)
        spoil(refs)
    table = torch.from_numpy(tab).to(DEV)
    shapes = [fr.shape[:2] for fr in frames]
    res = _run(lib, quality, shapes, lambda h, w, tail: lib.fr_jpeg_encode_refs_u8(_lib.ptr(table), len(frames), h, w, *tail), **kw)
    assert np.array_equal(arena.cpu().numpy(), host)
    return res


@pytest.mark.parametrize("hw,quality", jpeg_cases.CASES, ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else "q%d" % v)
def test_dense_batches_of_three_are_the_definitions_bytes(lib, hw, quality):
    H, W = hw
    for kinds in (jpeg_cases.CONTENTS[:3], jpeg_cases.CONTENTS[3:]):
        frames = np.stack([jpeg_cases.picture(k, H, W) for k in kinds])
        files, off, st, intact = encode_dense(lib, frames, quality)
        want = [jpeg_cases.reference(k, H, W, quality)[0] for k in kinds]
        assert list(st) == [0, 0, 0] and intact
        assert list(off) == list(np.cumsum([0] + [len(b) for b in want]))
        for k, got, ref in zip(kinds, files, want):
            assert got == ref, k


def test_a_table_of_frames_of_different_sizes_at_odd_offsets(lib):
    sizes = [(37, 51), (1, 1), (144, 176), (17, 300), (16, 16)]
    kinds = ["noise", "noise", "ramp", "noise", "pixels"]
    frames = [jpeg_cases.picture(k, h, w) for k, (h, w) in zip(kinds, sizes)]
    files, off, st, intact = encode_table(lib, frames, 75)
    assert list(st) == [0] * 5 and intact
    for k, (h, w), got in zip(kinds, sizes, files):
        assert got == jpeg_cases.reference(k, h, w, 75)[0], (k, h, w)
    assert list(off) == list(np.cumsum([0] + [len(b) for b in files]))


def test_seeded_fuzz_of_random_sizes(lib):
    rng = np.random.default_rng(20261021)
    for _ in range(4):
        quality = int(rng.integers(1, 96))
        frames = []
        for _ in range(5):
            h, w = (int(v) for v in rng.integers(1, 201, 2))
            pic = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            if rng.integers(2):                                   # a smooth picture under a little noise
                y, x = np.mgrid[0:h, 0:w]
                pic = ((np.stack([x * 2 + y, x + y * 3, 255 - x - y], axis=-1) & 255) + pic % 8).clip(0, 255).astype(np.uint8)
            frames.append(pic)
        files, off, st, intact = encode_table(lib, frames, quality, first=3, guard=7)
        assert list(st) == [0] * 5 and intact
        for pic, got in zip(frames, files):
            assert got == jpeg_ref.encode(pic, quality), (pic.shape, quality)


def test_no_frames_touch_nothing(lib):
    enc, (head, codes, qt) = _consts(80)
    out = torch.full((256,), 0xA5, dtype=torch.uint8, device=DEV)
    offsets = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    for call in (lib.fr_jpeg_encode_u8, lib.fr_jpeg_encode_refs_u8):
        assert call(None, 0, 16, 16, _lib.ptr(head), jpeg.HEADER_BYTES, _lib.ptr(codes), _lib.ptr(qt), 768, _lib.ptr(out), 256,
                    _lib.ptr(offsets), None, None, 0, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and offsets.tolist() == [-7, -7]
    assert enc.encode(torch.empty((0, 8, 8, 3), dtype=torch.uint8, device=DEV)) == []


def _noise_batch():
    """three noise frames of 40 x 56, the one whose largest coded row is the longest in the middle"""
    rng = np.random.default_rng(77)
    pics = [rng.integers(0, 256, (40, 56, 3), dtype=np.uint8) for _ in range(3)]
    stats = [jpeg_ref.new_stats() for _ in pics]
    refs = [jpeg_ref.encode(p, 95, s) for p, s in zip(pics, stats)]
    order = sorted(range(3), key=lambda i: max(stats[i]["row_bytes"]))
    order = [order[0], order[2], order[1]]
    rows = [max(stats[i]["row_bytes"]) for i in order]
    assert rows[1] > rows[0] and rows[1] > rows[2]
    return np.stack([pics[i] for i in order]), [refs[i] for i in order], rows


def test_a_row_past_its_budget_flags_its_frame_and_no_other(lib):
    """A bounds check: the budget is one byte short of frame 1's largest row, every store of the row kernel is bounded by it."""
    frames, refs, rows = _noise_batch()
    files, off, st, intact = encode_dense(lib, frames, 95)
    assert files == refs and list(st) == [0, 0, 0] and intact
    files, off, st, intact = encode_dense(lib, frames, 95, row_budget=rows[1] - 1)
    assert list(st) == [jpeg.OK, jpeg.OVERFLOW, jpeg.OK] and intact
    assert files == [refs[0], b"", refs[2]]
    assert list(off) == [0, len(refs[0]), len(refs[0]), len(refs[0]) + len(refs[2])]
    # with exactly the bytes the row needs it fits
    files, off, st, intact = encode_dense(lib, frames, 95, row_budget=rows[1])
    assert files == refs and list(st) == [0, 0, 0] and intact


def test_a_frame_past_the_streams_capacity_is_flagged(lib):
    frames, refs, _ = _noise_batch()
    files, off, st, intact = encode_dense(lib, frames, 95, capacity=len(refs[0]) + len(refs[1]) - 1)
    assert list(st) == [jpeg.OK, jpeg.OVERFLOW, jpeg.OVERFLOW] and intact
    assert files == [refs[0], b"", b""]
    files, off, st, intact = encode_dense(lib, frames, 95, capacity=sum(len(b) for b in refs))
    assert files == refs and list(st) == [0, 0, 0] and intact


def test_table_entries_without_a_picture_are_flagged_and_skipped(lib):
    sizes = [(40, 56), (16, 16), (37, 51), (8, 8), (17, 300)]
    frames = [jpeg_cases.picture("noise", h, w) for h, w in sizes]

    def spoil(refs):
        refs[1].data = None
        refs[2].H = 0
        refs[3].W = -4

    files, off, st, intact = encode_table(lib, frames, 75, spoil=spoil)
    assert list(st) == [jpeg.OK, jpeg.SKIPPED, jpeg.SKIPPED, jpeg.SKIPPED, jpeg.OK] and intact
    assert files[1:4] == [b"", b"", b""]
    assert files[0] == jpeg_cases.reference("noise", 40, 56, 75)[0] and files[4] == jpeg_cases.reference("noise", 17, 300, 75)[0]


def test_the_encoder_object_on_a_batch_and_on_a_table(lib, caplog):
    enc = jpeg.JpegEncoder(quality=75)
    frames = np.stack([jpeg_cases.picture(k, 37, 51) for k in ("noise", "ramp")])
    d = torch.from_numpy(frames).to(DEV)
    assert enc.encode(d) == [jpeg_cases.reference(k, 37, 51, 75)[0] for k in ("noise", "ramp")]
    assert enc.encode(d) == [jpeg_cases.reference(k, 37, 51, 75)[0] for k in ("noise", "ramp")]      # the cached buffers
    pics = [jpeg_cases.picture("noise", 17, 300), jpeg_cases.picture("blocks", 40, 56)]
    arena = torch.from_numpy(np.concatenate([p.reshape(-1) for p in pics])).to(DEV)
    tab, _ = frame_table([arena.data_ptr(), arena.data_ptr() + pics[0].nbytes], [p.shape[:2] for p in pics])
    table = torch.from_numpy(tab).to(DEV)
    got = enc.encode((arena, table), shapes=[p.shape[:2] for p in pics])
    assert got == [jpeg_cases.reference("noise", 17, 300, 75)[0], jpeg_cases.reference("blocks", 40, 56, 75)[0]]
    with pytest.raises(ValueError, match="shapes"):
        enc.encode((arena, table))
    with pytest.raises(ValueError, match="contiguous"):
        enc.encode(d[:, :, ::2])
    tight = jpeg.JpegEncoder(quality=95, row_budget=64)
    with caplog.at_level("WARNING"):
        assert tight.encode(d) == [None, None]
    assert "not encoded" in caplog.text
