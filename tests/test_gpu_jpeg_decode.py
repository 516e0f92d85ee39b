"""csrc/jpeg_decode.hip against its definition, tests/helpers/jpeg_decode_ref.py: ``==`` on bytes, no tolerance - the arithmetic
is integer.  Sizes below, at and across the MCU, widths around libjpeg's replication rule, one size of several chunks; 4:4:4 /
4:2:2 / 4:2:0 / gray; no DRI, DRI per row, DRI 3, optimised tables; files at odd byte offsets between guard bytes, guards behind
the workspace and between the destination frames; dense batches, a seeded fuzz, two table sets in one batch; and streams that
are not JPEG scans, each of which costs its frame a status word and nothing else."""
import numpy as np
import pytest
import torch

from facerecognition_infrenceengine_amd import _lib, jpeg_decode as J, jpeg_tables
from facerecognition_infrenceengine_amd.letterbox import frame_table
from tests.helpers import jpeg_decode_cases as cases, jpeg_decode_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SAMPLINGS = ("444", "422", "420", "gray")


def run_table(blobs, null=(), spoil=None):
    """fr_jpeg_decode_refs_u8 on files packed at odd byte offsets between 0xA5 guard bytes, destination frames with guard bytes
    between them, a workspace that ends in guard bytes.  ``null``: frames whose table entry has no destination; ``spoil(frames)``
    may edit the descriptors.  Returns (status, pictures - None where the header was turned away or the entry is null -, True when
    every guard byte is what it was, the destination bytes of every frame as they are on the device)."""
    lib = _lib.load()
    dec = J.JpegDecoder(DEV)
    frames, headers = dec.describe(blobs)
    n = len(blobs)
    data, spans = bytearray(b"\xa5"), []
    for f, hd in enumerate(headers):
        data += b"\xa5" * (3 + f % 2 + (len(data) + 1) % 2)                    # the scans start at odd offsets
        if hd is not None:
            frames["scan_off"][f] = len(data)
            data += bytes(blobs[f])[hd.scan:]
        spans.append(len(data))
    data += b"\xa5" * GUARD
    shapes = [(hd.H, hd.W) if hd is not None else (0, 0) for hd in headers]
    offs, at = [], 1
    for f, (h, w) in enumerate(shapes):
        at += 5 + f
        offs.append(at)
        at += h * w * 3
    arena = torch.full((at + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    tab, _ = frame_table([arena.data_ptr() + o if headers[f] is not None and f not in null else 0 for f, o in enumerate(offs)], shapes)
    if spoil is not None:
        spoil(frames)
    max_h, max_w = max(s[0] for s in shapes + [(1, 1)]), max(s[1] for s in shapes + [(1, 1)])
    segments = max([hd.segments for hd in headers if hd is not None] + [1])
    ws_bytes = int(lib.fr_jpeg_decode_workspace(n, max_h, max_w, segments))
    ws = torch.full((ws_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    status = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
    stream = torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).to(DEV)
    table = torch.from_numpy(frames.view(np.uint8).copy()).to(DEV)
    refs = torch.from_numpy(tab).to(DEV)
    qt, ht = dec._tables_on_device()
    natural = torch.from_numpy(jpeg_tables.ZIGZAG.astype(np.int32)).to(DEV)
    lib.fr_jpeg_decode_refs_u8(_lib.ptr(stream), len(data) - GUARD, _lib.ptr(table), n, max_h, max_w, segments, _lib.ptr(qt),
                               int(qt.shape[0]), _lib.ptr(ht), int(ht.shape[0]), _lib.ptr(natural), _lib.ptr(refs), _lib.ptr(status),
                               _lib.ptr(ws), ws_bytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    host, st = arena.cpu().numpy(), status.cpu().numpy()
    keep = np.ones(len(host), bool)
    raw = []
    for o, (h, w) in zip(offs, shapes):
        keep[o:o + h * w * 3] = False
        raw.append(host[o:o + h * w * 3])
    intact = bool((host[keep] == 0xA5).all()) and bool((ws[ws_bytes:] == 0xA5).all()) and st[n] == -7 and \
        bool((stream.cpu().numpy() == np.frombuffer(bytes(data), np.uint8)).all())
    pictures = [r.reshape(h, w, 3) if headers[f] is not None and f not in null else None for f, (r, (h, w)) in enumerate(zip(raw, shapes))]
    return st[:n], pictures, intact, raw


def _mixed(h, w):
    """16 files of one size: every sampling with every writer, contents and qualities going round"""
    kinds, qualities = ("noise", "ramp", "flats"), (10, 50, 75, 95, 100)
    out = []
    for i, sampling in enumerate(SAMPLINGS):
        for j, writer in enumerate(cases.WRITERS):
            out.append(cases.case(kinds[(i + j) % 3], h, w, qualities[(2 * i + j) % 5], sampling, writer))
    return out


@pytest.mark.parametrize("h,w", cases.SIZES)
def test_every_sampling_and_writer(h, w):
    files = _mixed(h, w)
    status, pictures, intact, _ = run_table([f[0] for f in files])
    assert intact
    assert (status == J.OK).all(), status
    for k, ((_, want), got) in enumerate(zip(files, pictures)):
        assert np.array_equal(got, want), (k, int(np.abs(got.astype(int) - want).max()))


def test_several_chunks():
    h, w = cases.LARGE
    files = [cases.case("noise", h, w, 100, "444"),            # 13 chunks of 8 KiB in one interval, slow to fall into step
             cases.case("noise", h, w, 90, "420"), cases.case("ramp", h, w, 75, "422", "dri_3"),
             cases.case("noise", h, w, 95, "420", "own"), cases.case("flats", h, w, 50, "gray", "optimize"),
             cases.case("noise", h, w, 85, "422", "dri_row")]
    hd = J.parse(files[0][0])
    assert hd.restart == 0 and len(files[0][0]) - hd.scan > 3 * ref.S * ref.LANES
    status, pictures, intact, _ = run_table([f[0] for f in files])
    assert intact and (status == J.OK).all(), status
    for k, ((_, want), got) in enumerate(zip(files, pictures)):
        assert np.array_equal(got, want), k


def test_dense_batches_and_two_table_sets():
    dec = J.JpegDecoder(DEV)
    for h, w in ((17, 33), (37, 51)):
        files = [cases.case("noise", h, w, 50, "420"), cases.case("flats", h, w, 95, "420", "optimize"), cases.case("ramp", h, w, 75, "444")]
        assert J.parse(files[0][0]).qtables != J.parse(files[1][0]).qtables and J.parse(files[0][0]).huffman != J.parse(files[1][0]).huffman
        frames, shapes, status = dec.decode_device([f[0] for f in files])
        assert isinstance(frames, torch.Tensor) and tuple(frames.shape) == (3, h, w, 3) and shapes == [(h, w)] * 3
        assert (status.cpu().numpy() == J.OK).all()
        assert np.array_equal(frames.cpu().numpy(), np.stack([f[1] for f in files]))
        out = torch.full((3, h, w, 3), 7, dtype=torch.uint8, device=DEV)
        got, _, status = dec.decode_device([f[0] for f in files], out=out)
        assert got is out and np.array_equal(out.cpu().numpy(), np.stack([f[1] for f in files]))
    assert len(dec._qrows) <= 6 and len(dec._hrows) <= 12        # cached by their bytes: the standard tables went up once


def test_seeded_fuzz():
    rng = np.random.default_rng(20260)
    blobs = []
    for k in range(24):
        h, w = int(rng.integers(1, 70)), int(rng.integers(1, 70))
        sampling = SAMPLINGS[int(rng.integers(4))]
        more = {}
        if rng.integers(2):
            more["restart_marker_blocks"] = int(rng.integers(1, 12))
        elif rng.integers(2):
            more["restart_marker_rows"] = int(rng.integers(1, 3))
        if rng.integers(2):
            more["optimize"] = True
        blobs.append(cases.pil_file(cases.picture(("noise", "ramp", "flats")[k % 3], h, w, seed=k), int(rng.integers(1, 101)), sampling, **more))
    dec = J.JpegDecoder(DEV)
    got = dec.decode(blobs)
    assert dec.last_fallbacks == {}
    for k, (blob, g) in enumerate(zip(blobs, got)):
        assert g is not None and np.array_equal(g, ref.decode(blob)[0]), k


def test_streams_that_are_no_scans_cost_a_status_word():
    """Ordinary bad uploads.  Every one sits between two good files of another size; its frame gets a status that is not OK and
    is not written, the neighbours come out right, every guard byte stays."""
    good, want = cases.case("noise", 37, 51, 90, "420")
    other, other_want = cases.case("ramp", 17, 33, 75, "444", "dri_3")
    scan = J.parse(good).scan
    rst = cases.pil_file(cases.picture("noise", 37, 51), 90, "420", "dri_3")
    at = rst.index(b"\xff\xd1", J.parse(rst).scan)
    rng = np.random.default_rng(5)
    bad = [good[:scan + k] for k in (1, 7, 100, 1000, len(good) - scan - 3)]           # cut inside the scan
    bad += [good[:scan] + b"\xff" * 300, good[:scan] + bytes(300), good[:scan],           # 0xFF bytes, zeros, no scan at all
            good[:scan] + rng.integers(0, 256, 500, dtype=np.uint8).tobytes(),          # noise
            rst[:at] + b"\xff\xd3" + rst[at + 2:], rst[:at] + rst[at + 2:],             # a marker out of order, one missing
            good + good[scan:]]                                                         # more blocks than the header says
    many = cases.pil_file(cases.picture("noise", 37, 51), 90, "444", "dri_3")
    assert J.parse(many).segments == 12
    marks = [m for m in range(J.parse(many).scan, len(many) - 1) if many[m] == 0xFF and 0xD0 <= many[m + 1] <= 0xD7]
    # interval 5 of 12 broken off (its tail zeroed, the markers in place): the entropy launch flags the frame while the frame's
    # other workgroups decode their intervals
    bad.insert(0, many[:marks[4] + 2 + 9] + bytes(marks[5] - marks[4] - 11) + many[marks[5]:])
    for b in bad[:-1]:
        with pytest.raises(ref.BadStream):
            ref.decode(b)
    blobs = [other]
    for b in bad:
        blobs += [b, good if len(blobs) % 4 == 1 else other]
    null = len(blobs)
    blobs += [good, other]                                                              # the first of them gets a null table entry
    status, pictures, intact, raw = run_table(blobs, null=(null,))
    assert intact
    for f, blob in enumerate(blobs):
        if f == null:
            assert status[f] == J.SKIPPED
        elif f % 2 == 1 and f < null:
            # the last case decodes its first scan's blocks and stops at the EOI: extra bytes behind the scan are not read
            if blob is bad[-1]:
                assert status[f] == J.OK and np.array_equal(pictures[f], want)
            else:
                assert status[f] == J.BAD_STREAM, (f, status[f])
                assert (raw[f] == 0xA5).all(), f
        else:
            assert status[f] == J.OK
            assert np.array_equal(pictures[f], want if blob is good else other_want), f


def test_descriptors_the_launches_cannot_follow_are_skipped():
    good, want = cases.case("noise", 37, 51, 90, "420")

    def spoil(frames):
        frames["scan_len"][1] = 1 << 27                  # past the end of the data
        frames["qsel"][2][1] = 99
        frames["acsel"][3][2] = -1
        frames["sampling"][4] = 4
        frames["H"][5] = 38                              # not the destination's
        frames["scan_off"][6] = -5
        frames["restart"][7] = 1                         # 12 intervals where the workspace has room for one
    status, pictures, intact, raw = run_table([good] * 9, spoil=spoil)
    assert intact
    assert list(status) == [J.OK] + [J.SKIPPED] * 7 + [J.OK]
    for f in (0, 8):
        assert np.array_equal(pictures[f], want)
    for f in range(1, 8):
        assert (raw[f] == 0xA5).all()


def test_decoder_names_what_it_turns_away():
    import io
    from PIL import Image
    good, want = cases.case("ramp", 17, 33, 75, "444")
    buf = io.BytesIO()
    Image.fromarray(np.asarray(want)[..., ::-1].copy()).save(buf, "JPEG", progressive=True)
    scan = J.parse(good).scan
    dec = J.JpegDecoder(DEV)
    got = dec.decode([good, buf.getvalue(), b"", good[:scan + 20], good])
    assert np.array_equal(got[0], want) and np.array_equal(got[4], want)
    assert got[1] is None and got[2] is None and got[3] is None
    assert "progressive" in dec.last_fallbacks[1] and "SOI" in dec.last_fallbacks[2] and "entropy" in dec.last_fallbacks[3]
    assert set(dec.last_fallbacks) == {1, 2, 3}
    assert dec.decode([]) == [] and dec.last_fallbacks == {}
