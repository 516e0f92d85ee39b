"""Which decode entry ``JpegDecoder.decode_device`` calls, with what destinations and orientation words - without a device: the
library is a recorder and the tensors live on the CPU, so the staging the entry is handed can be read back through its pointer."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from facerecognition_infrenceengine_amd import jpeg_decode as J
from tests.helpers import exif_cases as X, jpeg_decode_cases as cases

REF = np.dtype([("data", "<u8"), ("H", "<i4"), ("W", "<i4"), ("rest", "V16")])       # include/frhip.h fr_frame_ref, 32 bytes


class Recorder:
    """Stands in for the loaded library: a decode entry appends (name, args, the frame table and the orientation words it was
    handed, copied out while the call runs); a workspace query answers 64."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("fr_"):
            raise AttributeError(name)

        def entry(*args):
            args = tuple(a.value if isinstance(a, C.c_void_p) else a for a in args)
            if name.endswith("workspace"):
                return 64
            n = args[3]
            refs = np.frombuffer(C.string_at(args[12], 32 * n), REF).copy()
            words = np.frombuffer(C.string_at(args[13], 4 * n), "<i4").copy() if name == "fr_jpeg_decode_oriented_refs_u8" else None
            self.scan_off = np.frombuffer(C.string_at(args[2], 64 * n), J.FRAME)["scan_off"].copy()
            self.calls.append((name, args, refs, words))
            return 0
        return entry


class _Event:
    def record(self):
        pass

    def synchronize(self):
        pass


@pytest.fixture
def rec(monkeypatch):
    from facerecognition_infrenceengine_amd import _lib
    rec = Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    monkeypatch.setattr(torch.cuda, "device", lambda device=None: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    return rec


def _files():
    a = cases.case("noise", 17, 33, 90, "420")[0]
    b = cases.case("ramp", 17, 33, 75, "444")[0]
    return a, b


def test_without_orient_the_tag_is_never_read(rec, monkeypatch):
    def never(data):
        raise AssertionError("exif_orientation called without orient")
    monkeypatch.setattr(J, "exif_orientation", never)
    a, b = _files()
    dec = J.JpegDecoder("cpu")
    frames, shapes, status = dec.decode_device([X.with_orientation(a, 6), b])
    assert [c[0] for c in rec.calls] == ["fr_jpeg_decode_refs_u8"]
    assert len(rec.calls[0][1]) == 17
    assert shapes == [(17, 33), (17, 33)] and tuple(frames.shape) == (2, 17, 33, 3)
    assert dec.last_orientations == [1, 1]
    assert [(int(r["H"]), int(r["W"])) for r in rec.calls[0][2]] == [(17, 33)] * 2


def test_all_upright_files_take_the_old_entry(rec):
    a, b = _files()
    dec = J.JpegDecoder("cpu", orient=True)
    frames, shapes, _ = dec.decode_device([a, X.with_orientation(b, 1), X.with_orientation(a, 0), b"no JPEG"])
    assert [c[0] for c in rec.calls] == ["fr_jpeg_decode_refs_u8"]
    name, args, refs, _ = rec.calls[0]
    assert len(args) == 17 and args[1] >= 96 * 4 and args[12] == args[0] + 64 * 4
    assert dec.last_orientations == [1, 1, 1, 1] and shapes == [(17, 33)] * 3 + [None]
    assert int(refs[3]["data"]) == 0 and tuple(frames.shape) == (4, 17, 33, 3)
    # the same staging layout as without ``orient``: the first scan sits right behind the tables
    plain = J.JpegDecoder("cpu")
    plain.decode_device([a, X.with_orientation(b, 1), X.with_orientation(a, 0), b"no JPEG"])
    assert rec.calls[1][0] == "fr_jpeg_decode_refs_u8" and rec.calls[1][1][1] == args[1]


def test_one_turned_file_takes_the_new_entry_once(rec):
    a, b = _files()
    big = cases.case("noise", 37, 51, 90, "420")[0]
    dec = J.JpegDecoder("cpu", orient=True)
    blobs = [a, X.with_orientation(b, 6), b"junk", X.with_orientation(big, 3), X.with_orientation(big, 5)]
    frames, shapes, status = dec.decode_device(blobs)
    assert [c[0] for c in rec.calls] == ["fr_jpeg_decode_oriented_refs_u8"]
    name, args, refs, words = rec.calls[0]
    n = 5
    assert len(args) == 18 and args[3] == n
    assert (args[4], args[5]) == (37, 51)                 # max_H, max_W: CODED sizes (the turned 37 x 51 is 51 x 37)
    assert args[12] == args[0] + 64 * n and args[13] == args[0] + 96 * n        # one staging copy: tables, then the words
    assert list(words) == [1, 6, 1, 3, 5] == dec.last_orientations
    assert shapes == [(17, 33), (33, 17), None, (37, 51), (51, 37)]
    assert [(int(r["H"]), int(r["W"])) for r in refs] == [(17, 33), (33, 17), (0, 0), (37, 51), (51, 37)]
    assert isinstance(frames, tuple)                      # sizes differ: the arena
    arena = frames[0].data_ptr()
    offs = [int(r["data"]) - arena for r in refs if int(r["data"])]
    assert offs == [0, 1696, 3392, 9056] and all(o % 16 == 0 for o in offs)
    # the scans start behind the words, on a 16-byte boundary
    assert rec.scan_off[0] == (100 * n + 15) // 16 * 16 == 512 and all(int(o) % 16 == 0 for o in rec.scan_off)


def test_turned_files_of_one_oriented_size_stay_dense(rec):
    a, b = _files()
    tall = cases.case("noise", 33, 17, 90, "444")[0]
    dec = J.JpegDecoder("cpu", orient=True)
    frames, shapes, _ = dec.decode_device([X.with_orientation(a, 6), X.with_orientation(b, 8), tall])
    assert rec.calls[0][0] == "fr_jpeg_decode_oriented_refs_u8"
    assert shapes == [(33, 17)] * 3 and torch.is_tensor(frames) and tuple(frames.shape) == (3, 33, 17, 3)
    assert (rec.calls[0][1][4], rec.calls[0][1][5]) == (33, 33)
    out = torch.zeros((3, 33, 17, 3), dtype=torch.uint8)
    got, _, _ = dec.decode_device([X.with_orientation(a, 6), X.with_orientation(b, 8), tall], out=out)
    assert got is out and [int(r["data"]) for r in rec.calls[1][2]] == [out.data_ptr() + k * 33 * 17 * 3 for k in range(3)]


def test_mismatched_decoder_is_refused():
    from facerecognition_infrenceengine_amd import _lib
    from facerecognition_infrenceengine_amd.enrol import Enroller

    class App:
        device = "cpu"
    lib_load = _lib.load
    try:
        _lib.load = lambda: None
        with pytest.raises(ValueError, match="orient"):
            Enroller(App(), decoder=J.JpegDecoder("cpu", orient=True))
        with pytest.raises(ValueError, match="orient"):
            Enroller(App(), decoder=J.JpegDecoder("cpu"), orient=True)
        assert Enroller(App(), decoder=J.JpegDecoder("cpu", orient=True), orient=True).orient is True
        assert Enroller(App()).orient is False
    finally:
        _lib.load = lib_load
