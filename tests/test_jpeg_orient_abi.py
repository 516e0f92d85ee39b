"""fr_jpeg_decode_oriented_refs_u8 is declared, bound and exported under ABI 106 with the signature of fr_jpeg_decode_refs_u8 plus
one pointer; the old entry, the record and the workspace sizes are what they were; bad arguments are refused before any launch
(no GPU needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW, OLD = "fr_jpeg_decode_oriented_refs_u8", "fr_jpeg_decode_refs_u8"


def _header():
    return open(os.path.join(ROOT, "include", "frhip.h")).read()


def _library():
    from facerecognition_infrenceengine_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def _declared(code, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
    assert m, f"{name} is not declared in include/frhip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_entry_declared_bound_exported():
    _lib = _library()
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    old, new = _declared(code, OLD), _declared(code, NEW)
    assert len(new) == len(old) + 1 == 18
    extra = [a for a in new if a not in old]
    assert extra == ["const int32_t* orient"]
    assert [a for a in new if a in old] == old            # the old arguments, in their order
    P, I, L, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    assert _lib.SIGNATURES[OLD] == (I, [P, L, P, I, I, I, I, P, I, P, I, P, P, P, P, Z, P])
    at = new.index("const int32_t* orient")
    want = list(_lib.SIGNATURES[OLD][1])
    want.insert(at, P)
    assert _lib.SIGNATURES[NEW] == (I, want)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NEW), f"{NEW} is not exported by the built library"
    assert int(re.search(r"#define FR_ABI_VERSION (\d+)", text).group(1)) == 106 == _lib.ABI_VERSION
    assert _lib.load().fr_version() == 106
    comment = text[:text.index("#define FR_ABI_VERSION")]
    comment = comment[comment.rindex("/*"):]
    assert NEW in comment[comment.index("106:"):]


def test_record_and_workspace_are_what_they_were():
    from facerecognition_infrenceengine_amd import jpeg_decode as J
    lib = _library().load()
    assert J.FRAME.itemsize == 64
    struct = re.search(r"typedef struct \{([^}]*)\} fr_jpeg_frame;", _header()).group(1)
    assert [f for f, _ in re.findall(r"(\w+)(?:\[(\d+)\])?\s*[,;]", struct)] == list(J.FRAME.names)
    # coded sizes: a 37 x 51 file turned to 51 x 37 needs what it needed
    assert lib.fr_jpeg_decode_workspace(1, 16, 16, 1) == 16 + 3 * 2 * 2 * 128 + 3 * 16 * 16
    assert lib.fr_jpeg_decode_workspace(3, 37, 51, 5) == 3 * (64 + 3 * 5 * 7 * 128 + 3 * 48 * 64)
    assert lib.fr_jpeg_decode_workspace(64, 1080, 1920, 1) == 64 * (16 + 3 * 135 * 240 * 128 + 3 * 1088 * 1920)
    assert lib.fr_jpeg_decode_workspace(0, 16, 16, 1) == 0


def test_entry_refuses_bad_arguments_before_any_launch():
    _lib = _library()
    lib = _lib.load()
    one = ctypes.c_void_p(16)                  # never dereferenced: the arguments are rejected before any launch
    big = 1 << 40

    def call(data=one, data_bytes=1000, frames=one, n=1, H=64, W=96, segments=1, qtables=one, nq=2, htables=one, nh=4, natural=one,
             refs=one, orient=one, status=one, ws=one, ws_bytes=big):
        return lib.fr_jpeg_decode_oriented_refs_u8(data, data_bytes, frames, n, H, W, segments, qtables, nq, htables, nh, natural, refs,
                                                   orient, status, ws, ws_bytes, None)
    for arg in ("data", "frames", "qtables", "htables", "natural", "refs", "status", "ws"):
        for orient in (one, None):             # a null ``orient`` is no error: it means all 1
            with pytest.raises(_lib.FrError, match="fr_jpeg_decode_oriented_refs_u8: null pointer"):
                call(orient=orient, **{arg: None})
    for n in (-1, 65536):
        with pytest.raises(_lib.FrError, match="bad size"):
            call(n=n)
    for H, W in ((0, 96), (64, 0), (-2, 96), (64, -1), (65536, 96), (64, 65536)):
        with pytest.raises(_lib.FrError, match="bad size"):
            call(H=H, W=W)
    with pytest.raises(_lib.FrError, match="beyond 2 GiB"):
        call(H=10923, W=65535)
    for segments in (0, -1, (1 << 24) + 1):
        with pytest.raises(_lib.FrError, match="max_segments"):
            call(segments=segments)
    with pytest.raises(_lib.FrError, match="data_bytes"):
        call(data_bytes=-1)
    for kw in ({"nq": 0}, {"nh": 0}, {"nq": 65536}, {"nh": -3}):
        with pytest.raises(_lib.FrError, match="table count"):
            call(**kw)
    need = lib.fr_jpeg_decode_workspace(1, 64, 96, 1)
    with pytest.raises(_lib.FrError, match="workspace too small"):
        call(ws_bytes=need - 1)
    with pytest.raises(_lib.FrError, match="null pointer"):       # the size is enough: the next check is reached
        call(ws_bytes=need, frames=None)
    with pytest.raises(_lib.FrError, match="16-byte boundary"):
        call(ws=ctypes.c_void_p(24))
    nothing = dict(data=None, frames=None, qtables=None, htables=None, natural=None, refs=None, orient=None, status=None, ws=None,
                   ws_bytes=0)
    assert call(n=0, **nothing) == 0
    with pytest.raises(_lib.FrError, match="bad size"):
        call(n=0, H=0, **nothing)
