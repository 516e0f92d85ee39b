"""fr_jpeg_workspace, fr_jpeg_encode_u8 and fr_jpeg_encode_refs_u8 are declared, bound and exported under ABI 106, the host's
constants are the header's, and bad arguments are refused before any launch (no GPU needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fr_jpeg_workspace", "fr_jpeg_encode_u8", "fr_jpeg_encode_refs_u8")


def _header():
    return open(os.path.join(ROOT, "include", "frhip.h")).read()


def _library():
    from facerecognition_infrenceengine_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def _define(text, name):
    return int(re.search(r"#define %s (\d+)" % name, text).group(1))


def test_jpeg_entries_declared_bound_exported():
    _lib = _library()
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, f"{name} is not declared in include/frhip.h"
        res, args = _lib.SIGNATURES[name]
        assert len(args) == len(m.group(1).split(","))
        assert hasattr(cdll, name), f"{name} is not exported by the built library"
    P, I, L, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    assert _lib.SIGNATURES["fr_jpeg_workspace"] == (Z, [I, I, I, I])
    assert _lib.SIGNATURES["fr_jpeg_encode_u8"] == (I, [P, I, I, I, P, I, P, P, I, P, L, P, P, P, Z, P])
    assert _lib.SIGNATURES["fr_jpeg_encode_refs_u8"] == (I, [P, I, I, I, P, I, P, P, I, P, L, P, P, P, Z, P])
    assert int(re.search(r"#define FR_ABI_VERSION (\d+)", text).group(1)) == 106 == _lib.ABI_VERSION
    assert _lib.load().fr_version() == 106
    comment = text[:text.index("#define FR_ABI_VERSION")]
    comment = comment[comment.rindex("/*"):]
    for name in NAMES:
        assert name in comment[comment.index("106:"):], name


def test_constants_agree_with_the_host():
    from facerecognition_infrenceengine_amd import jpeg, jpeg_tables
    from tests.helpers import jpeg_ref
    text = _header()
    assert (_define(text, "FR_JPEG_OK"), _define(text, "FR_JPEG_OVERFLOW"), _define(text, "FR_JPEG_SKIPPED")) == \
        (jpeg.OK, jpeg.OVERFLOW, jpeg.SKIPPED) == (0, 1, 2)
    assert _define(text, "FR_JPEG_HEADER_BYTES") == jpeg.HEADER_BYTES == len(jpeg_ref.header(16, 16, 80))
    assert (_define(text, "FR_JPEG_AT_H"), _define(text, "FR_JPEG_AT_W"), _define(text, "FR_JPEG_AT_DRI")) == \
        (jpeg.AT_H, jpeg.AT_W, jpeg.AT_DRI)
    assert _define(text, "FR_JPEG_CODE_ROW") == jpeg_tables.CODE_ROW
    # the three patched fields are where the definition's header has them, and nothing else depends on the size
    a, b = jpeg_ref.header(0x1234, 0x5678, 80), jpeg_ref.header(1, 1, 80)
    assert a[jpeg.AT_H:jpeg.AT_H + 2] == b"\x12\x34" and a[jpeg.AT_W:jpeg.AT_W + 2] == b"\x56\x78"
    assert a[jpeg.AT_DRI:jpeg.AT_DRI + 2] == ((0x5678 + 15) // 16).to_bytes(2, "big")
    assert [i for i in range(len(a)) if a[i] != b[i]] == [jpeg.AT_H, jpeg.AT_H + 1, jpeg.AT_W, jpeg.AT_W + 1, jpeg.AT_DRI,
                                                          jpeg.AT_DRI + 1]


def test_the_hosts_header_is_the_definitions():
    from facerecognition_infrenceengine_amd import jpeg
    from tests.helpers import jpeg_ref
    for q in (1, 50, 80, 95):
        enc = jpeg.JpegEncoder(q)
        for h, w in ((1, 1), (37, 51), (1080, 1920), (65535, 65535)):
            assert enc.header(h, w) == jpeg_ref.header(h, w, q)
    for bad in ((0, 5), (5, 65536)):
        with pytest.raises(ValueError):
            jpeg.JpegEncoder().header(*bad)
    for bad in (0, 96):
        with pytest.raises(ValueError, match="quality"):
            jpeg.JpegEncoder(quality=bad)
    with pytest.raises(ValueError, match="row_budget"):
        jpeg.JpegEncoder(row_budget=0)
    assert jpeg.default_row_budget(1920) == 16 * 1920 * 3 and jpeg.default_row_budget(17) == 16 * 32 * 3


def test_workspace_size():
    lib = _library().load()
    assert lib.fr_jpeg_workspace(3, 40, 56, 100) == 48 + 9 * 100          # 9 row lengths, padded to 16 bytes; 9 segments
    assert lib.fr_jpeg_workspace(1, 1, 1, 1) == 16 + 1
    assert lib.fr_jpeg_workspace(64, 1080, 1920, 92160) == 64 * 68 * 4 + 64 * 68 * 92160
    assert lib.fr_jpeg_workspace(0, 16, 16, 8) == 0
    for bad in ((-1, 16, 16, 8), (65536, 16, 16, 8), (1, 0, 16, 8), (1, 16, 65536, 8), (1, 16, 16, 0)):
        assert lib.fr_jpeg_workspace(*bad) == 0


@pytest.mark.parametrize("entry", ["fr_jpeg_encode_u8", "fr_jpeg_encode_refs_u8"])
def test_entries_refuse_bad_arguments_before_any_launch(entry):
    _lib = _library()
    lib = _lib.load()
    one = ctypes.c_void_p(16)                  # never dereferenced: the arguments are rejected before any launch
    big = 1 << 40

    def call(frames=one, N=1, H=64, W=96, header=one, header_len=629, codes=one, qtables=one, row_budget=4608, out=one,
             capacity=1 << 20, offsets=one, status=one, ws=one, ws_bytes=big):
        return getattr(lib, entry)(frames, N, H, W, header, header_len, codes, qtables, row_budget, out, capacity, offsets, status,
                                   ws, ws_bytes, None)
    for arg in ("frames", "header", "codes", "qtables", "out", "offsets", "status", "ws"):
        with pytest.raises(_lib.FrError, match="null pointer"):
            call(**{arg: None})
    for N in (-1, 65536):
        with pytest.raises(_lib.FrError, match="bad size"):
            call(N=N)
    for H, W in ((0, 96), (64, 0), (-2, 96), (64, -1), (65536, 96), (64, 65536)):
        with pytest.raises(_lib.FrError, match="bad size"):
            call(H=H, W=W)
    with pytest.raises(_lib.FrError, match="beyond 2 GiB"):
        call(H=32768, W=32768)
    with pytest.raises(_lib.FrError, match="beyond 2 GiB"):
        call(H=10923, W=65535)                 # H*W*3 = 2^31 + 32767: the first height past the limit at that width
    for budget in (0, -5):
        with pytest.raises(_lib.FrError, match="row_budget"):
            call(row_budget=budget)
    for n in (0, 628, 630):
        with pytest.raises(_lib.FrError, match="header"):
            call(header_len=n)
    with pytest.raises(_lib.FrError, match="out_capacity"):
        call(capacity=-1)
    need = lib.fr_jpeg_workspace(1, 64, 96, 4608)
    assert need == 16 + 4 * 4608
    with pytest.raises(_lib.FrError, match="workspace too small"):
        call(ws_bytes=need - 1)
    with pytest.raises(_lib.FrError, match="null pointer"):       # the size is enough: the next check is reached
        call(ws_bytes=need, frames=None)
    # N = 0: FR_OK, nothing is read - not even the pointers; arguments no encoding exists for stay errors
    nothing = dict(frames=None, header=None, codes=None, qtables=None, out=None, offsets=None, status=None, ws=None, ws_bytes=0)
    assert call(N=0, **nothing) == 0
    with pytest.raises(_lib.FrError, match="row_budget"):
        call(N=0, row_budget=0, **nothing)
    with pytest.raises(_lib.FrError, match="bad size"):
        call(N=0, H=0)
