"""fr_gallery_pairs_above_f16 and fr_gallery_pairs_workspace are declared, bound and exported under ABI 106, and bad arguments are
refused before any launch (no GPU needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fr_gallery_pairs_workspace", "fr_gallery_pairs_above_f16")


def _header():
    return open(os.path.join(ROOT, "include", "frhip.h")).read()


def _library():
    from facerecognition_infrenceengine_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_pairs_entries_declared_bound_exported():
    _lib = _library()
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        m = re.search(r"\b(int|size_t)\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, f"{name} is not declared in include/frhip.h"
        res, args = _lib.SIGNATURES[name]
        assert res is (ctypes.c_int if m.group(1) == "int" else ctypes.c_size_t)
        assert len(args) == len(m.group(2).split(","))
        assert hasattr(cdll, name), f"{name} is not exported by the built library"
    P, I, L, F, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t
    assert _lib.SIGNATURES["fr_gallery_pairs_workspace"] == (Z, [L, L])
    assert _lib.SIGNATURES["fr_gallery_pairs_above_f16"] == (I, [P, P, L, I, F, I, L, I, P, P, P, P, Z, P])
    assert int(re.search(r"#define FR_ABI_VERSION (\d+)", text).group(1)) == 106 == _lib.ABI_VERSION
    assert _lib.load().fr_version() == 106


def test_pairs_entries_are_listed_in_the_106_comment():
    text = _header()
    comment = text[:text.index("#define FR_ABI_VERSION")]
    comment = comment[comment.rindex("/*"):]
    assert "106:" in comment
    for name in NAMES:
        assert name in comment[comment.index("106:"):], name


def test_pairs_flags_are_the_headers():
    from facerecognition_infrenceengine_amd import gallery
    text = _header()
    assert int(re.search(r"#define FR_PAIRS_OVERFLOW (\d+)", text).group(1)) == gallery.PAIRS_OVERFLOW == 1
    assert int(re.search(r"#define FR_PAIRS_NONFINITE (\d+)", text).group(1)) == gallery.PAIRS_NONFINITE == 2


def test_pairs_refuses_bad_arguments_before_any_launch():
    _lib = _library()
    lib = _lib.load()
    one = ctypes.c_void_p(16)                  # never dereferenced: the arguments are rejected before any launch
    big = lib.fr_gallery_pairs_workspace(300, 64)
    assert big >= 300 * 1024 + 64 * 8 + 4

    def call(N=300, D=512, capacity=64, max_ranges=0, p=one, counts=one, ws=one, wsb=big):
        return lib.fr_gallery_pairs_above_f16(p, None, N, D, 0.4, 0, capacity, max_ranges, p, p, counts, ws, wsb, None)
    with pytest.raises(_lib.FrError, match="N must be"):
        call(N=-1)
    with pytest.raises(_lib.FrError, match="N must be"):
        call(N=1 << 31)
    with pytest.raises(_lib.FrError, match="D must be 512"):
        call(D=256)
    with pytest.raises(_lib.FrError, match="capacity must be"):
        call(capacity=0)
    with pytest.raises(_lib.FrError, match="max_ranges must not be negative"):
        call(max_ranges=-1)
    with pytest.raises(_lib.FrError, match="null pointer"):
        call(p=None)
    with pytest.raises(_lib.FrError, match="null pointer"):
        call(counts=None)
    with pytest.raises(_lib.FrError, match="workspace too small"):
        call(ws=None)
    with pytest.raises(_lib.FrError, match="workspace too small"):
        call(wsb=big - 1)
    for N in (0, 1):                           # no pair: FR_OK, no row and no buffer is read
        assert call(N=N, p=None, counts=None, ws=None, wsb=0) == 0
        with pytest.raises(_lib.FrError, match="D must be 512"):
            call(N=N, D=128, p=None, counts=None, ws=None, wsb=0)
