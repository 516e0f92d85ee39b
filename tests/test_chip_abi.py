"""fr_face_chips_u8 and fr_face_chips_refs_u8 are declared, bound and exported, and bad arguments are refused before any launch (no
GPU needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fr_face_chips_u8", "fr_face_chips_refs_u8")


def _header():
    return open(os.path.join(ROOT, "include", "frhip.h")).read()


def _library():
    from facerecognition_infrenceengine_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_chip_entries_declared_bound_exported():
    _lib = _library()
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, f"{name} is not declared in include/frhip.h"
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(m.group(1).split(","))
        assert hasattr(cdll, name), f"{name} is not exported by the built library"
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["fr_face_chips_u8"] == (I, [P, I, I, I, P, I, I, I, P, P])
    assert _lib.SIGNATURES["fr_face_chips_refs_u8"] == (I, [P, I, P, I, I, I, P, P])
    # the binding, the header and the library agree on the version, and the version comment names the new entries
    assert int(re.search(r"#define FR_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == _lib.load().fr_version()
    comment = text[:text.index("#define FR_ABI_VERSION")]
    comment = comment[comment.rindex("/*"):]
    for name in NAMES:
        assert name in comment, name


def test_constants_agree_with_the_host():
    from facerecognition_infrenceengine_amd import chips
    from tests.helpers import chip_ref
    text = _header()
    assert int(re.search(r"#define FR_CHIP_MAX_SIDE (\d+)", text).group(1)) == chips.MAX_SIDE == chip_ref.MAX_SIDE == 4096
    assert (chips.MIN_SIZE, chips.MAX_SIZE) == (chip_ref.MIN_SIZE, chip_ref.MAX_SIZE) == (16, 256)
    assert chips.COORD_LIMIT == chip_ref.COORD_LIMIT == 1 << 20


def test_uniform_entry_refuses_bad_arguments_before_any_launch():
    _lib = _library()
    lib = _lib.load()
    one = ctypes.c_void_p(16)                  # never dereferenced: the arguments are rejected before any launch

    def call(frames=one, N=1, H=64, W=96, chips=one, F=1, size=112, fill=0, out=one):
        return lib.fr_face_chips_u8(frames, N, H, W, chips, F, size, fill, out, None)
    for arg in ("frames", "chips", "out"):
        with pytest.raises(_lib.FrError, match="null pointer"):
            call(**{arg: None})
    for N in (-1, 65536):
        with pytest.raises(_lib.FrError, match="bad size"):
            call(N=N)
    for H, W in ((0, 96), (64, 0), (-2, 96), (64, -1)):
        with pytest.raises(_lib.FrError, match="bad size"):
            call(H=H, W=W)
    with pytest.raises(_lib.FrError, match="beyond 2 GiB"):
        call(H=1, W=715827883)                 # H*W*3 = 2^31 + 1: the first width past the limit
    for F in (-1, (1 << 20) + 1):
        with pytest.raises(_lib.FrError, match="bad size"):
            call(F=F)
    for size in (15, 0, -112, 257):
        with pytest.raises(_lib.FrError, match="size"):
            call(size=size)
    # F = 0: FR_OK, nothing is read - not even the pointers; a shape no picture exists for stays an error
    assert call(frames=None, chips=None, out=None, F=0) == 0
    assert call(F=0) == 0
    with pytest.raises(_lib.FrError, match="size"):
        call(frames=None, chips=None, out=None, F=0, size=15)
    with pytest.raises(_lib.FrError, match="bad size"):
        call(F=0, H=0)
    with pytest.raises(_lib.FrError, match="bad size"):
        call(F=0, N=65536)


def test_table_entry_refuses_bad_arguments_before_any_launch():
    _lib = _library()
    lib = _lib.load()
    one = ctypes.c_void_p(16)

    def call(refs=one, n=1, chips=one, F=1, size=112, fill=0, out=one):
        return lib.fr_face_chips_refs_u8(refs, n, chips, F, size, fill, out, None)
    for arg in ("refs", "chips", "out"):
        with pytest.raises(_lib.FrError, match="null pointer"):
            call(**{arg: None})
    for n in (-1, 65536):
        with pytest.raises(_lib.FrError, match="bad size"):
            call(n=n)
    for F in (-1, (1 << 20) + 1):
        with pytest.raises(_lib.FrError, match="bad size"):
            call(F=F)
    for size in (15, 257):
        with pytest.raises(_lib.FrError, match="size"):
            call(size=size)
    assert call(refs=None, chips=None, out=None, F=0) == 0
    with pytest.raises(_lib.FrError, match="size"):
        call(F=0, size=300)
