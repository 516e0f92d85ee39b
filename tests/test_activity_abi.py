"""fr_frame_activity_u8 and fr_frame_activity_refs_u8 are declared, bound and exported under ABI 106, and bad arguments are
refused before any launch (no GPU needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fr_frame_activity_u8", "fr_frame_activity_refs_u8")


def _header():
    return open(os.path.join(ROOT, "include", "frhip.h")).read()


def _library():
    from facerecognition_infrenceengine_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_activity_entries_declared_bound_exported():
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
    assert _lib.SIGNATURES["fr_frame_activity_u8"] == (I, [P, I, I, I, P, I, P, P, P, I, P, P, P, I, I, I, P])
    assert _lib.SIGNATURES["fr_frame_activity_refs_u8"] == (I, [P, I, P, I, P, P, P, I, P, P, P, I, I, I, P])
    # the table form is the uniform form with (refs, nframes) in the place of (frames, N, H, W)
    assert _lib.SIGNATURES["fr_frame_activity_u8"][1][4:] == _lib.SIGNATURES["fr_frame_activity_refs_u8"][1][2:]
    assert int(re.search(r"#define FR_ABI_VERSION (\d+)", text).group(1)) == 106 == _lib.ABI_VERSION
    assert _lib.load().fr_version() == 106


def test_activity_entries_are_listed_in_the_106_comment():
    text = _header()
    comment = text[:text.index("#define FR_ABI_VERSION")]
    comment = comment[comment.rindex("/*"):]
    assert "106:" in comment
    for name in NAMES:
        assert name in comment[comment.index("106:"):], name


def _refusals(call):
    """the refusals both entries share; ``call(**overrides)`` makes the call with good arguments otherwise"""
    from facerecognition_infrenceengine_amd._lib import FrError
    for bad in ({"S": 0}, {"S": -1}, {"C": 0}, {"C": -5}):
        with pytest.raises(FrError, match="bad state size"):
            call(**bad)
    for thr in (-1, 256, 1000):
        with pytest.raises(FrError, match="thr"):
            call(thr=thr)
    for mc in (0, -3):
        with pytest.raises(FrError, match="min_cells"):
            call(min_cells=mc)
    with pytest.raises(FrError, match="max_idle"):
        call(max_idle=-1)
    with pytest.raises(FrError, match="bad size"):
        call(N=65536)
    with pytest.raises(FrError, match="bad size"):
        call(N=-1)
    for name in ("slot", "grid", "geom", "idle", "cur", "changed", "active"):
        with pytest.raises(FrError, match="null pointer"):
            call(**{name: None})
    # the edges of the ranges are not refused (N == 0: past the checks nothing is launched)
    assert call(N=0, thr=0, min_cells=1, max_idle=0) == 0 and call(N=0, thr=255, max_idle=2 ** 31 - 1) == 0


def test_uniform_entry_refuses_bad_arguments_before_any_launch():
    _lib = _library()
    lib = _lib.load()
    one = ctypes.c_void_p(16)                  # never dereferenced: the arguments are rejected before any launch

    def call(frames=one, N=1, H=32, W=48, slot=one, S=4, grid=one, geom=one, idle=one, C=6, cur=one, changed=one, active=one,
             thr=4, min_cells=2, max_idle=0):
        # only N == 0 gets past the checks in this file: a call that would launch is never made with these pointers (the
        # file runs on machines with a GPU too)
        assert N == 0 or any(v is None for v in (frames, slot, grid, geom, idle, cur, changed, active)) or \
            not (0 < N <= 65535 and H > 0 and W > 0 and H * W * 3 < 2 ** 31 and S > 0 and C > 0 and 0 <= thr <= 255
                 and min_cells >= 1 and max_idle >= 0)
        return lib.fr_frame_activity_u8(frames, N, H, W, slot, S, grid, geom, idle, C, cur, changed, active, thr, min_cells,
                                        max_idle, None)
    _refusals(call)
    for H, W in ((0, 48), (32, 0), (-16, 48), (32, -1)):
        with pytest.raises(_lib.FrError, match="bad frame size"):
            call(H=H, W=W)
    with pytest.raises(_lib.FrError, match="beyond 2 GiB"):
        call(H=32768, W=32768)
    with pytest.raises(_lib.FrError, match="beyond 2 GiB"):
        call(H=1, W=715827883)                 # H*W*3 = 2^31 + 1: the first width past the limit
    with pytest.raises(_lib.FrError, match="null pointer"):
        call(frames=None)
    # N == 0: FR_OK, nothing is read - not even the pointers
    assert call(frames=None, slot=None, grid=None, geom=None, idle=None, cur=None, changed=None, active=None, N=0) == 0
    with pytest.raises(_lib.FrError, match="bad frame size"):
        call(N=0, H=0)                         # arguments no judgment exists for stay an error


def test_table_entry_refuses_bad_arguments_before_any_launch():
    _lib = _library()
    lib = _lib.load()
    one = ctypes.c_void_p(16)

    def call(refs=one, N=1, slot=one, S=4, grid=one, geom=one, idle=one, C=6, cur=one, changed=one, active=one, thr=4,
             min_cells=2, max_idle=0):
        assert N == 0 or any(v is None for v in (refs, slot, grid, geom, idle, cur, changed, active)) or \
            not (0 < N <= 65535 and S > 0 and C > 0 and 0 <= thr <= 255 and min_cells >= 1 and max_idle >= 0)
        return lib.fr_frame_activity_refs_u8(refs, N, slot, S, grid, geom, idle, C, cur, changed, active, thr, min_cells,
                                             max_idle, None)
    _refusals(call)
    with pytest.raises(_lib.FrError, match="null pointer"):
        call(refs=None)
    assert call(refs=None, slot=None, grid=None, geom=None, idle=None, cur=None, changed=None, active=None, N=0) == 0
