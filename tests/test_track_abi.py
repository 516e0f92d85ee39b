"""fr_track_associate_f32 and fr_track_commit_f32 are declared, bound and exported, and bad arguments are refused before any
launch (no GPU needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fr_track_associate_f32", "fr_track_commit_f32")


def _header():
    return open(os.path.join(ROOT, "include", "frhip.h")).read()


def _library():
    from facerecognition_infrenceengine_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_track_entries_declared_bound_exported():
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
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib.SIGNATURES["fr_track_associate_f32"] == (I, [P, P, P, I, I, I, I, P, P, P, F, I, I, P, P, P, P])
    assert _lib.SIGNATURES["fr_track_commit_f32"] == (I, [P, P, P, P, I, I, I, I, P, P, P, P])
    assert int(re.search(r"#define FR_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == _lib.load().fr_version()


def test_track_entries_are_listed_in_the_version_comment():
    text = _header()
    comment = text[:text.index("#define FR_ABI_VERSION")]
    comment = comment[comment.rindex("/*"):]
    for name in NAMES:
        assert name in comment, name
    assert "ADDED under" in comment[comment.index(NAMES[0]):]


def test_associate_refuses_bad_arguments_before_any_launch():
    _lib = _library()
    lib = _lib.load()
    one = ctypes.c_void_p(16)                  # never dereferenced: the arguments are rejected before any launch

    def call(boxes=one, counts=one, slot=one, N=1, cap=8, S=4, T=32, tbox=one, tstate=one, next_id=one, iou_thr=0.5,
             max_reuse=4, max_misses=1, entry=one, need=one, tid=one):
        ptrs = (boxes, counts, slot, tbox, tstate, next_id, entry, need, tid)
        # only N == 0 gets past the checks in this file: a call that would launch is never made with these pointers (the
        # file runs on machines with a GPU too)
        assert N == 0 or any(p is None for p in ptrs) or \
            not (0 < N <= 65535 and 1 <= cap <= 64 and 1 <= T <= 64 and S >= 1 and max_reuse >= 0 and max_misses >= 0
                 and 0 < iou_thr <= 1)
        return lib.fr_track_associate_f32(boxes, counts, slot, N, cap, S, T, tbox, tstate, next_id, iou_thr, max_reuse,
                                          max_misses, entry, need, tid, None)
    for T in (0, 65, -1, 1000):
        with pytest.raises(_lib.FrError, match="T -?[0-9]+ outside 1 .. 64"):
            call(T=T)
    for cap in (0, -2, 65):
        with pytest.raises(_lib.FrError, match="cap -?[0-9]+ outside 1 .. 64"):
            call(cap=cap)
    with pytest.raises(_lib.FrError, match="max_reuse"):
        call(max_reuse=-1)
    with pytest.raises(_lib.FrError, match="max_misses"):
        call(max_misses=-1)
    for thr in (0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf")):
        with pytest.raises(_lib.FrError, match="iou_thr"):
            call(iou_thr=thr)
    for N in (65536, -1):
        with pytest.raises(_lib.FrError, match="bad size"):
            call(N=N)
    with pytest.raises(_lib.FrError, match="bad state size"):
        call(S=0)
    for name in ("boxes", "counts", "slot", "tbox", "tstate", "next_id", "entry", "need", "tid"):
        with pytest.raises(_lib.FrError, match="null pointer"):
            call(**{name: None})
    # the edges of the ranges are not refused, and N == 0 reads nothing - not even the pointers
    assert call(N=0, T=1, cap=1, max_reuse=0, max_misses=0, iou_thr=1.0) == 0
    assert call(N=0, T=64, cap=64, iou_thr=1e-30, max_reuse=2 ** 31 - 1) == 0
    assert call(N=0, boxes=None, counts=None, slot=None, tbox=None, tstate=None, next_id=None, entry=None, need=None,
                tid=None) == 0
    with pytest.raises(_lib.FrError, match="T 0 outside"):
        call(N=0, T=0)                         # arguments no rule exists for stay an error


def test_commit_refuses_bad_arguments_before_any_launch():
    _lib = _library()
    lib = _lib.load()
    one = ctypes.c_void_p(16)

    def call(entry=one, need=one, slot=one, counts=one, N=1, cap=8, S=4, T=32, bank=one, emb=one, normed=one):
        ptrs = (entry, need, slot, counts, bank, emb, normed)
        assert N == 0 or any(p is None for p in ptrs) or not (0 < N <= 65535 and 1 <= cap <= 64 and 1 <= T <= 64 and S >= 1)
        return lib.fr_track_commit_f32(entry, need, slot, counts, N, cap, S, T, bank, emb, normed, None)
    for T in (0, 65):
        with pytest.raises(_lib.FrError, match="T -?[0-9]+ outside 1 .. 64"):
            call(T=T)
    for cap in (0, 65):
        with pytest.raises(_lib.FrError, match="cap -?[0-9]+ outside 1 .. 64"):
            call(cap=cap)
    for N in (65536, -1):
        with pytest.raises(_lib.FrError, match="bad size"):
            call(N=N)
    with pytest.raises(_lib.FrError, match="bad state size"):
        call(S=-3)
    for name in ("entry", "need", "slot", "counts", "bank", "emb", "normed"):
        with pytest.raises(_lib.FrError, match="null pointer"):
            call(**{name: None})
    assert call(N=0) == 0 and call(N=0, entry=None, need=None, slot=None, counts=None, bank=None, emb=None, normed=None) == 0
