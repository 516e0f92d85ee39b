"""fr_track_fuse_f32 is declared, bound and exported under ABI 106, and bad arguments are refused before any launch (no GPU
needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fr_track_fuse_f32"
POINTERS = ("entry", "need", "tid", "slot", "counts", "normed", "tring", "ttmpl", "tmean", "query", "shots", "event")


def _header():
    return open(os.path.join(ROOT, "include", "frhip.h")).read()


def _library():
    from facerecognition_infrenceengine_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_fuse_entry_declared_bound_exported():
    _lib = _library()
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, code)
    assert m, f"{NAME} is not declared in include/frhip.h"
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    want = [P if "*" in a or a.startswith("fr_stream_t") else F if a.startswith("float") else I for a in args]
    assert [a.split()[-1].lstrip("*") for a in args] == ["entry", "need", "tid", "slot", "counts", "normed", "N", "cap", "S", "T", "K",
                                                        "join_thr", "tring", "ttmpl", "tmean", "query", "shots", "event", "stream"]
    assert _lib.SIGNATURES[NAME] == (I, want) == (I, [P, P, P, P, P, P, I, I, I, I, I, F, P, P, P, P, P, P, P])
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME), f"{NAME} is not exported by the built library"
    assert int(re.search(r"#define FR_ABI_VERSION (\d+)", text).group(1)) == 106 == _lib.ABI_VERSION == _lib.load().fr_version()


def test_fuse_entry_is_listed_in_the_version_comment():
    text = _header()
    comment = text[:text.index("#define FR_ABI_VERSION")]
    comment = comment[comment.rindex("/*"):]
    assert NAME in comment and "ADDED under" in comment[comment.index(NAME):]


def test_the_entries_before_it_keep_their_signatures():
    _lib = _library()
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib.SIGNATURES["fr_track_associate_f32"] == (I, [P, P, P, I, I, I, I, P, P, P, F, I, I, P, P, P, P])
    assert _lib.SIGNATURES["fr_track_commit_f32"] == (I, [P, P, P, P, I, I, I, I, P, P, P, P])
    assert _lib.SIGNATURES["fr_track_resolve_quality_i32"] == (I, [P, P, P, P, P, P, I, I, I, I, P, P, I, P, P, P, P])


def test_fuse_refuses_bad_arguments_before_any_launch():
    _lib = _library()
    lib = _lib.load()
    one = ctypes.c_void_p(16)                  # never dereferenced: the arguments are rejected before any launch

    def call(N=1, cap=8, S=4, T=32, K=10, join_thr=0.4, **ptrs):
        p = {k: ptrs.get(k, one) for k in POINTERS}
        assert set(ptrs) <= set(POINTERS)
        # only N == 0 gets past the checks in this file: a call that would launch is never made with these pointers (the file
        # runs on machines with a GPU too)
        assert N == 0 or any(v is None for v in p.values()) or \
            not (0 < N <= 65535 and 1 <= cap <= 64 and 1 <= T <= 64 and S >= 1 and 1 <= K <= 16 and -1 <= join_thr <= 1)
        return lib.fr_track_fuse_f32(p["entry"], p["need"], p["tid"], p["slot"], p["counts"], p["normed"], N, cap, S, T, K, join_thr,
                                     p["tring"], p["ttmpl"], p["tmean"], p["query"], p["shots"], p["event"], None)
    for K in (0, 17, -1, 1000):
        with pytest.raises(_lib.FrError, match="K -?[0-9]+ outside 1 .. 16"):
            call(K=K)
    for thr in (-1.0000001, 1.0000001, 2.0, -5.0, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(_lib.FrError, match="join_thr"):
            call(join_thr=thr)
    for T in (0, 65, -1, 1000):
        with pytest.raises(_lib.FrError, match="T -?[0-9]+ outside 1 .. 64"):
            call(T=T)
    for cap in (0, -2, 65):
        with pytest.raises(_lib.FrError, match="cap -?[0-9]+ outside 1 .. 64"):
            call(cap=cap)
    for N in (65536, -1):
        with pytest.raises(_lib.FrError, match="bad size"):
            call(N=N)
    for S in (0, -3):
        with pytest.raises(_lib.FrError, match="bad state size"):
            call(S=S)
    for name in POINTERS:
        with pytest.raises(_lib.FrError, match="null pointer"):
            call(**{name: None})
    # the edges of the ranges are not refused, and N == 0 reads nothing - not even the pointers
    assert call(N=0, T=1, cap=1, S=1, K=1, join_thr=-1.0) == 0
    assert call(N=0, T=64, cap=64, K=16, join_thr=1.0) == 0
    assert call(N=0, **{k: None for k in POINTERS}) == 0
    for kw in (dict(K=0), dict(K=17), dict(join_thr=float("nan"))):
        with pytest.raises(_lib.FrError):
            call(N=0, **kw)                    # arguments no rule exists for stay an error
