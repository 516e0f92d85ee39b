"""fr_gallery_first_above_blocked_f32 and fr_enrol_batch_f32 are declared, bound and exported under ABI 106, their limits are
the header's, and bad sizes are refused before any launch (no GPU needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fr_gallery_first_above_blocked_f32", "fr_enrol_batch_f32", "fr_enrol_batch_workspace")


def _header():
    return open(os.path.join(ROOT, "include", "frhip.h")).read()


def _library():
    from facerecognition_infrenceengine_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_enrol_batch_entries_declared_bound_exported():
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
    assert int(re.search(r"#define FR_ABI_VERSION (\d+)", text).group(1)) == 106 == _lib.ABI_VERSION
    assert _lib.load().fr_version() == 106


def test_enrol_constants_are_the_headers():
    from facerecognition_infrenceengine_amd import enrol
    text = _header()
    for macro, value in (("FR_ENROL_DONE", enrol.ENROL_DONE), ("FR_ENROL_NO_FACE", enrol.ENROL_NO_FACE),
                         ("FR_ENROL_DIFFERENT", enrol.ENROL_DIFFERENT), ("FR_ENROL_DUPLICATE", enrol.ENROL_DUPLICATE),
                         ("FR_ENROL_MAX_POSES", enrol.ENROL_MAX_POSES), ("FR_ENROL_MAX_JOBS", enrol.ENROL_MAX_JOBS)):
        assert int(re.search(r"#define %s (\d+)" % macro, text).group(1)) == value
    assert enrol.ENROL_MAX_JOBS >= 256
    assert set(enrol.STATUS_NAMES.values()) == {"done", "no_face", "different_people", "duplicate"}


def _enrol(lib, p, J, max_poses, D, ws_bytes):
    return lib.fr_enrol_batch_f32(p, p, 8, p, p, 4, p, J, max_poses, D, p, None, 0, 0.4, 0.4, p, p, p, p, p, p, p, p,
                                  ws_bytes, None)


def test_enrol_batch_refuses_bad_sizes_before_any_launch():
    from facerecognition_infrenceengine_amd import enrol
    _lib = _library()
    lib = _lib.load()
    assert _enrol(lib, None, 0, 0, 512, 0) == 0                      # J == 0: nothing is read
    one = ctypes.c_void_p(16)                  # never dereferenced: the sizes are rejected before any launch
    big = lib.fr_enrol_batch_workspace(enrol.ENROL_MAX_JOBS + 1, 0)
    with pytest.raises(_lib.FrError, match="D must be 512"):
        _enrol(lib, one, 1, 1, 256, big)
    with pytest.raises(_lib.FrError, match="at most %d jobs" % enrol.ENROL_MAX_JOBS):
        _enrol(lib, one, enrol.ENROL_MAX_JOBS + 1, 1, 512, big)
    with pytest.raises(_lib.FrError, match="at most %d images a job" % enrol.ENROL_MAX_POSES):
        _enrol(lib, one, 1, enrol.ENROL_MAX_POSES + 1, 512, big)
    with pytest.raises(_lib.FrError, match="null pointer"):
        _enrol(lib, None, 1, 1, 512, big)
    with pytest.raises(_lib.FrError, match="workspace too small"):
        _enrol(lib, one, 1, 1, 512, 8)
    assert lib.fr_enrol_batch_workspace(4, 0) >= 4 * (8 + 4 + enrol.ENROL_MAX_JOBS // 8)


def test_blocked_scan_refuses_bad_sizes_before_any_launch():
    _lib = _library()
    lib = _lib.load()
    args = lambda p, F, N, D, wsb: (p, p, None, None, F, N, D, 0.4, 0, 0, p, p, p, wsb, None)
    assert lib.fr_gallery_first_above_blocked_f32(*args(None, 0, 5, 512, 0)) == 0
    one = ctypes.c_void_p(16)
    with pytest.raises(_lib.FrError, match="D must be 512"):
        lib.fr_gallery_first_above_blocked_f32(*args(one, 1, 5, 256, 8))
    with pytest.raises(_lib.FrError, match="bad argument"):
        lib.fr_gallery_first_above_blocked_f32(*args(one, 1, 1 << 31, 512, 8))
    with pytest.raises(_lib.FrError, match="workspace needs 16 bytes"):
        lib.fr_gallery_first_above_blocked_f32(*args(one, 2, 5, 512, 8))


def test_enrol_host_refuses_too_many_jobs_or_poses():
    """enrol_batch / enrol_slots raise ValueError before anything runs: no engine and no device is touched."""
    from facerecognition_infrenceengine_amd import enrol
    en = enrol.Enroller.__new__(enrol.Enroller)                     # no engine: the checks come first
    with pytest.raises(ValueError, match="jobs a batch"):
        en.enrol_batch([[None]] * (enrol.ENROL_MAX_JOBS + 1), None)
    with pytest.raises(ValueError, match="images a job"):
        en.enrol_batch([[None] * (enrol.ENROL_MAX_POSES + 1)], None)
    with pytest.raises(ValueError, match="jobs a batch"):
        en.enrol_slots({}, [[0]] * (enrol.ENROL_MAX_JOBS + 1), None)
    with pytest.raises(ValueError, match="images a job"):
        en.enrol_slots({}, [[0] * (enrol.ENROL_MAX_POSES + 1)], None)
    with pytest.raises(ValueError, match="GalleryView and ids"):
        en.enrol_batch([[None]], None, commit=True)
