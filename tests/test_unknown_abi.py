"""fr_unknown_assign_batch_f32 is declared, bound and exported, and an empty batch reads no pointer (no GPU needed)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fr_unknown_assign_batch_f32"


def test_unknown_assign_entry_declared_bound_exported():
    from facerecognition_infrenceengine_amd import _lib
    text = open(os.path.join(ROOT, "include", "frhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, code)
    assert m, f"{NAME} is not declared in include/frhip.h"
    nargs = len(m.group(1).split(","))
    res, args = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(args) == nargs <= 22          # the call struct of tests/test_abi.py holds 22 slots
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME), f"{NAME} is not exported by the built library"
    assert int(re.search(r"#define FR_ABI_VERSION (\d+)", text).group(1)) == 106 == _lib.ABI_VERSION
    # the state layout the Python side indexes with is the header's
    from facerecognition_infrenceengine_amd.enrol import UnknownClusters
    for macro, value in (("FR_UNKNOWN_N", UnknownClusters.STATE_N), ("FR_UNKNOWN_OVERFLOW", UnknownClusters.STATE_OVERFLOW),
                         ("FR_UNKNOWN_HEADER", UnknownClusters.STATE_HEADER)):
        assert int(re.search(r"#define %s (\d+)" % macro, text).group(1)) == value


def test_unknown_assign_empty_batch_reads_no_pointer():
    import pytest
    from facerecognition_infrenceengine_amd import _lib
    lib = _lib.load()
    assert lib.fr_unknown_assign_batch_f32(None, None, 0, 512, 0.65, None, None, None, 0, 0, None, None, None, None) == 0
    with pytest.raises(_lib.FrError, match="D must be 512"):
        lib.fr_unknown_assign_batch_f32(None, None, 1, 256, 0.65, None, None, None, 4, 10, None, None, None, None)
    with pytest.raises(_lib.FrError, match="null pointer"):
        lib.fr_unknown_assign_batch_f32(None, None, 1, 512, 0.65, None, None, None, 4, 10, None, None, None, None)
    one = ctypes.c_void_p(16)                  # never dereferenced: the sizes are rejected before any launch
    with pytest.raises(_lib.FrError, match="must be positive"):
        lib.fr_unknown_assign_batch_f32(one, None, 1, 512, 0.65, one, one, one, 4, 0, one, one, one, None)
