"""fr_yuv420_to_bgr_u8 and fr_yuv420_to_bgr_refs_u8 are declared, bound and exported under ABI 106, and bad arguments are refused
before any launch (no GPU needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fr_yuv420_to_bgr_u8", "fr_yuv420_to_bgr_refs_u8")
BT601 = (16, 1220542, 2116026, -409993, -852492, 1673527)


def _header():
    return open(os.path.join(ROOT, "include", "frhip.h")).read()


def _library():
    from facerecognition_infrenceengine_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_yuv_entries_declared_bound_exported():
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
    assert _lib.SIGNATURES["fr_yuv420_to_bgr_u8"] == (I, [P, P, I, I, I, I, I, I, I, I, I, I, P])
    assert _lib.SIGNATURES["fr_yuv420_to_bgr_refs_u8"] == (I, [P, P, I, I, I, I, I, I, I, I, P])
    assert int(re.search(r"#define FR_ABI_VERSION (\d+)", text).group(1)) == 106 == _lib.ABI_VERSION
    assert _lib.load().fr_version() == 106


def test_yuv_entries_are_listed_in_the_106_comment_and_layout_ids_agree():
    from facerecognition_infrenceengine_amd import colour
    text = _header()
    comment = text[:text.index("#define FR_ABI_VERSION")]
    comment = comment[comment.rindex("/*"):]
    assert "106:" in comment
    for name in NAMES:
        assert name in comment[comment.index("106:"):], name
    assert int(re.search(r"#define FR_YUV_NV12 (\d+)", text).group(1)) == colour.LAYOUTS["nv12"] == 0
    assert int(re.search(r"#define FR_YUV_I420 (\d+)", text).group(1)) == colour.LAYOUTS["i420"] == 1


def test_uniform_entry_refuses_bad_arguments_before_any_launch():
    _lib = _library()
    lib = _lib.load()
    one = ctypes.c_void_p(16)                  # never dereferenced: the arguments are rejected before any launch

    def call(src=one, dst=one, N=1, H=4, W=6, layout=0, consts=BT601):
        return lib.fr_yuv420_to_bgr_u8(src, dst, N, H, W, layout, *consts, None)
    for H, W in ((3, 4), (4, 3), (5, 7)):
        with pytest.raises(_lib.FrError, match="odd size"):
            call(H=H, W=W)
    for H, W in ((0, 4), (4, 0), (-2, 4)):
        with pytest.raises(_lib.FrError, match="bad size"):
            call(H=H, W=W)
    with pytest.raises(_lib.FrError, match="bad size"):
        call(N=-1)
    for layout in (-1, 2, 99):
        with pytest.raises(_lib.FrError, match="unknown layout"):
            call(layout=layout)
    with pytest.raises(_lib.FrError, match="null pointer"):
        call(src=None)
    with pytest.raises(_lib.FrError, match="null pointer"):
        call(dst=None)
    with pytest.raises(_lib.FrError, match="beyond 2 GiB"):
        call(H=32768, W=32768)                 # 3 GiB of BGR
    with pytest.raises(_lib.FrError, match="beyond 2 GiB"):
        call(H=2, W=357913942)                 # H*W*3 = 2^31 + 4: the first even width past the limit
    with pytest.raises(_lib.FrError, match="bad constants"):
        call(consts=(16, 1 << 24, 0, 0, 0, 0))                     # 255 CY alone leaves int32
    with pytest.raises(_lib.FrError, match="bad constants"):
        call(consts=(16, 1220542, 1 << 24, 0, 0, 0))
    with pytest.raises(_lib.FrError, match="bad constants"):
        call(consts=(256, 1220542, 2116026, -409993, -852492, 1673527))
    # N = 0: FR_OK, nothing is read - not even the pointers
    assert call(src=None, dst=None, N=0) == 0
    assert call(N=0, layout=1) == 0
    with pytest.raises(_lib.FrError, match="odd size"):
        call(src=None, dst=None, N=0, H=3)     # a shape no conversion exists for stays an error


def test_conversion_kernels_hold_no_packed_shift_saturate(tmp_path):
    """csrc/yuv_to_bgr.hip sat8s: from clamp(v >> 20, 0, 255) on two neighbouring bytes hipcc forms gfx950's v_ashr_pk_u8_i32
    and then takes the upper 16 bits of its result for zero; on the MI355X they are not, and the bytes packed above came out
    wrong.  The kernels clamp before they shift; this disassembles them and checks that the instruction stays away."""
    import shutil
    import subprocess
    _lib = _library()
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("llvm-objdump not available")
    so = shutil.copy(_lib.LIB_PATH, tmp_path / "libfrhip.so")
    subprocess.run([objdump, "--offloading", str(so)], cwd=tmp_path, check=True, capture_output=True)
    cos = [f for f in os.listdir(tmp_path) if "amdgcn" in f]
    assert cos, "no device code objects found in libfrhip.so"
    seen = 0
    for f in cos:
        asm = subprocess.run([objdump, "-d", str(tmp_path / f)], capture_output=True, text=True, check=True).stdout
        for body in re.split(r"\n(?=[0-9a-f]+ <[^>]+>:)", asm):
            head = body.split("\n", 1)[0]
            if "yuv420_to_bgr" in head:
                seen += 1
                assert "global_store_dwordx4" in body or "flat_store_dwordx4" in body, head     # it is the kernel
                assert "v_ashr_pk_u8_i32" not in body, head
    assert seen == 2                             # the uniform and the table kernel


def test_table_entry_refuses_bad_arguments_before_any_launch():
    _lib = _library()
    lib = _lib.load()
    one = ctypes.c_void_p(16)

    def call(refs=one, srcs=one, n=1, layout=1, consts=BT601):
        return lib.fr_yuv420_to_bgr_refs_u8(refs, srcs, n, layout, *consts, None)
    with pytest.raises(_lib.FrError, match="unknown layout"):
        call(layout=2)
    with pytest.raises(_lib.FrError, match="null pointer"):
        call(refs=None)
    with pytest.raises(_lib.FrError, match="null pointer"):
        call(srcs=None)
    with pytest.raises(_lib.FrError, match="bad size"):
        call(n=-1)
    with pytest.raises(_lib.FrError, match="bad size"):
        call(n=65536)
    with pytest.raises(_lib.FrError, match="bad constants"):
        call(consts=(0, -1, 0, 0, 0, 0))
    assert call(refs=None, srcs=None, n=0) == 0
    assert call(n=0, layout=0) == 0
