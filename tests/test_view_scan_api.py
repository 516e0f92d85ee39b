"""The coarse view scan's host surface, without a device: EmbeddingManager(scan=...), the header and the binding."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("fr_gallery_match_view_f16", "fr_gallery_match_view_f16_workspace",
               "fr_gallery_match_view_f8", "fr_gallery_match_view_f8_workspace")


def _store():
    from facerecognition_infrenceengine_amd.processor import InMemoryStore
    store = InMemoryStore()
    rng = np.random.default_rng(0)
    for i in range(3):
        store.add_employee(f"e{i}", "acme", rng.standard_normal(512).astype(np.float32))
    return store


def test_embedding_manager_rejects_an_unknown_scan():
    from facerecognition_infrenceengine_amd.processor import EmbeddingManager
    with pytest.raises(ValueError, match="scan must be"):
        EmbeddingManager(store=_store(), scan="f9")


@pytest.mark.parametrize("scan", ["f32", "f16", "f8"])
def test_embedding_manager_takes_scan_without_a_device(scan):
    """Construction ingests the store on the host only; the device slab is made at the first get_matcher_for_company."""
    from facerecognition_infrenceengine_amd.processor import EmbeddingManager
    mgr = EmbeddingManager(store=_store(), device="cuda:0", scan=scan)
    assert mgr.scan == scan and mgr._gallery is None and len(mgr.embeddings) == 3


def test_embedding_manager_default_scan_is_f32():
    from facerecognition_infrenceengine_amd.processor import EmbeddingManager
    assert EmbeddingManager(store=_store()).scan == "f32"


def test_device_gallery_validates_scan_before_any_device_work():
    from facerecognition_infrenceengine_amd.gallery import DeviceGallery
    with pytest.raises(ValueError, match="scan must be"):
        DeviceGallery("cuda:0", capacity=8, scan="bf16")


def test_header_declares_the_view_scan_entries_and_the_binding_has_them():
    from facerecognition_infrenceengine_amd import _lib
    text = open(os.path.join(ROOT, "include", "frhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_ENTRIES + ("fr_gallery_update_rows_shadow",):
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared in frhip.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert int(re.search(r"#define FR_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == 106
    # the scan entries: (Q, S, G32, view, F, Nview, capacity, D, out_idx, out_score, workspace, bytes, stream)
    for name in ("fr_gallery_match_view_f16", "fr_gallery_match_view_f8"):
        res, args = _lib.SIGNATURES[name]
        assert res is _lib._I and args == [_lib._P] * 4 + [_lib._I, _lib._L, _lib._L, _lib._I] + [_lib._P] * 3 + [_lib._Z, _lib._P]
    assert "2^31" in text and "capacity" in text          # the supported size is stated where the entries are declared


def test_library_exports_the_entries_and_refuses_bad_arguments():
    """Argument checks come before any launch, so they run without a device."""
    import ctypes as C
    from facerecognition_infrenceengine_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(16)                   # never dereferenced
    for kind in ("f16", "f8"):
        fn = getattr(lib, f"fr_gallery_match_view_{kind}")
        wsz = getattr(lib, f"fr_gallery_match_view_{kind}_workspace")
        assert wsz(256, 1_000_000) > 0 and wsz(1, 0) > 0
        with pytest.raises(_lib.FrError, match="capacity .* must be below 2\\^31"):
            fn(one, one, one, one, 1, 10, 1 << 31, 512, one, one, one, 1 << 30, None)
        with pytest.raises(_lib.FrError, match="hold the view"):
            fn(one, one, one, one, 1, 10, 5, 512, one, one, one, 1 << 30, None)
        with pytest.raises(_lib.FrError, match="D must be 512"):
            fn(one, one, one, one, 1, 10, 16, 128, one, one, one, 1 << 30, None)
        with pytest.raises(_lib.FrError, match="null view"):
            fn(one, one, one, None, 1, 10, 16, 512, one, one, one, 1 << 30, None)
        with pytest.raises(_lib.FrError, match="workspace too small"):
            fn(one, one, one, one, 1, 10, 16, 512, one, one, one, 8, None)
        assert fn(None, None, None, None, 0, 10, 16, 512, None, None, None, 0, None) == 0      # F == 0: nothing to do
    with pytest.raises(_lib.FrError, match="shadow_kind"):
        lib.fr_gallery_update_rows_shadow(one, one, 3, one, one, 2, 512, 0, None)
    with pytest.raises(_lib.FrError, match="null pointer"):
        lib.fr_gallery_update_rows_shadow(one, None, 1, one, one, 2, 512, 0, None)
    assert lib.fr_gallery_update_rows_shadow(None, None, 2, None, None, 0, 512, 0, None) == 0
