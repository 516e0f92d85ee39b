"""The grouped view scan's host surface, without a device: the header, the binding, the argument checks of the two
entries (all before any launch) and the table building of GalleryViewSet (a pure host function)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fr_gallery_match_grouped_f32", "fr_gallery_match_grouped_workspace",
           "fr_gallery_topk_grouped_f32", "fr_gallery_topk_grouped_workspace")


def test_header_declares_the_grouped_entries_and_the_binding_has_them():
    from facerecognition_infrenceengine_amd import _lib
    text = open(os.path.join(ROOT, "include", "frhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared in frhip.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert name in text.split("#define FR_ABI_VERSION")[0] or name.endswith("_workspace")   # the 106 comment lists them
    assert int(re.search(r"#define FR_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == 106
    P, I, L, Z = _lib._P, _lib._I, _lib._L, _lib._Z
    # (Q, G, views, gtab, qmap, F, ngroups, max_view_len, capacity, D, [K,] out_idx, out_score, ws, bytes, seg_counts, seg_len, stream)
    assert _lib.SIGNATURES["fr_gallery_match_grouped_f32"] == (I, [P] * 5 + [I, I, L, L, I] + [P] * 3 + [Z, P, I, P])
    assert _lib.SIGNATURES["fr_gallery_topk_grouped_f32"] == (I, [P] * 5 + [I, I, L, L, I, I] + [P] * 3 + [Z, P, I, P])
    assert _lib.SIGNATURES["fr_gallery_match_grouped_workspace"] == (Z, [I, L])
    assert _lib.SIGNATURES["fr_gallery_topk_grouped_workspace"] == (Z, [I, L, I])
    for word in ("gtab", "qmap", "views", "max_view_len", "NOT WRITTEN"):      # the table layouts are spelt out
        assert word in text, word


def test_library_refuses_bad_arguments_before_any_launch():
    from facerecognition_infrenceengine_amd import _lib
    lib = _lib.load()
    assert lib.fr_version() == 106
    one = C.c_void_p(16)                   # never dereferenced
    big = 1 << 30

    def top1(Q=one, G=one, views=one, gtab=one, qmap=one, F=8, ngroups=2, longest=10, capacity=64, D=512, out_idx=one,
             out_score=one, ws=one, ws_bytes=big, counts=None, seg_len=0):
        return lib.fr_gallery_match_grouped_f32(Q, G, views, gtab, qmap, F, ngroups, longest, capacity, D, out_idx,
                                                out_score, ws, ws_bytes, counts, seg_len, None)

    def topk(K=5, Q=one, G=one, views=one, gtab=one, qmap=one, F=8, ngroups=2, longest=10, capacity=64, D=512,
             out_idx=one, out_score=one, ws=one, ws_bytes=big, counts=None, seg_len=0):
        return lib.fr_gallery_topk_grouped_f32(Q, G, views, gtab, qmap, F, ngroups, longest, capacity, D, K, out_idx,
                                               out_score, ws, ws_bytes, counts, seg_len, None)

    for fn in (top1, topk):
        with pytest.raises(_lib.FrError, match="D must be 512"):
            fn(D=128)
        for null in ("Q", "G", "views", "gtab", "qmap", "out_idx", "out_score"):
            with pytest.raises(_lib.FrError, match="null pointer"):
                fn(**{null: None})
        with pytest.raises(_lib.FrError, match="workspace too small"):
            fn(ws_bytes=8)
        with pytest.raises(_lib.FrError, match="workspace too small"):
            fn(ws=None)
        with pytest.raises(_lib.FrError, match="seg_len must divide F"):
            fn(counts=one, seg_len=3)
        with pytest.raises(_lib.FrError, match="seg_len must divide F"):
            fn(counts=one, seg_len=0)
        with pytest.raises(_lib.FrError, match="capacity .* must be below 2\\^31"):
            fn(capacity=1 << 31)
        assert fn(F=0, Q=None, G=None, views=None, gtab=None, qmap=None, out_idx=None, out_score=None, ws=None,
                  ws_bytes=0) == 0                                              # F == 0: nothing to do
        assert fn(ngroups=0, Q=None, G=None, views=None, gtab=None, qmap=None, out_idx=None, out_score=None, ws=None,
                  ws_bytes=0) == 0                                              # no group: nothing to do
    for K in (0, 17, -1):
        with pytest.raises(_lib.FrError, match="K must be 1..16"):
            topk(K=K)
    # the workspace holds the partial results of ngroups * 32 entries, as the plain entries' of F queries
    assert lib.fr_gallery_match_grouped_workspace(3, 1000) == lib.fr_gallery_match_workspace(96, 1000)
    assert lib.fr_gallery_topk_grouped_workspace(3, 1000, 5) == lib.fr_gallery_topk_workspace(96, 1000, 5)
    with pytest.raises(_lib.FrError, match="workspace too small"):
        top1(ws_bytes=lib.fr_gallery_match_grouped_workspace(2, 10) - 1)
    with pytest.raises(_lib.FrError, match="workspace too small"):
        topk(ws_bytes=lib.fr_gallery_topk_grouped_workspace(2, 10, 5) - 1)


def _check_tables(view_of, F, seg_len, lengths):
    from facerecognition_infrenceengine_amd.gallery import build_group_tables
    offsets = np.concatenate([[0], np.cumsum(lengths)])[:-1]
    gtab, qmap, longest = build_group_tables(view_of, F, seg_len, offsets, lengths)
    assert gtab.dtype == np.int64 and gtab.ndim == 2 and gtab.shape[1] == 2 and qmap.dtype == np.int32
    assert qmap.shape == (gtab.shape[0] * 32,)
    mapped = qmap[qmap >= 0]
    assert sorted(mapped.tolist()) == list(range(F))                # every slot exactly once
    per_slot = np.repeat(np.asarray(view_of), seg_len) if seg_len else np.asarray(view_of)
    for g in range(gtab.shape[0]):
        slots = qmap[g * 32:(g + 1) * 32]
        slots = slots[slots >= 0]
        assert 1 <= len(slots) <= 32 and (np.diff(slots) > 0).all()      # at most 32, in slot order
        v = set(per_slot[slots].tolist())
        assert len(v) == 1                                          # a group never mixes views
        v = v.pop()
        assert tuple(gtab[g]) == ((0, 0) if v < 0 else (offsets[v], lengths[v]))
    assert longest == max([lengths[v] for v in set(per_slot.tolist()) if v >= 0], default=0)
    return gtab, qmap


def test_group_tables_cover_every_slot_once_and_never_mix_views():
    lengths = [0, 1, 33, 130]
    _check_tables([f % 4 for f in range(70)], 70, 0, lengths)                       # round-robin: gathered slots
    _check_tables(np.random.default_rng(0).permutation([f % 4 for f in range(70)]).tolist(), 70, 0, lengths)
    _check_tables(sorted(f % 4 for f in range(70)), 70, 0, lengths)                 # contiguous
    gtab, qmap = _check_tables([2] * 33, 33, 0, lengths)                            # 33 slots of one view: two groups
    assert gtab.shape[0] == 2 and (qmap[32:] >= 0).sum() == 1 and (gtab == gtab[0]).all()
    gtab, _ = _check_tables([3, 1, 3, -1, 0, 3], 24, 4, lengths)                    # per segment; -1: no view -> (0, 0)
    assert gtab.shape[0] == 4
    gtab, _ = _check_tables([1] * 9, 9 * 16, 16, lengths)                           # 144 slots of one view: 5 groups
    assert gtab.shape[0] == 5
    gtab, qmap = _check_tables([], 0, 0, lengths)
    assert gtab.shape == (0, 2) and qmap.shape == (0,)


def test_group_tables_refuse_a_wrong_view_of():
    from facerecognition_infrenceengine_amd.gallery import build_group_tables
    with pytest.raises(ValueError, match="per query"):
        build_group_tables([0, 1], 3, 0, [0, 4], [4, 4])
    with pytest.raises(ValueError, match="per segment"):
        build_group_tables([0, 1], 12, 4, [0, 4], [4, 4])
    with pytest.raises(ValueError, match="outside"):
        build_group_tables([0, 2], 2, 0, [0, 4], [4, 4])
    gtab, qmap, longest = build_group_tables([None, 1], 2, 0, [0, 4], [4, 4])       # None: no view
    assert gtab.tolist() == [[0, 0], [4, 4]] and qmap[0] == 0 and qmap[32] == 1 and longest == 4
