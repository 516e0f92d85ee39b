"""Which C-ABI entries the gallery's host side launches, in what order and with what positional arguments, for every
form (matcher, view, view set, audit, decision, first_above) and scan kind - without a device: the library is a recorder,
the objects live on the CPU.  One argument out of place in these calls is a wrong answer on the GPU, not an error."""
import contextlib
import ctypes as C

import pytest
import torch

ANY = object()                 # a pointer slot whose tensor the call does not hand back (renormalised Q, workspace)
DIM, WS = 512, 64              # WS: what the recorder answers to every *_workspace query
K = 3


class Recorder:
    """Stands in for the loaded library: every fr_* attribute appends (name, args) - pointers as plain integers, a null
    pointer as None - and returns 64 for a workspace query, 0 otherwise."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("fr_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, tuple(a.value if isinstance(a, C.c_void_p) else a for a in args)))
            return WS if name.endswith("workspace") else 0
        return entry

    def take(self):
        calls, self.calls = self.calls, []
        return calls


@pytest.fixture
def rec(monkeypatch):
    from facerecognition_infrenceengine_amd import _lib
    rec = Recorder()
    monkeypatch.setattr(_lib, "require_gpu", lambda: None)
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    monkeypatch.setattr(torch.cuda, "device", lambda device=None: contextlib.nullcontext())
    return rec


def _p(t):
    return t.data_ptr() or None


def _same(call, name, *want):
    """``call`` is (name, args) with the given name; every slot of ``want`` that is a tensor is that tensor's pointer, ANY
    is not looked at, everything else compares equal (with its type: no float where an integer belongs)."""
    assert call[0] == name, (call[0], name)
    got = call[1]
    assert len(got) == len(want), (name, len(got), len(want))
    for n, (g, w) in enumerate(zip(got, want)):
        if w is ANY:
            assert g is not None, (name, n)
        elif torch.is_tensor(w):
            assert g == _p(w), (name, n, "pointer")
        else:
            assert g == w and type(g) is type(w), (name, n, g, w)


def _names(calls):
    return [c[0] for c in calls]


def _rows():
    return torch.eye(8, DIM)


def _queries(F=3):
    return torch.arange(F * DIM, dtype=torch.float32).reshape(F, DIM) + 1.0


def _matcher(rec, scan):
    from facerecognition_infrenceengine_amd.gallery import GalleryMatcher
    m = GalleryMatcher("cpu", scan=scan)
    m.set_rows([f"p{i}" for i in range(8)], _rows(), normalise=False)
    return m


def _gallery(rec, scan):
    from facerecognition_infrenceengine_amd.gallery import DeviceGallery
    g = DeviceGallery("cpu", capacity=4, scan=scan)
    g.upsert([f"p{i}" for i in range(8)], _rows())
    assert g.capacity == 8
    return g


SCANS = ("f32", "f16", "f8")
# what building the objects launches
SET_ROWS = {"f32": [], "f16": ["fr_f32_to_f16", "fr_gallery_gmax_update"], "f8": ["fr_f32_to_f8"]}
UPSERT = {"f32": ["fr_gallery_update_rows_f32"], "f16": ["fr_gallery_update_rows_shadow", "fr_gallery_gmax_update"],
          "f8": ["fr_gallery_update_rows_shadow"]}
# top-1, per scan kind: (workspace entry, scan entry)
MATCH = {"f32": ("fr_gallery_match_workspace", "fr_gallery_match_f32"),
         "f16": ("fr_gallery_match_f16_workspace", "fr_gallery_match_f16"),
         "f8": ("fr_gallery_match_f8_workspace", "fr_gallery_match_f8")}
MATCH_VIEW = {"f32": ("fr_gallery_match_workspace", "fr_gallery_match_view_f32"),
              "f16": ("fr_gallery_match_view_f16_workspace", "fr_gallery_match_view_f16"),
              "f8": ("fr_gallery_match_view_f8_workspace", "fr_gallery_match_view_f8")}
# top-K: the exact pair everywhere but scan="f16" with coarse_topk_min_rows reached
TOPK = {False: ("fr_gallery_topk_workspace", "fr_gallery_topk_f32"),
        True: ("fr_gallery_topk_f16_workspace", "fr_gallery_topk_f16")}
TOPK_VIEW = {False: ("fr_gallery_topk_workspace", "fr_gallery_topk_view_f32"),
             True: ("fr_gallery_topk_view_f16_workspace", "fr_gallery_topk_view_f16")}
GROUPED = {None: ("fr_gallery_match_grouped_workspace", "fr_gallery_match_grouped_f32"),
           K: ("fr_gallery_topk_grouped_workspace", "fr_gallery_topk_grouped_f32")}


@pytest.mark.parametrize("scan", SCANS)
def test_building_the_objects(rec, scan):
    from facerecognition_infrenceengine_amd.gallery import _SHADOW_KIND
    m = _matcher(rec, scan)
    calls = rec.take()
    assert _names(calls) == SET_ROWS[scan]
    if scan == "f16":
        _same(calls[0], "fr_f32_to_f16", m.G, m.G16, 8 * DIM, None)
        _same(calls[1], "fr_gallery_gmax_update", m.G, None, 8, DIM, m.gmax, None)
    if scan == "f8":
        _same(calls[0], "fr_f32_to_f8", m.G, m.G16, 8 * DIM, None)
    assert (m.G16 is None) == (scan == "f32") and (m.gmax is None) == (scan != "f16")
    g = _gallery(rec, scan)
    calls = rec.take()
    assert _names(calls) == UPSERT[scan]
    if scan == "f32":
        _same(calls[0], "fr_gallery_update_rows_f32", g.G, ANY, ANY, 8, DIM, 0, None)
    else:
        _same(calls[0], "fr_gallery_update_rows_shadow", g.G, g.S, _SHADOW_KIND[scan], ANY, ANY, 8, DIM, 0, None)
    if scan == "f16":
        _same(calls[1], "fr_gallery_gmax_update", g.G, ANY, 8, DIM, g.gmax, None)


@pytest.mark.parametrize("scan", SCANS)
def test_matcher_match_device(rec, scan):
    m = _matcher(rec, scan)
    rec.take()
    wsz, entry = MATCH[scan]
    coarse = () if scan == "f32" else (m.G16,)
    Q = _queries(3)
    idx, score = m.match_device(Q)
    calls = rec.take()
    assert _names(calls) == ["fr_l2norm_rows_f32", wsz, entry]
    _same(calls[0], "fr_l2norm_rows_f32", Q, ANY, 3, DIM, None)
    Qn = calls[0][1][1]
    assert calls[1][1] == (3, 8)
    _same(calls[2], entry, ANY, *coarse, m.G, 3, 8, DIM, 0, idx, score, ANY, WS, None, 0, None)
    assert calls[2][1][0] == Qn != _p(Q)                      # the scan reads the renormalised rows
    assert idx.shape == (3,) and idx.dtype == torch.int64 and score.shape == (3,) and score.dtype == torch.float32
    # renormalise=False, a row offset, padding counts
    counts = torch.tensor([2, 1], dtype=torch.int32)
    Q = _queries(4)
    idx, score = m.match_device(Q, renormalise=False, row_offset=5, counts=counts, seg_len=2)
    calls = rec.take()
    assert _names(calls) == [wsz, entry] and calls[0][1] == (4, 8)
    _same(calls[1], entry, Q, *coarse, m.G, 4, 8, DIM, 5, idx, score, ANY, WS, counts, 2, None)
    # F == 0: nothing is launched
    idx, score = m.match_device(Q[:0])
    assert rec.take() == []
    assert idx.shape == (0,) and idx.dtype == torch.int64 and score.shape == (0,) and score.dtype == torch.float32


@pytest.mark.parametrize("reached", [False, True])
@pytest.mark.parametrize("scan", SCANS)
def test_matcher_match_topk_device(rec, scan, reached):
    from facerecognition_infrenceengine_amd.gallery import last_topk
    m = _matcher(rec, scan)
    rec.take()
    m.coarse_topk_min_rows = 8 if reached else 9
    coarse = scan == "f16" and reached
    wsz, entry = TOPK[coarse]
    Q = _queries(3)
    idx, score = m.match_topk_device(Q, K)
    calls = rec.take()
    assert _names(calls) == ["fr_l2norm_rows_f32", wsz, entry]
    _same(calls[0], "fr_l2norm_rows_f32", Q, ANY, 3, DIM, None)
    assert calls[1][1] == (3, 8, K)
    info = last_topk()
    assert info["path"] == ("coarse" if coarse else "exact") and m.last_topk is info
    if coarse:
        assert info["flags"].shape == (3,) and info["flags"].dtype == torch.int32
        _same(calls[2], entry, ANY, m.G16, m.G, 3, 8, DIM, K, 0, m.gmax, idx, score, info["flags"], ANY, WS, None, 0, None)
    else:
        assert info["flags"] is None
        _same(calls[2], entry, ANY, m.G, 3, 8, DIM, K, 0, idx, score, ANY, WS, None, 0, None)
    assert calls[2][1][0] == calls[0][1][1]
    assert idx.shape == (3, K) and idx.dtype == torch.int64 and score.shape == (3, K) and score.dtype == torch.float32
    counts = torch.tensor([2, 1], dtype=torch.int32)
    Q = _queries(4)
    idx, score = m.match_topk_device(Q, K, renormalise=False, row_offset=5, counts=counts, seg_len=2)
    calls = rec.take()
    assert _names(calls) == [wsz, entry] and calls[0][1] == (4, 8, K)
    if coarse:
        _same(calls[1], entry, Q, m.G16, m.G, 4, 8, DIM, K, 5, m.gmax, idx, score, last_topk()["flags"], ANY, WS,
              counts, 2, None)
    else:
        _same(calls[1], entry, Q, m.G, 4, 8, DIM, K, 5, idx, score, ANY, WS, counts, 2, None)
    idx, score = m.match_topk_device(Q[:0], K)
    assert rec.take() == []
    assert idx.shape == (0, K) and idx.dtype == torch.int64 and score.shape == (0, K) and score.dtype == torch.float32
    assert last_topk() == {"path": "coarse" if coarse else "exact", "flags": None}


VIEW_IDS = ["p6", "p1", "p4", "nobody", "p0", "p7"]           # 5 of them are in the gallery


@pytest.mark.parametrize("scan", SCANS)
def test_view_match_device(rec, scan):
    g = _gallery(rec, scan)
    v = g.view(VIEW_IDS)
    rec.take()
    assert v.slots.tolist() == [6, 1, 4, 0, 7]
    wsz, entry = MATCH_VIEW[scan]
    Q = _queries(3)
    idx, score = v.match_device(Q)
    calls = rec.take()
    assert _names(calls) == ["fr_l2norm_rows_f32", wsz, entry]
    _same(calls[0], "fr_l2norm_rows_f32", Q, ANY, 3, DIM, None)
    assert calls[1][1] == (3, 5)
    if scan == "f32":
        _same(calls[2], entry, ANY, g.G, v.slots, 3, 5, DIM, idx, score, ANY, WS, None)
    else:
        _same(calls[2], entry, ANY, g.S, g.G, v.slots, 3, 5, 8, DIM, idx, score, ANY, WS, None)
    assert calls[2][1][0] == calls[0][1][1]
    idx, score = v.match_device(Q, renormalise=False)
    calls = rec.take()
    assert _names(calls) == [wsz, entry] and calls[1][1][0] == _p(Q)
    idx, score = v.match_device(Q[:0])
    assert rec.take() == []
    assert idx.shape == (0,) and idx.dtype == torch.int64 and score.shape == (0,) and score.dtype == torch.float32


@pytest.mark.parametrize("reached", [False, True])
@pytest.mark.parametrize("scan", SCANS)
def test_view_match_topk_device(rec, scan, reached):
    from facerecognition_infrenceengine_amd.gallery import last_topk
    g = _gallery(rec, scan)
    v = g.view(VIEW_IDS)
    rec.take()
    g.coarse_topk_min_rows = 5 if reached else 6
    coarse = scan == "f16" and reached
    wsz, entry = TOPK_VIEW[coarse]
    Q = _queries(3)
    idx, score = v.match_topk_device(Q, K)
    calls = rec.take()
    assert _names(calls) == ["fr_l2norm_rows_f32", wsz, entry]
    assert calls[1][1] == (3, 5, K)
    info = last_topk()
    assert info["path"] == ("coarse" if coarse else "exact") and v.last_topk is info
    if coarse:
        _same(calls[2], entry, ANY, g.S, g.G, v.slots, 3, 5, 8, DIM, K, g.gmax, idx, score, info["flags"], ANY, WS, None)
    else:
        assert info["flags"] is None
        _same(calls[2], entry, ANY, g.G, v.slots, 3, 5, DIM, K, idx, score, ANY, WS, None)
    assert calls[2][1][0] == calls[0][1][1]
    assert idx.shape == (3, K) and idx.dtype == torch.int64 and score.shape == (3, K) and score.dtype == torch.float32
    idx, score = v.match_topk_device(Q[:0], K, renormalise=False)
    assert rec.take() == []
    assert idx.shape == (0, K) and score.shape == (0, K) and score.dtype == torch.float32


@pytest.mark.parametrize("k", [None, K])
@pytest.mark.parametrize("scan", SCANS)
def test_view_set_is_always_the_grouped_exact_pair(rec, scan, k):
    from facerecognition_infrenceengine_amd.gallery import last_topk
    g = _gallery(rec, scan)
    g.coarse_topk_min_rows = 1
    v, w = g.view(VIEW_IDS), g.view(["p2", "p3"])
    vs = g.view_set([v, w])
    rec.take()
    assert vs.slots.tolist() == [6, 1, 4, 0, 7, 2, 3, 0]
    wsz, entry = GROUPED[k]
    kk = () if k is None else (k,)

    def scan_(Q, view_of, **kw):
        return vs.match_device(Q, view_of, **kw) if k is None else vs.match_topk_device(Q, view_of, k, **kw)
    Q = _queries(3)
    view_of = [1, 0, None]
    idx, score = scan_(Q, view_of)
    calls = rec.take()
    gtab, qmap, ngroups, longest = vs.tables(view_of, 3)
    assert (ngroups, longest) == (3, 5)
    assert _names(calls) == ["fr_l2norm_rows_f32", wsz, entry]
    _same(calls[0], "fr_l2norm_rows_f32", Q, ANY, 3, DIM, None)
    assert calls[1][1] == (3, 5) + kk
    _same(calls[2], entry, ANY, g.G, vs.slots, gtab, qmap, 3, 3, 5, 8, DIM, *kk, idx, score, ANY, WS, None, 0, None)
    assert calls[2][1][0] == calls[0][1][1]
    assert idx.shape == (3,) + kk and idx.dtype == torch.int64 and score.shape == (3,) + kk
    if k is not None:
        assert last_topk() == {"path": "exact", "flags": None} and vs.last_topk == last_topk()
    counts = torch.tensor([2, 1], dtype=torch.int32)
    Q = _queries(4)
    idx, score = scan_(Q, [0, 1], renormalise=False, counts=counts, seg_len=2)
    calls = rec.take()
    gtab, qmap, ngroups, longest = vs.tables([0, 1], 4, 2)
    assert _names(calls) == [wsz, entry] and calls[0][1] == (2, 5) + kk
    _same(calls[1], entry, Q, g.G, vs.slots, gtab, qmap, 4, 2, 5, 8, DIM, *kk, idx, score, ANY, WS, counts, 2, None)
    idx, score = scan_(Q[:0], [])
    assert rec.take() == []
    assert idx.shape == (0,) + kk and idx.dtype == torch.int64 and score.shape == (0,) + kk and score.dtype == torch.float32


@pytest.mark.parametrize("scan", SCANS)
def test_audit_and_decision(rec, scan):
    m, g = _matcher(rec, scan), _gallery(rec, scan)
    v = g.view(VIEW_IDS)
    vs = g.view_set([v])
    rec.take()
    keys, scores, counts = m.find_duplicates_device(0.5, True, 100, 7)
    calls = rec.take()
    assert _names(calls) == ["fr_gallery_pairs_workspace", "fr_gallery_pairs_above_f16"] and calls[0][1] == (8, 100)
    _same(calls[1], "fr_gallery_pairs_above_f16", m.G, None, 8, DIM, 0.5, 1, 100, 7, keys, scores, counts, ANY, WS, None)
    assert keys.shape == (100,) and keys.dtype == torch.int64 and scores.dtype == torch.float32 and counts.shape == (4,)
    keys, scores, counts = v.find_duplicates_device(max_pairs=10)
    calls = rec.take()
    assert _names(calls) == ["fr_gallery_pairs_workspace", "fr_gallery_pairs_above_f16"] and calls[0][1] == (5, 10)
    _same(calls[1], "fr_gallery_pairs_above_f16", g.G, v.slots, 5, DIM, 0.4, 0, 10, 0, keys, scores, counts, ANY, WS, None)
    with pytest.raises(ValueError, match="max_pairs"):
        m.find_duplicates_device(max_pairs=0)
    assert rec.take() == []
    idx, score = torch.zeros(3, dtype=torch.int64), torch.zeros(3)
    for obj, thr, unknown, want in ((m, 0.4, None, 0.4), (v, 0.5, 0.25, 0.25), (vs, 0.3, None, 0.3)):
        d = obj.decide_device(idx, score, thr, unknown)
        calls = rec.take()
        assert _names(calls) == ["fr_match_decide"]
        _same(calls[0], "fr_match_decide", idx, score, 3, thr, want, d, None)
        assert d.shape == (3,) and d.dtype == torch.int32
        assert obj.decide_device(idx[:0], score[:0], thr).shape == (0,) and rec.take() == []


@pytest.mark.parametrize("scan", SCANS)
def test_first_above(rec, scan):
    from facerecognition_infrenceengine_amd.enrol import first_above
    m, g = _matcher(rec, scan), _gallery(rec, scan)
    v = g.view(VIEW_IDS)
    rec.take()
    q = _queries(1)[0].numpy()
    first_above(rec, m, q, 0.4, inclusive=False)
    calls = rec.take()
    assert _names(calls) == ["fr_l2norm_rows_f32", "fr_gallery_first_above_f32"]
    assert calls[0][1][2:] == (1, DIM, None)
    _same(calls[1], "fr_gallery_first_above_f32", ANY, m.G, 1, 8, DIM, 0.4, 0, 0, ANY, ANY, ANY, 8, None)
    assert calls[1][1][0] == calls[0][1][1]
    first_above(rec, v, q, 0.25, inclusive=True)
    calls = rec.take()
    assert _names(calls) == ["fr_l2norm_rows_f32", "fr_gallery_first_above_blocked_f32"]
    _same(calls[1], "fr_gallery_first_above_blocked_f32", ANY, g.G, v.slots, None, 1, 5, DIM, 0.25, 1, 0, ANY, ANY, ANY,
          8, None)
    assert calls[1][1][0] == calls[0][1][1]


@pytest.mark.parametrize("scan", SCANS)
def test_stale_view_and_stale_set_launch_nothing(rec, scan):
    from facerecognition_infrenceengine_amd.enrol import first_above
    from facerecognition_infrenceengine_amd.gallery import GalleryViewSet, StaleViewError
    g = _gallery(rec, scan)
    v = g.view(VIEW_IDS)
    vs = g.view_set([v])
    g.upsert(["p8"], torch.ones(1, DIM))                      # a new id: the membership changed
    rec.take()
    Q = _queries(2)
    for call in (lambda: v.match_device(Q), lambda: v.match_topk_device(Q, K), lambda: v.find_duplicates_device(),
                 lambda: first_above(rec, v, Q[0].numpy(), 0.4, False), lambda: vs.match_device(Q, [0, 0]),
                 lambda: vs.match_topk_device(Q, [0, 0], K), lambda: g.view_set([v]), lambda: GalleryViewSet([v])):
        with pytest.raises(StaleViewError, match="is stale"):
            call()
        assert rec.take() == []
    with pytest.raises(ValueError, match="k must be 1..16"):  # k is judged first, on a stale view too
        v.match_topk_device(Q, 17)
    idx, score = g.view(VIEW_IDS).match_device(Q)             # a fresh view scans
    assert len(rec.take()) == 3
