"""The grouped view scan on the GPU (GalleryViewSet -> fr_gallery_match_grouped_f32 / fr_gallery_topk_grouped_f32): every
query of a batch through ITS OWN view, bit for bit what the view's own scan returns for that query alone, and against the
float64 reference of tests/helpers/topk_ref.py.

One gallery of 300 seeded unit rows; views of 0, 1, 33 and 130 rows (an empty view, a single row, a tail tile, five tiles
over two scan blocks), overlapping, in shuffled slot orders, one of them holding a row twice.  70 queries dealt
round-robin over the deck (0, 3, 1, 3, 2, 3): gathered, non-adjacent slots for every view, and view 3 gets 35 queries,
so two groups."""
import numpy as np
import pytest
import torch

from oracle import match as omatch
from tests.helpers import topk_ref as ref

pytestmark = pytest.mark.gpu

N, F = 300, 70
DECK = (0, 3, 1, 3, 2, 3)
LENGTHS = (0, 1, 33, 130)
ONE = 7                          # the row of the 1-row view: a one-hot row, so that -row scores exactly -1.0
DUP = 11                         # the row view 3 holds twice
SHARED = 23                      # a row views 2 and 3 both hold, at different positions
MINUS1 = np.float32(-1.0)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def _view_rows():
    """the gallery rows of each view, in view order"""
    rng = np.random.default_rng(5)
    pool = [r for r in rng.permutation(N).tolist() if r not in (ONE, DUP, SHARED)]
    v2 = pool[:31] + [ONE, SHARED]                          # row ONE also sits in view 1, at another position
    v2 = [v2[i] for i in rng.permutation(33)]
    v3 = pool[20:20 + 127] + [SHARED, DUP, DUP]             # 11 rows of view 2 again, the shared row, one row twice
    v3 = [v3[i] for i in rng.permutation(130)]
    assert v2.index(SHARED) != v3.index(SHARED) and v3.count(DUP) == 2 and len(set(v2) & set(v3)) >= 12
    return [[], [ONE], v2, v3]


def _gallery(scan, G, rows):
    from facerecognition_infrenceengine_amd.gallery import DeviceGallery
    g = DeviceGallery("cuda:0", capacity=512, scan=scan)
    order = np.random.default_rng(3).permutation(N)          # slots are not the row numbers
    g.upsert([f"r{i}" for i in order], G[order], normalise=False)
    views = [g.view([f"r{i}" for i in v]) for v in rows]
    assert [len(v) for v in views] == list(LENGTHS)
    return g, views


@pytest.fixture(scope="module")
def world():
    G, Q = ref.seeded_case(41, N, F)
    G[ONE] = 0.0
    G[ONE, 100] = 1.0
    rows = _view_rows()
    view_of = np.asarray([DECK[f % len(DECK)] for f in range(F)])
    assert (view_of == 3).sum() == 35                        # more than 32 queries of one view: two groups
    rng = np.random.default_rng(8)
    scale = rng.uniform(0.5, 2.0, F).astype(np.float32)
    planted = {}                                             # query -> position in its view
    for v in (2, 3):
        for f in np.nonzero(view_of == v)[0][:6]:
            pos = int(rng.integers(0, LENGTHS[v]))
            while rows[v][pos] in (DUP, SHARED, ONE):
                pos = int(rng.integers(0, LENGTHS[v]))
            Q[f] = (G[rows[v][pos]] + 0.02 * rng.standard_normal(512).astype(np.float32)) * scale[f]
            planted[int(f)] = pos
    ties = {}
    q3 = np.nonzero(view_of == 3)[0]
    q2 = np.nonzero(view_of == 2)[0]
    q1 = np.nonzero(view_of == 1)[0]
    ties["dup"] = int(q3[-1]); Q[q3[-1]] = G[DUP] * scale[q3[-1]]               # equals a row view 3 holds twice
    ties["shared3"] = int(q3[-2]); Q[q3[-2]] = G[SHARED] * scale[q3[-2]]        # a row of two views, asked in each
    ties["shared2"] = int(q2[-1]); Q[q2[-1]] = G[SHARED] * scale[q2[-1]]
    ties["minus"] = int(q1[-1]); Q[q1[-1]] = -G[ONE] * np.float32(2.0)          # exactly -1.0 after the renormalise
    g, views = _gallery("f32", G, rows)
    vs = g.view_set(views)
    Qd = torch.from_numpy(Q).cuda()
    want_idx, want_score = np.full(F, -9, np.int64), np.full(F, np.nan, np.float32)
    for v in range(4):                                       # the reference: every view's own scan of its own queries
        sel = np.nonzero(view_of == v)[0]
        i, s = views[v].match_device(Qd[torch.from_numpy(sel).cuda()])
        want_idx[sel], want_score[sel] = i.cpu().numpy(), s.cpu().numpy()
    return dict(G=G, Q=Q, Qd=Qd, rows=rows, view_of=view_of, planted=planted, ties=ties, g=g, views=views, vs=vs,
                want_idx=want_idx, want_score=want_score)


def _same(got, want_idx, want_score, sel=slice(None)):
    idx, score = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert idx.dtype == np.int64 and score.dtype == np.float32
    assert np.array_equal(idx[sel], want_idx[sel])
    assert np.array_equal(_bits(score[sel]), _bits(want_score[sel]))
    return idx, score


def test_top1_equals_each_views_own_scan_bit_for_bit(world):
    w = world
    _same(w["vs"].match_device(w["Qd"], w["view_of"].tolist()), w["want_idx"], w["want_score"])
    # the same queries in another slot order: other groups, other lanes - the same bits per query
    for perm in (np.random.default_rng(2).permutation(F), np.argsort(w["view_of"], kind="stable")):
        got = w["vs"].match_device(w["Qd"][torch.from_numpy(perm).cuda()], w["view_of"][perm].tolist())
        _same(got, w["want_idx"][perm], w["want_score"][perm])
    contiguous = w["view_of"][np.argsort(w["view_of"], kind="stable")]
    assert (np.diff(contiguous) >= 0).all()                  # the second order: the queries of every view adjacent
    # without the renormalise, on unit queries: still each view's own bits
    Qn = torch.nn.functional.normalize(w["Qd"], dim=1)
    want_i, want_s = np.empty(F, np.int64), np.empty(F, np.float32)
    for v in range(4):
        sel = np.nonzero(w["view_of"] == v)[0]
        i, s = w["views"][v].match_device(Qn[torch.from_numpy(sel).cuda()], renormalise=False)
        want_i[sel], want_s[sel] = i.cpu().numpy(), s.cpu().numpy()
    _same(w["vs"].match_device(Qn, w["view_of"].tolist(), renormalise=False), want_i, want_s)
    # queries without a view (None) report (-1, -1.0) and disturb no one
    of = [None if f % 5 == 0 else int(v) for f, v in enumerate(w["view_of"])]
    idx, score = (t.cpu().numpy() for t in w["vs"].match_device(w["Qd"], of))
    none = np.asarray([v is None for v in of])
    assert (idx[none] == -1).all() and (score[none] == MINUS1).all()
    assert np.array_equal(idx[~none], w["want_idx"][~none]) and np.array_equal(_bits(score[~none]), _bits(w["want_score"][~none]))


def test_exact_ties_follow_each_views_own_order(world):
    w = world
    idx, score = (t.cpu().numpy() for t in w["vs"].match_device(w["Qd"], w["view_of"].tolist()))
    rows, t = w["rows"], w["ties"]
    first, second = [p for p, r in enumerate(rows[3]) if r == DUP]
    assert idx[t["dup"]] == first < second                   # the duplicated row: its lower position
    assert idx[t["shared2"]] == rows[2].index(SHARED) and idx[t["shared3"]] == rows[3].index(SHARED)
    assert rows[2].index(SHARED) != rows[3].index(SHARED)     # one row, each view's own position
    assert _bits(score[t["shared2"]]) != _bits(np.float32(-1)) and abs(score[t["shared2"]] - 1) < 1e-6
    assert idx[t["minus"]] == -1 and score[t["minus"]] == MINUS1      # -row scores exactly -1.0: not '> -1'
    empty = w["view_of"] == 0
    assert (idx[empty] == -1).all() and (score[empty] == MINUS1).all()


def test_top1_against_the_float64_reference(world):
    w = world
    idx, score = (t.cpu().numpy() for t in w["vs"].match_device(w["Qd"], w["view_of"].tolist()))
    for v in (1, 2, 3):
        sel = np.nonzero(w["view_of"] == v)[0]
        # the query that equals the row view 3 holds twice is an exact tie of ranks 0 and 1: the reference rule calls
        # such a position ambiguous, and one of 35 is past its cap of 2 % - that query is pinned exactly by the tie test
        sel = sel[sel != w["ties"]["dup"]]
        Gv = w["G"][w["rows"][v]]
        S = ref.scores64(w["Q"][sel], Gv)
        ref.check(idx[sel, None], score[sel, None], S, 1)
        oi, _ = omatch.match_rows(w["Q"][sel], Gv)
        for k, f in enumerate(sel):
            if int(f) in w["planted"]:
                assert idx[f] == w["planted"][int(f)] == oi[k] and score[f] > 0.5
    assert len(w["planted"]) == 12


def test_padding_slots_and_empty_segments(world):
    w = world
    seg_len, nseg = 4, 17
    Fp = seg_len * nseg                                      # the first 68 queries, 17 segments of 4 slots
    seg_view = np.asarray([DECK[s % len(DECK)] for s in range(nseg)])
    counts = np.asarray([(0, 1, 4)[s % 3] for s in range(nseg)], np.int32)
    slot_view = np.repeat(seg_view, seg_len)
    real = (np.arange(Fp) % seg_len) < np.repeat(counts, seg_len)
    assert real.sum() and (~real).sum() and set(counts[seg_view == 3]) == {0, 1, 4}
    Qd = w["Qd"][:Fp]
    want_idx, want_score = np.full(Fp, -1, np.int64), np.full(Fp, -1.0, np.float32)
    for v in range(4):
        sel = np.nonzero((slot_view == v) & real)[0]
        if len(sel):
            i, s = w["views"][v].match_device(Qd[torch.from_numpy(sel).cuda()])
            want_idx[sel], want_score[sel] = i.cpu().numpy(), s.cpu().numpy()
    cd = torch.from_numpy(counts).cuda()
    idx, score = _same(w["vs"].match_device(Qd, seg_view.tolist(), counts=cd, seg_len=seg_len), want_idx, want_score)
    assert (idx[~real] == -1).all() and (score[~real] == MINUS1).all()
    # padding rows are never read: NaN there changes nothing anywhere
    Qnan = Qd.clone()
    Qnan[torch.from_numpy(~real).cuda()] = float("nan")
    _same(w["vs"].match_device(Qnan, seg_view.tolist(), counts=cd, seg_len=seg_len), want_idx, want_score)
    got = w["vs"].match_topk_device(Qnan, seg_view.tolist(), 3, counts=cd, seg_len=seg_len)
    assert np.array_equal(got[0][:, 0].cpu().numpy(), want_idx) and np.array_equal(_bits(got[1][:, 0].cpu().numpy()), _bits(want_score))
    assert (got[0][torch.from_numpy(~real).cuda()] == -1).all() and (got[1][torch.from_numpy(~real).cuda()] == -1.0).all()
    # a view whose segments are all empty: its groups find no work and report padding; the others are as before
    c2 = counts.copy()
    c2[seg_view == 3] = 0
    real2 = (np.arange(Fp) % seg_len) < np.repeat(c2, seg_len)
    w2i, w2s = np.where(real2, want_idx, -1), np.where(real2, want_score, MINUS1)
    idx, score = _same(w["vs"].match_device(Qnan, seg_view.tolist(), counts=torch.from_numpy(c2).cuda(), seg_len=seg_len), w2i, w2s)
    assert (idx[slot_view == 3] == -1).all() and (score[slot_view == 3] == MINUS1).all()


@pytest.mark.parametrize("K", [1, 3, 5, 16])
def test_topk_equals_each_views_own_topk_bit_for_bit(world, K):
    w = world
    want_idx, want_score = np.empty((F, K), np.int64), np.empty((F, K), np.float32)
    for v in range(4):
        sel = np.nonzero(w["view_of"] == v)[0]
        i, s = w["views"][v].match_topk_device(w["Qd"][torch.from_numpy(sel).cuda()], K)
        want_idx[sel], want_score[sel] = i.cpu().numpy(), s.cpu().numpy()
    idx, score = _same(w["vs"].match_topk_device(w["Qd"], w["view_of"].tolist(), K), want_idx, want_score)
    assert idx.shape == (F, K)
    assert np.array_equal(idx[:, 0], w["want_idx"]) and np.array_equal(_bits(score[:, 0]), _bits(w["want_score"]))
    for v in range(4):                                       # views shorter than K end in (-1, -1.0)
        sel, n = w["view_of"] == v, LENGTHS[v]
        assert (idx[sel][:, min(n, K):] == -1).all() and (score[sel][:, min(n, K):] == MINUS1).all()
    if K > 1:
        sel = (w["view_of"] == 3) | (w["view_of"] == 2)
        assert (idx[sel][:, :min(K, 33)] >= 0).all()         # and the others are filled
    perm = np.random.default_rng(4).permutation(F)
    _same(w["vs"].match_topk_device(w["Qd"][torch.from_numpy(perm).cuda()], w["view_of"][perm].tolist(), K),
          want_idx[perm], want_score[perm])


def test_coarse_gallery_runs_the_exact_scan(world, lib):
    """On a scan="f16" gallery the set still scans the f32 slab: the ids the coarse view scan gives, the exact bits."""
    from facerecognition_infrenceengine_amd import _lib
    from facerecognition_infrenceengine_amd.gallery import last_topk
    w = world
    g, views = _gallery("f16", w["G"], w["rows"])
    vs = g.view_set(views)
    idx, score = (t.cpu().numpy() for t in vs.match_device(w["Qd"], w["view_of"].tolist()))
    Qn = torch.empty_like(w["Qd"])
    lib.fr_l2norm_rows_f32(_lib.ptr(w["Qd"]), _lib.ptr(Qn), F, 512, _lib.stream_ptr())
    for v in range(4):
        sel = np.nonzero(w["view_of"] == v)[0]
        seld = torch.from_numpy(sel).cuda()
        ci, _ = views[v].match_device(w["Qd"][seld])                     # the coarse scan + exact re-rank
        assert np.array_equal(idx[sel], ci.cpu().numpy())
        q = Qn[seld].contiguous()
        ei = torch.empty(len(sel), dtype=torch.int64, device="cuda")
        es = torch.empty(len(sel), dtype=torch.float32, device="cuda")
        ws = torch.empty(lib.fr_gallery_match_workspace(len(sel), len(views[v])), dtype=torch.uint8, device="cuda")
        lib.fr_gallery_match_view_f32(_lib.ptr(q), _lib.ptr(g.G), _lib.ptr(views[v].slots), len(sel), len(views[v]), 512,
                                      _lib.ptr(ei), _lib.ptr(es), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
        assert np.array_equal(idx[sel], ei.cpu().numpy()) and np.array_equal(_bits(score[sel]), _bits(es.cpu().numpy()))
    assert np.array_equal(idx, w["want_idx"]) and np.array_equal(_bits(score), _bits(w["want_score"]))
    g.coarse_topk_min_rows = 1                                           # views would take the coarse top-K path ...
    ti, ts = vs.match_topk_device(w["Qd"], w["view_of"].tolist(), 5)
    assert last_topk()["path"] == "exact" and vs.last_topk["flags"] is None      # ... the set does not
    assert np.array_equal(ti[:, 0].cpu().numpy(), idx) and np.array_equal(_bits(ts[:, 0].cpu().numpy()), _bits(score))


def test_stale_sets_and_foreign_views_are_refused(world):
    from facerecognition_infrenceengine_amd.gallery import DeviceGallery, GalleryViewSet, StaleViewError
    w = world
    g = DeviceGallery("cuda:0", capacity=8)
    g.upsert(["a", "b", "c"], w["G"][:3], normalise=False)
    va, vb = g.view(["a", "b"]), g.view(["c"])
    vs = g.view_set([va, vb])
    q = w["Qd"][:4]
    idx, _ = vs.match_device(q, [0, 1, 0, 1])
    assert ((idx.cpu().numpy() >= 0) & (idx.cpu().numpy() < 2)).all()
    with pytest.raises(ValueError, match="one gallery"):
        g.view_set([va, w["views"][2]])
    g.upsert(["a"], w["G"][5:6], normalise=False)            # a row rewritten in place: no membership change
    vs.match_device(q, [0, 1, 0, 1])
    g.upsert(["d"], w["G"][3:4], normalise=False)            # a new id: the generation moves on
    with pytest.raises(StaleViewError):
        vs.match_device(q, [0, 1, 0, 1])
    with pytest.raises(StaleViewError):
        vs.match_topk_device(q, [0, 1, 0, 1], 3)
    with pytest.raises(StaleViewError):
        GalleryViewSet([va, g.view(["d"])])                  # views of two generations
    fresh = g.view_set([g.view(["a", "b", "d"]), g.view(["c"])])
    assert fresh.match_device(q, [0, 1, 0, 1])[0].shape == (4,)
