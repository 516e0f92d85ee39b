"""The gallery audit on the device (csrc/pair_scan.hip): find_duplicates returns the pair set and the score bits of
tests/helpers/pairs_ref.py - through a contiguous matcher, a shuffled view over a slab with decoys and NaN in its unused slots, every
`scan` of the device gallery, and the manager - and agrees with the duplicate check's own kernel row by row."""
import numpy as np
import pytest
import torch

from tests.helpers import pairs_ref as pr
from tests.helpers import scan_ref as sr

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL_KEY, SENTINEL_SCORE = -0x0123456789ABCDEF, F32(-7.25)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _matcher(G):
    from facerecognition_infrenceengine_amd.gallery import GalleryMatcher
    m = GalleryMatcher("cuda:0")
    m.set_rows(list(range(len(G))), np.array(G), normalise=False)      # a copy: the cases' arrays are read-only
    return m


def _slab_view(slab, view):
    """a GalleryView whose position p is slot view[p] of a device slab holding `slab` as it is (unused slots included)"""
    from facerecognition_infrenceengine_amd.gallery import DeviceGallery
    g = DeviceGallery("cuda:0", capacity=len(slab))
    g.G = _dev(slab)
    g.slot_of = {p: int(s) for p, s in enumerate(view)}
    g._next = len(slab)
    v = g.view(list(range(len(view))))
    assert torch.equal(v.slots.cpu(), torch.from_numpy(view))
    return v


def _same(found, ref):
    assert found.pairs.dtype == np.int64 and found.pairs.shape == (len(ref[0]), 2) and found.scores.dtype == F32, \
        (found.pairs.shape, ref[0].shape)
    assert pr.same((found.pairs, found.scores), ref), int((found.pairs != ref[0]).any(1).sum())
    assert found.ids == [(int(a), int(b)) for a, b in ref[0]]


@pytest.mark.parametrize("N", pr.GRID_NS)
def test_grid_cases_matcher_and_view(N):
    c = pr.grid_case(N)
    m = _matcher(c.G)
    slab, view = sr.view_slab(c.G, c.S, 300 + N)
    assert np.isnan(slab).any()
    v = _slab_view(slab, view)
    for thr in pr.GRID_THRS:
        for inclusive in (False, True):
            ref = pr.pairs_ref(c.G, thr, inclusive, S=c.S)
            low, high, _ = pr.candidates_ref(c.G, thr, c.S.astype(np.float64))
            for who in (m, v):                                     # the view: no decoy is read, the NaN slots neither count nor flag
                found = who.find_duplicates(thr=thr, inclusive=inclusive)
                _same(found, ref)
                assert low <= found.candidates <= high, (found.candidates, low, high)


def test_float_case_bits_and_candidates():
    c = pr.float_case()
    m = _matcher(c.G)
    for inclusive in (False, True):
        found = m.find_duplicates(thr=c.thr, inclusive=inclusive)
        _same(found, pr.pairs_ref(c.G, c.thr, inclusive, S=c.S))
        print("candidates", found.candidates, "bracket", c.bracket, "pairs", len(found))
        assert c.bracket[0] <= found.candidates <= c.bracket[1]
    v = _slab_view(*sr.view_slab(c.G, None, 11))
    _same(v.find_duplicates(thr=c.thr), pr.pairs_ref(c.G, c.thr, False, S=c.S))


def _ranges(who, thr, max_ranges):
    keys, scores, counts = who.find_duplicates_device(thr=thr, max_pairs=1 << 16, max_ranges=max_ranges)
    cnt = counts.cpu().numpy()
    assert cnt[2] == 0 and cnt[1] <= cnt[0]
    k = np.sort(keys[:cnt[1]].cpu().numpy())
    return np.stack([k >> 32, k & 0xFFFFFFFF], 1), int(cnt[3])


def test_one_block_walks_every_tile():
    """N = 300: max_ranges = 1 makes one block per query tile walk all five row tiles (both LDS buffers reused; the second query tile
    starts at tile 4), the plan's own choice is five ranges of one tile.  The float case in two ranges of seven tiles: the third query
    tile starts at the second range's tile 1, the odd buffer."""
    c = pr.grid_case(300)
    m = _matcher(c.G)
    ref = pr.pairs_ref(c.G, 0.5, False, S=c.S)[0]
    one, n1 = _ranges(m, 0.5, 1)
    own, n0 = _ranges(m, 0.5, 0)
    assert (n1, n0) == (1, 5), "the audit's plan changed: the case no longer reaches one block walking five tiles"
    assert np.array_equal(one, ref) and np.array_equal(own, ref)
    f = pr.float_case()
    mf = _matcher(f.G)
    two, n2 = _ranges(mf, f.thr, 2)
    assert n2 == 2 and _ranges(mf, f.thr, 0)[1] == 14
    assert np.array_equal(two, pr.pairs_ref(f.G, f.thr, False, S=f.S)[0])


@pytest.mark.parametrize("case", ["grid", "float"])
def test_agrees_with_the_duplicate_checks_kernel(lib, case):
    """fr_gallery_first_above_blocked_f32 with the view's rows as queries: for every b its first hit is min(partners of b, b itself),
    with the same score bits for that partner"""
    from facerecognition_infrenceengine_amd import _lib
    c, thr = (pr.grid_case(300), 0.5) if case == "grid" else (pr.float_case(), 0.4)
    v = _slab_view(*sr.view_slab(c.G, None, 23))
    found = v.find_duplicates(thr=thr)
    assert len(found) > 100
    N = c.N
    Q = v.rows().contiguous()
    idx = torch.empty(N, dtype=torch.int64, device="cuda")
    score = torch.empty(N, dtype=torch.float32, device="cuda")
    ws = torch.empty(N * 8, dtype=torch.uint8, device="cuda")
    lib.fr_gallery_first_above_blocked_f32(_lib.ptr(Q), _lib.ptr(v.gallery.G), _lib.ptr(v.slots), None, N, N, 512, float(thr), 0, 0,
                                           _lib.ptr(idx), _lib.ptr(score), _lib.ptr(ws), N * 8, _lib.stream_ptr())
    idx, score = idx.cpu().numpy(), score.cpu().numpy()
    first = {}
    for (a, b), s in zip(found.pairs.tolist(), found.scores):         # first[x] = (lowest partner of x, their score)
        for x, y in ((a, b), (b, a)):
            if x not in first or y < first[x][0]:
                first[x] = (y, s)
    for b in range(N):
        partner = min(first.get(b, (b, None))[0], b)                 # partners above b come after b itself, which passes (self score)
        assert idx[b] == partner, (b, idx[b], partner)
        if partner != b:
            assert F32(score[b]).view(np.uint32) == F32(first[b][1]).view(np.uint32)


def test_overflow_counts_subset_and_retry(lib):
    from facerecognition_infrenceengine_amd import _lib
    from facerecognition_infrenceengine_amd.gallery import DuplicateOverflowError
    c = pr.grid_case(130)
    m = _matcher(c.G)
    ref = pr.pairs_ref(c.G, 0.5, False, S=c.S)
    big = m.find_duplicates(thr=0.5)
    _same(big, ref)
    assert big.candidates > 16
    cap, room = 16, 64
    keys = torch.full((room,), SENTINEL_KEY, dtype=torch.int64, device="cuda")
    scores = torch.full((room,), float(SENTINEL_SCORE), dtype=torch.float32, device="cuda")
    counts = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.fr_gallery_pairs_workspace(c.N, cap), dtype=torch.uint8, device="cuda")
    lib.fr_gallery_pairs_above_f16(_lib.ptr(m.G), None, c.N, 512, 0.5, 0, cap, 0, _lib.ptr(keys), _lib.ptr(scores), _lib.ptr(counts),
                                   _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    cnt, k, s = counts.cpu().numpy(), keys.cpu().numpy(), scores.cpu().numpy()
    assert cnt[2] == 1 and cnt[0] == big.candidates and 0 <= cnt[1] <= cap
    assert (k[cap:] == SENTINEL_KEY).all() and (s[cap:] == SENTINEL_SCORE).all()
    assert (k[cnt[1]:cap] == SENTINEL_KEY).all() and (s[cnt[1]:cap] == SENTINEL_SCORE).all()
    truth = {(int(a), int(b)): sc for (a, b), sc in zip(*ref)}
    for key, sc in zip(k[:cnt[1]], s[:cnt[1]]):
        assert truth[(int(key) >> 32, int(key) & 0xFFFFFFFF)] == sc
    with pytest.raises(DuplicateOverflowError) as e:
        m.find_duplicates(thr=0.5, max_pairs=cap)
    assert e.value.needed == big.candidates and isinstance(e.value, _lib.FrError)
    _same(m.find_duplicates(thr=0.5, max_pairs=e.value.needed), ref)


def test_a_row_beyond_the_f16_range_is_refused():
    c = pr.grid_case(130)
    bad = np.array(c.G)
    bad[1] = pr.nonfinite_row(c.G)
    m = _matcher(bad)
    with pytest.raises(ValueError, match="f16 range"):
        m.find_duplicates(thr=0.5)
    _, _, counts = m.find_duplicates_device(thr=0.5)
    cnt = counts.cpu().numpy()
    assert cnt[1] == 0 and cnt[2] == 2
    slab, view = sr.view_slab(c.G, c.S, 77)
    unused = sorted(set(range(len(slab))) - set(view.tolist()))
    slab[unused[0]] = pr.nonfinite_row(c.G)                           # the same row where no position names it: no effect
    _same(_slab_view(slab, view).find_duplicates(thr=0.5), pr.pairs_ref(c.G, 0.5, False, S=c.S))
    with pytest.raises(ValueError, match="f16 range"):
        slab2 = np.array(slab)
        slab2[view[5]] = pr.nonfinite_row(c.G)
        _slab_view(slab2, view).find_duplicates(thr=0.5)


def test_every_scan_kind_gives_the_same_audit_and_a_stale_view_raises():
    from facerecognition_infrenceengine_amd.gallery import DeviceGallery, StaleViewError
    c = pr.grid_case(130)
    ref = pr.pairs_ref(c.G, 0.5, True, S=c.S)
    order = np.random.default_rng(3).permutation(c.N)
    for scan in ("f32", "f16", "f8"):
        g = DeviceGallery("cuda:0", capacity=64, scan=scan)
        g.upsert([int(i) for i in order], c.G[order], normalise=False)     # slots in another order than the view's positions
        v = g.view(list(range(c.N)))
        _same(v.find_duplicates(thr=0.5, inclusive=True), ref)
        g.upsert([1000], np.array(c.G[:1]), normalise=False)
        with pytest.raises(StaleViewError):
            v.find_duplicates(thr=0.5)
        with pytest.raises(StaleViewError):
            v.find_duplicates_device(thr=0.5)


def test_manager_finds_the_pair_the_reference_never_checks():
    from app.services import EmbeddingManager, InMemoryStore
    rng = np.random.default_rng(9)
    e = rng.standard_normal((8, 512)).astype(F32)
    store = InMemoryStore()
    store.add_employee("e1", "A", e[0], name="Ada")
    store.add_employee("e2", "A", e[1], name="Bob")
    store.add_employee("e3", "B", e[1], name="Bob again")             # the same person in another company
    store.add_employee("e4", "A", e[2], name="Cy")
    store.add_employee("e5", "B", e[3], name="Di")
    store.add_visitor("v1", "A", e[0], name="Ada visiting")           # an employee of A who is also a visitor of A
    store.add_visitor("v2", "A", e[4], name="Ed")
    store.add_visitor("v3", "B", e[5], name="Flo")
    em = EmbeddingManager(store=store, device="cuda:0")
    a = em.find_duplicates("A")
    assert len(a) == 1 and a[0]["score"] > 0.999
    assert {k: a[0][k] for k in ("a", "b", "a_type", "b_type", "a_name", "b_name")} == \
        {"a": "e1", "b": "v1", "a_type": "employee", "b_type": "visitor", "a_name": "Ada", "b_name": "Ada visiting"}
    assert em.find_duplicates("B") == [] and em.find_duplicates("nobody") == []
    everyone = em.find_duplicates()
    assert [(d["a"], d["b"]) for d in everyone] == [("e1", "v1"), ("e2", "e3")]
    assert everyone == em.find_duplicates(None, thr=0.4)
    store.employees[0]["status"] = "inactive"
    em.force_sync()
    assert em.find_duplicates("A") == []
    assert [(d["a"], d["b"]) for d in em.find_duplicates()] == [("e2", "e3")]
