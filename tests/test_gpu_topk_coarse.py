"""Certified coarse top-K (fr_gallery_topk_f16 / _view_f16 and everything above them).

The reference of every comparison is the exact f32 top-K (fr_gallery_topk_f32 / _view_f32, pinned to the float64 order of
tests/helpers/topk_ref.py by tests/test_gpu_topk.py), never the new path: results must be EQUAL, idx by torch.equal and
scores by their bits, whether a query was certified or answered by the exact fallback.  ``last_topk`` says which path ran."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

KS = (1, 4, 5, 16)
FS = (1, 37, 256, 300)
NS = (700, 5_003, 140_000)
NEVER = 1 << 40                   # coarse_topk_min_rows that no gallery reaches: the exact path


def _unit(rng, n):
    x = rng.standard_normal((n, 512)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _matcher(G, scan="f16", ids=None, min_rows=0):
    from facerecognition_infrenceengine_amd.gallery import GalleryMatcher
    m = GalleryMatcher("cuda:0", scan=scan)
    m.set_rows(list(range(len(G))) if ids is None else list(ids), G, normalise=False)
    m.coarse_topk_min_rows = min_rows
    return m


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return (a[0].shape == b[0].shape and torch.equal(a[0], b[0]) and a[1].dtype == b[1].dtype == torch.float32
            and torch.equal(_bits(a[1]), _bits(b[1])))


def _empty(idx, score):
    return bool((idx == -1).all()) and bool((score == -1.0).all())


def _both(m, Qd, K, **kw):
    """(coarse result, exact result, flags) of one matcher or view; the path of each call is asserted"""
    from facerecognition_infrenceengine_amd.gallery import last_topk
    owner = m.gallery if hasattr(m, "gallery") else m
    owner.coarse_topk_min_rows = 0
    got = m.match_topk_device(Qd, K, **kw)
    rec = last_topk()
    assert rec["path"] == "coarse" and m.last_topk is rec
    flags = rec["flags"]
    assert flags.dtype == torch.int32 and flags.shape == (Qd.shape[0],) and bool(((flags == 0) | (flags == 1)).all())
    owner.coarse_topk_min_rows = NEVER
    want = m.match_topk_device(Qd, K, **kw)
    assert last_topk()["path"] == "exact" and last_topk()["flags"] is None
    owner.coarse_topk_min_rows = 0
    return got, want, flags


def _queries(rng, G, F):
    """random queries off unit length; every third one is a noisy copy of a gallery row (a strong match with a margin)"""
    Q = rng.standard_normal((F, 512)).astype(np.float32)
    for f in range(0, F, 3):
        Q[f] = G[(f * 7919) % len(G)] + 0.03 * rng.standard_normal(512).astype(np.float32)
    Q *= rng.uniform(0.5, 2.0, (F, 1)).astype(np.float32)
    return Q


def _shuffled_gallery(rng, rows, scan="f16"):
    """a DeviceGallery filled out of id order: it grows from 64 slots, frees slots and reuses them"""
    from facerecognition_infrenceengine_amd.gallery import DeviceGallery
    n = len(rows)
    g = DeviceGallery("cuda:0", capacity=64, scan=scan)
    order = rng.permutation(n)
    a, b, c = n // 2, n // 14, n // 6
    g.upsert(order[:a].tolist(), rows[order[:a]])
    g.remove(order[b:c].tolist())
    g.upsert(order[a:].tolist(), rows[order[a:]])                  # reuses the freed slots, then grows again
    g.upsert(order[b:c].tolist(), rows[order[b:c]])
    return g


@gpu
@pytest.mark.parametrize("N", NS)
def test_bits_of_the_exact_topk_contiguous_and_view(N):
    """K x F x N of the issue on a contiguous f16 matcher and on a view of a shuffled, grown, slot-reusing f16 gallery."""
    rng = np.random.default_rng(40 + N % 97)
    G = _unit(rng, N)
    m = _matcher(G)
    g = _shuffled_gallery(rng, G)
    view = g.view(range(N))                                         # id order: a permutation of the slots
    assert len(view) == N and g.capacity > 64 and not torch.equal(view.slots, torch.arange(N, device="cuda"))
    f32 = _matcher(G, scan="f32")
    n_flag = 0
    for F in FS:
        Qd = torch.from_numpy(_queries(rng, G, F)).cuda()
        for K in KS:
            got, want, flags = _both(m, Qd, K)
            assert _same(got, want), (N, F, K)
            assert _same(got, f32.match_topk_device(Qd, K)), (N, F, K)       # and the f32 matcher's bits
            vgot, vwant, vflags = _both(view, Qd, K)
            assert _same(vgot, vwant) and _same(vgot, want), (N, F, K)
            t1 = f32.match_device(Qd)                                         # column 0 is the EXACT top-1 (f32 scan)
            assert torch.equal(vgot[0][:, 0], t1[0]) and torch.equal(_bits(vgot[1][:, 0]), _bits(t1[1]))
            n_flag += int(flags.sum()) + int(vflags.sum())
    print(f"N {N}: {n_flag} fallbacks over {2 * sum(FS) * len(KS)} queries")


@gpu
def test_row_offset_counts_mask_and_ties():
    rng = np.random.default_rng(41)
    N, seg, K = 3_001, 9, 5
    G = _unit(rng, N)
    m = _matcher(G)
    counts = [9, 0, 4, 1, 0, 0, 0, 0, 7]                               # slots 32..63 are padding only
    F = seg * len(counts)
    Q = _unit(rng, F)
    real = np.array([f % seg < counts[f // seg] for f in range(F)])
    Q[~real] = 0
    Qd = torch.from_numpy(Q).cuda()
    cd = torch.tensor(counts, dtype=torch.int32, device="cuda")
    got, want, flags = _both(m, Qd, K, renormalise=False, counts=cd, seg_len=seg)
    rm = torch.from_numpy(real).cuda()
    assert _same(got, want) and _empty(got[0][~rm], got[1][~rm]) and bool((got[0][rm][:, 0] >= 0).all())
    assert int(flags[~rm].sum()) == 0                                  # padding is never sent to the exact scan
    off = (1 << 33) + 5
    got, want, _ = _both(m, Qd[:4], K, renormalise=False, row_offset=off)
    assert _same(got, want) and int(got[0].min()) >= off
    got, want, _ = _both(_matcher(G[:3]), Qd[:4], K, renormalise=False, row_offset=off)
    assert _same(got, want) and bool((got[0][:, 3:] == -1).all()) and int(got[0][:, :3].min()) >= off
    # exact ties are ordered by row: one unit query planted in different tiles, ranges and lanes
    for N in (5_003, 140_000):
        G = _unit(rng, N)
        q = _unit(rng, 1)[0]
        rows = [7, 40, N // 2, N - 3] + ([131_072 + 7] if N > 131_079 else [])
        rows.sort()
        for r in rows:
            G[r] = q
        Qd = torch.from_numpy(np.stack([q * 1.7, q])).cuda()
        m = _matcher(G)
        for K in (2, 4, 8):
            got, want, _ = _both(m, Qd, K)
            assert _same(got, want)
            assert got[0][0, :min(K, len(rows))].tolist() == rows[:K]
            assert len(set(_bits(got[1][0, :min(K, len(rows))]).tolist())) == 1


@gpu
def test_three_copies_empty_view_short_minus_one_and_nan():
    """The edge cases the exact top-K pins (tests/test_gpu_topk.py), on the coarse path."""
    from facerecognition_infrenceengine_amd.gallery import DeviceGallery
    rng = np.random.default_rng(14)
    n = 700
    rows = _unit(rng, n)
    ids = [f"p{i}" for i in range(n)]
    g = DeviceGallery("cuda:0", capacity=64, scan="f16")
    order = rng.permutation(n)
    g.upsert([ids[i] for i in order[:400]], rows[order[:400]])
    g.remove([ids[i] for i in order[50:120]])
    g.upsert([ids[i] for i in order[400:]], rows[order[400:]])
    want_ids = [ids[i] for i in sorted(order[:50].tolist() + order[120:].tolist())][::3]
    q = rows[ids.index(want_ids[5])]
    g.upsert(["dup_a", "dup_b"], np.stack([q, q]))
    want_ids = want_ids[:40] + ["dup_b"] + want_ids[40:] + ["dup_a", "never_enrolled"]
    view = g.view(want_ids)
    Q = rng.standard_normal((37, 512)).astype(np.float32); Q[0] = q * 3
    Qd = torch.from_numpy(Q).cuda()
    for K in (1, 4, 16):
        got, want, _ = _both(view, Qd, K)
        assert _same(got, want)
    got, _, _ = _both(view, Qd, 4)
    assert got[0][0, :3].tolist() == [5, 40, len(view) - 1]            # the three copies of q, by VIEW position
    assert len(set(_bits(got[1][0, :3]).tolist())) == 1
    tids, _, _ = view.match_topk(Q, 4, min_score=0.9)
    assert tids[0] == [want_ids[5], "dup_b", "dup_a", None] and view.last_topk["path"] == "coarse"
    got, want, flags = _both(g.view([]), Qd, 3)                        # empty view
    assert got[0].shape == (37, 3) and _empty(*got) and _same(got, want) and int(flags.sum()) == 0
    # N < K
    Q5 = torch.from_numpy(rng.standard_normal((5, 512)).astype(np.float32)).cuda()
    got, want, flags = _both(_matcher(_unit(rng, 3)), Q5, 8)
    assert _same(got, want) and bool((got[0][:, :3] >= 0).all()) and _empty(got[0][:, 3:], got[1][:, 3:])
    assert int(flags.sum()) == 0                                       # every row was re-scored: nothing is unseen
    # rows scoring <= -1 are never listed
    e0 = np.zeros(512, np.float32); e0[0] = 1
    e1 = np.zeros(512, np.float32); e1[1] = 1
    qe = torch.from_numpy(e0[None]).cuda()
    got, want, _ = _both(_matcher(np.stack([-e0, e1, -e0, e0])), qe, 4, renormalise=False)
    assert _same(got, want) and got[0].tolist() == [[3, 1, -1, -1]] and got[1].tolist() == [[1.0, 0.0, -1.0, -1.0]]
    got, want, _ = _both(_matcher(np.stack([-e0, -e0])), qe, 2, renormalise=False)
    assert _same(got, want) and _empty(*got)
    # a NaN query: flagged, every slot empty, its neighbours untouched; an infinite element likewise flagged
    m = _matcher(_unit(rng, 70))
    Qn = Q5.clone(); Qn[2] = float("nan"); Qn[4, 9] = float("inf")
    got, want, flags = _both(m, Qn, 5)
    good, _, _ = _both(m, Q5, 5)
    assert _same(got, want) and _empty(got[0][2], got[1][2]) and flags[[2, 4]].tolist() == [1, 1]
    assert torch.equal(got[0][[0, 1, 3]], good[0][[0, 1, 3]])
    with pytest.raises(ValueError):
        m.match_topk_device(Q5, 17)


def _scores64(Q, G):
    """float64 [F,N] scores, in slices (the float64 copy of a large gallery is not kept)"""
    Q = Q.astype(np.float64)
    return np.concatenate([Q @ G[c:c + 25_000].astype(np.float64).T for c in range(0, len(G), 25_000)], axis=1)


def _planted(rng, G, Q, f, rows, scores):
    """G[rows[j]] = a unit row whose score against unit query Q[f] is scores[j]"""
    for r, s in zip(rows, scores):
        w = rng.standard_normal(512)
        w -= (w @ Q[f].astype(np.float64)) * Q[f]
        w /= np.linalg.norm(w)
        G[r] = (s * Q[f] + np.sqrt(1 - s * s) * w).astype(np.float32)


@gpu
def test_certification_happens_no_fallback_at_all():
    """200 000 seeded unit rows; per query 16 planted rows, scores 0.5 .. 0.9, 12 500 rows apart (a scan range of this
    gallery is 832 rows: each in a range of its own).  Every other score is below 0.3 (checked here, in float64), so
    the gap to anything unseen is > 0.19 against eps = 1.1e-3: no query may be flagged, for any K <= 16."""
    rng = np.random.default_rng(2024)
    N, F = 200_000, 48
    G, Q = _unit(rng, N), _unit(rng, F)
    scores = np.linspace(0.9, 0.5, 16)
    mine = np.zeros((F, N), bool)
    for f in range(F):
        rows = [j * 12_500 + 4 * f for j in range(16)]
        _planted(rng, G, Q, f, rows, scores)
        mine[f, rows] = True
    S = _scores64(Q, G)
    assert S[~mine].max() < 0.3 and np.abs(S[mine].reshape(F, 16) - scores).max() < 1e-6
    Qd = torch.from_numpy(Q).cuda()
    m = _matcher(G)
    g = _shuffled_gallery(rng, G)
    view = g.view(range(N))
    for K in range(1, 17):
        for who in (m, view):
            got, want, flags = _both(who, Qd, K, renormalise=False)
            assert int(flags.sum()) == 0, (K, flags.nonzero().flatten().tolist())
            assert _same(got, want)
            assert got[0][3].tolist() == [j * 12_500 + 12 for j in range(K)]


@gpu
def test_certification_refuses_when_it_must():
    """Query 0 has 4 096 rows within 1e-5 of one another's score, spread over the whole gallery: more than the 32 groups
    the re-rank re-scores, so the bound of the unseen rows reaches its K-th score and it must be flagged; the other
    queries (planted as above) stay certified; everything equals the exact top-K."""
    rng = np.random.default_rng(77)
    N, F = 140_000, 9
    G, Q = _unit(rng, N), _unit(rng, F)
    crowd = np.arange(4096) * (N // 4096) + 1
    _planted(rng, G, Q, 0, crowd, np.full(4096, 0.7))
    for f in range(1, F):
        _planted(rng, G, Q, f, [j * 8_700 + 4 * f + 2 for j in range(16)], np.linspace(0.9, 0.5, 16))
    s0 = G[crowd].astype(np.float64) @ Q[0].astype(np.float64)
    assert s0.max() - s0.min() < 1e-5
    Qd = torch.from_numpy(Q).cuda()
    for who in (_matcher(G), _shuffled_gallery(rng, G).view(range(N))):
        for K in (1, 5, 16):
            got, want, flags = _both(who, Qd, K, renormalise=False)
            assert flags.tolist() == [1] + [0] * (F - 1), (K, flags.tolist())
            assert _same(got, want) and bool((got[1][0] > 0.69).all())
    # one row of norm 50: eps grows 50-fold for every query.  Certified or flagged, the results are equal.
    G[1234] = 50 * _unit(rng, 1)[0]
    m = _matcher(G)
    assert abs(float(m.gmax) - 50) < 1e-4
    for K in (1, 5, 16):
        got, want, flags = _both(m, Qd, K, renormalise=False)
        assert _same(got, want) and int(flags[0]) == 1
        print(f"norm-50 row, K {K}: flags {flags.tolist()}")
    # a row the f16 copy cannot hold: Gmax = +inf, nothing certifies, results still equal
    G[99, 5] = 70_000.0
    m = _matcher(G)
    assert float(m.gmax) == float("inf")
    got, want, flags = _both(m, Qd, 4, renormalise=False)
    assert _same(got, want) and flags.tolist() == [1] * F


@gpu
def test_gmax_is_the_largest_norm_ever_written():
    """Tolerance from the kernel's reduction, not from a run: |row|^2 is 512 rounded products, 7 additions in a lane and 6
    levels of the wave butterfly - at most 14 roundings on any path, relative error <= 14 u (u = 2^-24); the square root
    halves that and rounds once: <= 8 u, against the float64 norm of the f32 row as stored."""
    from facerecognition_infrenceengine_amd.gallery import DeviceGallery
    tol = 8 * 2.0 ** -24 * (1 + 1e-6)
    rng = np.random.default_rng(5)
    g = DeviceGallery("cuda:0", capacity=8, scan="f16")
    assert float(g.gmax) == 0.0
    seen = 0.0

    def put(ids, rows):
        nonlocal seen
        g.upsert(ids, rows)
        seen = max(seen, float(np.linalg.norm(rows.astype(np.float64), axis=1).max()))
        got = float(g.gmax)
        assert abs(got - seen) <= tol * seen, (got, seen)

    put(list(range(6)), _unit(rng, 6) * rng.uniform(0.5, 1.5, (6, 1)).astype(np.float32))
    put([2, 3], 2.5 * _unit(rng, 2))                                    # overwrite in place: larger
    put([2], 0.1 * _unit(rng, 1))                                       # overwrite with a smaller row: the bound stays
    assert g.remove([3]) == 1
    assert abs(float(g.gmax) - seen) <= tol * seen                      # never shrinks on remove
    cap = g.capacity
    put(list(range(100, 140)), _unit(rng, 40) * rng.uniform(0.2, 3.0, (40, 1)).astype(np.float32))
    assert g.capacity > cap                                             # the scalar survives a capacity doubling
    put([7], 7.25 * _unit(rng, 1))
    assert DeviceGallery("cuda:0", capacity=8).gmax is None             # f32 gallery: no certificate, no scalar
    big = _unit(rng, 1); big[0, 3] = -65_600.0
    g.upsert([8], big)
    assert float(g.gmax) == float("inf")
    g.remove([8])
    assert float(g.gmax) == float("inf")
    rows = _unit(rng, 5_000) * rng.uniform(0.5, 4.0, (5_000, 1)).astype(np.float32)
    m = _matcher(rows)
    want = float(np.linalg.norm(rows.astype(np.float64), axis=1).max())
    assert abs(float(m.gmax) - want) <= tol * want
    m.set_rows([0, 1], _unit(rng, 2), normalise=False)                  # a new gallery: a new bound
    assert abs(float(m.gmax) - 1) < 1e-6


def _sharded_topk(G, Qs, q_max, K, scan):
    from facerecognition_infrenceengine_amd.distributed import HipOps, shard_rows
    R, N = len(Qs), len(G)
    ops = []
    for r in range(R):
        lo, hi = shard_rows(N, R, r)
        ops.append(HipOps(_matcher(G[lo:hi], scan=scan, ids=range(lo, hi)), lo))
    seg = q_max + 1
    Qn = [ops[r].renormalise(torch.from_numpy(Qs[r]).cuda()) for r in range(R)]
    allq = torch.cat([ops[r].pack_queries(Qn[r], q_max) for r in range(R)])
    cnt = ops[0].gathered_counts(allq, R, q_max)
    packs = []
    for r in range(R):
        idx, score = ops[r].scan_topk(allq, K, counts=cnt, seg_len=seg)
        assert ops[r].matcher.last_topk["path"] == ("coarse" if scan == "f16" else "exact")
        packs.append(ops[r].pack(idx.reshape(-1), score.reshape(-1)))
    allp = torch.cat(packs)
    return [ops[r].reduce_topk(allp, R, R * seg, K, r * seg, len(Qs[r])) for r in range(R)]


@gpu
@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_shards_over_f16_galleries_return_the_f32_lists(R):
    from facerecognition_infrenceengine_amd.distributed import HipOps, ShardedGalleryMatcher
    rng = np.random.default_rng(200 + R)
    N, q_max = 5_003, 16
    G = _unit(rng, N)
    fs = [(7 * r + 5) % (q_max + 1) for r in range(R)]
    if R > 1:
        fs[1] = 0
    Qs = [_unit(rng, f) * rng.uniform(0.5, 2.0, (f, 1)).astype(np.float32) for f in fs]
    for r in (7, 40, N // 2, N - 3):
        G[r] = Qs[0][0] / np.linalg.norm(Qs[0][0])                        # duplicates in different shards
    for K in (1, 4, 16):
        a, b = _sharded_topk(G, Qs, q_max, K, "f16"), _sharded_topk(G, Qs, q_max, K, "f32")
        for r in range(R):
            assert a[r][0].shape == (fs[r], K) and _same(a[r], b[r]), (R, K, r)
        assert a[0][0][0, :min(K, 4)].tolist() == [7, 40, N // 2, N - 3][:K]
        Q0 = torch.from_numpy(Qs[0]).cuda()
        one = ShardedGalleryMatcher(HipOps(_matcher(G), 0), q_max=q_max).match_topk(Q0, K)
        ref = ShardedGalleryMatcher(HipOps(_matcher(G, scan="f32"), 0), q_max=q_max).match_topk(Q0, K)
        assert _same(one, ref) and _same(one, a[0])


@gpu
def test_identify_over_an_f16_gallery_returns_the_f32_lists():
    import warnings
    from make_golden import synth_frame
    from facerecognition_infrenceengine_amd import FaceAnalysis
    from facerecognition_infrenceengine_amd.gallery import last_topk
    from facerecognition_infrenceengine_amd.processor import EmbeddingManager, FaceRecognitionProcessor, InMemoryStore
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        app = FaceAnalysis(name="buffalo_l", providers=["CUDAExecutionProvider", "CPUExecutionProvider"])
        app.prepare(ctx_id=0)
    frame = synth_frame(240, 320, 4)
    faces = app.get(frame)
    assert len(faces) >= 1
    store = InMemoryStore()
    rng = np.random.default_rng(3)
    for i in range(300):
        store.add_employee(f"e{i}", "acme" if i % 3 else "globex", rng.standard_normal(512), name=f"E{i}")
    store.add_employee("target", "acme", faces[0].normed_embedding, name="Target")
    store.add_visitor("near", "acme", faces[0].normed_embedding + 0.05 * rng.standard_normal(512).astype(np.float32),
                      name="Near")
    out = {}
    for scan in ("f32", "f16"):
        mgr = EmbeddingManager(store=store, scan=scan)
        mgr.get_matcher_for_company("acme")
        mgr._gallery.coarse_topk_min_rows = 0
        proc = FaceRecognitionProcessor(mgr, face_detector=app)
        out[scan] = [proc.identify(frame, "acme", k=k) for k in (1, 5, 16)]
        assert last_topk()["path"] == ("coarse" if scan == "f16" else "exact")
    for a, b in zip(out["f16"], out["f32"]):
        assert len(a) == len(b) == len(faces)
        for x, y in zip(a, b):
            assert [(c["person_id"], c["score"]) for c in x["candidates"]] == [(c["person_id"], c["score"]) for c in y["candidates"]]
    assert [c["person_id"] for c in out["f16"][1][0]["candidates"][:2]] == ["target", "near"]


def test_new_entries_check_their_arguments_before_any_launch():
    """No GPU needed: header, binding and library agree on the new entries, and bad arguments are refused."""
    from facerecognition_infrenceengine_amd import _lib
    lib = _lib.load()
    ONE = ctypes.c_void_p(4096)
    big = 1 << 40
    for K in (0, 17):
        with pytest.raises(_lib.FrError, match="K must be 1..16"):
            lib.fr_gallery_topk_f16(ONE, ONE, ONE, 1, 10, 512, K, 0, ONE, ONE, ONE, ONE, ONE, big, None, 0, None)
        with pytest.raises(_lib.FrError, match="K must be 1..16"):
            lib.fr_gallery_topk_view_f16(ONE, ONE, ONE, ONE, 1, 10, 10, 512, K, ONE, ONE, ONE, ONE, ONE, big, None)
        with pytest.raises(_lib.FrError, match="K must be 1..16"):
            lib.fr_gallery_topk_view_masked_f32(ONE, ONE, ONE, 1, 10, 512, K, ONE, ONE, ONE, big, ONE, None)
    with pytest.raises(_lib.FrError, match="D must be 512"):
        lib.fr_gallery_topk_f16(ONE, ONE, ONE, 1, 10, 256, 4, 0, ONE, ONE, ONE, ONE, ONE, big, None, 0, None)
    with pytest.raises(_lib.FrError, match="N must be 0..2\\^28"):
        lib.fr_gallery_topk_f16(ONE, ONE, ONE, 1, (1 << 28) + 1, 512, 4, 0, ONE, ONE, ONE, ONE, ONE, big, None, 0, None)
    with pytest.raises(_lib.FrError, match="null pointer"):                 # no Gmax scalar, no flags
        lib.fr_gallery_topk_f16(ONE, ONE, ONE, 1, 10, 512, 4, 0, None, ONE, ONE, ONE, ONE, big, None, 0, None)
    with pytest.raises(_lib.FrError, match="null pointer"):
        lib.fr_gallery_topk_f16(ONE, ONE, ONE, 1, 10, 512, 4, 0, ONE, ONE, ONE, None, ONE, big, None, 0, None)
    with pytest.raises(_lib.FrError, match="null view"):
        lib.fr_gallery_topk_view_f16(ONE, ONE, ONE, None, 1, 10, 10, 512, 4, ONE, ONE, ONE, ONE, ONE, big, None)
    with pytest.raises(_lib.FrError, match="capacity"):
        lib.fr_gallery_topk_view_f16(ONE, ONE, ONE, ONE, 1, 10, 5, 512, 4, ONE, ONE, ONE, ONE, ONE, big, None)
    with pytest.raises(_lib.FrError, match="seg_len must divide F"):
        lib.fr_gallery_topk_f16(ONE, ONE, ONE, 10, 10, 512, 4, 0, ONE, ONE, ONE, ONE, ONE, big, ONE, 3, None)
    with pytest.raises(_lib.FrError, match="null view"):
        lib.fr_gallery_topk_view_masked_f32(ONE, ONE, None, 1, 10, 512, 4, ONE, ONE, ONE, big, ONE, None)
    with pytest.raises(_lib.FrError, match="D must be 512"):
        lib.fr_gallery_gmax_update(ONE, None, 3, 64, ONE, None)
    with pytest.raises(_lib.FrError, match="null pointer"):
        lib.fr_gallery_gmax_update(ONE, None, 3, 512, None, None)
    assert lib.fr_gallery_gmax_update(None, None, 0, 512, None, None) == 0
    assert lib.fr_gallery_topk_f16(None, None, None, 0, 10, 512, 4, 0, None, None, None, None, None, 0, None, 0, None) == 0
    for F, N, K in ((1, 0, 1), (37, 700, 5), (256, 1_000_000, 16), (1024, 100_000, 4)):
        need = lib.fr_gallery_topk_f16_workspace(F, N, K)
        assert need == lib.fr_gallery_topk_view_f16_workspace(F, N, K)
        # the coarse lists, the spill bounds, the exact lists of the fallback and the exact scan's own workspace
        assert need > lib.fr_gallery_topk_workspace(F, N, K) + lib.fr_gallery_match_f16_workspace(F, N) - 256
        with pytest.raises(_lib.FrError, match="workspace too small"):
            lib.fr_gallery_topk_f16(ONE, ONE, ONE, F, N, 512, K, 0, ONE, ONE, ONE, ONE, ONE, need - 1, None, 0, None)


def test_path_choice_is_one_attribute():
    """Host logic alone: the crossover is one attribute per gallery, seeded from the module constant."""
    from facerecognition_infrenceengine_amd import gallery
    assert isinstance(gallery.COARSE_TOPK_MIN_ROWS, int) and gallery.COARSE_TOPK_MIN_ROWS > 0
    assert gallery.last_topk() is None or set(gallery.last_topk()) == {"path", "flags"}
