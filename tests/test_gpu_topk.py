"""Exact top-K gallery identification on the GPU (fr_gallery_topk_f32 and everything above it) against the float64
reference and comparison rule of tests/helpers/topk_ref.py, and bit for bit against the top-1 match, the view scan,
the sharded exchange and the processor."""
import os
import sys

import numpy as np
import pytest
import torch

from tests.helpers import topk_ref as ref

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

KS = (1, 2, 3, 5, 8, 16)
CASES = ((7, 20_000, 64), (8, 5_003, 37), (9, 100_003, 96))     # seed, N, F (ambiguous positions at K = 16: < 1 % each)


def _matcher(G, scan="f32", ids=None):
    from facerecognition_infrenceengine_amd.gallery import GalleryMatcher
    m = GalleryMatcher("cuda:0", scan=scan)
    m.set_rows(list(range(len(G))) if ids is None else list(ids), G, normalise=False)
    return m


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _empty(idx, score):
    return bool((idx == -1).all()) and bool((score == -1.0).all())


@pytest.mark.parametrize("seed,N,F", CASES)
def test_topk_against_float64_reference_and_column0_is_the_match(seed, N, F):
    """Every K against the reference; column 0 equals match_device bit for bit."""
    G, Q = ref.seeded_case(seed, N, F)
    S = ref.scores64(Q, G)
    m = _matcher(G)
    Qd = torch.from_numpy(Q).cuda()
    idx1, score1 = m.match_device(Qd)
    for K in KS:
        idx, score = m.match_topk_device(Qd, K)
        assert idx.shape == (F, K) and idx.dtype == torch.int64 and score.dtype == torch.float32
        assert torch.equal(idx[:, 0], idx1) and _bits_equal(score[:, 0], score1), K
        ref.check(idx.cpu().numpy(), score.cpu().numpy(), S, K)
        assert bool((score[:, :-1] >= score[:, 1:]).all())
        if K > 1:                                                   # a shorter list is a prefix of a longer one
            pi, ps = m.match_topk_device(Qd, K - 1)
            assert torch.equal(pi, idx[:, :K - 1]) and _bits_equal(ps, score[:, :K - 1])


@pytest.mark.parametrize("tag", ["g100", "g1000"])
def test_column0_on_the_reference_generated_vectors(golden, tag):
    d = golden("match_kat.npz")
    G, Q = d[f"{tag}_G"], d[f"{tag}_Q"]
    m = _matcher(G)
    Qd = torch.from_numpy(Q).cuda()
    idx1, score1 = m.match_device(Qd)
    ids, _, _ = m.match(Q, thr=0.4)
    assert np.array_equal(np.asarray([-1 if i is None else i for i in ids]), d[f"{tag}_live_pid"])
    for K in KS:
        idx, score = m.match_topk_device(Qd, K)
        assert torch.equal(idx[:, 0], idx1) and _bits_equal(score[:, 0], score1)
        assert int(idx[2, 0]) == 17                                 # exact tie 17 / 63 -> lowest row
        if K > 1:
            assert int(idx[2, 1]) == 63 and _bits_equal(score[2, 1:2], score[2, 0:1])
    tids, tscore, tidx = m.match_topk(Q, 3, min_score=0.4)
    assert tidx.shape == (len(Q), 3) and tscore.dtype == np.float32
    for f in range(len(Q)):
        assert tids[f][0] == ids[f]                                 # >= 0.4 on column 0 is the live decision
        assert all((i is None) == bool(s < 0.4) for i, s in zip(tids[f], tscore[f]))


@pytest.mark.parametrize("N", [5_003, 140_000])
def test_exact_ties_are_ordered_by_row(N):
    """One unit query planted in different tiles, waves and blocks (140 000 rows: past the 1024-block cap, so one
    lane meets two of them as well)."""
    rng = np.random.default_rng(11)
    G = rng.standard_normal((N, 512)).astype(np.float32); G /= np.linalg.norm(G, axis=1, keepdims=True)
    q = rng.standard_normal(512).astype(np.float32); q /= np.linalg.norm(q)
    rows = [7, 40, N // 2, N - 3]
    if N > 131_072 + 7:
        rows.insert(3, 131_072 + 7)                                 # same block, wave and lane as row 7, a later tile
    for r in rows:
        G[r] = q
    m = _matcher(G)
    Qd = torch.from_numpy(np.stack([q * 1.7, q])).cuda()
    n = len(rows)
    idx, score = m.match_topk_device(Qd, 8)
    for f in range(2):
        assert idx[f, :n].tolist() == rows
        assert len(set(_bits(score[f, :n]).tolist())) == 1          # bit-identical scores
        assert float(score[f, n]) < 0.5
    idx2, score2 = m.match_topk_device(Qd, 2)
    assert idx2.tolist() == [[7, 40]] * 2 and _bits_equal(score2, score[:, :2])
    idx4, _ = m.match_topk_device(Qd, 4)
    assert idx4.tolist() == [rows[:4]] * 2


def test_edges_empty_short_minus_one_nan_and_k_range(lib):
    from facerecognition_infrenceengine_amd import _lib
    rng = np.random.default_rng(12)
    Q = rng.standard_normal((5, 512)).astype(np.float32)
    Qd = torch.from_numpy(Q).cuda()
    # N = 0
    m = _matcher(np.zeros((0, 512), np.float32))
    for K in (1, 4, 16):
        idx, score = m.match_topk_device(Qd, K)
        assert idx.shape == (5, K) and _empty(idx, score)
    # N = 3, K = 8: three filled slots, then empty ones
    G = rng.standard_normal((3, 512)).astype(np.float32); G /= np.linalg.norm(G, axis=1, keepdims=True)
    m = _matcher(G)
    idx, score = m.match_topk_device(Qd, 8)
    ref.check(idx.cpu().numpy(), score.cpu().numpy(), ref.scores64(Q, G), 8)
    assert bool((idx[:, :3] >= 0).all()) and _empty(idx[:, 3:], score[:, 3:])
    # a score of exactly -1.0 is never listed (the reference's best starts at -1, strict '>')
    e0 = np.zeros(512, np.float32); e0[0] = 1
    e1 = np.zeros(512, np.float32); e1[1] = 1
    qe = torch.from_numpy(e0[None]).cuda()
    m = _matcher(np.stack([-e0, e1, -e0, e0]))
    idx, score = m.match_topk_device(qe, 4, renormalise=False)
    assert idx.tolist() == [[3, 1, -1, -1]] and score.tolist() == [[1.0, 0.0, -1.0, -1.0]]
    assert int(m.match_device(qe, renormalise=False)[0][0]) == 3
    m = _matcher(np.stack([-e0, -e0]))
    idx, score = m.match_topk_device(qe, 2, renormalise=False)
    assert _empty(idx, score) and int(m.match_device(qe, renormalise=False)[0][0]) == -1     # as the top-1 scan
    # F = 0, F = 1
    G = rng.standard_normal((70, 512)).astype(np.float32); G /= np.linalg.norm(G, axis=1, keepdims=True)
    m = _matcher(G)
    idx, score = m.match_topk_device(Qd[:0], 4)
    assert idx.shape == (0, 4) and score.shape == (0, 4)
    idx, score = m.match_topk_device(Qd[:1], 4)
    ref.check(idx.cpu().numpy(), score.cpu().numpy(), ref.scores64(Q[:1], G), 4)
    # a query of NaNs: every slot empty; its neighbours untouched
    Qn = Q.copy(); Qn[2] = np.nan
    idx, score = m.match_topk_device(torch.from_numpy(Qn).cuda(), 5)
    good, _ = m.match_topk_device(Qd, 5)
    assert _empty(idx[2], score[2]) and torch.equal(idx[[0, 1, 3, 4]], good[[0, 1, 3, 4]])
    # K outside 1..16: refused before any launch, by the host API and by the C ABI
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    out_i = torch.full((5, 17), 123, dtype=torch.int64, device="cuda")
    out_s = torch.zeros((5, 17), dtype=torch.float32, device="cuda")
    for K in (0, 17):
        with pytest.raises(ValueError):
            m.match_topk_device(Qd, K)
        with pytest.raises(_lib.FrError, match="K must be 1..16"):
            lib.fr_gallery_topk_f32(_lib.ptr(Qd), _lib.ptr(m.G), 5, 70, 512, K, 0, _lib.ptr(out_i), _lib.ptr(out_s),
                                    _lib.ptr(ws), ws.numel(), None, 0, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool((out_i == 123).all())


def test_padding_slots_and_row_offset():
    rng = np.random.default_rng(13)
    N, seg, K = 3_001, 9, 5
    G = rng.standard_normal((N, 512)).astype(np.float32); G /= np.linalg.norm(G, axis=1, keepdims=True)
    m = _matcher(G)
    counts = [9, 0, 4, 1, 0, 0, 0, 0, 7]                               # slots 32..63 are padding only: a group without work
    F = seg * len(counts)
    Q = rng.standard_normal((F, 512)).astype(np.float32); Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    real = np.array([f % seg < counts[f // seg] for f in range(F)])
    assert not real[32:64].any() and real[64:].any()
    Q[~real] = 0                                                       # what the exchange sends in padding rows
    Qd = torch.from_numpy(Q).cuda()
    cd = torch.tensor(counts, dtype=torch.int32, device="cuda")
    pi, ps = m.match_topk_device(Qd, K, renormalise=False, counts=cd, seg_len=seg)
    fi, fs = m.match_topk_device(Qd, K, renormalise=False)
    rm = torch.from_numpy(real).cuda()
    assert _empty(pi[~rm], ps[~rm])
    assert torch.equal(pi[rm], fi[rm]) and _bits_equal(ps[rm], fs[rm])
    t1i, t1s = m.match_device(Qd, renormalise=False, counts=cd, seg_len=seg)
    assert torch.equal(pi[:, 0], t1i) and _bits_equal(ps[:, 0], t1s)
    # row_offset: added to every filled idx and to no empty one
    off = (1 << 33) + 5
    m3 = _matcher(G[:3])
    oi, os_ = m3.match_topk_device(Qd[:4], K, renormalise=False, row_offset=off)
    zi, zs = m3.match_topk_device(Qd[:4], K, renormalise=False)
    assert bool((zi[:, :3] >= 0).all())
    assert torch.equal(oi[:, :3], zi[:, :3] + off) and bool((oi[:, 3:] == -1).all()) and _bits_equal(os_, zs)


def test_views_and_coarse_scan_matchers_return_the_same_bits():
    from facerecognition_infrenceengine_amd.gallery import DeviceGallery, StaleViewError
    rng = np.random.default_rng(14)
    n = 700
    rows = rng.standard_normal((n, 512)).astype(np.float32); rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    ids = [f"p{i}" for i in range(n)]
    g = DeviceGallery("cuda:0", capacity=64)                           # grows; slots out of id order
    order = rng.permutation(n)
    g.upsert([ids[i] for i in order[:400]], rows[order[:400]])
    g.remove([ids[i] for i in order[50:120]])
    g.upsert([ids[i] for i in order[400:]], rows[order[400:]])         # reuses the freed slots
    want = [ids[i] for i in sorted(order[:50].tolist() + order[120:].tolist())][::3]
    q = rows[ids.index(want[5])]
    g.upsert(["dup_a", "dup_b"], np.stack([q, q]))
    want = want[:40] + ["dup_b"] + want[40:] + ["dup_a", "never_enrolled"]
    view = g.view(want)
    assert len(view) == len(want) - 1 > 200
    Q = rng.standard_normal((37, 512)).astype(np.float32); Q[0] = q * 3
    Qd = torch.from_numpy(Q).cuda()
    m = _matcher(view.rows(), ids=view.ids)
    for K in (1, 4, 16):
        vi, vs = view.match_topk_device(Qd, K)
        mi, ms = m.match_topk_device(Qd, K)
        assert torch.equal(vi, mi) and _bits_equal(vs, ms)
        v1i, v1s = view.match_device(Qd)
        assert torch.equal(vi[:, 0], v1i) and _bits_equal(vs[:, 0], v1s)
    vi, vs = view.match_topk_device(Qd, 4)
    assert vi[0, :3].tolist() == [5, 40, len(view) - 1]                # the three copies of q, by VIEW position
    assert len(set(_bits(vs[0, :3]).tolist())) == 1
    tids, tscore, tidx = view.match_topk(Q, 4, min_score=0.9)
    assert tids[0] == [want[5], "dup_b", "dup_a", None] and np.array_equal(tidx, vi.cpu().numpy())
    ei, es = g.view([]).match_topk_device(Qd, 3)
    assert ei.shape == (37, 3) and _empty(ei, es)
    # coarse-scan matchers keep the f32 rows: their top-K is the exact f32 top-K
    G = m.G.cpu().numpy()
    mi, ms = m.match_topk_device(Qd, 8)
    for scan in ("f16", "f8"):
        ci, cs = _matcher(G, scan=scan).match_topk_device(Qd, 8)
        assert torch.equal(ci, mi) and _bits_equal(cs, ms), scan
    g.remove(["dup_a"])                                                # membership changed: the view is stale
    with pytest.raises(StaleViewError):
        view.match_topk_device(Qd, 4)
    with pytest.raises(StaleViewError):
        view.match_topk(Q, 4)


def _sharded_topk(G, Qs, q_max, K):
    """Every 'rank' r holds row shard r and the queries Qs[r]; the two all-gathers are torch.cat.  Returns per rank
    (idx [F,K], score [F,K], the rank's renormalised queries)."""
    from facerecognition_infrenceengine_amd.distributed import HipOps, reduce_packed_topk, shard_rows
    R, N = len(Qs), len(G)
    ops = []
    for r in range(R):
        lo, hi = shard_rows(N, R, r)
        ops.append(HipOps(_matcher(G[lo:hi], ids=range(lo, hi)), lo))
    seg = q_max + 1
    Qn = [ops[r].renormalise(torch.from_numpy(Qs[r]).cuda()) for r in range(R)]
    allq = torch.cat([ops[r].pack_queries(Qn[r], q_max) for r in range(R)])
    cnt = ops[0].gathered_counts(allq, R, q_max)
    packs, packs1 = [], []
    for r in range(R):
        idx, score = ops[r].scan_topk(allq, K, counts=cnt, seg_len=seg)
        assert idx.shape == (R * seg, K) and int(idx.view(R, seg, K)[:, q_max].max()) == -1     # the count row is padding
        packs.append(ops[r].pack(idx.reshape(-1), score.reshape(-1)))
        if K == 1:
            packs1.append(ops[r].pack(*ops[r].scan(allq, counts=cnt, seg_len=seg)))
    allp = torch.cat(packs)
    assert allp.shape == (R * R * seg * K, 3)
    out = []
    for r in range(R):
        F = len(Qs[r])
        bi, bs = ops[r].reduce_topk(allp, R, R * seg, K, r * seg, F)
        ti, ts = reduce_packed_topk(allp, R, R * seg, K, r * seg, F)                            # HIP reduce == torch reduce
        assert torch.equal(bi, ti) and _bits_equal(bs, ts)
        if K == 1:                                                                              # the existing exchange
            ei, es = ops[r].reduce(torch.cat(packs1), R, R * seg, r * seg, F)
            assert torch.equal(bi[:, 0], ei) and _bits_equal(bs[:, 0], es)
        out.append((bi, bs, Qn[r]))
    return out


@pytest.mark.parametrize("K", [1, 4, 16])
@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_shards_on_one_device_equal_the_unsharded_topk(R, K):
    from facerecognition_infrenceengine_amd.distributed import HipOps, ShardedGalleryMatcher
    rng = np.random.default_rng(100 + R)
    N, q_max = 5_003, 16
    G = rng.standard_normal((N, 512)).astype(np.float32); G /= np.linalg.norm(G, axis=1, keepdims=True)
    fs = [(7 * r + 5) % (q_max + 1) for r in range(R)]
    if R > 1:
        fs[1] = 0                                                         # a rank with no faces this step
    Qs = []
    for f in fs:
        Q = rng.standard_normal((f, 512)).astype(np.float32)
        Q /= np.linalg.norm(Q, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (f, 1)).astype(np.float32)
        Qs.append(Q)
    planted = [7, 40, N // 2, N - 3]
    for r in planted:
        G[r] = Qs[0][0] / np.linalg.norm(Qs[0][0])                        # duplicates in different shards
    whole = _matcher(G)
    out = _sharded_topk(G, Qs, q_max, K)
    for r in range(R):
        bi, bs, Qn = out[r]
        wi, ws = whole.match_topk_device(Qn, K, renormalise=False)
        assert bi.shape == (fs[r], K) and torch.equal(bi, wi) and _bits_equal(bs, ws), r     # bit for bit
    assert out[0][0][0, :min(K, 4)].tolist() == planted[:K]
    single = ShardedGalleryMatcher(HipOps(whole, 0), q_max=q_max)         # one rank, no exchange
    Q0 = torch.from_numpy(Qs[0]).cuda()
    ti, ts = single.match_topk(Q0, K)
    assert torch.equal(ti, out[0][0]) and _bits_equal(ts, out[0][1])
    if K == 1:
        si, ss = single.match(Q0)
        assert torch.equal(ti[:, 0], si) and _bits_equal(ts[:, 0], ss)


def test_shards_with_empty_shards_and_empty_gallery():
    rng = np.random.default_rng(5)
    Q = rng.standard_normal((3, 512)).astype(np.float32)
    G = rng.standard_normal((2, 512)).astype(np.float32); G /= np.linalg.norm(G, axis=1, keepdims=True)
    out = _sharded_topk(G, [Q, Q[:1], Q[:0], Q[:2]], 4, 4)               # 2 rows over 4 ranks: two empty shards
    wi, ws = _matcher(G).match_topk_device(torch.from_numpy(Q).cuda(), 4)
    assert torch.equal(out[0][0], wi) and _bits_equal(out[0][1], ws) and torch.equal(out[3][0], wi[:2])
    assert bool((wi[:, :2] >= 0).all()) and bool((wi[:, 2:] == -1).all())
    out = _sharded_topk(G[:0], [Q, Q[:1]], 4, 4)                         # empty gallery
    assert _empty(out[0][0], out[0][1]) and _empty(out[1][0], out[1][1])


@pytest.fixture(scope="module")
def app():
    import warnings
    from facerecognition_infrenceengine_amd import FaceAnalysis
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = FaceAnalysis(name="buffalo_l", providers=["CUDAExecutionProvider", "CPUExecutionProvider"])
        a.prepare(ctx_id=0)
    return a


def test_processor_identify(app):
    from make_golden import synth_frame
    from facerecognition_infrenceengine_amd.processor import EmbeddingManager, FaceRecognitionProcessor, InMemoryStore
    frame = synth_frame(240, 320, 4)
    faces = app.get(frame)
    assert len(faces) >= 1
    store = InMemoryStore()
    rng = np.random.default_rng(3)
    for i in range(30):
        store.add_employee(f"e{i}", "acme" if i % 3 else "globex", rng.standard_normal(512), name=f"E{i}")
    poses = [faces[0].normed_embedding + 0.01 * rng.standard_normal(512).astype(np.float32) for _ in range(3)]
    store.add_employee("target", "acme", np.mean(poses, axis=0), name="Target")
    store.add_visitor("near", "acme", faces[0].normed_embedding + 0.05 * rng.standard_normal(512).astype(np.float32),
                      name="Near")
    store.add_employee("other_co", "globex", faces[0].normed_embedding, name="Elsewhere")
    mgr = EmbeddingManager(store=store)
    proc = FaceRecognitionProcessor(mgr, face_detector=app)
    rec = proc.recognize(frame, "acme")
    res = proc.identify(frame, "acme", k=3)
    members = set(sum(store.company_member_ids("acme"), []))
    assert len(members) == 22 and len(res) == len(rec) == len(faces)
    for a, b in zip(res, rec):
        assert set(a) == {"bbox", "det_score", "candidates"}
        assert np.array_equal(a["bbox"], b["bbox"]) and a["det_score"] == b["det_score"]
        assert len(a["candidates"]) == 3                                  # 22 members, nothing filtered
        scores = [c["score"] for c in a["candidates"]]
        assert all(x >= y for x, y in zip(scores, scores[1:]))            # rank order
        assert all(set(c) == {"person_id", "person_info", "score"} and c["person_id"] in members
                   and c["person_info"] is mgr.employee_metadata[c["person_id"]] for c in a["candidates"])
        if b["person_id"] is not None:
            assert a["candidates"][0]["person_id"] == b["person_id"]
            assert a["candidates"][0]["score"] == b["recognition_score"]
    assert rec[0]["person_id"] == "target"
    assert [c["person_id"] for c in res[0]["candidates"][:2]] == ["target", "near"]
    assert res[0]["candidates"][1]["person_info"]["type"] == "visitor"
    cut = proc.identify(frame, "acme", k=3, min_score=0.5)                # min_score drops the tail
    assert [c["person_id"] for c in cut[0]["candidates"]] == ["target", "near"]
    for a, b in zip(cut, res):
        assert [c["person_id"] for c in a["candidates"]] == [c["person_id"] for c in b["candidates"] if c["score"] >= 0.5]
    one = proc.identify(frame, "globex", k=1)
    assert one[0]["candidates"][0]["person_id"] == "other_co"
    assert proc.identify(frame, "nobody") is None                         # no gallery: as recognize
    assert len(proc.identify(frame, "acme")[0]["candidates"]) == 5        # default k
    for k in (0, 17):
        with pytest.raises(ValueError):
            proc.identify(frame, "acme", k=k)


def test_topk_on_another_stream_leaves_the_match_alone():
    """The workspace is per call (GalleryMatcher._workspace): a top-K scan in flight on another stream of the same
    matcher changes nothing in a top-1 match, and the other way round."""
    G, Q = ref.seeded_case(21, 30_011, 70)
    m = _matcher(G)
    Qd = torch.from_numpy(Q).cuda()
    idx0, score0 = m.match_device(Qd)
    top0 = m.match_topk_device(Qd, 16)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    got, tops = [], []
    for _ in range(4):
        with torch.cuda.stream(side):
            tops.append(m.match_topk_device(Qd, 16))
        got.append(m.match_device(Qd))
    torch.cuda.synchronize()
    for (i, s), (ti, ts) in zip(got, tops):
        assert torch.equal(i, idx0) and _bits_equal(s, score0)
        assert torch.equal(ti, top0[0]) and _bits_equal(ts, top0[1])
    idx1, score1 = m.match_device(Qd)
    assert torch.equal(idx1, idx0) and _bits_equal(score1, score0)
