"""Top-K identification without a GPU: argument checks of the new C-ABI entries (nothing is launched), the torch forms
of the sharded top-K reduce, and the two-collective exchange of ``ShardedGalleryMatcher.match_topk`` over gloo with a
NumPy stand-in for the scan."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ONE = C.c_void_p(16)          # a non-null pointer that is never dereferenced: every check comes before any launch


@pytest.fixture(scope="module")
def lib():
    from facerecognition_infrenceengine_amd import _lib
    return _lib.load()


def test_topk_argument_checks_never_launch(lib):
    from facerecognition_infrenceengine_amd import _lib
    E = _lib.FrError
    big = 1 << 40
    for K in (0, 17, -3):
        with pytest.raises(E, match="K must be 1..16"):
            lib.fr_gallery_topk_f32(ONE, ONE, 1, 10, 512, K, 0, ONE, ONE, ONE, big, None, 0, None)
        with pytest.raises(E, match="K must be 1..16"):
            lib.fr_gallery_topk_view_f32(ONE, ONE, ONE, 1, 10, 512, K, ONE, ONE, ONE, big, None)
        with pytest.raises(E, match="K must be 1..16"):
            lib.fr_match_reduce_shards_topk(ONE, 2, 4, K, 0, 4, ONE, ONE, None)
    with pytest.raises(E, match="D must be 512"):
        lib.fr_gallery_topk_f32(None, None, 1, 10, 256, 4, 0, None, None, None, 0, None, 0, None)
    with pytest.raises(E, match="D must be 512"):
        lib.fr_gallery_topk_view_f32(None, None, ONE, 1, 10, 128, 4, None, None, None, 0, None)
    with pytest.raises(E, match="null view"):
        lib.fr_gallery_topk_view_f32(ONE, ONE, None, 1, 10, 512, 4, ONE, ONE, ONE, big, None)
    with pytest.raises(E, match="null pointer"):
        lib.fr_gallery_topk_f32(None, ONE, 1, 10, 512, 4, 0, ONE, ONE, ONE, big, None, 0, None)
    with pytest.raises(E, match="null pointer"):
        lib.fr_gallery_topk_f32(ONE, None, 1, 10, 512, 4, 0, ONE, ONE, ONE, big, None, 0, None)      # N > 0 needs G
    with pytest.raises(E, match="null pointer"):
        lib.fr_gallery_topk_view_f32(ONE, ONE, ONE, 1, 10, 512, 4, None, ONE, ONE, big, None)
    with pytest.raises(E, match="null pointer"):
        lib.fr_match_reduce_shards_topk(None, 2, 4, 4, 0, 4, ONE, ONE, None)
    with pytest.raises(E, match="seg_len must divide F"):
        lib.fr_gallery_topk_f32(ONE, ONE, 10, 10, 512, 4, 0, ONE, ONE, ONE, big, ONE, 3, None)
    with pytest.raises(E, match="seg_len must divide F"):
        lib.fr_gallery_topk_f32(ONE, ONE, 10, 10, 512, 4, 0, ONE, ONE, ONE, big, ONE, 0, None)
    with pytest.raises(E, match="negative size"):
        lib.fr_gallery_topk_f32(ONE, ONE, 1, -1, 512, 4, 0, ONE, ONE, ONE, big, None, 0, None)
    with pytest.raises(E, match="bad range"):
        lib.fr_match_reduce_shards_topk(ONE, 2, 4, 4, 2, 3, ONE, ONE, None)                          # q0 + F > n
    with pytest.raises(E, match="bad range"):
        lib.fr_match_reduce_shards_topk(ONE, 0, 4, 4, 0, 4, ONE, ONE, None)
    # F == 0: nothing to do, no pointer is read
    assert lib.fr_gallery_topk_f32(None, None, 0, 10, 512, 4, 0, None, None, None, 0, None, 0, None) == 0
    assert lib.fr_gallery_topk_view_f32(None, None, ONE, 0, 10, 512, 4, None, None, None, 0, None) == 0
    assert lib.fr_match_reduce_shards_topk(None, 2, 4, 4, 0, 0, None, None, None) == 0


def test_topk_workspace_monotone_and_one_byte_short_refused(lib):
    from facerecognition_infrenceengine_amd import _lib
    ws = lib.fr_gallery_topk_workspace
    Fs, Ns, Ks = (1, 31, 32, 33, 256, 1000), (0, 1, 127, 128, 129, 10_000, 131_073, 1_000_000), (1, 2, 3, 5, 8, 16)
    for F in Fs:
        for N in Ns:
            for K in Ks:
                w = ws(F, N, K)
                assert w >= 12 * K * F                                    # at least one block's lists
                assert ws(F + 1, N, K) >= w and ws(F, N + 1, K) >= w and ws(F, 2 * N + 64, K) >= w
                if K < 16:
                    assert ws(F, N, K + 1) >= w
    for F, N, K in ((1, 0, 1), (37, 5003, 5), (256, 1_000_000, 16)):
        need = ws(F, N, K)
        with pytest.raises(_lib.FrError, match="workspace too small"):
            lib.fr_gallery_topk_f32(ONE, ONE, F, N, 512, K, 0, ONE, ONE, ONE, need - 1, None, 0, None)
        with pytest.raises(_lib.FrError, match="workspace too small"):
            lib.fr_gallery_topk_view_f32(ONE, ONE, ONE, F, max(N, 1), 512, K, ONE, ONE, ONE, ws(F, max(N, 1), K) - 1, None)
        with pytest.raises(_lib.FrError, match="workspace too small"):
            lib.fr_gallery_topk_f32(ONE, ONE, F, N, 512, K, 0, ONE, ONE, None, need, None, 0, None)   # no buffer at all


def test_gallery_api_rejects_k_out_of_range_before_touching_the_device():
    """ValueError comes before any device work: checked on objects that never saw a GPU."""
    from facerecognition_infrenceengine_amd import gallery
    from facerecognition_infrenceengine_amd.processor import FaceRecognitionProcessor
    m = gallery.GalleryMatcher.__new__(gallery.GalleryMatcher)
    v = gallery.GalleryView.__new__(gallery.GalleryView)
    v.generation, v.gallery = 0, type("G", (), {"generation": 0})()
    Q = torch.zeros((2, 512))
    for k in (0, 17, -1):
        with pytest.raises(ValueError, match="k must be 1..16"):
            m.match_topk_device(Q, k)
        with pytest.raises(ValueError, match="k must be 1..16"):
            m.match_topk(Q, k)
        with pytest.raises(ValueError, match="k must be 1..16"):
            v.match_topk_device(Q, k)
        with pytest.raises(ValueError, match="k must be 1..16"):
            FaceRecognitionProcessor(None, face_detector=object()).identify(np.zeros((8, 8, 3), np.uint8), "c", k=k)
    assert gallery.TOPK_MAX == 16


def test_reduce_candidates_topk_tie_rule_and_empties():
    from facerecognition_infrenceengine_amd.distributed import reduce_candidates_topk
    ninf = -1.0
    # R = 2 shards, F = 4 queries, K = 3
    s = torch.tensor([[[0.9, 0.5, 0.1], [0.5, 0.5, 0.2], [0.7, ninf, ninf], [ninf, ninf, ninf]],
                      [[0.8, 0.5, 0.3], [0.5, 0.4, 0.3], [0.7, 0.6, 0.1], [ninf, ninf, ninf]]])
    i = torch.tensor([[[40, 41, 42], [10, 30, 11], [90, -1, -1], [-1, -1, -1]],
                      [[12, 13, 14], [20, 21, 22], [50, 51, 52], [-1, -1, -1]]])
    bi, bs = reduce_candidates_topk(s, i, 3)
    assert bi.tolist() == [[40, 12, 13],          # 0.9, 0.8, then 0.5 twice: the lower global row (13 < 41) first
                           [10, 20, 30],          # three rows at 0.5 in two shards: rows ascending
                           [50, 90, 51],          # same score in two shards: lower row first; a shard with 1 row of 3
                           [-1, -1, -1]]          # nothing anywhere
    assert torch.equal(bs, torch.tensor([[0.9, 0.8, 0.5], [0.5, 0.5, 0.5], [0.7, 0.7, 0.6], [-1.0, -1.0, -1.0]]))
    assert bi.dtype == torch.int64 and bs.dtype == torch.float32
    b1, s1 = reduce_candidates_topk(s, i, 1)
    assert b1.tolist() == [[40], [10], [50], [-1]] and s1[3, 0] == -1.0
    # fewer candidates than k over all shards: the tail is empty
    bi, bs = reduce_candidates_topk(s[:, 2:3, :2], i[:, 2:3, :2], 2)
    assert bi.tolist() == [[50, 90]]
    bi, bs = reduce_candidates_topk(torch.tensor([[[0.3, ninf]], [[ninf, ninf]]]), torch.tensor([[[5, -1]], [[-1, -1]]]), 2)
    assert bi.tolist() == [[5, -1]] and bs.tolist() == [[pytest.approx(0.3), -1.0]]
    # rows beyond 2^31 survive the reduce; the stale score of an empty slot is never looked at
    bi, bs = reduce_candidates_topk(torch.tensor([[[0.5, 9.0]], [[0.5, 0.25]]]),
                                    torch.tensor([[[(1 << 33) + 1, -1]], [[1 << 33, 7]]]), 2)
    assert bi.tolist() == [[1 << 33, (1 << 33) + 1]] and bs.tolist() == [[0.5, 0.5]]


def test_reduce_packed_topk_reads_the_flat_candidate_block():
    from facerecognition_infrenceengine_amd.distributed import (pack_candidates, reduce_candidates_topk,
                                                                reduce_packed_topk)
    rng = np.random.default_rng(3)
    R, n, k = 3, 7, 4
    score = torch.from_numpy(-np.sort(-rng.random((R, n, k)).astype(np.float32), axis=2).copy())
    idx = torch.from_numpy(rng.permutation(R * n * k).reshape(R, n, k).astype(np.int64) + (1 << 32))
    idx[1, :, 2:] = -1                                                        # a shard with 2 rows only
    allp = torch.cat([pack_candidates(idx[r].reshape(-1), score[r].reshape(-1)) for r in range(R)])
    assert allp.shape == (R * n * k, 3) and allp.dtype == torch.int32
    gi, gs = reduce_packed_topk(allp, R, n, k, 2, 4)
    wi, ws = reduce_candidates_topk(score[:, 2:6], idx[:, 2:6], k)
    assert torch.equal(gi, wi) and torch.equal(gs, ws)
    assert (gs[:, :-1] >= gs[:, 1:]).all() and (gi >= (1 << 32)).all()


# ---------------------------------------------------------------- gloo: the exchange with K candidates per slot
class NumpyTopkOps:
    """CPU stand-in for distributed.HipOps: float32 ``Qn @ G.T`` and a stable argsort behind the ops ``match`` and
    ``match_topk`` use, with the torch pack / reduce forms."""

    def __init__(self, shard, lo):
        self.shard, self.lo = np.asarray(shard, np.float32), lo

    def renormalise(self, Q):
        q = Q.numpy()
        return torch.from_numpy((q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)) if len(q) else Q.clone()

    def scan_topk(self, Q, k, counts=None, seg_len=0):
        q = Q.numpy()
        n = len(q)
        idx, score = np.full((n, k), -1, np.int64), np.full((n, k), -1.0, np.float32)
        pad = np.zeros(n, bool)
        if counts is not None:
            pad = (np.arange(n) % seg_len) >= counts.numpy()[np.arange(n) // seg_len]
        for f in np.flatnonzero(~pad):
            s = np.array([np.dot(q[f], g) for g in self.shard], np.float32)   # one dot per row: no dependence on batch shape
            order = np.argsort(-s, kind="stable")
            order = order[s[order] > -1.0][:k]
            idx[f, :len(order)], score[f, :len(order)] = order + self.lo, s[order]
        return torch.from_numpy(idx), torch.from_numpy(score)

    def scan(self, Q, counts=None, seg_len=0):
        idx, score = self.scan_topk(Q, 1, counts, seg_len)
        return idx[:, 0].contiguous(), score[:, 0].contiguous()

    def pack_queries(self, Qn, q_max):
        from facerecognition_infrenceengine_amd.distributed import pack_queries
        return pack_queries(Qn, q_max)

    def gathered_counts(self, allq, world, q_max):
        from facerecognition_infrenceengine_amd.distributed import gathered_counts
        return gathered_counts(allq, world, q_max)

    def pack(self, idx, score):
        from facerecognition_infrenceengine_amd.distributed import pack_candidates
        return pack_candidates(idx, score)

    def reduce(self, allp, world, n, q0, F):
        from facerecognition_infrenceengine_amd.distributed import reduce_packed
        return reduce_packed(allp, world, n, q0, F)

    def reduce_topk(self, allp, world, n, k, q0, F):
        from facerecognition_infrenceengine_amd.distributed import reduce_packed_topk
        return reduce_packed_topk(allp, world, n, k, q0, F)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _worker(rank, world, port, G, Qs, ks, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from facerecognition_infrenceengine_amd.distributed import ShardedGalleryMatcher, shard_rows
    lo, hi = shard_rows(len(G), world, rank)
    m = ShardedGalleryMatcher(NumpyTopkOps(G[lo:hi], lo), q_max=8)
    Q = torch.from_numpy(Qs[rank])
    res = {"match": tuple(t.numpy() for t in m.match(Q))}
    for k in ks:
        res[k] = tuple(t.numpy() for t in m.match_topk(Q, k))
    res["match_after"] = tuple(t.numpy() for t in m.match(Q))
    out[rank] = res
    dist.barrier()
    dist.destroy_process_group()


def _run(world, N, fs, ks=(1, 5)):
    rng = np.random.default_rng(77 + N)
    G = rng.standard_normal((N, 512)).astype(np.float32)
    if N:
        G /= np.linalg.norm(G, axis=1, keepdims=True)
    Qs = []
    for f in fs:
        Q = rng.standard_normal((f, 512)).astype(np.float32)
        Q /= np.linalg.norm(Q, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (f, 1)).astype(np.float32)
        Qs.append(Q)
    if N > 40:                                                    # duplicate rows in DIFFERENT shards
        q = Qs[0][0] / np.linalg.norm(Qs[0][0])
        G[3] = q; G[N // 2 + 1] = q; G[N - 2] = q
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), G, Qs, ks, out), nprocs=world, join=True)
    whole = NumpyTopkOps(G, 0)
    for r in range(world):
        Qn = whole.renormalise(torch.from_numpy(Qs[r]))
        for k in ks:
            wi, ws = whole.scan_topk(Qn, k)
            gi, gs = out[r][k]
            assert gi.shape == (fs[r], k) and gi.dtype == np.int64 and gs.dtype == np.float32
            assert np.array_equal(gi, wi.numpy()), (r, k, gi, wi)
            assert np.array_equal(gs.view(np.int32), ws.numpy().view(np.int32)), (r, k)      # bit for bit
        w1i, w1s = whole.scan(Qn)
        for key in ("match", "match_after"):                                                 # match() is what it was
            assert np.array_equal(out[r][key][0], w1i.numpy()) and np.array_equal(out[r][key][1], w1s.numpy())
        if 1 in ks and fs[r]:
            assert np.array_equal(out[r][1][0][:, 0], out[r]["match"][0])
    return out


def test_world2_sharded_topk_equals_unsharded():
    out = _run(2, 101, [5, 3])
    assert out[0][5][0][0, :3].tolist() == [3, 51, 99]            # the planted duplicates: global rows ascending
    assert len(set(out[0][5][1][0, :3].tolist())) == 1


def test_world2_topk_rank_without_faces_and_empty_shard():
    _run(2, 64, [8, 0])                                           # one rank has no faces this step
    out = _run(2, 1, [2, 2])                                      # 1 row over 2 ranks: an empty shard, 1 filled slot
    assert out[1][5][0][:, 1:].tolist() == [[-1] * 4] * 2 and (out[1][5][1][:, 1:] == -1.0).all()
    out = _run(2, 0, [1, 2])                                      # empty gallery
    assert (out[0][5][0] == -1).all() and (out[1][5][1] == -1.0).all()


def test_world4_sharded_topk_equals_unsharded():
    out = _run(4, 257, [1, 8, 0, 4])
    assert out[0][5][0][0, :3].tolist() == [3, 129, 255]
