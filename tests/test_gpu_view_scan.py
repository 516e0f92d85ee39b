"""GPU: the coarse f16 / fp8 scan of a DeviceGallery's shadow slab through a view's slot list.

Ids must EQUAL the exact scan's (0 mismatches): the oracle's and the same view's on a scan="f32" gallery.  Scores are
the f32 re-scores: atol 3e-6 against another summation order of the same f32 dot (the figure test_gpu_match.py holds
for exactly this comparison)."""
import pickle
from datetime import datetime, timedelta

import numpy as np
import pytest
import torch

from oracle import match as omatch

pytestmark = pytest.mark.gpu
ATOL = 3e-6


def _galleries(scan, ids, rows, capacity, normalise=False):
    """The same operations on a coarse gallery and on an f32 one: (coarse, exact)."""
    from facerecognition_infrenceengine_amd.gallery import DeviceGallery
    out = []
    for s in (scan, "f32"):
        g = DeviceGallery("cuda:0", capacity=capacity, scan=s)
        g.upsert(ids, rows, normalise=normalise)
        out.append(g)
    return out


def _scattered(scan, G, seed):
    """G's rows upserted under ids 0..N-1 in a shuffled order together with filler ids that are then removed: the view
    of ids 0..N-1 in order is a permutation of slots with holes between them."""
    N = len(G)
    rng = np.random.default_rng(seed)
    nfill = max(3, N // 50)
    fill = rng.standard_normal((nfill, 512)).astype(np.float32)
    ids = list(range(N)) + [f"hole{k}" for k in range(nfill)]
    rows = np.concatenate([G, fill])
    order = rng.permutation(len(ids))
    coarse, exact = _galleries(scan, [ids[k] for k in order], rows[order], capacity=N + nfill + 37)
    for g in (coarse, exact):
        assert g.remove([f"hole{k}" for k in range(nfill)]) == nfill
    return coarse, exact


def _shadow_is_exact(g, lib):
    """The shadow rows of the live slots hold exactly fr_f32_to_f16 / fr_f32_to_f8 of the f32 rows in the same slots."""
    from facerecognition_infrenceengine_amd import _lib
    live = torch.tensor(sorted(g.slot_of.values()), dtype=torch.int64, device=g.device)
    rows = g.G[live].contiguous()
    if g.scan == "f16":
        want = torch.empty(rows.shape, dtype=torch.float16, device=g.device)
        lib.fr_f32_to_f16(_lib.ptr(rows), _lib.ptr(want), rows.numel(), _lib.stream_ptr())
        got, want = g.S[live].view(torch.int16), want.view(torch.int16)
    else:
        want = torch.empty(rows.shape, dtype=torch.uint8, device=g.device)
        lib.fr_f32_to_f8(_lib.ptr(rows), _lib.ptr(want), rows.numel(), _lib.stream_ptr())
        got = g.S[live]
    assert g.S.shape == (g.capacity, 512) and torch.equal(got, want)


@pytest.mark.parametrize("scan", ["f16", "f8"])
@pytest.mark.parametrize("N,F", [(1, 1), (33, 5), (63, 300), (4097, 130), (100_000, 256), (20_000, 700)])
def test_view_scan_ids_equal_oracle_and_f32_view(N, F, scan, lib):
    """The inputs of test_coarse_scan_with_f32_rerank_matches_f32_oracle (same seeds, duplicate rows, near-duplicate),
    scattered over a larger slab."""
    rng = np.random.default_rng(N * 7 + F)
    G = rng.standard_normal((N, 512)).astype(np.float32); G /= np.linalg.norm(G, axis=1, keepdims=True)
    Q = rng.standard_normal((F, 512)).astype(np.float32); Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    if N > 3:
        G[N - 1] = Q[0]; G[N // 2] = Q[0]
        Q[1 % F] = G[N // 3] + 0.01 * rng.standard_normal(512).astype(np.float32)
    coarse, exact = _scattered(scan, G, seed=N + F)
    view, ref = coarse.view(range(N)), exact.view(range(N))
    assert len(view) == N and torch.equal(view.slots, ref.slots)
    assert not torch.equal(view.slots, torch.arange(N, device="cuda")) or N == 1        # really a gather
    assert np.array_equal(view.rows().cpu().numpy(), G)
    Qd = torch.from_numpy(Q).cuda()
    idx, score = view.match_device(Qd)
    ei, es = ref.match_device(Qd)
    oi, os_ = omatch.match_rows_fast(Q, G)
    idx, score = idx.cpu().numpy(), score.cpu().numpy()
    print(f"{scan} N={N} F={F}: mismatches vs oracle {int((idx != oi).sum())}, vs f32 view {int((idx != ei.cpu().numpy()).sum())}, "
          f"max |score - oracle| {np.abs(score - os_).max():.2e}, max |score - f32 view| {np.abs(score - es.cpu().numpy()).max():.2e}")
    assert np.array_equal(idx, oi)
    assert np.array_equal(idx, ei.cpu().numpy())
    np.testing.assert_allclose(score, os_, atol=ATOL, rtol=0)
    np.testing.assert_allclose(score, es.cpu().numpy(), atol=ATOL, rtol=0)
    if N > 3:
        assert int(idx[0]) == N // 2                     # duplicate rows: the lower VIEW position
    _shadow_is_exact(coarse, lib)


@pytest.mark.parametrize("scan", ["f16", "f8"])
def test_view_order_decides_ties_not_slot_order(scan):
    """Two identical rows: whichever the VIEW lists first wins, wherever the slab keeps them."""
    rng = np.random.default_rng(5)
    G = rng.standard_normal((300, 512)).astype(np.float32); G /= np.linalg.norm(G, axis=1, keepdims=True)
    G[250] = G[10]
    coarse, exact = _galleries(scan, list(range(300)), G, capacity=512)
    Q = torch.from_numpy(G[10:11].copy()).cuda()
    for ids, want in ((list(range(300)), 10), (list(range(299, -1, -1)), 49)):
        idx, _ = coarse.view(ids).match_device(Q)
        ei, _ = exact.view(ids).match_device(Q)
        assert int(idx[0]) == want == int(ei[0])


@pytest.mark.parametrize("scan", ["f16", "f8"])
def test_subset_and_small_views(scan):
    """A view that is a strict subset of the slab: rows outside it that would win must not; views of 0, 1, 63, 64, 65
    rows (a 64-row tile that ends inside, at and past the view)."""
    rng = np.random.default_rng(77)
    N, F = 5000, 40
    G = rng.standard_normal((N, 512)).astype(np.float32); G /= np.linalg.norm(G, axis=1, keepdims=True)
    Q = rng.standard_normal((F, 512)).astype(np.float32); Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    member = list(range(N - 1, -1, -3))                                  # every third row, in reverse order
    inside = set(member)
    outside = [i for i in range(N) if i not in inside]
    for f in range(10):                                                  # exact copies of the query OUTSIDE the view
        G[outside[37 * f + 5]] = Q[f]
    Q[10] = G[member[17]] + 0.01 * rng.standard_normal(512).astype(np.float32)
    coarse, exact = _galleries(scan, list(range(N)), G, capacity=8192)
    Qd = torch.from_numpy(Q).cuda()
    view = coarse.view(member)
    idx, score = view.match_device(Qd)
    oi, os_ = omatch.match_rows_fast(Q, G[member])
    ei, es = exact.view(member).match_device(Qd)
    assert np.array_equal(idx.cpu().numpy(), oi) and torch.equal(idx, ei) and int(idx[10]) == 17
    np.testing.assert_allclose(score.cpu().numpy(), os_, atol=ATOL, rtol=0)
    assert float(score[:10].max()) < 0.5                                 # the planted copies scored 1.0: they did not win
    # empty view
    idx, score = coarse.view([]).match_device(Qd)
    assert (idx == -1).all() and (score == -1).all()
    idx, score = coarse.view(["nobody"]).match_device(Qd)                # ids the gallery does not hold are skipped
    assert (idx == -1).all() and (score == -1).all()
    for n in (1, 63, 64, 65):
        ids = outside[100:100 + n]
        idx, score = coarse.view(ids).match_device(Qd)
        oi, os_ = omatch.match_rows_fast(Q, G[ids])
        ei, _ = exact.view(ids).match_device(Qd)
        assert np.array_equal(idx.cpu().numpy(), oi) and torch.equal(idx, ei), n
        np.testing.assert_allclose(score.cpu().numpy(), os_, atol=ATOL, rtol=0)


@pytest.mark.parametrize("scan", ["f16", "f8"])
def test_shadow_stays_coherent_through_overwrite_reuse_and_grow(scan, lib):
    from facerecognition_infrenceengine_amd.gallery import StaleViewError
    rng = np.random.default_rng(13)

    def unit(n):
        x = rng.standard_normal((n, 512)).astype(np.float32)
        return x / np.linalg.norm(x, axis=1, keepdims=True)

    mirror = {i: r for i, r in zip(range(100), unit(100))}
    coarse, exact = _galleries(scan, list(mirror), np.stack(list(mirror.values())), capacity=128)
    Q = unit(12)

    def check():
        _shadow_is_exact(coarse, lib)
        ids = list(mirror)
        Qs = Q.copy(); Qs[0] = mirror[ids[-1]]; Qs[1] = mirror[ids[len(ids) // 2]]      # two present rows, exactly
        Qd = torch.from_numpy(Qs).cuda()
        view = coarse.view(ids)
        idx, score = view.match_device(Qd)
        ei, es = exact.view(ids).match_device(Qd)
        oi, os_ = omatch.match_rows_fast(Qs, np.stack([mirror[i] for i in ids]))
        assert torch.equal(idx, ei) and np.array_equal(idx.cpu().numpy(), oi)
        assert int(idx[0]) == len(ids) - 1 and int(idx[1]) == len(ids) // 2
        np.testing.assert_allclose(score.cpu().numpy(), os_, atol=ATOL, rtol=0)
        return view

    v0 = check()
    # 1. overwrite existing ids in place: membership unchanged, the old view stays valid and sees the new rows
    new = unit(10)
    for g in (coarse, exact):
        g.upsert(list(range(20, 30)), new)
    mirror.update(zip(range(20, 30), new))
    check()
    idx, _ = v0.match_device(torch.from_numpy(new[3:4].copy()).cuda())
    assert int(idx[0]) == 23
    # the device-normalised form converts the NORMALISED row
    raw = (rng.standard_normal((4, 512)) * 3).astype(np.float32)
    for g in (coarse, exact):
        g.upsert([40, 41, 42, 43], raw, normalise=True)
    got = coarse.G[[coarse.slot_of[i] for i in (40, 41, 42, 43)]].cpu().numpy()
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() < 1e-6
    mirror.update(zip((40, 41, 42, 43), got))
    check()
    # 2. remove, then an upsert that reuses the freed slots
    freed = [coarse.slot_of[i] for i in (5, 6, 7)]
    for g in (coarse, exact):
        assert g.remove([5, 6, 7]) == 3
    for i in (5, 6, 7):
        del mirror[i]
    with pytest.raises(StaleViewError):
        v0.match_device(torch.from_numpy(Q).cuda())
    v1 = check()
    new = unit(2)
    for g in (coarse, exact):
        g.upsert(["a", "b"], new)
    mirror.update(zip(["a", "b"], new))
    assert {coarse.slot_of["a"], coarse.slot_of["b"]} <= set(freed) and coarse.capacity == 128
    with pytest.raises(StaleViewError):
        v1.match_device(torch.from_numpy(Q).cuda())
    v2 = check()
    # 3. an upsert that forces the slab to double: the shadow moves with it
    more = unit(200)
    for g in (coarse, exact):
        g.upsert([f"m{k}" for k in range(200)], more)
    mirror.update(zip([f"m{k}" for k in range(200)], more))
    assert coarse.capacity == 512 and coarse.S.shape[0] == 512
    with pytest.raises(StaleViewError):
        v2.match_device(torch.from_numpy(Q).cuda())
    check()
    assert exact.S is None                                               # scan="f32" keeps no shadow


def test_fp8_view_scan_saturates_instead_of_nan_on_non_unit_rows():
    """The inputs of test_fp8_scan_saturates_instead_of_nan_on_non_unit_rows through upsert(normalise=False) and
    match_device(renormalise=False): an element past 1.75 (x 256 > 448) saturates in the shadow row."""
    from facerecognition_infrenceengine_amd.gallery import DeviceGallery
    rng = np.random.default_rng(31)
    N = 3000
    G = rng.standard_normal((N, 512)).astype(np.float32); G /= np.linalg.norm(G, axis=1, keepdims=True)
    Q = rng.standard_normal((6, 512)).astype(np.float32); Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    G[1234] = 3.0 * Q[0]
    G[1234, 7] = 2.5
    Q[1] = 4.0 * G[77]; Q[1, 3] = 2.2
    g = DeviceGallery("cuda:0", capacity=4096, scan="f8")
    order = rng.permutation(N)
    g.upsert([int(i) for i in order], G[order], normalise=False)
    idx, score = g.view(range(N)).match_device(torch.from_numpy(Q).cuda(), renormalise=False)
    S = Q @ G.T
    oi = S.argmax(axis=1)
    assert np.array_equal(idx.cpu().numpy(), oi) and int(oi[0]) == 1234 and int(oi[1]) == 77
    np.testing.assert_allclose(score.cpu().numpy(), S[np.arange(6), oi], rtol=2e-6, atol=3e-6)
    assert not torch.isnan(score).any()
    assert int(g.S[g.slot_of[1234], 7]) == 0x7E                          # e4m3 +448, not the NaN code 0x7F


@pytest.mark.parametrize("scan,N", [("f16", 1_000_000), ("f8", 1_250_000)])
def test_view_scan_full_size(scan, N):
    """The sizes and inputs of test_coarse_scan_full_size on a scattered slab: planted rows come back exactly, 256
    unplanted queries (near-ties of random rows) equal the f32 view scan."""
    from facerecognition_infrenceengine_amd.gallery import DeviceGallery
    g = torch.Generator(device="cuda").manual_seed(3)
    G = torch.randn((N, 512), generator=g, device="cuda"); G /= G.norm(dim=1, keepdim=True)
    rows = torch.randperm(N, generator=g, device="cuda")[:2048]
    Q = G[rows] + 0.02 * torch.randn((2048, 512), generator=g, device="cuda")
    Q[1024:] = torch.randn((1024, 512), generator=g, device="cuda")
    nfill = 1000
    order = torch.randperm(N + nfill, generator=g, device="cuda")
    gal = DeviceGallery("cuda:0", capacity=N + nfill + 4096, scan=scan)
    chunk = 250_000                                                      # ids >= N are fillers, removed below
    for c in range(0, N + nfill, chunk):
        o = order[c:c + chunk]
        gal.upsert(o.tolist(), torch.where((o < N)[:, None], G[o.clamp(max=N - 1)], G[(o % 1000)].flip(1)))
    assert gal.remove(range(N, N + nfill)) == nfill
    view = gal.view(range(N))
    assert len(view) == N and int(view.slots.max()) >= N
    idx, score = view.match_device(Q)
    assert torch.equal(idx[:1024], rows[:1024]) and float(score[:1024].min()) > 0.8
    exact = DeviceGallery("cuda:0", capacity=1, scan="f32")              # the same f32 rows and slots, f32 view scan
    exact.G, exact.slot_of, exact.generation = gal.G, gal.slot_of, gal.generation
    ei, es = exact.view(range(N)).match_device(Q[1024:1024 + 256])
    print(f"{scan} N={N}: mismatches vs f32 view {int((idx[1024:1280] != ei).sum())}, "
          f"max |score diff| {float((score[1024:1280] - es).abs().max()):.2e}")
    assert torch.equal(idx[1024:1024 + 256], ei)
    torch.testing.assert_close(score[1024:1024 + 256], es, atol=ATOL, rtol=0)
    Qn = Q[1024:1032] / Q[1024:1032].norm(dim=1, keepdim=True)
    assert torch.equal(idx[1024:1032], (G @ Qn.T).argmax(dim=0))


def test_api_f16_manager_equals_f32_manager_across_a_sync():
    """Two EmbeddingManagers over one store, scan="f32" and scan="f16": recognize_batch and CameraProcessor.process_frame
    on the same frames give the same person ids and decisions, before and after an incremental sync that changes a
    matched person's row."""
    import os
    import sys
    import warnings
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import synth_frame
    from facerecognition_infrenceengine_amd import FaceAnalysis
    from facerecognition_infrenceengine_amd.processor import (CameraProcessor, EmbeddingManager,
                                                              FaceRecognitionProcessor, InMemoryStore)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        app = FaceAnalysis(name="buffalo_l", providers=["CUDAExecutionProvider", "CPUExecutionProvider"])
        app.prepare(ctx_id=0)
    frames = [synth_frame(240, 320, s) for s in (4, 5, 6, 21)]
    rng = np.random.default_rng(9)
    store = InMemoryStore()
    for i in range(300):
        store.add_employee(f"n{i}", "acme" if i % 2 else "other", rng.standard_normal(512).astype(np.float32), name=f"N{i}")
    for k in (0, 2):
        for j, f in enumerate(app.get(frames[k])):
            store.add_employee(f"face{k}_{j}", "acme", f.embedding, name=f"F{k}{j}")
    mgrs = {s: EmbeddingManager(store=store, device="cuda:0", scan=s) for s in ("f32", "f16")}

    class Sink:
        def __init__(self): self.rec, self.unk = [], 0
        def process_detection(self, pid, info, cam, ts, score): self.rec.append((pid, score))
        def process_unknown_detection(self, cam, ts, emb, bbox): self.unk += 1

    def run(mgr):
        proc = FaceRecognitionProcessor(mgr, face_detector=app)
        batch = proc.recognize_batch(frames, "acme")
        sinks, stats = [], []
        for f in frames:
            sinks.append(Sink())
            stats.append(CameraProcessor(mgr, sinks[-1], face_detector=app).process_frame(f, "cam0"))
        assert mgr._gallery.scan == mgr.scan and (mgr._gallery.S is None) == (mgr.scan == "f32")
        return batch, sinks, stats

    def same(a, b):
        (ba, sa, ta), (bb, sb, tb) = a, b
        assert len(ba) == len(bb) == len(frames)
        for fa, fb in zip(ba, bb):
            assert [r["person_id"] for r in fa] == [r["person_id"] for r in fb]
            for x, y in zip(fa, fb):
                assert np.array_equal(x["bbox"], y["bbox"])
                assert abs(float(x["recognition_score"]) - float(y["recognition_score"])) <= ATOL
        assert ta == tb and sum(t["faces"] for t in ta) >= 1
        for x, y in zip(sa, sb):
            assert [p for p, _ in x.rec] == [p for p, _ in y.rec] and x.unk == y.unk
        return [r["person_id"] for f in ba for r in f if r["person_id"] is not None]

    hit = same(run(mgrs["f32"]), run(mgrs["f16"]))
    assert hit and all(p.startswith("face") for p in hit)
    # the first matched person is re-enrolled with another face: an incremental sync rewrites that row (and its coarse copy)
    later = datetime.utcnow() + timedelta(seconds=5)
    store.employee_blobs[hit[0]] = pickle.dumps(rng.standard_normal(512).astype(np.float32))
    next(d for d in store.employees if d["_id"] == hit[0])["lastUpdated"] = later
    for m in mgrs.values():
        m.force_sync()
    again = same(run(mgrs["f32"]), run(mgrs["f16"]))
    assert hit[0] not in again
