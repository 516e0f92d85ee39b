"""Enrolment in batches: fr_enrol_batch_f32 / fr_gallery_first_above_blocked_f32 against the CPU oracle
(oracle/enrol.py), against the one-job entries bit for bit, at the limit of the in-batch chain, and end to end."""
import os
import pickle
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DIM = 512
STATUS = {"done": 0, "no_face": 1, "different_people": 2, "duplicate": 3}


class _FakeApp:
    device = torch.device("cuda:0")


def _unit(v):
    return (v / np.linalg.norm(v)).astype(np.float32)


def _person(rng):
    return _unit(rng.standard_normal(DIM))


def _pose(rng, u, s=0.5):
    n = rng.standard_normal(DIM)
    return _unit(u + s * n / np.linalg.norm(n))


def _slots(images, cap, rng):
    """images: per image a list of (embedding, box) faces -> the dict detect_embed_slots returns (unused slots hold noise)"""
    n = len(images)
    E = rng.standard_normal((n * cap, DIM)).astype(np.float32)
    box = (rng.random((n, cap, 4)) * 500).astype(np.float32)
    counts = np.zeros(n, np.int32)
    for i, faces in enumerate(images):
        counts[i] = len(faces)
        for s, (e, b) in enumerate(faces):
            E[i * cap + s], box[i, s] = e, b
    dev = _FakeApp.device
    return {"counts": torch.from_numpy(counts).to(dev), "bbox": torch.from_numpy(box).to(dev),
            "normed_embedding": torch.from_numpy(E).to(dev)}


def _view_of(rows, ids, rng):
    """The rows as a GalleryView whose slot order is a permutation of the slab"""
    from facerecognition_infrenceengine_amd.gallery import DeviceGallery
    dg = DeviceGallery("cuda:0", capacity=max(len(ids), 1))
    perm = rng.permutation(len(ids))
    if len(ids):
        dg.upsert([ids[k] for k in perm], rows[perm], normalise=False)
    view = dg.view(ids)
    assert len(ids) < 2 or not np.array_equal(view.slots.cpu().numpy(), np.arange(len(ids)))
    return view


def _host(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---------------------------------------------------------------- 1. planted batch against the CPU oracle
BOX = (10.0, 20.0, 110.0, 140.0)


def _planted():
    rng = np.random.default_rng(7)
    A, X, Y, Z, W, V = (_person(rng) for _ in range(6))
    G = np.stack([_person(rng) for _ in range(300)])
    G[17], G[250] = _pose(rng, A), _pose(rng, A)
    one = lambda u: [(_pose(rng, u), BOX)]
    sized = lambda u, w, h: (_pose(rng, u), (5.0, 7.0, 5.0 + w, 7.0 + h))
    jobs = [
        [one(X), one(X), one(X)],
        [one(A), one(A)],
        [one(X), one(X)],
        [one(Y), one(Z), one(Z)],
        [[], []],
        [one(W), [], one(W)],
        [one(Y)],
        [[(_unit(A + X), BOX)]],
        [one(X)],
        [[sized(A, 40.0, 40.0), sized(A, 30.0, 30.0), sized(V, 80.5, 90.25), sized(A, 90.25, 80.5)]],
        [one(Y), one(Y), one(Z)],
    ]
    want = ["done", "duplicate", "duplicate", "different_people", "no_face", "done", "done", "duplicate", "duplicate", "done",
            "different_people"]
    return jobs, G, want


def _oracle_loop(jobs, G, sim_thr=0.4, dup_thr=0.4):
    """The definition: the jobs one after the other through oracle/enrol.py, a done job's unit row appended to the gallery.
    Returns per job (status, pair, dup position, chosen slots, avg, blob) and the smallest distance of any cosine the
    batch could be asked about to its threshold."""
    from oracle import enrol as o
    stored, owner, res, margin = [g for g in G], list(range(len(G))), [], np.inf
    for j, job in enumerate(jobs):
        faces, embs = [], []
        for im in job:
            if not im:
                faces.append(-1)
                continue
            k = o.largest_face_index([np.asarray(b, np.float32) for _, b in im])
            faces.append(k)
            embs.append(im[k][0])
        if not embs:
            res.append(("no_face", (-1, -1), -1, faces, None, None))
            continue
        for a in range(len(embs)):
            for b in range(a + 1, len(embs)):
                margin = min(margin, abs(o.cosine(embs[a], embs[b]) - sim_thr))
        ok, pair = o.check_image_similarity(embs, sim_thr)
        if not ok:
            res.append(("different_people", pair, -1, faces, None, None))
            continue
        avg = np.mean(embs, axis=0)
        assert avg.dtype == np.float32
        margin = min([margin] + [abs(o.cosine(avg, r) - dup_thr) for r in stored])
        dup, k = o.check_duplicate(avg, stored, dup_thr)
        if dup:
            res.append(("duplicate", (-1, -1), owner[k], faces, avg, None))
            continue
        res.append(("done", (-1, -1), -1, faces, avg, pickle.dumps(avg)))
        stored.append(_unit(avg))
        owner.append(len(G) + j)
    return res, margin


@pytest.fixture(scope="module")
def planted():
    jobs, G, want = _planted()
    res, margin = _oracle_loop(jobs, G)
    return jobs, G, want, res, margin


@pytest.mark.parametrize("kind", ["view", "matcher"])
def test_planted_batch_against_the_oracle(planted, kind):
    from facerecognition_infrenceengine_amd.enrol import Enroller
    from facerecognition_infrenceengine_amd.gallery import GalleryMatcher
    jobs, G, want, res, margin = planted
    # preconditions of the construction (asserted, not skipped): the scenario is the listed one, every job is compared,
    # and no decision hangs on a cosine near its threshold
    assert [r[0] for r in res] == want and len(res) == len(jobs) == 11
    print("smallest distance of a cosine to its threshold:", margin)
    assert margin >= 1e-3
    assert res[1][2] == 17 and res[2][2] == 300 + 0 and res[7][2] == 17 and res[8][2] == 300 + 0
    assert res[3][1] == (0, 1) and res[10][1] == (0, 2) and res[9][3] == [2] and res[5][3] == [0, -1, 0]
    rng = np.random.default_rng(70)
    ids = [f"p{i}" for i in range(len(G))]
    if kind == "view":
        gallery = _view_of(G, ids, rng)
    else:
        gallery = GalleryMatcher("cuda:0")
        gallery.set_rows(ids, G, normalise=False)
    images = [im for job in jobs for im in job]
    job_images, k = [], 0
    for job in jobs:
        job_images.append(list(range(k, k + len(job))))
        k += len(job)
    out = _host(Enroller(_FakeApp()).enrol_slots(_slots(images, 4, rng), job_images, gallery))
    k = 0
    for j, (status, pair, pos, faces, avg, blob) in enumerate(res):
        assert out["status"][j] == STATUS[status], j
        assert tuple(out["pair"][j]) == tuple(pair), j
        assert out["dup_pos"][j] == pos, j
        assert list(out["face"][k:k + len(faces)]) == faces, j
        k += len(faces)
        if avg is None:
            assert not out["avg"][j].any() and not out["row"][j].any()
        else:
            assert np.array_equal(out["avg"][j], avg), j                # the bits of np.mean(rows, axis=0)
            if blob is not None:
                assert pickle.dumps(out["avg"][j].copy()) == blob
            assert abs(np.linalg.norm(out["row"][j].astype(np.float64)) - 1) < 1e-6
        if status == "duplicate":
            assert out["dup_score"][j] > 0.4
        else:
            assert out["dup_score"][j] == 0


# ---------------------------------------------------------------- 2. against the one-job entries, bit for bit
def _one_job_entries(lib, found_rows, Gcur, ncur, sim_thr, dup_thr):
    """One job through fr_cosine_matrix_f32, fr_mean_rows_f32, fr_l2norm_rows_f32 and fr_gallery_first_above_f32"""
    from facerecognition_infrenceengine_amd._lib import ptr
    dev = Gcur.device
    K = len(found_rows)
    x = torch.from_numpy(np.stack(found_rows)).to(dev).contiguous()
    cos = torch.empty((K, K), dtype=torch.float32, device=dev)
    lib.fr_cosine_matrix_f32(ptr(x), ptr(x), K, K, DIM, ptr(cos), None)
    c = cos.cpu().numpy()
    for a in range(K):
        for b in range(a + 1, K):
            if c[a, b] < np.float32(sim_thr):
                return "different_people", (a, b), None, None, -1, 0.0
    avg = torch.empty((1, DIM), dtype=torch.float32, device=dev)
    q = torch.empty_like(avg)
    idx = torch.empty(1, dtype=torch.int64, device=dev)
    score = torch.empty(1, dtype=torch.float32, device=dev)
    ws = torch.empty(8, dtype=torch.uint8, device=dev)
    lib.fr_mean_rows_f32(ptr(x), K, DIM, ptr(avg), None)
    lib.fr_l2norm_rows_f32(ptr(avg), ptr(q), 1, DIM, None)
    lib.fr_gallery_first_above_f32(ptr(q), ptr(Gcur), 1, ncur, DIM, float(dup_thr), 0, 0, ptr(idx),
                                   ptr(score), ptr(ws), 8, None)
    i = int(idx.item())
    return ("duplicate" if i >= 0 else "done"), (-1, -1), avg, q, i, float(score.item())


def test_batch_equals_the_one_job_entries_bit_for_bit(lib):
    from facerecognition_infrenceengine_amd._lib import ptr
    from facerecognition_infrenceengine_amd.enrol import Enroller
    rng = np.random.default_rng(11)
    N, J = 4099, 40
    people = [_person(rng) for _ in range(12)]
    G = np.stack([_person(rng) for _ in range(N)])
    for k, p in enumerate(people[:4]):                                # four of the people are in the gallery already
        G[100 + 900 * k] = _pose(rng, p, 0.7)
    # pose noise 0.9 .. 1.5: the cosine of two poses of one person is about 1 / (1 + s^2), 0.55 .. 0.31 - both sides of 0.4;
    # one person per job, now and then a pose of somebody else
    jobs = []
    for _ in range(J):
        u = people[rng.integers(len(people))] if rng.random() < 0.85 else _person(rng)
        jobs.append([[(_pose(rng, u if rng.random() < 0.9 else people[rng.integers(len(people))], rng.uniform(0.9, 1.5)), BOX)]
                     for _ in range(rng.integers(1, 4))])
    ids = list(range(N))
    view = _view_of(G, ids, rng)
    dev = view.device
    Gcur = torch.zeros((N + J, DIM), dtype=torch.float32, device=dev)
    Gcur[:N] = view.rows()
    ncur, owner = N, []
    want = []
    with torch.cuda.device(dev):
        for j, job in enumerate(jobs):
            st, pair, avg, q, i, score = _one_job_entries(lib, [im[0][0] for im in job], Gcur, ncur, 0.4, 0.4)
            if st == "done":                                          # the row as upsert(normalise=True) stores it
                slot = torch.tensor([ncur], dtype=torch.int64, device=dev)
                lib.fr_gallery_update_rows_f32(ptr(Gcur), ptr(slot), ptr(avg), 1, DIM, 1, None)
                ncur += 1
                owner.append(j)
            pos = -1 if i < 0 else (i if i < N else N + owner[i - N])
            want.append((st, pair, pos, score, None if avg is None else avg.cpu().numpy()[0],
                         None if q is None else q.cpu().numpy()[0]))
    stored = Gcur[N:ncur].cpu().numpy()
    images = [im for job in jobs for im in job]
    job_images, k = [], 0
    for job in jobs:
        job_images.append(list(range(k, k + len(job))))
        k += len(job)
    out = _host(Enroller(_FakeApp()).enrol_slots(_slots(images, 2, rng), job_images, view))
    kinds = [w[0] for w in want]
    print({s: kinds.count(s) for s in set(kinds)}, "in-batch duplicates:", sum(w[2] >= N for w in want))
    # the scenario exercises every outcome, in-batch duplicates included
    assert set(kinds) == {"done", "different_people", "duplicate"} and any(w[2] >= N for w in want) and any(0 <= w[2] < N for w in want)
    for j, (st, pair, pos, score, avg, q) in enumerate(want):
        assert out["status"][j] == STATUS[st], j
        assert tuple(out["pair"][j]) == pair, j
        assert out["dup_pos"][j] == pos, j
        assert out["dup_score"][j].tobytes() == np.float32(score).tobytes(), j
        if avg is None:
            assert not out["avg"][j].any() and not out["row"][j].any()
        else:
            assert out["avg"][j].tobytes() == avg.tobytes(), j
            assert out["row"][j].tobytes() == q.tobytes(), j
    for k, j in enumerate(owner):                                     # and the row the gallery update stores is that row
        assert out["row"][j].tobytes() == stored[k].tobytes()


# ---------------------------------------------------------------- 3. the blocked scan alone
@pytest.mark.parametrize("N", [0, 3, 4099])
@pytest.mark.parametrize("F", [1, 5, 70])
def test_blocked_scan_equals_first_above(lib, F, N):
    from facerecognition_infrenceengine_amd._lib import ptr
    rng = np.random.default_rng(100 * F + N)
    dev = torch.device("cuda:0")
    cap = N + 37
    slab = np.stack([_person(rng) for _ in range(cap)])
    perm = rng.permutation(cap)[:N].astype(np.int64)
    Q = np.stack([_person(rng) for _ in range(F)])
    if N:
        for f in range(0, F, 2):                                      # every other query: its row planted twice (or thrice)
            spots = rng.choice(N, size=min(N, 3), replace=False)
            for p in spots:
                slab[perm[p]] = Q[f]                                  # a later query may overwrite a spot: still planted rows
    take = (rng.random(F) < 0.7).astype(np.int32)
    take[0] = 1
    if F > 1:
        take[1] = 0
    slab_d, Q_d = torch.from_numpy(slab).to(dev), torch.from_numpy(Q).to(dev)
    view_d, take_d = torch.from_numpy(perm).to(dev), torch.from_numpy(take).to(dev)
    dense_d = slab_d[view_d].contiguous() if N else torch.empty((0, DIM), dtype=torch.float32, device=dev)
    ws = torch.empty(F * 8, dtype=torch.uint8, device=dev)

    def old(thr, inclusive):
        idx = torch.empty(F, dtype=torch.int64, device=dev)
        score = torch.empty(F, dtype=torch.float32, device=dev)
        for f in range(F):                                            # per query, on the gathered rows
            lib.fr_gallery_first_above_f32(ptr(Q_d[f]), ptr(dense_d), 1, N, DIM, thr, inclusive, 0, ptr(idx[f:]),
                                           ptr(score[f:]), ptr(ws), 8, None)
        return idx.cpu().numpy(), score.cpu().numpy()

    def new(thr, inclusive, through_view, mask):
        idx = torch.full((F,), -7, dtype=torch.int64, device=dev)
        score = torch.full((F,), -7.0, dtype=torch.float32, device=dev)
        lib.fr_gallery_first_above_blocked_f32(ptr(Q_d), ptr(slab_d if through_view else dense_d),
                                               ptr(view_d) if through_view else None, ptr(take_d) if mask else None, F, N,
                                               DIM, thr, inclusive, 0, ptr(idx), ptr(score), ptr(ws), F * 8, None)
        return idx.cpu().numpy(), score.cpu().numpy()

    with torch.cuda.device(dev):
        i0, s0 = old(0.4, 0)
        if N:
            assert N < F or (i0[::2] >= 0).all()                      # the planted rows are found (N = 3: they overwrite each other)
        # a threshold that IS a score: '>' and '>=' part there
        thrs = [0.4] + ([float(s0[0])] if N else [])
        for thr in thrs:
            for inclusive in (0, 1):
                wi, wsc = (i0, s0) if (thr, inclusive) == (0.4, 0) else old(thr, inclusive)
                for through_view in (False, True):
                    for mask in (False, True):
                        gi, gs = new(thr, inclusive, through_view, mask)
                        ei = np.where(take == 0, -1, wi) if mask else wi
                        es = np.where(take == 0, np.float32(0), wsc) if mask else wsc
                        assert np.array_equal(gi, ei), (thr, inclusive, through_view, mask)
                        assert gs.tobytes() == es.astype(np.float32).tobytes(), (thr, inclusive, through_view, mask)
        if N:
            a, _ = old(thrs[-1], 0)
            b, _ = old(thrs[-1], 1)
            assert a[0] != b[0] or N < F                             # the two comparisons really differ at that threshold


# ---------------------------------------------------------------- 4. the chain at its limit
@pytest.mark.parametrize("case", ["one_person", "all_distinct", "alternating"])
def test_chain_at_the_job_limit(case):
    from facerecognition_infrenceengine_amd.enrol import ENROL_MAX_JOBS, Enroller
    from facerecognition_infrenceengine_amd.gallery import GalleryMatcher
    rng = np.random.default_rng(5)
    J = ENROL_MAX_JOBS
    P, R = _person(rng), _person(rng)
    if case == "one_person":
        who = [P] * J
    elif case == "alternating":
        who = [P, R] * (J // 2)
    images = [[(_person(rng) if case == "all_distinct" else _pose(rng, who[j]), BOX)] for j in range(J)]
    out = _host(Enroller(_FakeApp()).enrol_slots(_slots(images, 1, rng), [[j] for j in range(J)], GalleryMatcher("cuda:0")))
    if case == "all_distinct":
        assert (out["status"] == STATUS["done"]).all() and (out["dup_pos"] == -1).all()
        return
    first = 1 if case == "one_person" else 2
    assert (out["status"][:first] == STATUS["done"]).all() and (out["status"][first:] == STATUS["duplicate"]).all()
    want = np.zeros(J, np.int64) if case == "one_person" else np.arange(J) % 2        # empty gallery: N + i = i
    assert np.array_equal(out["dup_pos"][first:], want[first:])
    assert (out["dup_score"][first:] > 0.7).all()                     # two poses at noise 0.5: cosine about 0.8


# ---------------------------------------------------------------- 5. end to end
def test_enrol_batch_end_to_end():
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import synth_frame
    from facerecognition_infrenceengine_amd import FaceAnalysis
    from facerecognition_infrenceengine_amd.enrol import Enroller, EnrolBatchResult
    from facerecognition_infrenceengine_amd.gallery import DeviceGallery
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        app = FaceAnalysis(name="buffalo_l").prepare(ctx_id=0)
    en = Enroller(app)
    f4, f5 = synth_frame(240, 320, 4), synth_frame(240, 320, 5)
    blank = np.zeros((8, 8, 3), np.uint8)
    planted = en.process_image(f5)
    assert planted is not None
    rng = np.random.default_rng(1)
    G = rng.standard_normal((50, 512)).astype(np.float32)
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    G[7] = planted
    gids = [f"p{i}" for i in range(50)]
    jobs = [[f4, f4], [blank], [f5], [f4]]
    ids = ["new0", "new1", "new2", "new3"]

    def fresh_view():
        dg = DeviceGallery("cuda:0", capacity=64)
        dg.upsert(gids, G, normalise=False)
        return dg.view(gids)

    # the definition: enrol() job by job, a done job's row upserted before the next job
    view, want = fresh_view(), []
    for j, job in enumerate(jobs):
        r = en.enrol(job, view)
        want.append(r)
        if r["status"] == "done":
            view.gallery.upsert([ids[j]], r["embedding"][None], normalise=True)
            view = view.gallery.view(view.ids + [ids[j]])
    assert [r["status"] for r in want] == ["done", "no_face", "duplicate", "duplicate"]
    assert want[2]["duplicate_id"] == "p7" and want[3]["duplicate_id"] == "new0"
    assert en.check_duplicate(want[0]["embedding"], view) == (True, "new0")      # check_duplicate takes a view
    assert en.check_duplicate(planted, view) == (True, "p7")

    view0 = fresh_view()
    got = en.enrol_batch(jobs, view0, ids=ids, commit=True)
    assert isinstance(got, EnrolBatchResult) and len(got) == len(jobs)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g["status"] == w["status"] and g.get("pair") == w.get("pair"), j
        assert g.get("duplicate_id") == w.get("duplicate_id"), j
        if "embedding" in w:
            a, b = g["embedding"].astype(np.float64), w["embedding"].astype(np.float64)
            c = a @ b / (np.linalg.norm(a) * np.linalg.norm(b))
            print("job", j, "cosine of the two embeddings", c)
            assert g["embedding"].dtype == np.float32 and c >= 1 - 5e-4
        if g["status"] == "done":
            assert g["blob"] == pickle.dumps(g["embedding"]) and len(g["blob"]) == 2200
    assert got[3]["duplicate_of_job"] == 0 and "duplicate_of_job" not in got[2]
    # committed: the next batch, holding the same persons, sees this one's rows
    assert got.view.ids == gids + ["new0"] and got.view.generation == view0.gallery.generation
    with pytest.raises(Exception, match="stale"):
        en.enrol_batch([[f4]], view0)                                 # the old view is stale after the commit
    again = en.enrol_batch([[f4], [f4, f4], [f5]], got.view, ids=["x", "y", "z"], commit=True)
    assert [r["status"] for r in again] == ["duplicate"] * 3
    assert [r["duplicate_id"] for r in again] == ["new0", "new0", "p7"]
    assert again.view.ids == got.view.ids                             # nothing was enrolled
    # encoded bytes: what does not decode is an image without a face
    assert [r["status"] for r in en.enrol_batch([[b"not an image"], []], got.view)] == ["no_face", "no_face"]
