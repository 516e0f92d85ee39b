"""GPU end to end: face quality through the engine and its callers, on seeded 160 x 120 frames with the suite's synthetic
weights.  The reference for every verdict is tests/helpers/quality_ref.py on the crops that fr_warp_affine_5pt_slots writes; the
``sharp_min`` of the rejecting cases is the median of the reference's own sharpness over the faces found, so the reference alone
decides which faces go and which stay - and the fixture asserts that there are some of each."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from tests.helpers import quality_ref as qr

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

SEEDS = (9, 18, 19, 20, 21, 23, 3, 26)           # seed 3: a frame without a face
CAMS = ["lobby", "dock", 2, 3, 4, 5, 6, ("roof", 1)]
INF = float("inf")
ACCEPT = dict(min_eye=0, mean_lo=0, mean_hi=255, contrast_min=0, sharp_min=0, clip_max=qr.N, yaw_max=INF, pitch_lo=-INF,
              pitch_hi=INF)


class Sink:
    def __init__(self):
        self.calls = []

    def process_detection(self, pid, info, cam, ts, score):
        self.calls.append(("rec", cam, pid))

    def process_unknown_detection(self, cam, ts, emb, bbox):
        self.calls.append(("unk", cam, bbox))

    def process_unknown_cluster(self, cam, ts, cluster, is_new, count, bbox):
        self.calls.append(("clu", cam, cluster))


@pytest.fixture(scope="module")
def world():
    """The engine, the frames on host and device, the plain slot results, the crops of the slot warp with the reference's
    metrics on them (computed once), and the two quality objects."""
    from facerecognition_infrenceengine_amd import FaceAnalysis, FaceQuality, _lib
    from make_golden import synth_frame
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        app = FaceAnalysis(name="buffalo_l").prepare(ctx_id=0)
    assert app.synthetic and app.det_size is None
    frames = [synth_frame(120, 160, s) for s in SEEDS]
    dev = torch.from_numpy(np.stack(frames)).cuda()
    plain = app.detect_embed_slots(dev, compact_embed=True)
    N, cap = plain["bbox"].shape[:2]
    crops = torch.zeros((N * cap, 112, 112, 8), dtype=torch.float16, device="cuda")
    kps = plain["kps"].contiguous()
    app.lib.fr_warp_affine_5pt_slots(_lib.ptr(dev), N, 120, 160, _lib.ptr(kps), _lib.ptr(plain["counts"]), cap, 112, _lib.ptr(crops),
                                     _lib.stream_ptr())
    counts = plain["counts"].cpu().numpy()
    held = np.array([s % cap < counts[s // cap] for s in range(N * cap)])
    accept = FaceQuality(**ACCEPT)
    ref_accept = qr.measure(crops.cpu().numpy(), kps.cpu().numpy().reshape(-1, 5, 2), qr.ACCEPT_ALL, counts, cap)
    assert held.sum() >= 8 and (ref_accept[2][held] == 0).all()              # nothing is mirrored: accept-all accepts all
    median = int(np.median(ref_accept[0][held, 2]))
    lim = qr.ACCEPT_ALL.replace(sharp_min=median)
    ref = (ref_accept[0], ref_accept[1], np.array([qr.verdict_of(i, f, lim) if h else -1
                                                   for i, f, h in zip(ref_accept[0], ref_accept[1], held)], np.int32))
    fit, unfit = held & (ref[2] == 0), held & (ref[2] > 0)
    assert fit.sum() >= 2 and unfit.sum() >= 2, (fit.sum(), unfit.sum())     # otherwise the cases below would show nothing
    assert set(ref[2][unfit]) == {qr.BLURRED}
    return dict(app=app, frames=frames, dev=dev, plain=plain, N=N, cap=cap, crops=crops, counts=counts, held=held, ref=ref,
                ref_accept=ref_accept, fit=fit, unfit=unfit, accept=accept, strict=FaceQuality(**dict(ACCEPT, sharp_min=median)))


def _same_faces(a, b, held, N, cap):
    """every tensor of two slot results, bit for bit; the detector's rows of empty slots are not defined"""
    assert torch.equal(a["counts"], b["counts"])
    h = torch.from_numpy(held).cuda()
    for k in ("bbox", "kps", "det_score"):
        x, y = a[k].reshape(N * cap, -1)[h], b[k].reshape(N * cap, -1)[h]
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), k
    for k in ("embedding", "normed_embedding"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def _metrics_equal(r, ref, N, cap):
    qi, qf, v = (r[k].cpu().numpy() for k in ("quality", "quality_f", "quality_verdict"))
    assert qi.shape == (N, cap, 8) and qf.shape == (N, cap, 4) and v.shape == (N, cap)
    assert np.array_equal(qi.reshape(-1, 8), ref[0])
    assert np.array_equal(qf.reshape(-1, 4).view(np.uint32), ref[1].view(np.uint32))
    assert np.array_equal(v.reshape(-1), ref[2])


def test_accept_all_is_the_call_without_quality(world):
    w = world
    r = w["app"].detect_embed_slots(w["dev"], compact_embed=True, quality=w["accept"])
    _same_faces(r, w["plain"], w["held"], w["N"], w["cap"])
    assert set(r) == set(w["plain"]) | {"quality", "quality_f", "quality_verdict"}
    _metrics_equal(r, w["ref_accept"], w["N"], w["cap"])


def test_rejected_faces_are_not_embedded(world):
    w = world
    app, N, cap = w["app"], w["N"], w["cap"]
    r = app.detect_embed_slots(w["dev"], compact_embed=True, quality=w["strict"])
    _metrics_equal(r, w["ref"], N, cap)
    sel = torch.from_numpy(np.flatnonzero(w["fit"])).cuda()
    gathered = w["crops"].index_select(0, sel)
    emb, normed = app.embed_slots(gathered)
    assert torch.equal(r["embedding"][sel].view(torch.int32), emb.view(torch.int32))
    assert torch.equal(r["normed_embedding"][sel].view(torch.int32), normed.view(torch.int32))
    place = torch.zeros(512, device="cuda")
    place[0] = 1.0
    others = torch.from_numpy(np.flatnonzero(~w["fit"])).cuda()              # rejected and empty slots alike
    assert (r["embedding"][others] == place).all() and (r["normed_embedding"][others] == place).all()


def test_get_reports_quality_and_embeds_every_face(world):
    w = world
    app, cap = w["app"], w["cap"]
    for f in (0, 5, 6):
        base = app.get(w["frames"][f])
        faces = app.get(w["frames"][f], quality=w["strict"])
        assert len(faces) == len(base) == w["counts"][f]
        for j, (a, b) in enumerate(zip(faces, base)):
            s = f * cap + j
            assert np.array_equal(a.bbox, b.bbox) and "quality" not in b
            assert a.quality == w["strict"].describe(w["ref"][0][s], w["ref"][1][s], w["ref"][2][s])
            assert a.quality_ok == bool(w["fit"][s]) and a.quality["reasons"] == ([] if w["fit"][s] else ["blurred"])
            assert np.isfinite(a.embedding).all() and abs(np.linalg.norm(a.normed_embedding) - 1) < 1e-3 and a.embedding[1:].any()
    app.enable_graphs(True)                                                  # a call with quality runs eagerly all the same
    try:
        assert [f.quality_ok for f in app.get(w["frames"][0], quality=w["strict"])] == [bool(x) for x in w["fit"][:w["counts"][0]]]
    finally:
        app.enable_graphs(False)


def _processor(w, with_placeholder):
    """30 noise rows, the placeholder row of a rejected slot as a person of its own, and every face of the frames"""
    from facerecognition_infrenceengine_amd.processor import EmbeddingManager, FaceRecognitionProcessor, InMemoryStore
    rng = np.random.default_rng(9)
    store = InMemoryStore()
    for i in range(30):
        store.add_employee(f"n{i}", "acme", rng.standard_normal(512).astype(np.float32), name=f"N{i}")
    if with_placeholder:
        e0 = np.zeros(512, np.float32)
        e0[0] = 1
        store.add_employee("placeholder", "acme", e0, name="Nobody")
    E = w["plain"]["embedding"].cpu().numpy()
    for s in np.flatnonzero(w["held"]):
        store.add_employee(f"face{s}", "acme", E[s], name=f"F{s}")
    mgr = EmbeddingManager(store=store, device="cuda:0")
    return FaceRecognitionProcessor(mgr, face_detector=w["app"]), mgr


def test_recognize_batch_reports_a_rejected_face_as_unknown(world):
    w = world
    cap = w["cap"]
    proc, _ = _processor(w, True)
    plain = proc.recognize_batch(w["frames"], "acme")
    assert all("quality" not in d and "quality_ok" not in d for res in plain for d in res)
    assert all(d["person_id"] for res in plain for d in res)                 # every face is in the gallery
    for company in ("acme", ["acme"] * len(w["frames"])):                    # the plain and the mixed-company form
        res = proc.recognize_batch(w["frames"], company, quality=w["strict"])
        for f, faces in enumerate(res):
            assert len(faces) == w["counts"][f]
            for j, d in enumerate(faces):
                s = f * cap + j
                assert d["quality"] == w["strict"].describe(w["ref"][0][s], w["ref"][1][s], w["ref"][2][s])
                assert d["quality_ok"] == bool(w["fit"][s])
                if w["fit"][s]:
                    assert d["person_id"] == plain[f][j]["person_id"] and d["recognition_score"] > 0.45
                else:                                                        # its row IS the planted placeholder's
                    assert d["person_id"] is None and d["person_info"] == {"name": "Unknown", "type": "unknown"}
                    assert d["recognition_score"] == 0 and d["quality"]["reasons"] == ["blurred"]
        ident = proc.identify_batch(w["frames"], company, k=3, quality=w["strict"])
        for f, faces in enumerate(ident):
            for j, d in enumerate(faces):
                s = f * cap + j
                assert d["quality_ok"] == bool(w["fit"][s]) and bool(d["candidates"]) == bool(w["fit"][s])
    assert all("quality" not in d for res in proc.identify_batch(w["frames"], "acme", k=3) for d in res)


@pytest.mark.parametrize("with_placeholder", [True, False])
def test_process_batch_drops_rejected_faces(world, with_placeholder):
    """with the placeholder planted a rejected slot's row is "recognised", without it the row is unknown: either way the face
    reaches no manager call and no cluster"""
    from facerecognition_infrenceengine_amd.enrol import UnknownClusters
    from facerecognition_infrenceengine_amd.processor import CameraProcessor, EmbeddingManager, InMemoryStore
    w = world
    cap = w["cap"]
    rng = np.random.default_rng(10)
    store = InMemoryStore()
    for i in range(30):                                                      # noise rows only: every fit face is unknown
        store.add_employee(f"n{i}", "acme", rng.standard_normal(512).astype(np.float32), name=f"N{i}")
    if with_placeholder:
        e0 = np.zeros(512, np.float32)
        e0[0] = 1
        store.add_employee("placeholder", "acme", e0, name="Nobody")
    mgr = EmbeddingManager(store=store, device="cuda:0")
    sink, bank = Sink(), UnknownClusters("cuda:0")
    stats = CameraProcessor(mgr, sink, face_detector=w["app"], unknown_clusters=bank).process_batch(w["frames"], CAMS,
                                                                                                   quality=w["strict"])
    fit_of = [int(w["fit"][f * cap:(f + 1) * cap].sum()) for f in range(w["N"])]
    unfit_of = [int(w["unfit"][f * cap:(f + 1) * cap].sum()) for f in range(w["N"])]
    for f, st in enumerate(stats):
        assert st["faces"] == w["counts"][f] and st["low_quality"] == unfit_of[f]
        assert st["recognized"] + st["unknown"] <= fit_of[f] and len(st["unknown_clusters"]) == st["unknown"]
        assert st["recognized"] == 0
    assert sum(st["unknown"] for st in stats) >= 2                           # the fit faces do reach the clusters
    assert len(sink.calls) == sum(st["unknown"] for st in stats) and all(c[0] == "clu" for c in sink.calls)
    assert [c[1] for c in sink.calls] == [CAMS[f] for f, st in enumerate(stats) for _ in range(st["unknown"])]
    assert sum(bank.counts) == len(sink.calls)                            # no cluster counts a rejected face
    # the same call without quality: no new key, and the rejected faces are back
    sink2 = Sink()
    stats2 = CameraProcessor(mgr, sink2, face_detector=w["app"], unknown_clusters=UnknownClusters("cuda:0")).process_batch(
        w["frames"], CAMS)
    assert all("low_quality" not in st for st in stats2)
    assert len(sink2.calls) > len(sink.calls)


def test_enroller_refuses_an_unfit_pose_image(world):
    from facerecognition_infrenceengine_amd import GalleryMatcher
    from facerecognition_infrenceengine_amd.enrol import Enroller, largest_face_index
    w = world
    from facerecognition_infrenceengine_amd import Face, FaceQuality
    app, cap = w["app"], w["cap"]
    # the reference's sharpness of every frame's LARGEST face (the one enrolment takes); their median is this case's sharp_min,
    # so the reference alone says which pose images are refused
    bbox = w["plain"]["bbox"].cpu().numpy()
    sharp_of = {}
    for f in range(w["N"]):
        if w["counts"][f]:
            j = largest_face_index([Face(bbox=b) for b in bbox[f, :w["counts"][f]]])
            sharp_of[f] = int(w["ref"][0][f * cap + j, 2])
    thr = int(np.median(list(sharp_of.values())))
    q = FaceQuality(**dict(ACCEPT, sharp_min=thr))
    good = [f for f, s in sharp_of.items() if s >= thr]
    bad = [f for f, s in sharp_of.items() if s < thr]
    assert len(good) >= 2 and bad, sharp_of                                  # the premise
    m = GalleryMatcher("cuda:0")
    rng = np.random.default_rng(3)
    m.set_rows(list(range(20)), rng.standard_normal((20, 512)).astype(np.float32))
    en = Enroller(app, quality=q)
    frames = w["frames"]
    out = en.enrol([frames[good[0]], frames[6], frames[bad[0]], frames[good[1]]], m)     # frames[6] shows no face: skipped
    assert out == {"status": "low_quality", "image": 2, "reasons": ["blurred"]}
    ok = en.enrol([frames[good[0]], frames[good[1]]], m)
    assert ok["status"] in ("done", "different_people", "duplicate")
    plain = Enroller(app).enrol([frames[good[0]], frames[bad[0]]], m)
    assert plain["status"] != "low_quality"
    with pytest.raises(ValueError, match="quality"):
        en.enrol_batch([[frames[good[0]]]], m)
    with pytest.raises(ValueError, match="quality"):
        en.enrol_slots(w["plain"], [[0]], m)


def test_combinations_that_are_refused(world):
    from facerecognition_infrenceengine_amd import FaceTracks
    w = world
    app, q = w["app"], w["accept"]
    with pytest.raises(ValueError, match="compact_embed"):
        app.detect_embed_slots(w["dev"], quality=q)
    with pytest.raises(ValueError, match="crops_out"):
        app.detect_embed_slots(w["dev"], compact_embed=True, crops_out=w["crops"], quality=q)
    tracks = FaceTracks("cuda:0", slots=8)
    with pytest.raises(ValueError, match="tracks"):
        app.detect_embed_slots(w["dev"], compact_embed=True, tracks=tracks, camera_ids=CAMS, quality=q)
    proc, _ = _processor(w, False)
    for call in (proc.recognize_batch, proc.identify_batch):
        with pytest.raises(ValueError, match="tracks"):
            call(w["frames"], "acme", tracks=tracks, camera_ids=CAMS, quality=q)
