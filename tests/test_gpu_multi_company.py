"""GPU end to end: one batch whose frames belong to different companies (FaceRecognitionProcessor.recognize_batch /
identify_batch with a per-frame company list, CameraManager.process_batch with one) against the same batch asked for one
company at a time - the only form there was before."""
import os
import queue
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

SEEDS = (4, 6, 5, 6, 21, 4)
IDS = ["acme", "globex", "initech", "acme", "nobody", "globex"]


@pytest.fixture(scope="module")
def app():
    from facerecognition_infrenceengine_amd import FaceAnalysis
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = FaceAnalysis(name="buffalo_l", providers=["CUDAExecutionProvider", "CPUExecutionProvider"])
        a.prepare(ctx_id=0)
    assert a.synthetic
    return a


@pytest.fixture(scope="module")
def world(app):
    """Three companies with rows (the faces of seeds 4 and 6 are enrolled for acme AND for globex, under each
    company's own ids; initech has noise rows only), a fourth id without rows; every single-company answer once."""
    from facerecognition_infrenceengine_amd.processor import EmbeddingManager, FaceRecognitionProcessor, InMemoryStore
    from make_golden import synth_frame
    frames = [synth_frame(240, 320, s) for s in SEEDS]
    rng = np.random.default_rng(9)
    store = InMemoryStore()
    for i in range(45):
        c = ("acme", "globex", "initech")[i % 3]
        store.add_employee(f"{c}_n{i}", c, rng.standard_normal(512).astype(np.float32), name=f"N{i}")
    for k in (0, 1):                                         # seeds 4 and 6
        faces = app.get(frames[k])
        assert faces
        for j, f in enumerate(faces):
            store.add_employee(f"acme_face{SEEDS[k]}_{j}", "acme", f.embedding, name=f"A{k}{j}")
            store.add_employee(f"globex_face{SEEDS[k]}_{j}", "globex", f.embedding, name=f"G{k}{j}")
    mgr = EmbeddingManager(store=store, device="cuda:0")
    proc = FaceRecognitionProcessor(mgr, face_detector=app)
    single = {c: proc.recognize_batch(frames, c) for c in sorted(set(IDS))}
    return dict(frames=frames, mgr=mgr, proc=proc, single=single)


def _same_faces(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x["bbox"], y["bbox"]) and x["person_id"] == y["person_id"]
        assert x["person_info"] == y["person_info"] and x["det_score"] == y["det_score"]
        assert abs(float(x["recognition_score"]) - float(y["recognition_score"])) < 5e-4


def test_mixed_recognize_batch_equals_the_single_company_batches(world):
    w = world
    assert w["single"]["nobody"] is None                     # a plain str: what it always returned
    assert all(isinstance(w["single"][c], list) and len(w["single"][c]) == 6 for c in ("acme", "globex", "initech"))
    got = w["proc"].recognize_batch(w["frames"], IDS)
    assert isinstance(got, list) and len(got) == 6
    for f, c in enumerate(IDS):
        if c == "nobody":
            assert got[f] is None                            # no gallery: None stands in, the other frames are served
        else:
            _same_faces(got[f], w["single"][c][f])
    # the frames of enrolled faces are recognised under their OWN company's ids
    for f in (0, 1, 3, 5):
        known = [r["person_id"] for r in got[f] if r["person_id"] is not None]
        assert known and all(p.startswith(IDS[f] + "_face") for p in known), (f, known)
    assert all(r["person_id"] is None for r in got[2])       # initech enrolled no face
    # a tuple is taken as a list; a wrong length is refused; only companies without rows: nothing runs
    _same_faces(w["proc"].recognize_batch(w["frames"][:2], ("acme", "globex"))[1], w["single"]["globex"][1])
    with pytest.raises(ValueError, match="one company id per frame"):
        w["proc"].recognize_batch(w["frames"], IDS[:3])
    assert w["proc"].recognize_batch(w["frames"][:2], ["nobody", "nowhere"]) == [None, None]
    assert w["proc"].recognize_batch(w["frames"][:2], "nobody") is None


def test_manager_hands_out_one_view_set_over_one_generation(world):
    mgr = world["mgr"]
    vs, metas, index_of = mgr.get_matchers_for_companies(IDS)
    assert index_of == [0, 1, 2, 0, None, 1] and len(vs) == 3 == len(metas)      # distinct companies once
    assert all(v.generation == vs.generation == mgr._gallery.generation for v in vs.views)
    for c, v in (("acme", 0), ("globex", 1), ("initech", 2)):
        view, meta = mgr.get_matcher_for_company(c)
        assert vs.views[v] is view and metas[v] is meta      # the cache get_matcher_for_company fills
    assert mgr.get_matchers_for_companies(IDS)[0] is vs      # and the set itself is kept


def test_identify_batch_equals_itself_per_company_and_agrees_with_recognize(world):
    w = world
    got = w["proc"].identify_batch(w["frames"], IDS, k=5)
    rec = w["proc"].recognize_batch(w["frames"], IDS)
    assert len(got) == 6
    for c in sorted(set(IDS)):
        one = w["proc"].identify_batch(w["frames"], c, k=5)
        assert isinstance(one, list) and len(one) == 6
        for f in [f for f, x in enumerate(IDS) if x == c]:
            if c == "nobody":
                assert got[f] is None and one[f] is None
                continue
            assert len(got[f]) == len(one[f]) == len(rec[f])
            for x, y, r in zip(got[f], one[f], rec[f]):
                assert np.array_equal(x["bbox"], y["bbox"]) and x["det_score"] == y["det_score"]
                assert [k["person_id"] for k in x["candidates"]] == [k["person_id"] for k in y["candidates"]]
                assert all(abs(float(a["score"]) - float(b["score"])) < 5e-4 for a, b in zip(x["candidates"], y["candidates"]))
                assert len(x["candidates"]) == 5 and np.array_equal(x["bbox"], r["bbox"])
                scores = [float(k["score"]) for k in x["candidates"]]
                assert scores == sorted(scores, reverse=True)
                if r["person_id"] is not None:               # candidates[0] is the row recognize_batch matched
                    assert x["candidates"][0]["person_id"] == r["person_id"]
                    assert abs(float(x["candidates"][0]["score"]) - float(r["recognition_score"])) < 5e-4
                else:
                    assert float(x["candidates"][0]["score"]) < w["proc"].recognition_threshold
    assert sum(r["person_id"] is not None for f in rec if f for r in f) >= 4
    hi = w["proc"].identify_batch(w["frames"], IDS, k=5, min_score=0.9)
    for fa, fb in zip(hi, got):                              # min_score cuts each ranked list where it falls below
        for x, y in zip(fa or (), fb or ()):
            keep = [k["person_id"] for k in y["candidates"] if k["score"] >= 0.9]
            assert [k["person_id"] for k in x["candidates"]] == keep and len(keep) < 5
    with pytest.raises(ValueError, match="k must be"):
        w["proc"].identify_batch(w["frames"], IDS, k=17)


def test_camera_batcher_takes_a_company_per_frame(world):
    from facerecognition_infrenceengine_amd.camera import CameraManager
    w = world
    cm = CameraManager(w["mgr"], processor=w["proc"])
    cm.result_queue = queue.Queue(maxsize=10)
    batch = [(10 + s, f.copy()) for s, f in enumerate(w["frames"])]
    got = cm.process_batch(batch, IDS)
    assert cm.stats["batches"] == 1 and cm.stats["frames"] == 6 and cm.stats["largest_batch"] == 6
    for f, c in enumerate(IDS):
        if c == "nobody":
            assert got[f] is None
        else:
            _same_faces(got[f], w["single"][c][f])
    outs = [cm.result_queue.get_nowait() for _ in range(6)]
    assert [s for s, _ in outs] == [10, 11, 12, 13, 14, 15] and all(o.shape == (240, 320, 3) for _, o in outs)
    assert np.array_equal(outs[4][1], w["frames"][4])        # no gallery: the frame leaves untouched
    assert not np.array_equal(outs[0][1], w["frames"][0])    # a served frame leaves annotated
