"""GPU end to end: ``recognize_batch`` / ``identify_batch`` with face tracks.  The contract: a face the camera's previous frame
showed at the same place, alone, keeps the embedding it was given (the embed net does not run for it) for ``max_reuse`` turns,
and that held embedding goes through the CURRENT call's gallery scan - the identity is never cached.  One engine without
``det_size`` (frames of one size) and one with ``det_size=(640, 640)`` and frames of two sizes.

The comparisons with the untracked call are exact where two identical untracked calls agree exactly (established first, per
engine, and printed); otherwise ``recognition_score`` is held to the 5e-4 of tests/test_gpu_activity_batch.py and everything
else stays exact.  A carried face is compared with the turn that embedded it by score BITS either way: the same embedding row
through the same scan."""
import os
import sys
import warnings
from datetime import datetime

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

CAMS = ["lobby", "dock", ("gate", 3), 17, "roof"]
# The synthetic detector finds "faces" in noise, and in most frames some of them overlap.  The rule never carries a face that
# another track of its camera touches (the crossing guard), so the cases about carrying use frames whose faces are finite and
# pairwise disjoint - the fixture asserts that premise on the engine's own boxes - and CROWDED is a frame whose faces are not,
# for the case about the guard.
SIZES = {"uniform": [(240, 320, 5), (240, 320, 2), (240, 320, 15), (240, 320, 46), (240, 320, 28)],
         "det_size": [(480, 640, 13), (240, 320, 3), (240, 320, 12), (480, 640, 23), (240, 320, 21)]}
SWAPPED = 1                                      # the frame replaced by another seed's frame
SWAP_SEED = {"uniform": 33, "det_size": 14}
CROWDED = (240, 320, 4)


@pytest.fixture(scope="module")
def app():
    from facerecognition_infrenceengine_amd import FaceAnalysis
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = FaceAnalysis(name="buffalo_l").prepare(ctx_id=0)
    assert a.synthetic and a.det_size is None
    return a


def _bits(x):
    return np.float32(x).view(np.uint32)


def _faces_equal(a, b, exact):
    """one frame's entry against another's (the track keys aside); False instead of an assertion"""
    if a is None or b is None:
        return a is None and b is None
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if not (np.array_equal(x["bbox"], y["bbox"]) and x["det_score"] == y["det_score"]):
            return False
        if "candidates" in x:
            if [c["person_id"] for c in x["candidates"]] != [c["person_id"] for c in y["candidates"]]:
                return False
            pairs = [(c["score"], d["score"]) for c, d in zip(x["candidates"], y["candidates"])]
        else:
            if x["person_id"] != y["person_id"] or x["person_info"] != y["person_info"]:
                return False
            pairs = [(x["recognition_score"], y["recognition_score"])]
        for s, t in pairs:
            if not (_bits(s) == _bits(t) if exact else abs(float(s) - float(t)) < 5e-4):
                return False
    return True


def _touching(eng, frame):
    """the faces of a frame, and how many of them have a non-finite box or a neighbour at IoU > 0 (the tracks' own metric)"""
    from tests.helpers.list_ref import F32Metric
    b = np.array([f.bbox for f in eng.get(frame)], np.float32).reshape(-1, 4)
    area, bad = F32Metric.area(b), 0
    for i in range(len(b)):
        with np.errstate(all="ignore"):
            o = F32Metric.overlap(b[i], area[i], b, area, 0)
        o[i] = 0
        bad += int(not np.isfinite(b[i]).all() or not (o <= 0).all())
    return len(b), bad


def _processor(eng, frames, one_person=False):
    """a store with 40 random rows and every face of frames 0, 1, 3 planted for two companies (``one_person``: the first face of
    frame 0 alone); the planted documents"""
    from facerecognition_infrenceengine_amd.processor import EmbeddingManager, FaceRecognitionProcessor, InMemoryStore
    rng = np.random.default_rng(9)
    store = InMemoryStore()
    for i in range(40):
        c = ("acme", "globex")[i % 2]
        store.add_employee(f"{c}_n{i}", c, rng.standard_normal(512).astype(np.float32), name=f"N{i}")
    planted = {}
    for k in (0, 1, 3):
        for j, f in enumerate(eng.get(frames[k])):
            planted[f"acme_face{k}_{j}"] = store.add_employee(f"acme_face{k}_{j}", "acme", f.embedding, name=f"A{k}{j}")
            store.add_employee(f"globex_face{k}_{j}", "globex", f.embedding, name=f"G{k}{j}")
            if one_person:
                break
        if one_person:
            break
    assert len(planted) >= (1 if one_person else 2)
    return FaceRecognitionProcessor(EmbeddingManager(store=store, device="cuda:0"), face_detector=eng), planted


@pytest.fixture(scope="module", params=["uniform", "det_size"])
def world(app, request):
    from make_golden import synth_frame
    eng = app if request.param == "uniform" else app.clone_with(det_size=(640, 640))
    frames = [synth_frame(h, w, s) for h, w, s in SIZES[request.param]]
    h, w, _ = SIZES[request.param][SWAPPED]
    swapped = list(frames)
    swapped[SWAPPED] = synth_frame(h, w, SWAP_SEED[request.param])
    crowded = list(frames)
    crowded[2] = synth_frame(*CROWDED)
    for f in frames + [swapped[SWAPPED]]:                        # the premise of every case about carrying
        n, bad = _touching(eng, f)
        assert n >= 1 and bad == 0, (n, bad)
    n, bad = _touching(eng, crowded[2])
    assert n > bad >= 2 or n == bad >= 2, (n, bad)               # the premise of the case about the guard
    proc, _ = _processor(eng, frames)
    # are two identical untracked calls the same bits?  They decide how the comparisons with the untracked call are held.
    first, second = proc.recognize_batch(frames, "acme"), proc.recognize_batch(frames, "acme")
    exact = all(_faces_equal(a, b, True) for a, b in zip(first, second))
    print(f"[{request.param}] two identical untracked recognize_batch calls agree exactly: {exact}")
    assert all(_faces_equal(a, b, exact) for a, b in zip(first, second))
    assert sum(len(r) for r in first) >= 3 and any(r["person_id"] for res in first for r in res)
    assert all("track_id" not in r and "tracked" not in r for res in first for r in res)
    return dict(kind=request.param, eng=eng, proc=proc, frames=frames, swapped=swapped, crowded=crowded, touching=bad,
                exact=exact, untracked=first, faces=sum(len(r) for r in first))


def _tracks(**kw):
    from facerecognition_infrenceengine_amd import FaceTracks
    return FaceTracks(slots=8, **kw)


def _count_forwards(monkeypatch, eng):
    """the faces each call of the embedder's forward was given"""
    calls = []
    real = eng.rec.forward

    def counting(crops, *a, **kw):
        calls.append(int(crops.shape[0]))
        return real(crops, *a, **kw)
    monkeypatch.setattr(eng.rec, "forward", counting)
    return calls


def _ids(res):
    return [None if frame is None else [r["track_id"] for r in frame] for frame in res]


def _same_answers(a, b):
    """person ids and score bits of two turns, face for face"""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert len(x) == len(y)
        for p, q in zip(x, y):
            assert np.array_equal(p["bbox"], q["bbox"]) and p["det_score"] == q["det_score"]
            assert p["person_id"] == q["person_id"] and _bits(p["recognition_score"]) == _bits(q["recognition_score"])


def test_max_reuse_zero_is_the_untracked_call_with_stable_ids(world):
    w, tracks = world, _tracks(max_reuse=0)
    turns = [w["proc"].recognize_batch(w["frames"], "acme", tracks=tracks, camera_ids=CAMS) for _ in range(3)]
    for t in turns:
        assert len(t) == 5 and all(_faces_equal(a, b, w["exact"]) for a, b in zip(t, w["untracked"]))
        assert all(r["tracked"] is False and isinstance(r["track_id"], int) and r["track_id"] >= 0 for res in t for r in res)
        assert _ids(t) == _ids(turns[0])
    for res in turns[0]:                                         # a camera's faces have distinct ids, counted from 0
        assert sorted(r["track_id"] for r in res) == list(range(len(res)))
    assert tracks.stats == {"faces": 3 * w["faces"], "embedded": 3 * w["faces"], "carried": 0, "untracked": 0}
    assert len(tracks) == 5 and tracks.slot_of("dock") is not None and tracks.slot_of("nobody") is None


def test_identical_frames_are_embedded_once_per_max_reuse_plus_one_turns(world, monkeypatch):
    w, tracks = world, _tracks(max_reuse=3)
    forwards = _count_forwards(monkeypatch, w["eng"])
    t1 = w["proc"].recognize_batch(w["frames"], "acme", tracks=tracks, camera_ids=CAMS)
    assert forwards == [w["faces"]]                              # turn 1 embeds every face
    assert all(_faces_equal(a, b, w["exact"]) for a, b in zip(t1, w["untracked"]))
    assert all(r["tracked"] is False for res in t1 for r in res)
    for turn in (2, 3, 4):
        t = w["proc"].recognize_batch(w["frames"], "acme", tracks=tracks, camera_ids=CAMS)
        assert forwards == [w["faces"]], turn                    # the embedder is not called at all
        assert all(r["tracked"] is True for res in t for r in res), turn
        assert _ids(t) == _ids(t1)
        _same_answers(t, t1)
    assert any(r["person_id"] for res in t1 for r in res)
    t5 = w["proc"].recognize_batch(w["frames"], "acme", tracks=tracks, camera_ids=CAMS)
    assert forwards == [w["faces"]] * 2                          # turn 5 re-embeds
    assert all(r["tracked"] is False for res in t5 for r in res) and _ids(t5) == _ids(t1)
    assert all(_faces_equal(a, b, w["exact"]) for a, b in zip(t5, w["untracked"]))
    assert tracks.stats == {"faces": 5 * w["faces"], "embedded": 2 * w["faces"], "carried": 3 * w["faces"], "untracked": 0}


def test_the_scan_of_the_current_call_answers_for_a_carried_face(world):
    """a planted person leaves the store between two identical turns: the carried face comes back Unknown.  The person is the
    only planted row of this store: the synthetic embedder's faces resemble one another, and with several planted the scan would
    answer with the next of them"""
    w, tracks = world, _tracks(max_reuse=3)
    proc, planted = _processor(w["eng"], w["frames"], one_person=True)
    t1 = proc.recognize_batch(w["frames"], "acme", tracks=tracks, camera_ids=CAMS)
    (gone,) = planted
    planted[gone]["status"] = "inactive"
    planted[gone]["lastUpdated"] = datetime.utcnow()
    proc.embedding_manager.force_sync()
    t2 = proc.recognize_batch(w["frames"], "acme", tracks=tracks, camera_ids=CAMS)
    assert all(r["tracked"] is True for res in t2 for r in res)
    seen = 0
    for a, b in zip(t1, t2):
        for p, q in zip(a, b):
            if p["person_id"] == gone:
                assert q["person_id"] is None and q["person_info"]["type"] == "unknown" and q["recognition_score"] == 0
                seen += 1
            else:
                assert q["person_id"] == p["person_id"]
    assert seen >= 1


def test_a_replaced_frame_is_embedded_under_new_ids_and_the_others_are_carried(world, monkeypatch):
    w, tracks = world, _tracks(max_reuse=3)
    t1 = w["proc"].recognize_batch(w["frames"], "acme", tracks=tracks, camera_ids=CAMS)
    forwards = _count_forwards(monkeypatch, w["eng"])
    t2 = w["proc"].recognize_batch(w["swapped"], "acme", tracks=tracks, camera_ids=CAMS)
    alone = w["proc"].recognize_batch([w["swapped"][SWAPPED]], "acme")[0]
    assert len(alone) >= 1 and forwards[0] == len(alone) and len(forwards) == 2     # the swapped frame's faces, then `alone`
    old = {r["track_id"] for r in t1[SWAPPED]}
    assert all(r["tracked"] is False and r["track_id"] >= 0 and r["track_id"] not in old for r in t2[SWAPPED])
    assert _faces_equal(t2[SWAPPED], alone, False)
    for k in range(5):
        if k != SWAPPED:
            assert all(r["tracked"] is True for r in t2[k]) and _ids(t2)[k] == _ids(t1)[k]
            _same_answers([t2[k]], [t1[k]])


def test_faces_that_touch_are_embedded_every_turn(world, monkeypatch):
    """the crossing guard, end to end: in a frame whose faces overlap, exactly the faces with a neighbour (or without a finite
    box, which never match a track) go through the embedder again; everything else is carried"""
    w, tracks = world, _tracks(max_reuse=3)
    want = w["proc"].recognize_batch(w["crowded"], "acme")
    forwards = _count_forwards(monkeypatch, w["eng"])
    t1 = w["proc"].recognize_batch(w["crowded"], "acme", tracks=tracks, camera_ids=CAMS)
    total = sum(len(r) for r in t1)
    assert forwards == [total] and all(_faces_equal(a, b, w["exact"]) for a, b in zip(t1, want))
    for turn in (2, 3):
        t = w["proc"].recognize_batch(w["crowded"], "acme", tracks=tracks, camera_ids=CAMS)
        assert forwards[-1] == w["touching"] and len(forwards) == turn
        assert sum(not r["tracked"] for r in t[2]) == w["touching"]
        assert all(r["tracked"] is True for k in (0, 1, 3, 4) for r in t[k])
        assert all(_faces_equal(a, b, False) for a, b in zip(t, want))


def test_an_unchanged_frame_does_not_move_its_cameras_tracks(world):
    """a frame the gate answers UNCHANGED never reaches the tracks, and the camera's next active turn continues its count"""
    from facerecognition_infrenceengine_amd import ActivityGate
    from facerecognition_infrenceengine_amd.processor import UNCHANGED
    w, tracks = world, _tracks(max_reuse=3)

    def call(frames, gate):
        return w["proc"].recognize_batch(frames, "acme", gate=gate, tracks=tracks, camera_ids=CAMS)

    def sinces(cam):
        st = tracks.tstate[tracks.slot_of(cam)].cpu().numpy()
        return sorted(st[st[:, 0] == 1][:, 1].tolist())
    quiet = [k for k in range(5) if k != SWAPPED]
    a, b, c = (ActivityGate(slots=8, max_hw=(480, 640)) for _ in range(3))
    t1 = call(w["frames"], a)                                    # a gate's first frames are active: every face is new
    assert all(r is not UNCHANGED for r in t1) and all(r["tracked"] is False for res in t1 for r in res)
    state1 = tracks.tstate.cpu().numpy().copy()
    t2 = call(w["swapped"], a)                                   # one frame active: only its camera's tracks move
    assert [r is UNCHANGED for r in t2] == [k != SWAPPED for k in range(5)]
    state2 = tracks.tstate.cpu().numpy().copy()
    for k, cam in enumerate(CAMS):
        s = tracks.slot_of(cam)
        assert np.array_equal(state2[s], state1[s]) == (k != SWAPPED), cam
    t3 = call(w["frames"], b)                                    # a new gate: all active, the quiet cameras' faces are carried
    assert all(r is not UNCHANGED for r in t3)
    for k in quiet:
        assert all(r["tracked"] is True for r in t3[k]) and sinces(CAMS[k]) == [1] * len(t1[k])
    state3 = tracks.tstate.cpu().numpy().copy()
    t4 = call(w["frames"], b)                                    # nothing moved: no frame reaches the tracks
    assert all(r is UNCHANGED for r in t4)
    assert np.array_equal(tracks.tstate.cpu().numpy(), state3)
    t5 = call(w["frames"], c)                                    # active again: since goes on from 1, the idle turn did not count
    for k in quiet:
        assert all(r["tracked"] is True for r in t5[k]) and sinces(CAMS[k]) == [2] * len(t1[k])
        assert _ids(t5)[k] == _ids(t1)[k]
        _same_answers([t5[k]], [t1[k]])


def test_forget_embeds_the_cameras_faces_under_new_ids(world):
    w, tracks = world, _tracks(max_reuse=3)
    t1 = w["proc"].recognize_batch(w["frames"], "acme", tracks=tracks, camera_ids=CAMS)
    cam = next(k for k in range(5) if len(t1[k]) >= 1)
    tracks.forget(CAMS[cam])
    assert len(tracks) == 4 and tracks.slot_of(CAMS[cam]) is None
    t2 = w["proc"].recognize_batch(w["frames"], "acme", tracks=tracks, camera_ids=CAMS)
    old = {r["track_id"] for r in t1[cam]}
    assert all(r["tracked"] is False and r["track_id"] not in old for r in t2[cam])
    for k in range(5):
        if k != cam:
            assert all(r["tracked"] is True for r in t2[k]) and _ids(t2)[k] == _ids(t1)[k]
    tracks.forget("never seen")                                  # unknown ids are ignored


def test_a_failed_embed_pass_drops_the_tracks_it_moved(world, monkeypatch):
    """the embedder fails between the two launches: the bank misses the turn's rows, so nothing of those cameras is carried next"""
    w, tracks = world, _tracks(max_reuse=3)
    t1 = w["proc"].recognize_batch(w["frames"], "acme", tracks=tracks, camera_ids=CAMS)

    def failing(crops, *a, **kw):
        raise RuntimeError("the embedder is down")
    with monkeypatch.context() as m:
        m.setattr(w["eng"].rec, "forward", failing)
        with pytest.raises(RuntimeError, match="the embedder is down"):
            w["proc"].recognize_batch(w["swapped"], "acme", tracks=tracks, camera_ids=CAMS)
    assert int(tracks.tstate[:, :, 0].sum()) == 0 and len(tracks) == 5
    t3 = w["proc"].recognize_batch(w["frames"], "acme", tracks=tracks, camera_ids=CAMS)
    assert all(r["tracked"] is False for res in t3 for r in res)
    assert all(_faces_equal(a, b, w["exact"]) for a, b in zip(t3, w["untracked"]))
    for k in range(5):
        assert not {r["track_id"] for r in t3[k]} & {r["track_id"] for r in t1[k]}


def test_per_frame_company_lists(world):
    w, proc = world, world["proc"]
    companies = ["acme", "nobody", "acme", "globex", "globex"]
    tracks = _tracks(max_reuse=3)
    want = proc.recognize_batch(w["frames"], companies)
    t1 = proc.recognize_batch(w["frames"], companies, tracks=tracks, camera_ids=CAMS)
    t2 = proc.recognize_batch(w["frames"], companies, tracks=tracks, camera_ids=CAMS)
    assert t1[1] is None and t2[1] is None
    assert all(_faces_equal(a, b, w["exact"]) for a, b in zip(t1, want))
    for k in (0, 2, 3, 4):
        assert all(r["tracked"] is False for r in t1[k]) and all(r["tracked"] is True for r in t2[k])
        _same_answers([t2[k]], [t1[k]])
    assert all(r["person_id"] is None or r["person_id"].startswith("globex_") for r in t2[3])
    tracks = _tracks(max_reuse=3)
    want = proc.identify_batch(w["frames"], companies, k=3)
    i1 = proc.identify_batch(w["frames"], companies, k=3, tracks=tracks, camera_ids=CAMS)
    i2 = proc.identify_batch(w["frames"], companies, k=3, tracks=tracks, camera_ids=CAMS)
    assert i1[1] is None and all(_faces_equal(a, b, w["exact"]) for a, b in zip(i1, want))
    for k in (0, 2, 3, 4):
        assert all("candidates" in r and r["tracked"] is True for r in i2[k])
        assert _faces_equal(i2[k], i1[k], True) and _ids(i2)[k] == _ids(i1)[k]


def test_argument_errors_and_the_untracked_call_afterwards(world):
    w, proc, tracks = world, world["proc"], _tracks()
    with pytest.raises(ValueError, match="camera_ids"):
        proc.recognize_batch(w["frames"], "acme", tracks=tracks)
    with pytest.raises(ValueError, match="camera_ids"):
        proc.identify_batch(w["frames"], ["acme"] * 5, tracks=tracks)
    with pytest.raises(ValueError, match="repeated"):
        proc.recognize_batch(w["frames"], "acme", tracks=tracks, camera_ids=CAMS[:4] + CAMS[:1])
    with pytest.raises(ValueError, match="one camera id per frame"):
        proc.recognize_batch(w["frames"], "acme", tracks=tracks, camera_ids=CAMS[:3])
    import torch
    dev = torch.from_numpy(np.stack(w["frames"][1:3])).to("cuda:0") if w["kind"] == "uniform" else \
        [torch.from_numpy(f).to("cuda:0") for f in w["frames"][1:3]]
    with pytest.raises(ValueError, match="compact_embed"):
        w["eng"].detect_embed_slots(dev, compact_embed=False, tracks=tracks, camera_ids=CAMS[:2])
    with pytest.raises(ValueError, match="camera_ids"):
        w["eng"].detect_embed_slots(dev, compact_embed=True, tracks=tracks)
    assert len(tracks) == 0 and int(tracks.tstate.abs().sum()) == 0          # no refused call took a slot or moved state
    # no gallery: the None of the untracked call comes first and the tracks do not move
    assert proc.recognize_batch(w["frames"], "nobody", tracks=tracks, camera_ids=CAMS) is None
    assert len(tracks) == 0
    r = w["eng"].detect_embed_slots(dev, compact_embed=True, tracks=tracks, camera_ids=CAMS[:2])
    assert r["track_id"].dtype == torch.int32 and r["track_id"].shape == r["carried"].shape == r["det_score"].shape
    assert int(r["carried"].sum()) == 0
    again = proc.recognize_batch(w["frames"], "acme")
    assert all(_faces_equal(a, b, w["exact"]) for a, b in zip(again, w["untracked"]))
    assert all("track_id" not in r for res in again for r in res)
