"""Tracks that judge above the engine without a GPU (fakes, as tests/test_camera_tracks.py has them): ``CameraManager`` hands
``FaceTracks(..., quality=q)`` on as ``tracks=`` alone - no ``quality=`` keyword, annotate and the dead-source path as under
plain tracks - and the processor's dict assembly for each action: embedded, carried (whatever this frame's verdict) and
rejected.  The two-argument form keeps raising (tests/test_camera_quality.py pins it too)."""
import queue

import numpy as np
import pytest
import torch

EMBED, CARRY, REJECT = 1, 2, 3
BLUR = 16


class JudgingTracks:
    """what CameraManager and the argument checks see of ``FaceTracks(..., quality=q)``"""

    def __init__(self, quality):
        self.quality, self.forgotten = quality, []

    def forget(self, camera_id):
        self.forgotten.append(camera_id)


class FakeProcessor:
    def __init__(self):
        self.calls, self.annotated = [], []

    def recognize_batch(self, frames, company_id, **kw):
        self.calls.append(kw)
        return [[{"bbox": np.array([1, 1, 3, 3]), "person_id": None, "person_info": {"name": "Unknown", "type": "unknown"},
                  "det_score": 0.9, "recognition_score": 0, "track_id": 4, "tracked": False, "quality": {"ok": False},
                  "quality_ok": False}] for _ in frames]

    def annotate(self, frame, res):
        self.annotated.append(res)
        return frame


def _batch(sources):
    return [(s, np.full((8, 8, 3), s, np.uint8)) for s in sources]


def test_camera_manager_needs_no_new_argument():
    from facerecognition_infrenceengine_amd.camera import CameraManager
    from facerecognition_infrenceengine_amd.quality import FaceQuality
    tracks, proc = JudgingTracks(FaceQuality()), FakeProcessor()
    cm = CameraManager(embedding_manager=None, processor=proc, tracks=tracks)
    cm.result_queue = queue.Queue(maxsize=8)
    res = cm.process_batch(_batch([3, 1]), "acme")
    assert proc.calls == [{"tracks": tracks, "camera_ids": [3, 1]}]          # the quality travels inside the tracks
    assert cm.quality is None and len(proc.annotated) == 2 and cm.result_queue.qsize() == 2
    assert res[0][0]["quality_ok"] is False and res[0][0]["track_id"] == 4
    cm._forget(3)                                                            # the dead-source path
    assert tracks.forgotten == [3]
    with pytest.raises(ValueError, match="tracks"):                          # the two-argument form keeps raising
        CameraManager(embedding_manager=None, processor=proc, tracks=tracks, quality=FaceQuality())


def test_annotate_takes_the_judged_tracked_dicts():
    from facerecognition_infrenceengine_amd.processor import FaceRecognitionProcessor
    proc = FaceRecognitionProcessor(embedding_manager=None, face_detector=object())
    frame = np.zeros((16, 16, 3), np.uint8)
    res = FakeProcessor().recognize_batch([frame], "acme")[0]
    res.append(dict(res[0], person_id="p1", person_info={"name": "P", "type": "employee"}, recognition_score=0.7, tracked=True))
    out = proc.annotate(frame.copy(), res)
    assert out.shape == frame.shape and out.any()


def _columns():
    """slot results of one frame, cap 4: embedded, carried though unfit, rejected, carried and fit"""
    qi = torch.zeros((1, 4, 8), dtype=torch.int32)
    qi[0, :, 2] = torch.tensor([80, 3, 2, 90])                               # sharp
    return {"counts": torch.tensor([4], dtype=torch.int32), "bbox": torch.arange(4.0).repeat(1, 4, 1),
            "det_score": torch.full((1, 4), 0.9),
            "track_id": torch.tensor([[5, 6, -1, 8]], dtype=torch.int32), "carried": torch.tensor([[0, 1, 0, 1]], dtype=torch.int32),
            "track_action": torch.tensor([[EMBED, CARRY, REJECT, CARRY]], dtype=torch.int32), "quality": qi,
            "quality_f": torch.full((1, 4, 4), 400.0), "quality_verdict": torch.tensor([[0, BLUR, BLUR, 0]], dtype=torch.int32)}


def test_recognize_dicts_for_each_action():
    from facerecognition_infrenceengine_amd.processor import _SlotFaces
    idx, score = torch.arange(4), torch.tensor([0.5 + j / 10 for j in range(4)])
    host = _SlotFaces(_columns(), 1, idx, score, None, dec=torch.ones(4, dtype=torch.int32))
    assert [bool(host.fit(0, j)) for j in range(4)] == [True, True, False, True]
    ids, meta = ["a", "b", "c", "d"], {k: {"name": k.upper(), "type": "employee"} for k in "abcd"}
    faces = host.frames([(ids, meta)], None, 1)[0]
    assert len(faces) == 4 and all(np.array_equal(f["bbox"], np.arange(4)) and f["det_score"] == np.float32(0.9) for f in faces)
    assert [f["person_id"] for f in faces] == ["a", "b", None, "d"]          # the carried unfit face keeps its row's answer
    assert [f["recognition_score"] for f in faces] == [np.float32(0.5), np.float32(0.6), 0, np.float32(0.8)]
    assert faces[2]["person_info"] == {"name": "Unknown", "type": "unknown"} and faces[2]["recognition_score"] == 0
    assert [f["tracked"] for f in faces] == [False, True, False, True] and [f["track_id"] for f in faces] == [5, 6, -1, 8]
    assert [f["quality_ok"] for f in faces] == [True, False, False, True]    # this frame's verdict, whatever the action
    assert [f["quality"]["sharp"] for f in faces] == [80, 3, 2, 90] and faces[1]["quality"]["reasons"] == ["blurred"]


def test_identify_dicts_for_each_action():
    from facerecognition_infrenceengine_amd.processor import _SlotFaces
    ids, meta = ["a", "b"], {k: {"name": k.upper(), "type": "employee"} for k in "ab"}
    rows, scores = torch.tensor([1, 0]).repeat(4, 1), torch.tensor([0.8, 0.6]).repeat(4, 1)
    faces = _SlotFaces(_columns(), 1, rows, scores, None).frames([(ids, meta)], None, 1)[0]
    assert [len(f["candidates"]) for f in faces] == [2, 2, 0, 2]
    assert [c["person_id"] for c in faces[0]["candidates"]] == ["b", "a"]
    assert all({"track_id", "tracked", "quality", "quality_ok"} <= set(f) for f in faces)


def test_plain_quality_and_plain_tracks_columns_are_as_they_were():
    from facerecognition_infrenceengine_amd.processor import _SlotFaces
    scan = (1, torch.arange(4), torch.zeros(4), None, torch.ones(4, dtype=torch.int32))
    r = _columns()
    del r["track_action"]                                                    # the quality-only call: the verdict decides
    host = _SlotFaces(r, *scan)
    assert host.action is None and [bool(host.fit(0, j)) for j in range(4)] == [True, False, False, True]
    host = _SlotFaces({k: v for k, v in r.items() if not k.startswith("quality")}, *scan)    # the tracks-only call
    assert host.quality is None and host.fit(0, 0) is True
    assert set(host.face(0, 0, ["a"] * 4, {"a": {}})) == {"bbox", "person_id", "person_info", "det_score", "recognition_score",
                                                            "track_id", "tracked"}


def test_the_two_argument_form_keeps_raising():
    from facerecognition_infrenceengine_amd import FaceAnalysis
    from facerecognition_infrenceengine_amd.processor import FaceRecognitionProcessor
    from facerecognition_infrenceengine_amd.quality import FaceQuality
    q = FaceQuality()
    tracks = JudgingTracks(q)
    proc = FaceRecognitionProcessor(embedding_manager=None, face_detector=object())
    for call in (proc.recognize_batch, proc.identify_batch):
        with pytest.raises(ValueError, match="quality together with tracks"):
            call([np.zeros((4, 6, 3), np.uint8)], "acme", tracks=tracks, camera_ids=["a"], quality=q)
    app = FaceAnalysis()
    app.det = object()
    with pytest.raises(ValueError, match="quality together with tracks"):
        app.detect_embed_slots(None, compact_embed=True, tracks=tracks, camera_ids=[1], quality=q)


def test_face_tracks_validates_the_new_arguments():
    import inspect
    from facerecognition_infrenceengine_amd.tracks import CARRY as C, EMBED as E, REJECT as R, FaceTracks
    assert (E, C, R) == (EMBED, CARRY, REJECT)
    sig = inspect.signature(FaceTracks.__init__).parameters
    assert sig["quality"].default is None and sig["max_age"].default == 8
    assert "judgment, not a measurement" in inspect.getdoc(FaceTracks).split("max_age=8")[1]
    with pytest.raises(ValueError, match="max_age"):
        FaceTracks(max_age=-1)
    for bad in (object(), "strict", 3):
        with pytest.raises(ValueError, match="FaceQuality"):
            FaceTracks(quality=bad)
