"""Face quality above the engine without a GPU (fakes, as tests/test_camera_gate.py has them): ``FaceQuality`` validates and
describes, ``CameraManager`` hands it to the processor, ``Enroller`` refuses an unfit pose image and its batch forms, the engine
refuses the combinations it does not serve, and every default is "no quality"."""
import queue

import numpy as np
import pytest


class FakeProcessor:
    def __init__(self):
        self.calls = []

    def recognize_batch(self, frames, company_id, **kw):
        self.calls.append((len(frames), company_id, kw))
        return [[{"tag": i}] for i in range(len(frames))]

    def annotate(self, frame, res):
        return frame


def _batch(sources):
    return [(s, np.full((4, 6, 3), s, np.uint8)) for s in sources]


def test_exports_and_defaults():
    import inspect
    from app.services import FaceQuality
    from facerecognition_infrenceengine_amd import FaceQuality as exported
    from facerecognition_infrenceengine_amd.quality import REASONS
    assert FaceQuality is exported
    q = FaceQuality()
    assert q.limits() == (144.0, 40, 215, 100, 50, 1600, 0.5, 0.25, 0.75)
    assert [bit for bit, _ in REASONS] == [1, 2, 4, 8, 16, 32, 64, 128]
    assert "judgment, not a measurement" in inspect.getdoc(FaceQuality)
    assert FaceQuality(min_eye=7.5).min_eye2 == 56.25


@pytest.mark.parametrize("bad", [dict(min_eye=-1), dict(min_eye=float("nan")), dict(min_eye=float("inf")), dict(mean_lo=-1),
                                 dict(mean_hi=256), dict(contrast_min=-1), dict(sharp_min=-5), dict(clip_max=6401),
                                 dict(clip_max=-1), dict(yaw_max=-0.1), dict(yaw_max=float("nan")),
                                 dict(pitch_lo=0.8, pitch_hi=0.2), dict(pitch_lo=float("nan"))])
def test_arguments_are_validated(bad):
    from facerecognition_infrenceengine_amd.quality import FaceQuality
    with pytest.raises(ValueError):
        FaceQuality(**bad)


def test_describe():
    from facerecognition_infrenceengine_amd.quality import FaceQuality
    qi = np.array([120, 900, 33, 10, 20, 0, 0, 0], np.int32)
    qf = np.array([400.0, 200.0, 190.0, 400.0], np.float32)
    assert FaceQuality.describe(qi, qf, 0) == {"mean": 120, "contrast": 900, "sharp": 33, "dark": 10, "bright": 20, "eye_dist": 20.0,
                                               "ok": True, "reasons": []}
    d = FaceQuality.describe(qi, qf, 16 | 64)
    assert d["ok"] is False and d["reasons"] == ["blurred", "yaw"]
    assert FaceQuality.describe(qi, qf, 255)["reasons"] == ["small", "dark", "bright", "flat", "blurred", "clipped", "yaw", "pitch"]
    empty = FaceQuality.describe(np.zeros(8, np.int32), np.zeros(4, np.float32), -1)
    assert empty["ok"] is False and empty["reasons"] == []


def test_camera_manager_passes_quality_on():
    from facerecognition_infrenceengine_amd.camera import CameraManager
    from facerecognition_infrenceengine_amd.quality import FaceQuality
    q = FaceQuality()
    proc = FakeProcessor()
    cm = CameraManager(embedding_manager=None, processor=proc, quality=q)
    cm.result_queue = queue.Queue(maxsize=8)
    cm.process_batch(_batch([0, 1]), "acme")
    assert proc.calls == [(2, "acme", {"quality": q})]
    plain = FakeProcessor()
    cm = CameraManager(embedding_manager=None, processor=plain)
    cm.result_queue = queue.Queue(maxsize=8)
    cm.process_batch(_batch([0, 1]), "acme")
    assert plain.calls == [(2, "acme", {})]                                 # no new keyword without it
    with pytest.raises(ValueError, match="tracks"):
        CameraManager(embedding_manager=None, processor=proc, quality=q, tracks=object())


class FakeEngine:
    """``get`` answers from a table image tag -> [(bbox, fit)]; records the keywords it was called with"""
    device = "cpu"

    def __init__(self, table):
        self.table, self.calls = table, []

    def get(self, image, **kw):
        from facerecognition_infrenceengine_amd.face_analysis import Face
        self.calls.append(kw)
        faces = []
        for bbox, fit in self.table[int(image[0, 0, 0])]:
            f = Face(bbox=np.array(bbox, np.float32), normed_embedding=np.ones(512, np.float32))
            if "quality" in kw:
                f["quality"], f["quality_ok"] = {"ok": fit, "reasons": [] if fit else ["blurred", "yaw"]}, fit
            faces.append(f)
        return faces


def _image(tag):
    return np.full((4, 6, 3), tag, np.uint8)


def test_enroller_refuses_the_first_unfit_pose_image():
    from facerecognition_infrenceengine_amd.enrol import Enroller
    from facerecognition_infrenceengine_amd.quality import FaceQuality
    table = {0: [((0, 0, 10, 10), True)],
             1: [],                                                         # no face: skipped, as ever
             2: [((0, 0, 5, 5), False), ((0, 0, 30, 30), True)],            # the LARGEST face decides: fit
             3: [((0, 0, 40, 40), False), ((0, 0, 5, 5), True)],            # largest unfit
             4: [((0, 0, 9, 9), False)]}
    q = FaceQuality()
    eng = FakeEngine(table)
    en = Enroller(eng, quality=q)
    assert en.process_image(_image(2)) is not None and eng.calls[-1] == {"quality": q}
    out = en.enrol([_image(0), _image(1), _image(2), _image(3), _image(4)], matcher=None)
    assert out == {"status": "low_quality", "image": 3, "reasons": ["blurred", "yaw"]}
    assert len(eng.calls) == 1 + 4                                          # image 4 was not looked at
    with pytest.raises(ValueError, match="quality"):
        en.enrol_batch([[_image(0)]], None)
    with pytest.raises(ValueError, match="quality"):
        en.enrol_slots({}, [[0]], None)
    plain = FakeEngine(table)
    assert Enroller(plain).process_image(_image(3)) is not None and plain.calls == [{}]      # the old call, no new keyword


def test_engine_refuses_what_it_does_not_serve():
    from facerecognition_infrenceengine_amd import FaceAnalysis
    from facerecognition_infrenceengine_amd.quality import FaceQuality
    app = FaceAnalysis()
    app.det = object()                                                      # "prepared": the checks come before any device work
    q = FaceQuality()
    with pytest.raises(ValueError, match="compact_embed"):
        app.detect_embed_slots(None, quality=q)
    with pytest.raises(ValueError, match="crops_out"):
        app.detect_embed_slots(None, compact_embed=True, crops_out=object(), quality=q)
    with pytest.raises(ValueError, match="tracks"):
        app.detect_embed_slots(None, compact_embed=True, tracks=object(), camera_ids=[1, 2], quality=q)


def test_recognize_batch_refuses_quality_with_tracks():
    from facerecognition_infrenceengine_amd.processor import FaceRecognitionProcessor
    from facerecognition_infrenceengine_amd.quality import FaceQuality
    proc = FaceRecognitionProcessor(embedding_manager=None, face_detector=object())
    for call in (proc.recognize_batch, proc.identify_batch):
        with pytest.raises(ValueError, match="tracks"):
            call([_image(0)], "acme", tracks=object(), camera_ids=["a"], quality=FaceQuality())
