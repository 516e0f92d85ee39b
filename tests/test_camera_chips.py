"""CameraManager with chips (no GPU: a stub processor): ``chips`` travels to the processor call with or without a ``hud``, each
source's latest face dicts are kept with their chips, and ``GET /api/camera/faces`` serves them; without chips the calls are the
ones made today."""
import base64
import queue

import numpy as np
import pytest

from facerecognition_infrenceengine_amd.processor import UNCHANGED


class StubProcessor:
    """answers every frame with one face whose chip names the frame; frames whose first byte is 255 are UNCHANGED"""

    def __init__(self):
        self.faces_calls, self.batch_calls = [], []

    def _results(self, frames, kw):
        out = []
        for f in frames:
            tag = int(f.flat[0])
            if tag == 255:
                out.append(UNCHANGED)
                continue
            r = {"bbox": np.array([1, 2, 3 + tag, 4]), "person_id": None, "person_info": {"name": "Unknown", "type": "unknown"},
                 "det_score": 0.5, "recognition_score": 0}
            if kw.get("chips") is not None:
                r["chip"] = b"\xff\xd8chip%d" % tag
            out.append([r])
        return out

    def recognize_batch(self, frames, company_id, **kw):
        self.batch_calls.append(([int(f.flat[0]) for f in frames], company_id, kw))
        return self._results(frames, kw)

    def recognize_faces_batch(self, frames, company_id, hud, return_results=False, held=None, **kw):
        self.faces_calls.append(([int(f.flat[0]) for f in frames], company_id, hud, kw))
        return [np.zeros((2, 3, 3), np.uint8) for _ in frames], self._results(frames, kw)

    def annotate(self, frame, res):
        return frame


class Gate:
    def forget(self, camera_id):
        pass


def _manager(**kw):
    from facerecognition_infrenceengine_amd.camera import CameraManager
    proc = StubProcessor()
    cm = CameraManager(embedding_manager=None, processor=proc, **kw)
    cm.result_queue = queue.Queue(maxsize=64)
    return cm, proc


def _batch(sources, shape=(4, 6, 3), tags=None):
    return [(s, np.full(shape, s if tags is None else tags[k], np.uint8)) for k, s in enumerate(sources)]


def test_chips_travel_without_and_with_a_hud():
    chips = object()
    cm, proc = _manager(chips=chips)                          # no hud needed
    cm.process_batch(_batch([3, 4]), "acme")
    assert proc.faces_calls == [] and proc.batch_calls == [([3, 4], "acme", {"chips": chips})]
    hud, red = object(), object()
    cm, proc = _manager(chips=chips, hud=hud, redact=red)
    cm.process_batch(_batch([3, 4]), "acme")
    assert proc.faces_calls[0][3] == {"redact": red, "redact_keys": [3, 4], "chips": chips} and proc.batch_calls == []


def test_without_chips_no_new_keyword_is_passed_and_nothing_is_kept():
    cm, proc = _manager(hud=object())
    cm.process_batch(_batch([0, 1]), "acme")
    assert proc.faces_calls[0][3] == {}
    cm, proc = _manager()
    cm.process_batch(_batch([0, 1]), "acme")
    assert proc.batch_calls == [([0, 1], "acme", {})]
    assert cm.chips is None and cm.latest_faces(0) is None and cm._faces == {}


def test_latest_faces_keeps_each_sources_last_processed_frame():
    cm, _ = _manager(chips=object(), gate=Gate())
    assert cm.latest_faces("a") is None
    cm.process_batch(_batch(["a", "b"], tags=[1, 2]), "acme")
    assert cm.latest_faces("a")[0]["chip"] == b"\xff\xd8chip1" and cm.latest_faces("b")[0]["chip"] == b"\xff\xd8chip2"
    # an UNCHANGED frame leaves its source's faces as they are; the other source moves on
    res = cm.process_batch(_batch(["a", "b"], tags=[255, 7]), "acme")
    assert cm.latest_faces("a")[0]["chip"] == b"\xff\xd8chip1" and cm.latest_faces("b")[0]["chip"] == b"\xff\xd8chip7"
    assert res[0] is cm._held["a"] and res[0][0]["chip"] == b"\xff\xd8chip1"
    cm._forget("a")
    assert cm.latest_faces("a") is None and cm.latest_faces("b") is not None


def test_the_faces_route():
    pytest.importorskip("flask")
    from facerecognition_infrenceengine_amd.server import create_app
    cm, _ = _manager(chips=object())
    client = create_app(None, cm).test_client()
    miss = client.get("/api/camera/faces?source=lobby")
    assert miss.status_code == 404 and miss.get_json() == {"status": "error", "message": "No faces from this source"}
    cm.process_batch(_batch(["lobby", 5], tags=[9, 4]), "acme")
    got = client.get("/api/camera/faces?source=lobby")
    assert got.status_code == 200
    body = got.get_json()
    assert body == [{"bbox": [1, 2, 12, 4], "person_info": {"name": "Unknown", "type": "unknown"}, "recognition_score": 0.0,
                     "detection_score": 0.5, "chip": base64.b64encode(b"\xff\xd8chip9").decode()}]
    assert base64.b64decode(client.get("/api/camera/faces?source=5").get_json()[0]["chip"]) == b"\xff\xd8chip4"   # an int source by its text
    assert client.get("/api/camera/faces?source=6").status_code == 404
    # a face without a chip, and one whose chip is an array (encode=None), are served with null
    with cm._latest_lock:
        cm._faces["lobby"] = [dict(cm._faces["lobby"][0], chip=None), dict(cm._faces["lobby"][0], chip=np.zeros((16, 16, 3), np.uint8))]
    assert [f["chip"] for f in client.get("/api/camera/faces?source=lobby").get_json()] == [None, None]
    # a manager without chips knows no faces
    plain, _ = _manager()
    plain.company_of["lobby"] = "acme"
    assert create_app(None, plain).test_client().get("/api/camera/faces?source=lobby").status_code == 404
