"""CameraManager with a redactor (no GPU: a stub processor): ``redact`` needs a ``hud``, travels to ``recognize_faces_batch`` with the
frames' sources as its keys, and a source that is gone is forgotten; without one the calls are the ones made today."""
import queue

import numpy as np
import pytest


class StubProcessor:
    def __init__(self):
        self.faces_calls, self.batch_calls, self.turn = [], [], 0

    def recognize_batch(self, frames, company_id, **kw):
        self.batch_calls.append(([int(f.flat[0]) for f in frames], company_id, kw))
        return [[] for _ in frames]

    def recognize_faces_batch(self, frames, company_id, hud, return_results=False, held=None, **kw):
        self.turn += 1
        self.faces_calls.append(([int(f.flat[0]) for f in frames], company_id, hud, kw))
        return [np.full((2, 3, 3), 100 + int(f.flat[0]), np.uint8) for f in frames], [[{"tag": self.turn}] for _ in frames]

    def annotate(self, frame, res):
        return frame


class StubRedactor:
    def __init__(self, fail=False):
        self.forgotten, self.fail = [], fail

    def forget(self, key):
        self.forgotten.append(key)
        if self.fail:
            raise RuntimeError("no such key")


def _manager(**kw):
    from facerecognition_infrenceengine_amd.camera import CameraManager
    proc = StubProcessor()
    cm = CameraManager(embedding_manager=None, processor=proc, **kw)
    cm.result_queue = queue.Queue(maxsize=64)
    return cm, proc


def _batch(sources, shape=(4, 6, 3)):
    return [(s, np.full(shape, s, np.uint8)) for s in sources]


def test_redact_without_a_hud_raises():
    from facerecognition_infrenceengine_amd.camera import CameraManager
    with pytest.raises(ValueError, match="redact needs a hud"):
        CameraManager(embedding_manager=None, processor=StubProcessor(), redact=StubRedactor())
    cm, _ = _manager(hud=object(), redact=None)
    assert cm.redact is None


def test_the_redactor_and_the_sources_are_passed_through():
    hud, red = object(), StubRedactor()
    cm, proc = _manager(hud=hud, redact=red)
    cm.process_batch(_batch([3, 4, 5]), "acme")
    frames, company, got_hud, kw = proc.faces_calls[0]
    assert (frames, company) == ([3, 4, 5], "acme") and got_hud is hud
    assert kw == {"redact": red, "redact_keys": [3, 4, 5]} and kw["redact"] is red
    q = []
    while not cm.result_queue.empty():
        q.append(cm.result_queue.get_nowait())
    assert [s for s, _ in q] == [3, 4, 5] and all(int(f[0, 0, 0]) == 100 + s for s, f in q)      # what the call returned is queued
    # beside an encoder, a gate and YUV frames the other arguments travel as they did
    class Gate:
        def forget(self, camera_id):
            pass
    gate, enc = Gate(), object()
    cm, proc = _manager(hud=hud, redact=red, gate=gate, encode=enc, pixel_format="nv12")
    cm.process_batch(_batch([7, 8], shape=(6, 4)), ["a", "b"])
    assert proc.faces_calls[0][3] == {"gate": gate, "camera_ids": [7, 8], "pixel_format": "nv12", "matrix": "bt601", "encode": enc,
                                      "redact": red, "redact_keys": [7, 8]}
    # frames of two sizes go in two calls, each with the sources of its own frames
    cm, proc = _manager(hud=hud, redact=red)
    cm.process_batch([(0, np.zeros((4, 6, 3), np.uint8)), (1, np.ones((8, 6, 3), np.uint8)), (2, np.full((4, 6, 3), 2, np.uint8))], "acme")
    assert sorted(c[3]["redact_keys"] for c in proc.faces_calls) == [[0, 2], [1]]


def test_without_a_redactor_no_new_keyword_is_passed():
    cm, proc = _manager(hud=object())
    cm.process_batch(_batch([0, 1]), "acme")
    assert proc.faces_calls[0][3] == {}
    cm, proc = _manager()
    cm.process_batch(_batch([0, 1]), "acme")
    assert proc.faces_calls == [] and proc.batch_calls == [([0, 1], "acme", {})]


def test_a_stopped_source_is_forgotten():
    red = StubRedactor()
    cm, _ = _manager(hud=object(), redact=red)
    cm._forget("lobby")
    cm._forget(("dock", 2))
    assert red.forgotten == ["lobby", ("dock", 2)]
    # a redactor that fails to forget does not take the camera loop down
    bad = StubRedactor(fail=True)
    cm, _ = _manager(hud=object(), redact=bad)
    cm._forget(5)
    assert bad.forgotten == [5]
    # the real one: the history of the source is gone, the others' stays
    from facerecognition_infrenceengine_amd.redact import Redactor
    real = Redactor(margin=0, linger=2)
    box = {"bbox": [1, 1, 5, 5], "person_info": {"type": "unknown"}}
    real.regions([[box], [box]], [(20, 20)] * 2, keys=["a", "b"])
    cm, _ = _manager(hud=object(), redact=real)
    cm._forget("a")
    cnt, _, _ = real.regions([[], []], [(20, 20)] * 2, keys=["a", "b"])
    assert cnt.tolist() == [0, 1]
