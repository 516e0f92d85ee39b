"""CameraManager with a HUD (no GPU: a stub processor): with a ``hud`` the batch goes through ``recognize_faces_batch`` and the frames
that call returns are queued; YUV captures need one; without one the calls are the ones made today."""
import queue

import numpy as np
import pytest


class StubProcessor:
    """Records every call.  ``recognize_faces_batch`` returns frames filled with 100 + source, so a queued frame shows where it
    came from; sources named in ``still`` are answered UNCHANGED."""

    def __init__(self):
        self.batch_calls, self.faces_calls, self.annotated, self.still, self.turn = [], [], [], set(), 0

    def _results(self, frames):
        from facerecognition_infrenceengine_amd.processor import UNCHANGED
        self.turn += 1
        return [UNCHANGED if int(f.flat[0]) in self.still else [{"tag": (int(f.flat[0]), self.turn)}] for f in frames]

    def recognize_batch(self, frames, company_id, **kw):
        self.batch_calls.append(([int(f.flat[0]) for f in frames], company_id, kw))
        return self._results(frames)

    def recognize_faces_batch(self, frames, company_id, hud, return_results=False, held=None, **kw):
        self.faces_calls.append(([int(f.flat[0]) for f in frames], company_id, hud, return_results, held,
                                 None if held is None else dict(held), kw))
        return [np.full((2, 3, 3), 100 + int(f.flat[0]), np.uint8) for f in frames], self._results(frames)

    def annotate(self, frame, res):
        self.annotated.append((int(frame.flat[0]), res))
        return frame


def _manager(**kw):
    from facerecognition_infrenceengine_amd.camera import CameraManager
    proc = StubProcessor()
    cm = CameraManager(embedding_manager=None, processor=proc, **kw)
    cm.result_queue = queue.Queue(maxsize=64)
    return cm, proc


def _batch(sources, shape=(4, 6, 3)):
    return [(s, np.full(shape, s, np.uint8)) for s in sources]


def _queued(cm):
    out = []
    while True:
        try:
            out.append(cm.result_queue.get_nowait())
        except queue.Empty:
            return out


def test_with_a_hud_the_processors_frames_are_queued():
    hud = object()
    cm, proc = _manager(hud=hud)
    res = cm.process_batch(_batch([0, 1, 2]), "acme")
    assert proc.batch_calls == [] and proc.annotated == []
    frames, company, got_hud, return_results, held, _, kw = proc.faces_calls[0]
    assert (frames, company, return_results, kw) == ([0, 1, 2], "acme", True, {}) and got_hud is hud and held is cm._held
    assert [r[0]["tag"] for r in res] == [(0, 1), (1, 1), (2, 1)]
    q = _queued(cm)
    assert [s for s, _ in q] == [0, 1, 2]
    assert all(f.shape == (2, 3, 3) and int(f[0, 0, 0]) == 100 + s for s, f in q)          # the drawn frames, not the input
    assert cm.stats["frames"] == 3 and cm.stats["batches"] == 1


def test_with_a_gate_held_results_are_kept_and_handed_to_the_draw():
    class Gate:
        def forget(self, camera_id):
            pass
    gate, hud = Gate(), object()
    cm, proc = _manager(hud=hud, gate=gate)
    first = cm.process_batch(_batch([0, 1]), "acme")
    assert proc.faces_calls[0][6] == {"gate": gate, "camera_ids": [0, 1]} and proc.faces_calls[0][5] == {}
    assert cm._held == {0: first[0], 1: first[1]}
    proc.still = {0}
    second = cm.process_batch(_batch([0, 1]), "acme")
    assert proc.faces_calls[1][4] is cm._held and proc.faces_calls[1][5] == {0: first[0], 1: first[1]}    # what the draw was given
    assert second[0] is first[0] and second[1][0]["tag"] == (1, 2) and cm._held[1] is second[1]
    assert cm.stats["gated_frames"] == 1
    assert [int(f[0, 0, 0]) for _, f in _queued(cm)] == [100, 101, 100, 101]


def test_yuv_frames_travel_with_their_format_and_need_a_hud():
    from facerecognition_infrenceengine_amd.camera import CameraManager
    for fmt in ("nv12", "i420"):
        with pytest.raises(ValueError, match="hud"):
            CameraManager(embedding_manager=None, processor=StubProcessor(), pixel_format=fmt)
    cm, proc = _manager(hud=object(), pixel_format="nv12", matrix="bt709")
    cm.process_batch(_batch([3, 4], shape=(6, 4)), ["a", "b"])
    assert proc.faces_calls[0][:2] == ([3, 4], ["a", "b"])
    assert proc.faces_calls[0][6] == {"pixel_format": "nv12", "matrix": "bt709"}
    assert [s for s, _ in _queued(cm)] == [3, 4]
    # BGR with a hud passes no format on
    cm, proc = _manager(hud=object())
    cm.process_batch(_batch([3]), "a")
    assert proc.faces_calls[0][6] == {}


def test_without_a_hud_the_calls_are_the_ones_made_today():
    cm, proc = _manager()
    batch = _batch([0, 1])
    res = cm.process_batch(batch, "acme")
    assert proc.faces_calls == [] and proc.batch_calls == [([0, 1], "acme", {})]              # no new keyword
    assert proc.annotated == [(0, res[0]), (1, res[1])]
    q = _queued(cm)
    assert [s for s, _ in q] == [0, 1] and all(f is batch[k][1] for k, (_, f) in enumerate(q))   # the host frames themselves
    assert cm.hud is None and cm.pixel_format == "bgr" and cm.matrix == "bt601"
