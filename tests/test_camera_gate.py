"""CameraManager with an activity gate (no GPU: a fake processor and a fake gate): an UNCHANGED entry is served from the results
held for that source, gated frames are counted, a stopped or dead source is forgotten, and without a gate the processor call
is the one it always was."""
import queue
import time

import numpy as np


class FakeGate:
    def __init__(self):
        self.forgotten = []

    def forget(self, camera_id):
        self.forgotten.append(camera_id)


class FakeProcessor:
    """Answers UNCHANGED for the sources named in ``still``, a one-face list tagged (source, turn) otherwise."""

    def __init__(self):
        self.calls, self.annotated, self.still, self.turn = [], [], set(), 0

    def recognize_batch(self, frames, company_id, **kw):
        from facerecognition_infrenceengine_amd.processor import UNCHANGED
        self.turn += 1
        self.calls.append(([int(f[0, 0, 0]) for f in frames], company_id, kw))
        return [UNCHANGED if int(f[0, 0, 0]) in self.still else [{"tag": (int(f[0, 0, 0]), self.turn)}] for f in frames]

    def annotate(self, frame, res):
        self.annotated.append((int(frame[0, 0, 0]), res))
        return frame


def _manager(gate):
    from facerecognition_infrenceengine_amd.camera import CameraManager
    proc = FakeProcessor()
    cm = CameraManager(embedding_manager=None, processor=proc, gate=gate)
    cm.result_queue = queue.Queue(maxsize=64)
    return cm, proc


def _batch(sources):
    return [(s, np.full((4, 6, 3), s, np.uint8)) for s in sources]


def test_unchanged_sentinel_is_its_own_value():
    import pickle
    from facerecognition_infrenceengine_amd import processor
    from app.services import UNCHANGED, ActivityGate
    from facerecognition_infrenceengine_amd import ActivityGate as exported
    assert UNCHANGED is processor.UNCHANGED and ActivityGate is exported
    assert UNCHANGED is not None and UNCHANGED != [] and repr(UNCHANGED) == "UNCHANGED"
    assert pickle.loads(pickle.dumps(UNCHANGED)) is UNCHANGED


def test_unchanged_entries_are_served_from_the_held_results():
    gate = FakeGate()
    cm, proc = _manager(gate)
    first = cm.process_batch(_batch([0, 1, 2]), "acme")
    assert [r[0]["tag"] for r in first] == [(0, 1), (1, 1), (2, 1)] and cm.stats["gated_frames"] == 0
    # the gate and the sources, as camera ids, travel with the call
    assert proc.calls[0][2] == {"gate": gate, "camera_ids": [0, 1, 2]}
    proc.still = {0, 2}
    proc.annotated.clear()
    second = cm.process_batch(_batch([0, 1, 2]), "acme")
    assert second[0] is first[0] and second[2] is first[2]               # the held lists
    assert second[1][0]["tag"] == (1, 2)                                   # the processed frame's own, and it is held now
    assert proc.annotated == [(0, first[0]), (1, second[1]), (2, first[2])]      # the NEW frames, drawn with the held results
    assert cm.stats["gated_frames"] == 2 and cm.stats["frames"] == 6 and cm.stats["batches"] == 2
    proc.still = {0, 1, 2}
    third = cm.process_batch(_batch([2, 1]), "acme")                       # another order, a source absent
    assert third[0] is first[2] and third[1] is second[1] and cm.stats["gated_frames"] == 4
    assert proc.calls[2][2]["camera_ids"] == [2, 1]
    assert [cm.result_queue.get_nowait()[0] for _ in range(8)] == [0, 1, 2, 0, 1, 2, 2, 1]


def test_frames_of_two_sizes_take_their_own_sources_along():
    gate = FakeGate()
    cm, proc = _manager(gate)
    odd = [(0, np.full((4, 6, 3), 0, np.uint8)), (1, np.full((2, 2, 3), 1, np.uint8)), (2, np.full((4, 6, 3), 2, np.uint8))]
    cm.process_batch(odd, ["a", "b", "a"])
    assert [(tags, c, kw["camera_ids"]) for tags, c, kw in proc.calls] == [([0, 2], "a", [0, 2]), ([1], "b", [1])]


def test_no_gallery_is_held_like_any_result():
    """None (no gallery) from the processor is what the source's later UNCHANGED frames get: they leave untouched."""
    gate = FakeGate()
    cm, proc = _manager(gate)
    proc.recognize_batch = lambda frames, company_id, **kw: None
    assert cm.process_batch(_batch([5]), "nobody") == [None] and cm.stats["gated_frames"] == 0
    assert proc.annotated == []


def test_stop_forgets_every_source_and_drops_the_held_results():
    gate = FakeGate()
    cm, proc = _manager(gate)

    class Cap:
        def __init__(self, source):
            self.source = source

        def read(self):
            time.sleep(0.001)
            return True, np.full((4, 6, 3), self.source, np.uint8)

        def release(self):
            pass
    cm.capture_factory = Cap
    cm.start_cameras([3, 4], "acme", display=lambda s, f: None)
    deadline = time.time() + 10
    while time.time() < deadline and not {3, 4} <= set(cm._held):
        time.sleep(0.005)
    assert {3, 4} <= set(cm._held)
    cm.stop_cameras()
    assert sorted(gate.forgotten) == [3, 4] and cm._held == {} and cm.company_of == {}


def test_a_dead_source_is_forgotten():
    gate = FakeGate()
    from facerecognition_infrenceengine_amd.camera import CameraManager

    class DeadCap:
        def __init__(self, source):
            pass

        def read(self):
            return False, None

        def release(self):
            pass
    cm = CameraManager(None, processor=FakeProcessor(), capture_factory=DeadCap, reopen_after=1000, dead_after=1, gate=gate)
    cm._held[7] = [{"tag": 7}]
    cm.running = True
    cm.capture_frames(7, queue.Queue(maxsize=2))                           # one failed read: dead, no back-off sleep before it
    assert cm.stats["dead_sources"] == [7] and gate.forgotten == [7] and 7 not in cm._held


def test_without_a_gate_the_call_is_the_old_one():
    cm, proc = _manager(None)
    res = cm.process_batch(_batch([0, 1]), "acme")
    assert proc.calls == [([0, 1], "acme", {})]                            # no new keyword
    assert [r[0]["tag"] for r in res] == [(0, 1), (1, 1)] and "gated_frames" not in cm.stats
    cm.stop_cameras()                                                      # nothing to forget, nothing breaks
