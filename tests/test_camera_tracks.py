"""CameraManager with face tracks (no GPU: a fake processor, fake tracks and a fake gate): the tracks and the sources travel with
the processor call, beside a gate when there is one; a forgotten source frees its track slot too; without tracks the call is the
one it always was.  And the argument rule ``recognize_batch`` / ``identify_batch`` apply to ``camera_ids``."""
import queue

import numpy as np
import pytest


class Fake:
    def __init__(self):
        self.forgotten = []

    def forget(self, camera_id):
        self.forgotten.append(camera_id)


class FakeProcessor:
    def __init__(self):
        self.calls = []

    def recognize_batch(self, frames, company_id, **kw):
        self.calls.append(kw)
        return [[{"tag": int(f[0, 0, 0])}] for f in frames]

    def annotate(self, frame, res):
        return frame


def _manager(**kw):
    from facerecognition_infrenceengine_amd.camera import CameraManager
    proc = FakeProcessor()
    cm = CameraManager(embedding_manager=None, processor=proc, **kw)
    cm.result_queue = queue.Queue(maxsize=64)
    return cm, proc


def _batch(sources):
    return [(s, np.full((4, 6, 3), s, np.uint8)) for s in sources]


def test_tracks_travel_with_the_call_and_a_dead_source_is_forgotten():
    tracks = Fake()
    cm, proc = _manager(tracks=tracks)
    cm.process_batch(_batch([3, 1]), "acme")
    assert proc.calls == [{"tracks": tracks, "camera_ids": [3, 1]}]
    assert "gated_frames" not in cm.stats
    cm._forget(3)
    assert tracks.forgotten == [3]


def test_tracks_beside_a_gate_share_the_camera_ids():
    tracks, gate = Fake(), Fake()
    cm, proc = _manager(tracks=tracks, gate=gate)
    cm.process_batch(_batch([0, 2]), "acme")
    assert proc.calls == [{"gate": gate, "tracks": tracks, "camera_ids": [0, 2]}]
    cm._forget(2)
    assert tracks.forgotten == [2] and gate.forgotten == [2]


def test_without_tracks_the_call_is_the_one_it_was():
    cm, proc = _manager()
    cm.process_batch(_batch([0, 1]), "acme")
    assert proc.calls == [{}] and cm.tracks is None


def test_camera_ids_rule_is_shared_by_gate_and_tracks():
    from facerecognition_infrenceengine_amd.processor import _check_gate
    tracks = Fake()
    assert _check_gate(None, None, 3) is None and _check_gate(None, None, 3, None) is None
    assert _check_gate(None, ["a", "b"], 2, tracks) == ["a", "b"]
    assert _check_gate(Fake(), ("a", "b"), 2, tracks) == ["a", "b"]
    with pytest.raises(ValueError, match="tracks need camera_ids"):
        _check_gate(None, None, 2, tracks)
    with pytest.raises(ValueError, match="a gate needs camera_ids"):
        _check_gate(Fake(), None, 2, tracks)
    with pytest.raises(ValueError, match="one camera id per frame"):
        _check_gate(None, ["a"], 2, tracks)
    with pytest.raises(ValueError, match="repeated"):
        _check_gate(None, ["a", "a"], 2, tracks)
    with pytest.raises(ValueError, match="camera_ids come with a gate"):
        _check_gate(None, ["a", "b"], 2)


def test_face_tracks_is_exported():
    from app.services import FaceTracks
    from facerecognition_infrenceengine_amd import FaceTracks as exported
    from facerecognition_infrenceengine_amd.tracks import FaceTracks as own
    assert FaceTracks is exported is own
    for bad in ({"entries": 0}, {"entries": 65}, {"slots": 0}, {"iou_thr": 0.0}, {"iou_thr": 1.5}, {"max_reuse": -1},
                {"max_misses": -1}):
        with pytest.raises(ValueError):
            own(**bad)
