"""CameraManager with a JPEG encoder and the two routes that serve its frames (no GPU: a stub processor): with ``encode`` the
processor call gets it and the ``bytes`` it returns are queued and kept; without one the calls and the four old routes are the
ones of today."""
import queue

import numpy as np
import pytest


class StubProcessor:
    """``recognize_faces_batch`` returns, per frame, the bytes b"JPEG<source>.<turn>" when it is given an encoder and an array
    otherwise; every call is recorded."""

    def __init__(self):
        self.faces_calls, self.batch_calls, self.turn, self.refuse = [], [], 0, set()

    def recognize_batch(self, frames, company_id, **kw):
        self.batch_calls.append(([int(f.flat[0]) for f in frames], company_id, kw))
        return [[] for _ in frames]

    def recognize_faces_batch(self, frames, company_id, hud, return_results=False, held=None, **kw):
        self.turn += 1
        self.faces_calls.append(([int(f.flat[0]) for f in frames], company_id, hud, kw))
        if kw.get("encode") is not None:
            out = [None if int(f.flat[0]) in self.refuse else b"JPEG%d.%d" % (int(f.flat[0]), self.turn) for f in frames]
        else:
            out = [np.full((2, 3, 3), 100 + int(f.flat[0]), np.uint8) for f in frames]
        return out, [[] for _ in frames]

    def annotate(self, frame, res):
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


class Embeddings:
    def get_stats(self):
        return {"total_embeddings": 3}

    def force_sync(self):
        pass


def test_the_manager_queues_and_keeps_bytes():
    hud, enc = object(), object()
    cm, proc = _manager(hud=hud, encode=enc)
    assert cm.latest_jpeg(0) is None
    cm.process_batch(_batch([0, 1]), "acme")
    frames, company, got_hud, kw = proc.faces_calls[0]
    assert (frames, company) == ([0, 1], "acme") and got_hud is hud and kw == {"encode": enc} and kw["encode"] is enc
    assert _queued(cm) == [(0, b"JPEG0.1"), (1, b"JPEG1.1")]
    assert cm.latest_jpeg(0) == b"JPEG0.1" and cm.latest_jpeg(1) == b"JPEG1.1" and cm.latest_jpeg(2) is None
    cm.process_batch(_batch([1]), "acme")
    assert cm.latest_jpeg(0) == b"JPEG0.1" and cm.latest_jpeg(1) == b"JPEG1.2"
    assert cm.latest_jpeg(1, after=0, timeout=0) == (2, b"JPEG1.2") and cm.latest_jpeg(1, after=2, timeout=0) == (2, None)
    # a frame the encoder turned away is queued as the None it is and does not replace the last good picture
    proc.refuse = {1}
    cm.process_batch(_batch([1]), "acme")
    assert _queued(cm) == [(1, b"JPEG1.2"), (1, None)] and cm.latest_jpeg(1) == b"JPEG1.2"
    # YUV captures and the other options travel as before, the encoder beside them
    cm, proc = _manager(hud=hud, encode=enc, pixel_format="nv12", matrix="bt709")
    cm.process_batch(_batch([3], shape=(6, 4)), "acme")
    assert proc.faces_calls[0][3] == {"pixel_format": "nv12", "matrix": "bt709", "encode": enc}
    assert cm.source_named("3") == 3 and cm.source_named("4") is None


def test_latest_frame_returns_whatever_was_queued():
    cm, proc = _manager(hud=object(), encode=object())
    cm.capture_factory = lambda s: None
    cm.process_batch(_batch([5]), "acme")
    (source, item), = _queued(cm)
    with cm._latest_lock:
        cm.latest[source] = item                     # what the default consumer does with a queued item
    assert cm.latest_frame(5) == b"JPEG5.1" == cm.latest_jpeg(5)


def test_encode_without_a_hud_raises_and_without_encode_nothing_changes():
    from facerecognition_infrenceengine_amd.camera import CameraManager
    with pytest.raises(ValueError, match="hud"):
        CameraManager(embedding_manager=None, processor=StubProcessor(), encode=object())
    cm, proc = _manager(hud=object())
    cm.process_batch(_batch([0]), "acme")
    assert proc.faces_calls[0][3] == {} and cm.encode is None               # no new keyword reaches the processor
    (source, frame), = _queued(cm)
    assert isinstance(frame, np.ndarray) and cm.latest_jpeg(0) is None
    cm, proc = _manager()
    cm.process_batch(_batch([0]), "acme")
    assert proc.faces_calls == [] and proc.batch_calls == [([0], "acme", {})]


def test_snapshot_route():
    from facerecognition_infrenceengine_amd.server import create_app
    cm, proc = _manager(hud=object(), encode=object())
    c = create_app(Embeddings(), cm).test_client()
    r = c.get("/api/camera/snapshot?source=0")                              # before the first frame
    assert r.status_code == 404 and r.get_json()["status"] == "error" and r.get_json()["message"]
    assert r.headers["Access-Control-Allow-Origin"] == "*"
    cm.process_batch(_batch([0]) + [("rtsp://lobby/1", _batch([7])[0][1])], "acme")
    r = c.get("/api/camera/snapshot?source=0")
    assert r.status_code == 200 and r.mimetype == "image/jpeg" and r.data == b"JPEG0.1"
    assert r.headers["Access-Control-Allow-Origin"] == "*" and r.headers["Access-Control-Allow-Headers"] == "Content-Type"
    r = c.get("/api/camera/snapshot", query_string={"source": "rtsp://lobby/1"})
    assert r.status_code == 200 and r.data.startswith(b"JPEG")
    assert c.get("/api/camera/snapshot?source=9").status_code == 404
    # a manager without an encoder: 404, whatever it holds
    plain, _ = _manager(hud=object())
    plain.process_batch(_batch([0]), "acme")
    c = create_app(Embeddings(), plain).test_client()
    for route in ("/api/camera/snapshot?source=0", "/api/camera/stream?source=0"):
        r = c.get(route)
        assert r.status_code == 404 and r.get_json()["status"] == "error" and "encoder" in r.get_json()["message"]


def test_stream_route_sends_one_part_per_new_frame():
    from facerecognition_infrenceengine_amd.server import create_app
    cm, proc = _manager(hud=object(), encode=object())
    cm.process_batch(_batch([0]), "acme")
    c = create_app(Embeddings(), cm).test_client()
    r = c.get("/api/camera/stream?source=0", buffered=False)
    assert r.status_code == 200 and r.headers["Content-Type"] == "multipart/x-mixed-replace; boundary=frame"
    assert r.headers["Access-Control-Allow-Origin"] == "*"
    parts = iter(r.response)
    first = next(parts)
    assert first == b"--frame\r\nContent-Type: image/jpeg\r\nContent-Length: 7\r\n\r\nJPEG0.1\r\n"
    cm.process_batch(_batch([0]), "acme")                                   # the next frame arrives: the next part
    cm.process_batch(_batch([0]), "acme")                                   # and one the viewer was too slow for
    second = next(parts)
    assert second == b"--frame\r\nContent-Type: image/jpeg\r\nContent-Length: 7\r\n\r\nJPEG0.3\r\n"
    r.close()
    assert c.get("/api/camera/stream?source=9").status_code == 404


def test_the_four_old_routes_answer_as_before():
    from facerecognition_infrenceengine_amd.server import create_app
    started, stopped = [], []

    class Cam:
        def start_cameras(self, sources, company_id):
            started.append((sources, company_id))

        def stop_cameras(self):
            stopped.append(1)
    app = create_app(Embeddings(), Cam())
    rules = sorted(str(r) for r in app.url_map.iter_rules() if r.endpoint != "static")
    assert rules == ["/api/camera/snapshot", "/api/camera/start", "/api/camera/stop", "/api/camera/stream",
                     "/api/embeddings/stats", "/api/embeddings/sync"]
    c = app.test_client()
    r = c.get("/api/embeddings/stats")
    assert r.status_code == 200 and r.get_json() == {"total_embeddings": 3}
    r = c.post("/api/embeddings/sync")
    assert r.status_code == 200 and r.get_json() == {"status": "success", "message": "Sync completed"}
    r = c.post("/api/camera/start", json={"sources": [0]})
    assert r.status_code == 400 and r.get_json() == {"status": "error", "message": "Company ID required"}
    r = c.post("/api/camera/start", json={"sources": [0, 1], "company_id": "c1"})
    assert r.status_code == 200 and r.get_json() == {"status": "success", "message": "Camera started"}
    r = c.post("/api/camera/stop")
    assert r.status_code == 200 and r.get_json() == {"status": "success", "message": "Camera stopped"} and stopped == [1]
    # a manager that has never heard of an encoder answers the new routes with 404, not an error
    assert c.get("/api/camera/snapshot?source=0").status_code == 404
