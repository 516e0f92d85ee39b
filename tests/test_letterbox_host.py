"""``det_size`` on the host (no GPU): the one geometry definition, the numpy reference canvas, and the camera batcher's
single call for a mixed-size batch."""
import queue

import numpy as np
import pytest

from facerecognition_infrenceengine_amd.letterbox import check_det_size, frame_table, letterbox_geometry


@pytest.mark.parametrize("hw,det_size,want", [
    ((1080, 1920), (640, 640), (360, 640, 1 / 3)),
    ((480, 640), (640, 640), (480, 640, 1.0)),
    ((1920, 1080), (640, 640), (640, 360, 1 / 3)),              # portrait
    ((1000, 1777), (640, 640), (360, 640, 0.36)),
    # 640 / (1280 / 910) is 455 exactly; in doubles the quotient is 454.99999999999994 and int() truncates it
    ((1280, 910), (640, 640), (640, 454, 0.5)),
    ((1080, 1920), (640, 480), (360, 640, 1 / 3)),              # non-square canvas, width first
    ((1920, 1080), (320, 256), (256, 144, 256 / 1920)),
    ((33, 47), (640, 640), (449, 640, 449 / 33)),               # upscaled
])
def test_geometry(hw, det_size, want):
    nh, nw, s = letterbox_geometry(hw[0], hw[1], det_size)
    assert (nh, nw) == want[:2]
    assert isinstance(s, np.float32) and s == np.float32(want[2]) == np.float32(nh / hw[0])
    assert nh <= det_size[1] and nw <= det_size[0] and (nh == det_size[1] or nw == det_size[0])


def test_geometry_refuses_a_frame_that_leaves_no_pixels():
    with pytest.raises(ValueError):
        letterbox_geometry(1, 2000, (640, 640))                 # nh = int(640 / 2000) = 0
    with pytest.raises(ValueError):
        letterbox_geometry(2000, 1, (640, 640))
    with pytest.raises(ValueError):
        letterbox_geometry(0, 10, (640, 640))
    with pytest.raises(ValueError):
        check_det_size((640, 0))
    assert check_det_size(None) is None and check_det_size(320) == (320, 320) and check_det_size([640, 480]) == (640, 480)


def test_frame_table_layout():
    from facerecognition_infrenceengine_amd import _lib
    import ctypes
    assert ctypes.sizeof(_lib.FrameRef) == 32
    tab, scale = frame_table([4096, 8192], [(1080, 1920), (480, 640)], (640, 640))
    assert tab.dtype == np.uint8 and tab.shape == (64,) and scale.dtype == np.float32
    words = tab.view(np.int32).reshape(2, 8)
    assert tab.view(np.int64).reshape(2, 4)[:, 0].tolist() == [4096, 8192]
    assert words[:, 2:6].tolist() == [[1080, 1920, 360, 640], [480, 640, 480, 640]]
    assert scale.tolist() == [np.float32(1 / 3), 1.0]
    tab, scale = frame_table([16], [(10, 12)])                  # a table for the warps alone
    assert tab.view(np.int32)[2:6].tolist() == [10, 12, 0, 0] and scale.tolist() == [1.0]


def test_reference_canvas_of_an_equal_size_frame_is_the_frame_plus_padding():
    from tests.helpers.letterbox_ref import canvas_ref
    rng = np.random.default_rng(0)
    frame = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)
    canvas, s = canvas_ref(frame, (640, 640))
    assert s == 1.0 and canvas.shape == (640, 640, 3)
    assert np.array_equal(canvas[:480], frame) and not canvas[480:].any()
    frame = rng.integers(0, 256, (100, 75, 3), dtype=np.uint8)   # portrait, non-square canvas
    canvas, s = canvas_ref(frame, (96, 100))
    assert s == 1.0 and np.array_equal(canvas[:, :75], frame) and not canvas[:, 75:].any()


class _FakeProcessor:
    def __init__(self):
        self.calls = []

    def recognize_batch(self, frames, company_id):
        self.calls.append([f.shape for f in frames])
        return [[{"tag": int(f[0, 0, 0])}] for f in frames]

    def annotate(self, frame, res):
        out = frame.copy()
        out[0, 0, 1] = res[0]["tag"] + 100
        return out


class _MixedProcessor(_FakeProcessor):
    accepts_mixed_sizes = True


def _batch():
    shapes = [(48, 64), (24, 32), (48, 64), (108, 192), (24, 32)]
    frames = []
    for i, (h, w) in enumerate(shapes):
        f = np.zeros((h, w, 3), np.uint8)
        f[0, 0, 0] = i
        frames.append(f)
    return [(f"cam{i}", f) for i, f in enumerate(frames)]


@pytest.mark.parametrize("mixed", [True, False])
def test_camera_batcher_makes_one_call_for_mixed_sizes_when_the_processor_takes_them(mixed):
    from facerecognition_infrenceengine_amd.camera import CameraManager
    proc = _MixedProcessor() if mixed else _FakeProcessor()
    cm = CameraManager(None, processor=proc)
    cm.result_queue = queue.Queue(maxsize=10)
    batch = _batch()
    results = cm.process_batch(batch, "acme")
    if mixed:
        assert proc.calls == [[f.shape for _, f in batch]]                      # ONE call, batch order
    else:                                                                       # grouped by shape, first appearance first
        assert proc.calls == [[(48, 64, 3)] * 2, [(24, 32, 3)] * 2, [(108, 192, 3)]]
    assert [r[0]["tag"] for r in results] == [0, 1, 2, 3, 4]                    # results in batch order
    outs = [cm.result_queue.get_nowait() for _ in range(5)]
    assert [s for s, _ in outs] == [f"cam{i}" for i in range(5)]                # queue order
    assert [int(o[0, 0, 1]) for _, o in outs] == [100, 101, 102, 103, 104]      # every frame annotated with ITS result
    assert [o.shape for _, o in outs] == [f.shape for _, f in batch]
    assert cm.stats["batches"] == 1 and cm.stats["frames"] == 5
