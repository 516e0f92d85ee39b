"""GPU end to end: ``recognize_faces_batch(..., hud, encode=enc)`` - the engine pass, the HUD drawn on the ring's device frames,
the drawn frames encoded on the device, the JPEG stream read back.  The bytes are tests/helpers/jpeg_ref.py of the arrays the
same call returns without ``encode``, and the results are that call's."""
import os
import sys
import warnings

import numpy as np
import pytest

from tests.helpers import jpeg_ref, yuv_ref

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

SEEDS = (9, 11, 0, 3)                  # 120 x 160 frames with 2, 2, 1 and 0 faces
QUALITY = 80


@pytest.fixture(scope="module")
def world():
    from facerecognition_infrenceengine_amd import FaceAnalysis
    from facerecognition_infrenceengine_amd.processor import EmbeddingManager, FaceRecognitionProcessor, InMemoryStore
    from make_golden import synth_frame
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        eng = FaceAnalysis(name="buffalo_l").prepare(ctx_id=0)
    assert eng.synthetic and eng.det_size is None
    frames = [synth_frame(120, 160, s) for s in SEEDS]
    rng = np.random.default_rng(3)
    store = InMemoryStore()
    for i in range(30):
        store.add_employee(f"n{i}", "acme", rng.standard_normal(512).astype(np.float32), name=f"N{i}")
    faces = eng.get(frames[0]) + eng.get(frames[2])
    assert len(faces) >= 2
    store.add_employee("e0", "acme", faces[0].embedding, name="Ada Lovelace", employeeId="E-0042")
    store.add_visitor("v0", "acme", faces[-1].embedding, name="A Visitor")
    proc = FaceRecognitionProcessor(EmbeddingManager(store=store, device="cuda:0"), face_detector=eng)
    return dict(eng=eng, proc=proc, frames=frames)


def _same_results(a, b):
    """two result lists of a batch: everything exact but the recognition score, held to the 5e-4 of the other batch tests"""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is None:
            continue
        assert len(x) == len(y)
        for p, q in zip(x, y):
            assert np.array_equal(p["bbox"], q["bbox"]) and p["det_score"] == q["det_score"]
            assert p["person_id"] == q["person_id"] and p["person_info"] == q["person_info"]
            assert abs(float(p["recognition_score"]) - float(q["recognition_score"])) < 5e-4


def _both(proc, frames, hud, enc, **kw):
    """the call without and with ``encode``: the arrays, the bytes; the results must agree"""
    arrays, res = proc.recognize_faces_batch(frames, "acme", hud, return_results=True, **kw)
    coded, res_coded = proc.recognize_faces_batch(frames, "acme", hud, return_results=True, encode=enc, **kw)
    _same_results(res, res_coded)
    assert len(coded) == len(arrays) and all(isinstance(b, bytes) for b in coded)
    for k, (a, b) in enumerate(zip(arrays, coded)):
        assert b == jpeg_ref.encode(a, QUALITY), k
    return arrays, coded, res


def test_bgr_frames_full_size_and_previews(world):
    from facerecognition_infrenceengine_amd import Hud, JpegEncoder
    proc, frames, enc = world["proc"], world["frames"], JpegEncoder(QUALITY)
    arrays, coded, res = _both(proc, frames, Hud(), enc)
    assert sum(len(r) for r in res) >= 3 and not np.array_equal(arrays[0], frames[0])          # a HUD is in the picture
    assert coded[0][:2] == b"\xff\xd8" and coded[0][-2:] == b"\xff\xd9" and coded[0][:629] == enc.header(120, 160)
    arrays, coded, _ = _both(proc, frames, Hud(out_size=(80, 60)), enc)
    assert arrays[0].shape == (60, 80, 3) and coded[0][:629] == enc.header(60, 80)
    # without return_results: the bytes alone
    alone = proc.recognize_faces_batch(frames, "acme", Hud(out_size=(80, 60)), encode=enc)
    assert alone == coded


def test_nv12_frames_full_size_and_previews(world):
    from facerecognition_infrenceengine_amd import Hud, JpegEncoder
    proc, enc = world["proc"], JpegEncoder(QUALITY)
    nv12 = [yuv_ref.bgr_to_yuv420(f, "nv12") for f in world["frames"]]
    _both(proc, nv12, Hud(), enc, pixel_format="nv12")
    _both(proc, nv12, Hud(out_size=(96, 96)), enc, pixel_format="nv12")


def test_frames_of_two_sizes_through_a_det_size_engine(world):
    from facerecognition_infrenceengine_amd import Hud, JpegEncoder
    from facerecognition_infrenceengine_amd.processor import FaceRecognitionProcessor
    from make_golden import synth_frame
    eng = world["eng"].clone_with(det_size=(640, 640))
    proc = FaceRecognitionProcessor(world["proc"].embedding_manager, face_detector=eng)
    frames = [world["frames"][0], synth_frame(240, 320, 4), world["frames"][1]]
    enc = JpegEncoder(QUALITY)
    arrays, coded, res = _both(proc, frames, Hud(), enc)
    assert [a.shape for a in arrays] == [f.shape for f in frames] and sum(len(r) for r in res) >= 3
    assert coded[1][:629] == enc.header(240, 320)
    _both(proc, frames, Hud(out_size=(80, 60)), enc)


def test_the_ring_turn_is_released(world):
    """more calls than the ring is deep (2): a turn that was not released would make the third upload wait for ever"""
    from facerecognition_infrenceengine_amd import Hud, JpegEncoder
    proc, frames, hud, enc = world["proc"], world["frames"], Hud(), JpegEncoder(QUALITY)
    first = proc.recognize_faces_batch(frames, "acme", hud, encode=enc)
    for _ in range(3):
        assert proc.recognize_faces_batch(frames, "acme", hud, encode=enc) == first
    _same_results(proc.recognize_batch(frames, "acme"), proc.recognize_faces_batch(frames, "acme", hud, True, encode=enc)[1])
    # a budget no row fits: None per frame, and the turn is still released
    tight = JpegEncoder(QUALITY, row_budget=8)
    assert proc.recognize_faces_batch(frames, "acme", hud, encode=tight) == [None] * 4
    assert proc.recognize_faces_batch(frames, "acme", hud, encode=enc) == first
