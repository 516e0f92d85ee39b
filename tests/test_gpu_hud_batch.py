"""GPU end to end: ``recognize_faces_batch`` - the engine pass of ``recognize_batch``, then the HUD drawn on the ring's device frames
and read back.  The pictures are those of tests/helpers/hud_ref.py applied to the input frames and the results the call returns,
byte for byte; the results are ``recognize_batch``'s."""
import os
import sys
import warnings

import numpy as np
import pytest

from tests.helpers import hud_ref, letterbox_ref, yuv_ref

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

SEEDS = (9, 11, 0, 3)                  # 120 x 160 frames with 2, 2, 1 and 0 faces (seed 9: overlapping, one partly outside)
OTHER = (6, 10, 2, 5)
CAMS = ["lobby", ("dock", 2), 7, "roof"]


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
    other = [synth_frame(120, 160, s) for s in OTHER]
    rng = np.random.default_rng(3)
    store = InMemoryStore()
    for i in range(30):
        store.add_employee(f"n{i}", ("acme", "globex")[i % 2], rng.standard_normal(512).astype(np.float32), name=f"N{i}")
    faces = eng.get(frames[0]) + eng.get(frames[2])
    assert len(faces) >= 2
    store.add_employee("e0", "acme", faces[0].embedding, name="Ada Lovelace", employeeId="E-0042")
    store.add_visitor("v0", "acme", faces[-1].embedding, name="Zoë Visitor")
    proc = FaceRecognitionProcessor(EmbeddingManager(store=store, device="cuda:0"), face_detector=eng)
    return dict(eng=eng, proc=proc, frames=frames, other=other)


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


def test_frames_are_hud_ref_of_the_inputs_and_results_are_recognize_batchs(world):
    from facerecognition_infrenceengine_amd import Hud
    proc, frames = world["proc"], world["frames"]
    keep = [f.copy() for f in frames]
    out, res = proc.recognize_faces_batch(frames, "acme", Hud(), return_results=True)
    _same_results(res, proc.recognize_batch(frames, "acme"))
    assert res[3] == [] and sum(len(r) for r in res) >= 3
    assert {r["person_info"]["type"] for fr in res for r in fr} & {"employee", "visitor"}      # a panel with a name is in the picture
    assert len(out) == 4 and all(np.array_equal(a, b) for a, b in zip(frames, keep))      # the caller's frames are not drawn on
    for k in range(4):
        assert out[k].dtype == np.uint8 and out[k].shape == (120, 160, 3)
        assert np.array_equal(out[k], hud_ref.draw_results(frames[k], res[k])), k
    assert np.array_equal(out[3], frames[3]) and not np.array_equal(out[0], frames[0])
    # without return_results: the frames alone; scale and max_chars reach the kernel
    again = proc.recognize_faces_batch(frames, "acme", Hud(scale=2, max_chars=12))
    assert isinstance(again, list) and len(again) == 4
    for k in range(4):
        assert np.array_equal(again[k], hud_ref.draw_results(frames[k], res[k], scale=2, max_chars=12)), k
    # a company without a gallery: None, as recognize_batch, and the frames come back undrawn
    out, none = proc.recognize_faces_batch(frames, "nobody", Hud(), return_results=True)
    assert none is None and all(np.array_equal(a, b) for a, b in zip(out, frames))
    # a company per frame (the grouped scan): strangers to globex's gallery are drawn as unknown, "nobody"'s frame undrawn
    companies = ["globex", "acme", "nobody", "globex"]
    out, res = proc.recognize_faces_batch(frames, companies, Hud(), return_results=True)
    _same_results(res, proc.recognize_batch(frames, companies))
    assert res[2] is None and res[0] and all(r["person_info"]["type"] == "unknown" for r in res[0])
    for k in range(4):
        assert np.array_equal(out[k], hud_ref.draw_results(frames[k], res[k])), k
    with pytest.raises(ValueError, match="hud"):
        proc.recognize_faces_batch(frames, "acme", None)


def test_previews_are_the_reference_on_the_oracles_resize(world):
    from facerecognition_infrenceengine_amd import Hud
    proc, frames = world["proc"], world["frames"]
    out, res = proc.recognize_faces_batch(frames, "acme", Hud(out_size=(80, 60)), return_results=True)
    for k in range(4):
        small, _ = letterbox_ref.canvas_ref(frames[k], (80, 60))
        assert out[k].shape == (60, 80, 3)
        assert np.array_equal(out[k], hud_ref.draw_results(small, res[k], out_hw=(60, 80), frame_hw=(120, 160))), k
    # a canvas of another aspect: the picture top-left, zero padding, the HUD laid out on the canvas
    out, res = proc.recognize_faces_batch(frames, "acme", Hud(out_size=(96, 96)), return_results=True)
    for k in range(4):
        small, _ = letterbox_ref.canvas_ref(frames[k], (96, 96))
        assert np.array_equal(out[k], hud_ref.draw_results(small, res[k], out_hw=(72, 96), frame_hw=(120, 160))), k


def test_nv12_input_gives_the_picture_of_the_converted_frames(world):
    from facerecognition_infrenceengine_amd import Hud
    proc = world["proc"]
    nv12 = [yuv_ref.bgr_to_yuv420(f, "nv12") for f in world["frames"]]
    bgr = [yuv_ref.yuv420_to_bgr(f, "nv12") for f in nv12]
    out, res = proc.recognize_faces_batch(nv12, "acme", Hud(), return_results=True, pixel_format="nv12")
    _same_results(res, proc.recognize_batch(bgr, "acme"))
    assert sum(len(r) for r in res) >= 2
    for k in range(4):
        assert np.array_equal(out[k], hud_ref.draw_results(bgr[k], res[k])), k


def test_a_gated_repeat_is_drawn_from_held(world):
    from facerecognition_infrenceengine_amd import ActivityGate, Hud
    from facerecognition_infrenceengine_amd.processor import UNCHANGED
    proc, frames, hud = world["proc"], world["frames"], Hud()
    gate, held = ActivityGate(slots=8, max_hw=(480, 640)), {}
    out1, res1 = proc.recognize_faces_batch(frames, "acme", hud, return_results=True, held=held, gate=gate, camera_ids=CAMS)
    assert all(r is not UNCHANGED for r in res1)
    held.update(zip(CAMS, res1))
    out2, res2 = proc.recognize_faces_batch(frames, "acme", hud, return_results=True, held=held, gate=gate, camera_ids=CAMS)
    assert res2 == [UNCHANGED] * 4                                       # the engine did not run, the results are the caller's
    for k in range(4):
        assert np.array_equal(out2[k], hud_ref.draw_results(frames[k], res1[k])), k
        assert np.array_equal(out2[k], out1[k])
    # without held, an unchanged frame comes back undrawn
    out3 = proc.recognize_faces_batch(frames, "acme", hud, gate=gate, camera_ids=CAMS)
    assert all(np.array_equal(a, b) for a, b in zip(out3, frames))


def test_the_ring_turn_is_released_and_every_batch_gets_its_own_picture(world):
    """more calls than the ring is deep (2): a turn that was not released would make the third upload wait for ever"""
    from facerecognition_infrenceengine_amd import Hud
    proc, hud = world["proc"], Hud()
    for frames in (world["frames"], world["other"], world["frames"], world["other"], world["other"]):
        out, res = proc.recognize_faces_batch(frames, "acme", hud, return_results=True)
        for k in range(4):
            assert np.array_equal(out[k], hud_ref.draw_results(frames[k], res[k])), k
    assert sum(len(r) for r in res) >= 3
    _same_results(proc.recognize_batch(world["other"], "acme"), res)     # and the plain call still runs behind it


def test_frames_of_two_sizes_through_a_det_size_engine(world):
    """the frame-table entry of the kernel behind the same call: the arena is drawn in place and cut at the ring's offsets, and
    the previews come from the table's rows with the preview's geometry"""
    from facerecognition_infrenceengine_amd import Hud
    from facerecognition_infrenceengine_amd.processor import FaceRecognitionProcessor
    from make_golden import synth_frame
    eng = world["eng"].clone_with(det_size=(640, 640))
    proc = FaceRecognitionProcessor(world["proc"].embedding_manager, face_detector=eng)
    frames = [world["frames"][0], synth_frame(240, 320, 4), world["frames"][1]]
    out, res = proc.recognize_faces_batch(frames, "acme", Hud(), return_results=True)
    assert sum(len(r) for r in res) >= 3
    for k, f in enumerate(frames):
        assert out[k].shape == f.shape and np.array_equal(out[k], hud_ref.draw_results(f, res[k])), k
    out, res = proc.recognize_faces_batch(frames, "acme", Hud(out_size=(80, 60)), return_results=True)
    for k, f in enumerate(frames):
        small, _ = letterbox_ref.canvas_ref(f, (80, 60))
        assert np.array_equal(out[k], hud_ref.draw_results(small, res[k], out_hw=(60, 80), frame_hw=f.shape[:2])), k
