"""GPU end to end: ``recognize_faces_batch(..., hud, redact=r)`` - the engine pass on the unmasked pixels, then on the ring's device
frames: resize to previews, REDACT, draw the HUD, encode or copy out.  The pictures are tests/helpers/hud_ref.py drawn on
tests/helpers/redact_ref.py of the input frames, byte for byte, with the regions worked out here from the results the call
returns; the results are ``recognize_batch``'s."""
import os
import sys
import warnings

import numpy as np
import pytest

from tests.helpers import hud_ref, jpeg_ref, letterbox_ref, redact_ref, yuv_ref

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

SEEDS = (9, 11, 0, 3)                  # 120 x 160 frames with 2, 2, 1 and 0 faces (seed 9: overlapping, one partly outside)
CAMS = ["lobby", ("dock", 2), 7, "roof"]
MARGIN, BLOCK = 25, 8


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


def _region(result, frame_hw, out_hw=None, margin=MARGIN):
    """the issue's rule, restated: ordered int() box, grown by margin percent of its own sides, mapped outward onto a preview"""
    xa, ya, xb, yb = (int(v) for v in result["bbox"])
    x1, y1, x2, y2 = min(xa, xb), min(ya, yb), max(xa, xb), max(ya, yb)
    dx, dy = (x2 - x1 + 1) * margin // 100, (y2 - y1 + 1) * margin // 100
    x1, y1, x2, y2 = x1 - dx, y1 - dy, x2 + dx, y2 + dy
    if out_hw is not None:
        (H, W), (nh, nw) = frame_hw, out_hw
        x1, x2 = x1 * nw // W, ((x2 + 1) * nw + W - 1) // W - 1
        y1, y2 = y1 * nh // H, ((y2 + 1) * nh + H - 1) // H - 1
    return x1, y1, x2, y2


def _expected(frame, results, out_size=None, out_hw=None, who=None, block=BLOCK, mode=0, colour=(0, 0, 0), extra=(), **hud_kw):
    """hud_ref on redact_ref of ``frame`` (or of its preview); ``results`` None: nothing ran, the whole picture is masked"""
    hw = frame.shape[:2]
    picture = frame if out_size is None else letterbox_ref.canvas_ref(frame, out_size)[0]
    ph, pw = hw if out_hw is None else out_hw
    if results is None:
        regions = [(0, 0, pw - 1, ph - 1)]
    else:
        regions = [_region(r, hw, out_hw) for r in results if who is None or r["person_info"]["type"] in who] + list(extra)
    masked = redact_ref.redact(picture, np.array(regions, np.int64).reshape(-1, 4), block, mode, colour)
    if out_size is None:
        return hud_ref.draw_results(masked, results, **hud_kw)
    return hud_ref.draw_results(masked, results, out_hw=out_hw, frame_hw=hw, **hud_kw)


def test_full_size_frames_are_hud_ref_on_redact_ref_and_the_results_are_recognize_batchs(world):
    from facerecognition_infrenceengine_amd import Hud, Redactor
    proc, frames = world["proc"], world["frames"]
    keep = [f.copy() for f in frames]
    plain = proc.recognize_batch(frames, "acme")
    out, res = proc.recognize_faces_batch(frames, "acme", Hud(), return_results=True, redact=Redactor(block=BLOCK))
    _same_results(res, plain)                                # the engine saw the unmasked pixels
    assert res[3] == [] and sum(len(r) for r in res) >= 3
    assert all(np.array_equal(a, b) for a, b in zip(frames, keep))       # the caller's frames are neither masked nor drawn on
    for k in range(4):
        assert out[k].dtype == np.uint8 and out[k].shape == (120, 160, 3)
        assert np.array_equal(out[k], _expected(frames[k], res[k])), k
        assert (not np.array_equal(out[k], hud_ref.draw_results(frames[k], res[k]))) == bool(res[k])     # a mosaic is in the picture
    assert np.array_equal(out[3], frames[3])                 # the engine ran and found no face: untouched
    # fill, employees only, another block; scale reaches the HUD as before
    r = Redactor(mode="fill", colour=(9, 8, 200), block=5, who=("employee",), margin=MARGIN)
    out, res = proc.recognize_faces_batch(frames, "acme", Hud(scale=2), return_results=True, redact=r)
    kinds = {x["person_info"]["type"] for fr in res for x in fr}
    assert "employee" in kinds and kinds - {"employee"}                      # someone is masked and someone is spared
    for k in range(4):
        assert np.array_equal(out[k], _expected(frames[k], res[k], who=("employee",), block=5, mode=1, colour=(9, 8, 200), scale=2)), k
    # without return_results: the frames alone
    again = proc.recognize_faces_batch(frames, "acme", Hud(scale=2), redact=r)
    assert isinstance(again, list) and all(np.array_equal(a, b) for a, b in zip(again, out))


def test_previews_are_redacted_in_preview_pixels_with_the_regions_mapped_outward(world):
    from facerecognition_infrenceengine_amd import Hud, Redactor
    proc, frames = world["proc"], world["frames"]
    for out_size, out_hw in (((80, 60), (60, 80)), ((96, 96), (72, 96))):
        out, res = proc.recognize_faces_batch(frames, "acme", Hud(out_size=out_size), return_results=True,
                                              redact=Redactor(block=4))
        _same_results(res, proc.recognize_batch(frames, "acme"))
        for k in range(4):
            assert out[k].shape == (out_size[1], out_size[0], 3)
            assert np.array_equal(out[k], _expected(frames[k], res[k], out_size, out_hw, block=4)), (out_size, k)
        assert not np.array_equal(out[0], hud_ref.draw_results(letterbox_ref.canvas_ref(frames[0], out_size)[0], res[0],
                                                               out_hw=out_hw, frame_hw=(120, 160)))


def test_nv12_input_gives_the_picture_of_the_converted_frames(world):
    from facerecognition_infrenceengine_amd import Hud, Redactor
    proc = world["proc"]
    nv12 = [yuv_ref.bgr_to_yuv420(f, "nv12") for f in world["frames"]]
    bgr = [yuv_ref.yuv420_to_bgr(f, "nv12") for f in nv12]
    out, res = proc.recognize_faces_batch(nv12, "acme", Hud(), return_results=True, pixel_format="nv12", redact=Redactor(block=BLOCK))
    _same_results(res, proc.recognize_batch(bgr, "acme"))
    assert sum(len(r) for r in res) >= 2
    for k in range(4):
        assert np.array_equal(out[k], _expected(bgr[k], res[k])), k


def test_a_gated_repeat_is_redacted_from_held(world):
    from facerecognition_infrenceengine_amd import ActivityGate, Hud, Redactor
    from facerecognition_infrenceengine_amd.processor import UNCHANGED
    proc, frames, hud, r = world["proc"], world["frames"], Hud(), Redactor(block=BLOCK)
    gate, held = ActivityGate(slots=8, max_hw=(480, 640)), {}
    kw = dict(return_results=True, gate=gate, camera_ids=CAMS, redact=r)
    out1, res1 = proc.recognize_faces_batch(frames, "acme", hud, held=held, **kw)
    assert all(x is not UNCHANGED for x in res1)
    held.update(zip(CAMS, res1))
    out2, res2 = proc.recognize_faces_batch(frames, "acme", hud, held=held, **kw)
    assert res2 == [UNCHANGED] * 4                           # the engine did not run, the regions are the held results'
    for k in range(4):
        assert np.array_equal(out2[k], _expected(frames[k], res1[k])), k
        assert np.array_equal(out2[k], out1[k])
    # unchanged with nothing held: nothing is known about the frame, so all of it is masked; "pass" lets it through
    out3, _ = proc.recognize_faces_batch(frames, "acme", hud, **kw)
    for k in range(4):
        assert np.array_equal(out3[k], _expected(frames[k], None)), k
    out4, _ = proc.recognize_faces_batch(frames, "acme", hud, **dict(kw, redact=Redactor(block=BLOCK, unprocessed="pass")))
    assert all(np.array_equal(a, b) for a, b in zip(out4, frames))


def test_without_a_gallery_the_frames_come_back_wholly_pixelated(world):
    from facerecognition_infrenceengine_amd import Hud, Redactor
    proc, frames = world["proc"], world["frames"]
    out, none = proc.recognize_faces_batch(frames, "nobody", Hud(), return_results=True, redact=Redactor(block=16))
    assert none is None
    for k in range(4):
        assert np.array_equal(out[k], redact_ref.redact(frames[k], [(0, 0, 159, 119)], 16)), k
        cell = out[k][112:120, 144:160].reshape(-1, 3)       # the cut cell of the last row: 8 x 16 pixels, one value
        assert (cell == cell[0]).all()
    # previews: the picture's area of the canvas is masked, the padding stays zero
    out, _ = proc.recognize_faces_batch(frames, "nobody", Hud(out_size=(96, 96)), return_results=True, redact=Redactor(block=16))
    small = letterbox_ref.canvas_ref(frames[0], (96, 96))[0]
    assert np.array_equal(out[0], redact_ref.redact(small, [(0, 0, 95, 71)], 16)) and not out[0][72:].any()
    out, _ = proc.recognize_faces_batch(frames, "nobody", Hud(), return_results=True, redact=Redactor(unprocessed="pass"))
    assert all(np.array_equal(a, b) for a, b in zip(out, frames))
    # a company per frame: "nobody"'s frame is masked as a whole, the others by their faces
    companies = ["acme", "acme", "nobody", "acme"]
    out, res = proc.recognize_faces_batch(frames, companies, Hud(), return_results=True, redact=Redactor(block=BLOCK))
    assert res[2] is None
    for k in range(4):
        assert np.array_equal(out[k], _expected(frames[k], res[k])), k


def test_linger_keeps_the_last_frames_region_masked(world):
    """a frame pair of one camera whose second frame shows no face at that place: the first frame's regions are still masked in
    the second, and gone in the third"""
    from facerecognition_infrenceengine_amd import Hud, Redactor
    proc, frames = world["proc"], world["frames"]
    r, hud = Redactor(block=BLOCK, linger=1), Hud()
    first = [frames[0], frames[1]]
    second = [frames[3], frames[3]]                          # seed 3: no face anywhere
    cams = ["a", "b"]
    out1, res1 = proc.recognize_faces_batch(first, "acme", hud, return_results=True, redact=r, redact_keys=cams)
    out2, res2 = proc.recognize_faces_batch(second, "acme", hud, return_results=True, redact=r, redact_keys=cams)
    out3, res3 = proc.recognize_faces_batch(second, "acme", hud, return_results=True, redact=r, redact_keys=cams)
    assert res2 == [[], []] and all(len(x) >= 1 for x in res1)
    for k in range(2):
        assert np.array_equal(out1[k], _expected(first[k], res1[k])), k
        past = [_region(x, (120, 160)) for x in res1[k]]
        assert np.array_equal(out2[k], _expected(second[k], [], extra=past)), k
        assert not np.array_equal(out2[k], second[k])        # the place is masked though no face was found there
        assert np.array_equal(out3[k], second[k])            # one frame later the history has run out
    r.forget("a")
    with pytest.raises(ValueError, match="keys"):            # linger without keys is refused, and the ring turn is released
        proc.recognize_faces_batch(second, "acme", hud, redact=r)
    out, _ = proc.recognize_faces_batch(first, "acme", hud, return_results=True, redact=r, redact_keys=cams)
    assert np.array_equal(out[0], out1[0])


def test_frames_of_two_sizes_through_a_det_size_engine(world):
    """the frame-table entry of the kernel behind the same call: the arena is redacted and drawn in place and cut at the ring's
    offsets; the previews come from the table's rows"""
    from facerecognition_infrenceengine_amd import Hud, Redactor
    from facerecognition_infrenceengine_amd.processor import FaceRecognitionProcessor
    from make_golden import synth_frame
    eng = world["eng"].clone_with(det_size=(640, 640))
    proc = FaceRecognitionProcessor(world["proc"].embedding_manager, face_detector=eng)
    frames = [world["frames"][0], synth_frame(240, 320, 4), world["frames"][1]]
    out, res = proc.recognize_faces_batch(frames, "acme", Hud(), return_results=True, redact=Redactor(block=BLOCK))
    _same_results(res, proc.recognize_batch(frames, "acme"))
    assert sum(len(r) for r in res) >= 3
    for k, f in enumerate(frames):
        assert out[k].shape == f.shape and np.array_equal(out[k], _expected(f, res[k])), k
    out, res = proc.recognize_faces_batch(frames, "acme", Hud(out_size=(80, 60)), return_results=True, redact=Redactor(block=4))
    for k, f in enumerate(frames):
        assert np.array_equal(out[k], _expected(f, res[k], (80, 60), (60, 80), block=4)), k


def test_with_encode_the_bytes_are_jpeg_ref_of_the_same_picture(world):
    from facerecognition_infrenceengine_amd import Hud, JpegEncoder, Redactor
    proc, frames, enc = world["proc"], world["frames"], JpegEncoder(80)
    for out_size, out_hw in ((None, None), ((80, 60), (60, 80))):
        hud, r = Hud(out_size=out_size), Redactor(block=4)
        arrays, res = proc.recognize_faces_batch(frames, "acme", hud, return_results=True, redact=r)
        coded, res_coded = proc.recognize_faces_batch(frames, "acme", hud, return_results=True, redact=r, encode=enc)
        _same_results(res, res_coded)
        assert len(coded) == 4 and all(isinstance(b, bytes) for b in coded)
        for k in range(4):
            assert np.array_equal(arrays[k], _expected(frames[k], res[k], out_size, out_hw, block=4)), (out_size, k)
            assert coded[k] == jpeg_ref.encode(arrays[k], 80), (out_size, k)
        assert coded[0] != jpeg_ref.encode(proc.recognize_faces_batch(frames, "acme", hud)[0], 80)      # and not the unmasked one's
