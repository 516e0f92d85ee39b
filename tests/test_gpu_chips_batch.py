"""GPU end to end: the batch calls with ``chips=c`` - the engine pass, then one launch that cuts every selected face's square out of
the ring's full-size device frames, in front of the previews, the redactor and the HUD.  A chip is tests/helpers/chip_ref.py applied
to the host frame at the result's ``square()``, byte for byte; an encoded chip is tests/helpers/jpeg_ref.py of that array; every
other key of every face dict is what the call returns without chips."""
import os
import sys
import warnings

import numpy as np
import pytest

from tests.helpers import chip_ref, jpeg_ref, yuv_ref

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

SEEDS = (9, 11, 0, 3)                  # 120 x 160 frames with 2, 2, 1 and 0 faces (seed 9: overlapping, one partly outside)
CAMS = ["lobby", ("dock", 2), 7, "roof"]
FILL = (3, 60, 200)


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


def _same_but_chip(with_chips, plain):
    """every key of every face dict but ``chip`` is what the call without chips returns, exactly"""
    assert len(with_chips) == len(plain)
    for x, y in zip(with_chips, plain):
        if not isinstance(y, list):
            assert x is y
            continue
        assert len(x) == len(y)
        for p, q in zip(x, y):
            assert set(p) == set(q) | {"chip"}
            for key, v in q.items():
                if isinstance(v, np.ndarray):
                    assert np.array_equal(p[key], v) and p[key].dtype == v.dtype, key
                else:
                    assert p[key] == v and type(p[key]) is type(v), key


def _want(c, frame, result):
    return chip_ref.chip([frame], (0,) + c.square(result), c.size, c.fill)


def _check_arrays(c, frames, results, selected=lambda r: True):
    n = 0
    for f, res in zip(frames, results):
        for r in res if isinstance(res, list) else ():
            if not selected(r):
                assert r["chip"] is None
                continue
            assert isinstance(r["chip"], np.ndarray) and r["chip"].dtype == np.uint8 and r["chip"].shape == (c.size, c.size, 3)
            assert np.array_equal(r["chip"], _want(c, f, r)), r["bbox"]
            n += 1
    return n


def test_recognize_batch_chips_are_the_definition_on_the_host_frames(world):
    from facerecognition_infrenceengine_amd import FaceChips, JpegEncoder
    proc, frames = world["proc"], world["frames"]
    plain = proc.recognize_batch(frames, "acme")
    for size, margin in ((112, 30), (16, 0), (48, 400)):               # bilinear, box, and squares far past the frame
        c = FaceChips(size=size, margin=margin, encode=None, fill=FILL)
        res = proc.recognize_batch(frames, "acme", chips=c)
        _same_but_chip(res, plain)
        assert res[3] == [] and _check_arrays(c, frames, res) == sum(len(r) for r in plain) >= 3
    # who: employees only; the others carry None
    c = FaceChips(size=48, encode=None, who=("employee",))
    res = proc.recognize_batch(frames, "acme", chips=c)
    kinds = [r["person_info"]["type"] for fr in res for r in fr]
    assert "employee" in kinds and set(kinds) - {"employee"}
    assert _check_arrays(c, frames, res, lambda r: r["person_info"]["type"] == "employee") == kinds.count("employee")
    # encoded: the JPEG of exactly those arrays, by the device encoder
    arrays = proc.recognize_batch(frames, "acme", chips=FaceChips(size=112, encode=None))
    for enc, q in ((FaceChips(size=112), 85), (FaceChips(size=112, encode=JpegEncoder(60)), 60)):
        coded = proc.recognize_batch(frames, "acme", chips=enc)
        _same_but_chip(coded, plain)
        for fa, fc in zip(arrays, coded):
            for a, b in zip(fa, fc):
                assert isinstance(b["chip"], bytes) and b["chip"] == jpeg_ref.encode(a["chip"], q)
    # no gallery: None as ever, nothing to chip; a company per frame: the frame without a gallery has none
    assert proc.recognize_batch(frames, "nobody", chips=c) is None
    mixed = proc.recognize_batch(frames, ["acme", "nobody", "acme", "acme"], chips=FaceChips(size=16, encode=None))
    assert mixed[1] is None and _check_arrays(FaceChips(size=16, encode=None), frames, mixed) >= 2


def test_with_a_hud_and_a_redactor_chips_show_the_original_pixels(world):
    from facerecognition_infrenceengine_amd import FaceChips, Hud, JpegEncoder, Redactor
    proc, frames = world["proc"], world["frames"]
    keep = [f.copy() for f in frames]
    red = Redactor(block=8, who=("employee",))
    c = FaceChips(size=112, encode=None, fill=FILL)
    for hud in (Hud(), Hud(out_size=(80, 60))):
        want_out, plain = proc.recognize_faces_batch(frames, "acme", hud, return_results=True, redact=red)
        out, res = proc.recognize_faces_batch(frames, "acme", hud, return_results=True, redact=red, chips=c)
        _same_but_chip(res, plain)
        assert all(np.array_equal(a, b) for a, b in zip(out, want_out))          # the pictures are the ones without chips
        # masked faces have no chip; the others' show neither HUD pixel nor mosaic: they are the definition on the input frames
        spared = lambda r: r["person_info"]["type"] != "employee"
        n = _check_arrays(c, frames, res, spared)
        assert n >= 1 and any(r["chip"] is None for fr in res for r in fr)
    assert all(np.array_equal(a, b) for a, b in zip(frames, keep))
    # masked=True: the explicit opt-out, every face is chipped from the unmasked frame
    open_c = FaceChips(size=112, encode=None, fill=FILL, masked=True)
    out, res = proc.recognize_faces_batch(frames, "acme", Hud(), return_results=True, redact=red, chips=open_c)
    assert _check_arrays(open_c, frames, res) == sum(len(r) for r in res) and not any(r["chip"] is None for fr in res for r in fr)
    # without a redactor, with both encoders: pictures and chips are JPEG, each of its own quality
    enc_c = FaceChips(size=48)
    coded, res = proc.recognize_faces_batch(frames, "acme", Hud(), return_results=True, encode=JpegEncoder(80), chips=enc_c)
    plain_coded = proc.recognize_faces_batch(frames, "acme", Hud(), encode=JpegEncoder(80))
    assert coded == plain_coded
    for f, fr in zip(frames, res):
        for r in fr:
            assert r["chip"] == jpeg_ref.encode(_want(enc_c, f, r), 85)


def test_nv12_chips_come_from_the_converted_frames(world):
    from facerecognition_infrenceengine_amd import FaceChips
    proc = world["proc"]
    nv12 = [yuv_ref.bgr_to_yuv420(f, "nv12") for f in world["frames"]]
    bgr = [yuv_ref.yuv420_to_bgr(f, "nv12") for f in nv12]
    c = FaceChips(size=112, encode=None, fill=FILL)
    res = proc.recognize_batch(nv12, "acme", pixel_format="nv12", chips=c)
    _same_but_chip(res, proc.recognize_batch(nv12, "acme", pixel_format="nv12"))
    assert _check_arrays(c, bgr, res) >= 2


def test_frames_of_two_sizes_through_a_det_size_engine(world):
    from facerecognition_infrenceengine_amd import FaceChips, Hud
    from facerecognition_infrenceengine_amd.processor import FaceRecognitionProcessor
    from make_golden import synth_frame
    eng = world["eng"].clone_with(det_size=(640, 640))
    proc = FaceRecognitionProcessor(world["proc"].embedding_manager, face_detector=eng)
    frames = [world["frames"][0], synth_frame(240, 320, 4), world["frames"][1]]
    for size in (112, 32):
        c = FaceChips(size=size, encode=None, fill=FILL)
        res = proc.recognize_batch(frames, "acme", chips=c)
        _same_but_chip(res, proc.recognize_batch(frames, "acme"))
        assert _check_arrays(c, frames, res) >= 3
    out, res = proc.recognize_faces_batch(frames, "acme", Hud(), return_results=True, chips=c)
    assert _check_arrays(c, frames, res) >= 3


def test_a_gated_call_chips_the_active_frames_only(world):
    from facerecognition_infrenceengine_amd import ActivityGate, FaceChips
    from facerecognition_infrenceengine_amd.processor import UNCHANGED
    proc, frames = world["proc"], world["frames"]
    gate = ActivityGate(slots=8, max_hw=(480, 640))
    c = FaceChips(size=48, encode=None, fill=FILL)
    first = proc.recognize_batch(frames, "acme", gate=gate, camera_ids=CAMS, chips=c)
    assert all(r is not UNCHANGED for r in first) and _check_arrays(c, frames, first) >= 3
    turn2 = [frames[1], frames[0], frames[2], frames[2]]                 # camera 7 shows what it showed
    second = proc.recognize_batch(turn2, "acme", gate=gate, camera_ids=CAMS, chips=c)
    assert second[2] is UNCHANGED and all(isinstance(second[k], list) for k in (0, 1, 3))
    assert _check_arrays(c, turn2, second) == sum(len(second[k]) for k in (0, 1, 3)) >= 3
    third = proc.recognize_batch(turn2, "acme", gate=gate, camera_ids=CAMS, chips=c)
    assert third == [UNCHANGED] * 4                                       # nothing ran: nothing to chip


def test_identify_batch_chips(world):
    from facerecognition_infrenceengine_amd import FaceChips
    proc, frames = world["proc"], world["frames"]
    c = FaceChips(size=112, encode=None, fill=FILL)
    res = proc.identify_batch(frames, "acme", k=3, chips=c)
    _same_but_chip(res, proc.identify_batch(frames, "acme", k=3))
    assert _check_arrays(c, frames, res) >= 3
    top = FaceChips(size=16, encode=None, who=lambda r: bool(r["candidates"]) and r["candidates"][0]["score"] > 0.9)
    res = proc.identify_batch(frames, "acme", k=3, chips=top)
    hit = lambda r: bool(r["candidates"]) and r["candidates"][0]["score"] > 0.9
    assert 1 <= _check_arrays(top, frames, res, hit) < sum(len(r) for r in res)


class Sink:
    """records the manager calls in order"""

    def __init__(self):
        self.calls = []

    def process_detection(self, pid, info, cam, ts, score):
        self.calls.append(("rec", cam, pid))

    def process_unknown_detection(self, cam, ts, emb, bbox):
        self.calls.append(("unk", cam, bbox))

    def process_unknown_cluster(self, cam, ts, cluster, is_new, count, bbox):
        self.calls.append(("clu", cam, cluster, is_new, bbox))


class ChipSink(Sink):
    def process_face_chip(self, cam, ts, person_id, cluster, bbox, chip):
        self.calls.append(("chip", cam, person_id, cluster, bbox, chip))


def test_process_batch_gives_one_thumbnail_per_new_unknown_cluster(world):
    """a gallery in which the faces of frame 0 are enrolled with their component in the span of the other frames' faces taken out
    (as tests/test_gpu_process_batch.py builds its "mixed" gallery): frame 0's faces are recognised, the others are unknown"""
    from facerecognition_infrenceengine_amd import FaceChips
    from facerecognition_infrenceengine_amd.enrol import UnknownClusters
    from facerecognition_infrenceengine_amd.processor import CameraProcessor, EmbeddingManager, InMemoryStore
    eng, frames = world["eng"], world["frames"]
    emb = [[f.normed_embedding.astype(np.float64) for f in eng.get(fr)] for fr in frames]
    U = np.stack(emb[1] + emb[2])
    proj = np.linalg.pinv(U) @ U
    rng = np.random.default_rng(9)
    store = InMemoryStore()
    for i in range(30):
        store.add_employee(f"n{i}", "acme", rng.standard_normal(512).astype(np.float32), name=f"N{i}")
    for j, e in enumerate(emb[0]):
        store.add_employee(f"face0_{j}", "acme", (e - proj @ e).astype(np.float32), name=f"F0{j}")
    mgr = EmbeddingManager(store=store, device="cuda:0")
    cams = [0, 1, 2, 3]
    plain_sink = Sink()
    plain = CameraProcessor(mgr, plain_sink, face_detector=eng, unknown_clusters=UnknownClusters("cuda:0")).process_batch(frames, cams)
    assert sum(s["unknown"] for s in plain) >= 2 and sum(s["recognized"] for s in plain) >= 1

    c = FaceChips(size=48, encode=None, fill=FILL, who=lambda r: r.get("is_new"))
    sink = ChipSink()
    cp = CameraProcessor(mgr, sink, face_detector=eng, unknown_clusters=UnknownClusters("cuda:0"))
    stats = cp.process_batch(frames, cams, chips=c)
    assert [{k: v for k, v in s.items() if k != "chips"} for s in stats] == plain
    assert [x for x in sink.calls if x[0] != "chip"] == plain_sink.calls           # every other call is the one made without chips
    new = [x for x in sink.calls if x[0] == "clu" and x[3]]
    got = [x for x in sink.calls if x[0] == "chip"]
    assert len(got) == len(new) >= 1                                               # exactly one per new cluster
    for x in got:                                                                  # right behind its detection call
        before = sink.calls[sink.calls.index(x) - 1]
        assert before[0] == "clu" and before[3] == 1 and before[1] == x[1] and before[2] == x[3] and before[4] == x[4]
        assert x[2] is None
        want = chip_ref.chip([frames[x[1]]], (0,) + c.square({"bbox": x[4]}), 48, FILL)
        assert np.array_equal(x[5], want)
    flat = [(f, chip) for f, s in enumerate(stats) for _, chip in s["chips"]]       # the stats carry the same chips, frame by frame
    assert len(flat) == len(got) and all(f == g[1] and np.array_equal(chip, g[5]) for (f, chip), g in zip(flat, got))
    # the same frames again: no cluster is new, no thumbnail
    sink.calls.clear()
    again = cp.process_batch(frames, cams, chips=c)
    assert not [x for x in sink.calls if x[0] == "chip"] and all(s["chips"] == [] for s in again)
    # recognised faces too, with their person id; a manager without the method gets no such call but the stats carry the chips
    everyone = FaceChips(size=16, encode=None)
    sink2 = ChipSink()
    CameraProcessor(mgr, sink2, face_detector=eng, unknown_clusters=UnknownClusters("cuda:0")).process_batch(frames, cams, chips=everyone)
    recs = [i for i, x in enumerate(sink2.calls) if x[0] == "rec"]
    assert recs and all(sink2.calls[i + 1][0] == "chip" and sink2.calls[i + 1][2] == sink2.calls[i][2] for i in recs)
    assert len([x for x in sink2.calls if x[0] == "chip"]) == len([x for x in sink2.calls if x[0] != "chip"])
    mute = Sink()
    st = CameraProcessor(mgr, mute, face_detector=eng, unknown_clusters=UnknownClusters("cuda:0")).process_batch(frames, cams, chips=everyone)
    assert mute.calls == plain_sink.calls and sum(len(s["chips"]) for s in st) == len(mute.calls)
