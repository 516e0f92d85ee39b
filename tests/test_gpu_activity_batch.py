"""GPU end to end: ``recognize_batch`` / ``identify_batch`` with an activity gate.  The contract: an inactive frame's entry is
``UNCHANGED`` and the engine does not run for it; the entries of the active frames are what the same call returns, without a
gate, for exactly those frames with their company ids.  One engine without ``det_size`` (frames of one size, the device
gather) and one with ``det_size=(640, 640)`` and frames of two sizes (the selected rows of the ring's frame table).

The comparisons are exact where two identical ungated calls agree exactly (established first, per engine, and printed);
otherwise ``recognition_score`` is held to the 5e-4 of tests/test_gpu_multi_company.py and everything else stays exact."""
import os
import sys
import warnings

import numpy as np
import pytest

from tests.helpers import activity_ref, yuv_ref

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

CAMS = ["lobby", "dock", ("gate", 3), 17, "roof"]
SIZES = {"uniform": [(240, 320, 4), (240, 320, 6), (240, 320, 5), (240, 320, 21), (240, 320, 7)],
         "det_size": [(480, 640, 0), (240, 320, 4), (240, 320, 6), (480, 640, 5), (240, 320, 21)]}
MOVED = (1, 3)                                   # the frames that change in the third turn


@pytest.fixture(scope="module")
def app():
    from facerecognition_infrenceengine_amd import FaceAnalysis
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = FaceAnalysis(name="buffalo_l").prepare(ctx_id=0)
    assert a.synthetic and a.det_size is None
    return a


def _faces_equal(a, b, exact):
    """one frame's entry against another's; False instead of an assertion"""
    if a is None or b is None:
        return a is None and b is None
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if not (np.array_equal(x["bbox"], y["bbox"]) and x["det_score"] == y["det_score"]):
            return False
        if "candidates" in x:
            if [c["person_id"] for c in x["candidates"]] != [c["person_id"] for c in y["candidates"]]:
                return False
            pairs = [(c["score"], d["score"]) for c, d in zip(x["candidates"], y["candidates"])]
        else:
            if x["person_id"] != y["person_id"] or x["person_info"] != y["person_info"]:
                return False
            pairs = [(x["recognition_score"], y["recognition_score"])]
        for s, t in pairs:
            same = np.float32(s).view(np.uint32) == np.float32(t).view(np.uint32) if exact else abs(float(s) - float(t)) < 5e-4
            if not same:
                return False
    return True


@pytest.fixture(scope="module", params=["uniform", "det_size"])
def world(app, request):
    from facerecognition_infrenceengine_amd.processor import EmbeddingManager, FaceRecognitionProcessor, InMemoryStore
    from make_golden import synth_frame
    eng = app if request.param == "uniform" else app.clone_with(det_size=(640, 640))
    frames = [synth_frame(h, w, s) for h, w, s in SIZES[request.param]]
    moved = [f.copy() for f in frames]
    for k in MOVED:                              # a 48 x 48 patch of another seed's frame: nine cells move
        h, w, _ = SIZES[request.param][k]
        moved[k][64:112, 96:144] = synth_frame(h, w, 33)[64:112, 96:144]
    rng = np.random.default_rng(9)
    store = InMemoryStore()
    for i in range(40):
        c = ("acme", "globex")[i % 2]
        store.add_employee(f"{c}_n{i}", c, rng.standard_normal(512).astype(np.float32), name=f"N{i}")
    enrolled = 0
    for k in (0, 1, 3):
        for j, f in enumerate(eng.get(frames[k])):
            store.add_employee(f"acme_face{k}_{j}", "acme", f.embedding, name=f"A{k}{j}")
            store.add_employee(f"globex_face{k}_{j}", "globex", f.embedding, name=f"G{k}{j}")
            enrolled += 1
    assert enrolled >= 2
    proc = FaceRecognitionProcessor(EmbeddingManager(store=store, device="cuda:0"), face_detector=eng)
    # 1. are two identical ungated calls the same bits?  They decide how the comparisons below are held.
    first, second = proc.recognize_batch(frames, "acme"), proc.recognize_batch(frames, "acme")
    exact = all(_faces_equal(a, b, True) for a, b in zip(first, second))
    print(f"[{request.param}] two identical ungated recognize_batch calls agree exactly: {exact}")
    assert all(_faces_equal(a, b, exact) for a, b in zip(first, second))
    assert sum(len(r) for r in first) >= 3 and any(r["person_id"] for res in first for r in res)
    return dict(kind=request.param, eng=eng, proc=proc, frames=frames, moved=moved, exact=exact, ungated=first)


def _gate():
    from facerecognition_infrenceengine_amd import ActivityGate
    return ActivityGate(slots=8, max_hw=(480, 640))


def _count_engine_passes(monkeypatch, eng):
    calls = []
    real = type(eng).detect_embed_slots

    def counting(self, *a, **kw):
        calls.append(1)
        return real(self, *a, **kw)
    monkeypatch.setattr(type(eng), "detect_embed_slots", counting)
    return calls


def _three_turns(w, monkeypatch, call, companies):
    """``call(frames, companies, **gate keywords)`` over the three turns: all new, all the same, frames MOVED changed."""
    from facerecognition_infrenceengine_amd.processor import UNCHANGED
    gate, n = _gate(), len(w["frames"])
    per_frame = isinstance(companies, list)
    ungated = call(w["frames"], companies)
    t1 = call(w["frames"], companies, gate=gate, camera_ids=CAMS)
    assert len(t1) == n and all(_faces_equal(a, b, w["exact"]) for a, b in zip(t1, ungated))      # every frame active: the call itself
    passes = _count_engine_passes(monkeypatch, w["eng"])
    t2 = call(w["frames"], companies, gate=gate, camera_ids=CAMS)
    assert len(t2) == n and all(r is UNCHANGED for r in t2)
    assert passes == []                                                  # nothing but the upload and the gate ran
    idle = gate.idle.cpu().tolist()
    assert [idle[gate.slot_of(c)] for c in CAMS] == [1] * n
    t3 = call(w["moved"], companies, gate=gate, camera_ids=CAMS)
    assert len(passes) == 1
    want = call([w["moved"][k] for k in MOVED], [companies[k] for k in MOVED] if per_frame else companies)
    for k in range(n):
        if k in MOVED:
            assert t3[k] is not UNCHANGED and _faces_equal(t3[k], want[MOVED.index(k)], w["exact"]), k
        else:
            assert t3[k] is UNCHANGED, k
    idle = gate.idle.cpu().tolist()
    assert [idle[gate.slot_of(c)] for c in CAMS] == [0 if k in MOVED else 2 for k in range(n)]
    return t1, t3


def test_recognize_batch_runs_the_engine_on_the_active_frames_only(world, monkeypatch):
    t1, t3 = _three_turns(world, monkeypatch, world["proc"].recognize_batch, "acme")
    assert any(r["person_id"] for res in t1 for r in res)


def test_recognize_batch_with_a_company_per_frame(world, monkeypatch):
    """frame 1 belongs to a company without rows: None, as without a gate - in the first turn and in the third, where it is one of
    the two active frames"""
    companies = ["acme", "nobody", "acme", "globex", "globex"]
    t1, t3 = _three_turns(world, monkeypatch, world["proc"].recognize_batch, companies)
    assert t1[1] is None and t3[1] is None and isinstance(t3[3], list)
    assert all(r["person_id"] is None or r["person_id"].startswith("globex_") for r in t3[3])


def test_identify_batch_gives_the_same_three_turns(world, monkeypatch):
    proc = world["proc"]
    t1, t3 = _three_turns(world, monkeypatch, lambda f, c, **kw: proc.identify_batch(f, c, k=3, **kw), "acme")
    assert all("candidates" in r for res in t1 for r in res)
    _three_turns(world, monkeypatch, lambda f, c, **kw: proc.identify_batch(f, c, k=3, **kw),
                 ["globex", "globex", "nobody", "acme", "acme"])


def test_nv12_frames_get_the_verdicts_and_results_of_their_converted_frames(world):
    from facerecognition_infrenceengine_amd.processor import UNCHANGED
    w, proc = world, world["proc"]
    turns = []
    for frames in (w["frames"], w["frames"], w["moved"]):
        nv12 = [yuv_ref.bgr_to_yuv420(f, "nv12") for f in frames]
        turns.append((nv12, [yuv_ref.yuv420_to_bgr(f, "nv12") for f in nv12]))
    g_yuv, g_bgr = _gate(), _gate()
    verdicts = []
    for nv12, bgr in turns:
        got = proc.recognize_batch(nv12, "acme", pixel_format="nv12", gate=g_yuv, camera_ids=CAMS)
        want = proc.recognize_batch(bgr, "acme", gate=g_bgr, camera_ids=CAMS)
        verdicts.append([r is UNCHANGED for r in got])
        assert verdicts[-1] == [r is UNCHANGED for r in want]
        assert all(a is b if a is UNCHANGED else _faces_equal(a, b, w["exact"]) for a, b in zip(got, want))
    assert verdicts == [[False] * 5, [True] * 5, [k not in MOVED for k in range(5)]]
    for name in ("grid", "geom", "idle"):                                # the gates saw the same bytes
        assert np.array_equal(getattr(g_yuv, name).cpu().numpy(), getattr(g_bgr, name).cpu().numpy()), name
    # and the grid of a camera is the oracle's cell means of its last processed (converted) frame
    cells = activity_ref.cell_means(turns[2][1][1])
    assert np.array_equal(g_yuv.grid[g_yuv.slot_of(CAMS[1])].cpu().numpy()[:len(cells)], cells)


def test_argument_errors_and_the_ungated_call_afterwards(world):
    from facerecognition_infrenceengine_amd.processor import UNCHANGED
    w, proc, gate = world, world["proc"], _gate()
    with pytest.raises(ValueError, match="camera_ids"):
        proc.recognize_batch(w["frames"], "acme", gate=gate)
    with pytest.raises(ValueError, match="one camera id per frame"):
        proc.recognize_batch(w["frames"], "acme", gate=gate, camera_ids=CAMS[:3])
    with pytest.raises(ValueError, match="repeated"):
        proc.recognize_batch(w["frames"], "acme", gate=gate, camera_ids=CAMS[:4] + CAMS[:1])
    with pytest.raises(ValueError, match="camera_ids"):
        proc.identify_batch(w["frames"], ["acme"] * 5, gate=gate)
    with pytest.raises(ValueError, match="gate"):
        proc.recognize_batch(w["frames"], "acme", camera_ids=CAMS)
    assert len(gate) == 0                                                # no refused call took a slot
    # no gallery: the None of the ungated call comes first and the gate is not consulted
    assert proc.recognize_batch(w["frames"], "nobody", gate=gate, camera_ids=CAMS) is None
    assert proc.recognize_batch(w["frames"], ["nobody"] * 5, gate=gate, camera_ids=CAMS) == [None] * 5
    assert len(gate) == 0 and int(gate.geom.abs().sum()) == 0
    # gated calls (one of them with every frame inactive), then the ungated call: what it always returned
    proc.recognize_batch(w["frames"], "acme", gate=gate, camera_ids=CAMS)
    assert proc.recognize_batch(w["frames"], "acme", gate=gate, camera_ids=CAMS) == [UNCHANGED] * 5
    again = proc.recognize_batch(w["frames"], "acme")
    assert all(_faces_equal(a, b, w["exact"]) for a, b in zip(again, w["ungated"]))
