"""GPU end to end: tracks that fuse (``FaceTracks(..., template=K)``) through the engine and the processor, on the seeded
160 x 120 frames of tests/test_gpu_quality_pipeline.py, three turns each.  ``template=1`` is the call without templates bit for
bit, for plain and for judging tracks; under ``template=3`` the query, the shots and the events are those of
tests/helpers/track_template_ref.py driven by the columns the call itself handed its fuse launch, and ``recognize_batch`` answers
with a scan of the reference's query."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from tests import test_gpu_track_batch as tb
from tests.helpers.track_template_ref import JOINED, NONE, READ, RESTARTED, STARTED, TrackTemplateRef
from tests.test_gpu_quality_pipeline import ACCEPT, CAMS, SEEDS

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
TURNS = 3
NEW = {"query", "template_shots", "template_event"}


@pytest.fixture(scope="module")
def world():
    """The engine, the frames of the three turns on host and device (turn 2: the same scenes under a little seeded pixel noise,
    so that a re-embedded face's row is near its template and not equal to it), a processor whose gallery holds every face, and
    a quality rule that rejects the faces below the median sharpness of those the accept-all rule measured."""
    from facerecognition_infrenceengine_amd import FaceAnalysis, FaceQuality
    from facerecognition_infrenceengine_amd.processor import EmbeddingManager, FaceRecognitionProcessor, InMemoryStore
    from make_golden import synth_frame
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        app = FaceAnalysis(name="buffalo_l").prepare(ctx_id=0)
    assert app.synthetic and app.det_size is None
    frames = [synth_frame(120, 160, s) for s in SEEDS]
    rng = np.random.default_rng(31)
    noisy = [np.clip(f.astype(np.int16) + rng.integers(-2, 3, f.shape), 0, 255).astype(np.uint8) for f in frames]
    turns = [frames, frames, noisy]
    dev = [torch.from_numpy(np.stack(t)).cuda() for t in turns]
    plain = app.detect_embed_slots(dev[0], compact_embed=True)
    counts = plain["counts"].cpu().numpy()
    N, cap = plain["bbox"].shape[:2]
    held = np.array([s % cap < counts[s // cap] for s in range(N * cap)])
    assert held.sum() >= 8
    rng = np.random.default_rng(9)
    store = InMemoryStore()
    for i in range(30):
        store.add_employee(f"n{i}", "acme", rng.standard_normal(512).astype(np.float32), name=f"N{i}")
    E = plain["embedding"].cpu().numpy()
    for s in np.flatnonzero(held):
        store.add_employee(f"face{s}", "acme", E[s], name=f"F{s}")
    mgr = EmbeddingManager(store=store, device="cuda:0")
    proc = FaceRecognitionProcessor(mgr, face_detector=app)
    accept = FaceQuality(**ACCEPT)
    sharp = sorted(d["quality"]["sharp"] for res in proc.recognize_batch(frames, "acme", quality=accept) for d in res)
    median = sharp[len(sharp) // 2]
    assert sharp[0] < median
    return dict(app=app, turns=turns, dev=dev, proc=proc, mgr=mgr, N=N, cap=cap, faces=int(held.sum()),
                half=FaceQuality(**dict(ACCEPT, sharp_min=median)))


def _tracks(**kw):
    from facerecognition_infrenceengine_amd import FaceTracks
    return FaceTracks(slots=8, max_reuse=1, **kw)                    # embed, carry, embed over the three turns


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _held(r):
    n, cap = r["det_score"].shape
    return (torch.arange(cap, device="cuda:0")[None, :] < r["counts"][:, None]).reshape(-1)


@pytest.mark.parametrize("judging", [False, True])
def test_depth_one_is_the_call_without_templates_bit_for_bit(world, judging):
    w = world
    kw = {"quality": w["half"]} if judging else {}
    off, one = _tracks(**kw), _tracks(template=1, **kw)
    assert off.template == 0 and not any(hasattr(off, k) for k in ("tring", "ttmpl", "tmean"))     # off: no state more
    assert "joined" not in off.stats and one.stats["joined"] == one.stats["restarted"] == 0
    events = set()
    for turn in range(TURNS):
        a = w["app"].detect_embed_slots(w["dev"][turn], compact_embed=True, tracks=off, camera_ids=CAMS)
        b = w["app"].detect_embed_slots(w["dev"][turn], compact_embed=True, tracks=one, camera_ids=CAMS)
        assert set(b) == set(a) | NEW and not NEW & set(a)
        h = _held(a)
        for k in a:                                                   # every tensor of the slot dict
            if k in ("bbox", "kps", "det_score"):                     # the detector's rows of empty slots are not defined
                assert _bits_equal(a[k].reshape(h.numel(), -1)[h], b[k].reshape(h.numel(), -1)[h]), (turn, k)
            else:
                assert _bits_equal(a[k], b[k]), (turn, k)
        assert _bits_equal(b["query"], b["normed_embedding"]), turn   # K = 1: the template is the last embedded row
        assert torch.equal(off.tstate, one.tstate) and _bits_equal(off.bank, one.bank) and _bits_equal(off.tbox, one.tbox)
        ev, shots = b["template_event"].reshape(-1), b["template_shots"].reshape(-1)
        assert ((ev != NONE) == (shots == 1)).all() and (ev[~h] == NONE).all() and int(shots.max()) <= 1
        events |= set(ev.cpu().tolist())
    assert {STARTED, READ} <= events and (JOINED in events or RESTARTED in events)
    off, one = _tracks(**kw), _tracks(template=1, **kw)
    for turn in range(TURNS):
        for call, ckw in ((w["proc"].recognize_batch, {}), (w["proc"].identify_batch, {"k": 3}),
                          (w["proc"].recognize_batch, {"mixed": True})):
            company = ["acme"] * w["N"] if ckw.pop("mixed", False) else "acme"
            a = call(w["turns"][turn], company, tracks=off, camera_ids=CAMS, **ckw)
            b = call(w["turns"][turn], company, tracks=one, camera_ids=CAMS, **ckw)
            for x, y in zip(a, b):
                assert tb._faces_equal(x, y, True) and len(x) == len(y)
                for p, q in zip(x, y):
                    assert set(q) == set(p) | {"template_shots"} and q["template_shots"] in (0, 1)
                    assert all(p[k] == q[k] for k in ("track_id", "tracked") + (("quality", "quality_ok") if judging else ()))
        assert torch.equal(off.tstate, one.tstate)
    assert {k: v for k, v in one.stats.items() if k not in ("joined", "restarted")} == off.stats
    assert one.stats["joined"] + one.stats["restarted"] >= 1


class Spy:
    """records what a FaceTracks hands its fuse launch, and runs the reference beside it"""

    def __init__(self, tracks):
        self.tracks, self.inner, self.calls = tracks, tracks.fuse_device, []
        self.ref = TrackTemplateRef(tracks.slots, tracks.entries, tracks.template, tracks.join_thr)
        tracks.fuse_device = self

    def __call__(self, entry, need, tid, counts, camera_ids, normed):
        got = self.inner(entry, need, tid, counts, camera_ids, normed)
        slot = np.array([self.tracks.slot_of(c) for c in camera_ids], np.int32)
        want = self.ref.fuse(*(t.cpu().numpy() for t in (entry, need, tid)), slot, counts.cpu().numpy(), normed.cpu().numpy())
        self.calls.append((got, want))
        return got


def test_depth_three_is_the_reference_driven_by_the_calls_own_columns(world):
    w = world
    tracks = _tracks(template=3)
    spy = Spy(tracks)
    events = []
    for turn in range(TURNS):
        r = w["app"].detect_embed_slots(w["dev"][turn], compact_embed=True, tracks=tracks, camera_ids=CAMS)
        (got, want), = spy.calls[turn:]
        assert got[0] is r["query"] and got[1] is r["template_shots"] and got[2] is r["template_event"]
        assert r["query"].shape == (w["N"] * w["cap"], 512) and r["template_shots"].shape == (w["N"], w["cap"])
        for k, g, x in zip(("query", "template_shots", "template_event"), got, want):
            g = g.cpu().numpy()
            assert g.dtype == x.dtype and np.array_equal(g.view(np.uint32), x.view(np.uint32)), (turn, k)
        events.append(want[2])
    for name, dev_state, ref_state in (("tring", tracks.tring, spy.ref.tring), ("ttmpl", tracks.ttmpl, spy.ref.ttmpl),
                                       ("tmean", tracks.tmean, spy.ref.tmean)):
        assert np.array_equal(dev_state.cpu().numpy().view(np.uint32), ref_state.view(np.uint32)), name
    assert (events[0] != NONE).sum() == w["faces"] and set(events[0].reshape(-1)) == {NONE, STARTED}
    assert (events[1] == READ).any() and ((events[2] == JOINED) | (events[2] == RESTARTED)).any()
    assert any((want[1] >= 2).any() for _, want in spy.calls)         # some template holds more than one shot ...
    normed = r["normed_embedding"].cpu().numpy()                      # ... and on the noisy turn is not the frame's own row
    fused = spy.calls[2][1][1].reshape(-1) >= 2
    assert fused.any() and all(not np.array_equal(a, b) for a, b in zip(spy.calls[2][1][0][fused], normed[fused]))


def test_recognize_batch_scans_the_reference_query(world):
    w = world
    proc, cap = w["proc"], w["cap"]
    tracks = _tracks(template=3)
    spy = Spy(tracks)
    matcher, _ = w["mgr"].get_matcher_for_company("acme")
    for turn in range(TURNS):
        mixed = turn == 1
        res = proc.recognize_batch(w["turns"][turn], ["acme"] * w["N"] if mixed else "acme", tracks=tracks, camera_ids=CAMS)
        want = spy.calls[turn][1]
        q = torch.from_numpy(want[0]).cuda()
        idx, score = matcher.match_device(q)
        dec = matcher.decide_device(idx, score, proc.recognition_threshold).cpu().numpy()
        idx, score = idx.cpu().numpy(), score.cpu().numpy()
        for f, faces in enumerate(res):
            for j, d in enumerate(faces):
                s = f * cap + j
                assert d["template_shots"] == want[1][f, j]
                if dec[s] == 1:
                    assert d["person_id"] == matcher.ids[idx[s]], (turn, f, j)
                    if mixed:                                         # the grouped scan: the same row, its own launch shape
                        assert abs(float(d["recognition_score"]) - float(score[s])) < 1e-5, (turn, f, j)
                    else:
                        assert np.float32(d["recognition_score"]).view(np.uint32) == score[s].view(np.uint32), (turn, f, j)
                else:
                    assert d["person_id"] is None and d["recognition_score"] == 0
        if turn == 0:                                                 # the gallery holds every face of these frames
            assert all(d["person_id"] is not None for faces in res for d in faces)
    ident = proc.identify_batch(w["turns"][2], "acme", k=2, tracks=tracks, camera_ids=CAMS)
    want = spy.calls[TURNS][1]
    idx, score = matcher.match_topk_device(torch.from_numpy(want[0]).cuda(), 2)
    idx, score = idx.cpu().numpy(), score.cpu().numpy()
    for f, faces in enumerate(ident):
        for j, d in enumerate(faces):
            s = f * cap + j
            assert d["template_shots"] == want[1][f, j]
            assert [c["person_id"] for c in d["candidates"]] == [matcher.ids[i] for i in idx[s] if i >= 0]
            assert [np.float32(c["score"]).view(np.uint32) for c in d["candidates"]] == \
                [x.view(np.uint32) for x, i in zip(score[s], idx[s]) if i >= 0]
    joined = sum(int((c[1][2] == JOINED).sum()) for c in spy.calls)
    restarted = sum(int((c[1][2] == RESTARTED).sum()) for c in spy.calls)
    assert tracks.stats["joined"] == joined and tracks.stats["restarted"] == restarted and joined + restarted >= 1


def test_bad_template_arguments_are_refused():
    from facerecognition_infrenceengine_amd import FaceTracks
    for kw in (dict(template=17), dict(template=-1), dict(template=3, join_thr=float("nan")), dict(join_thr=float("nan")),
               dict(template=3, join_thr=1.5), dict(template=3, join_thr=-1.5)):
        with pytest.raises(ValueError, match="template|join_thr"):
            FaceTracks(slots=8, **kw)
    plain = FaceTracks(slots=8)
    z = torch.zeros((1, 4), dtype=torch.int32, device="cuda:0")
    with pytest.raises(ValueError, match="do not fuse"):
        plain.fuse_device(z, z, z, torch.zeros(1, dtype=torch.int32, device="cuda:0"), ["a"],
                          torch.zeros((4, 512), device="cuda:0"))
    assert FaceTracks(slots=8, template=16, join_thr=-1.0).tring.shape == (8, 32, 16, 512)
