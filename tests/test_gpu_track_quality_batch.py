"""GPU end to end: tracks that judge (``FaceTracks(..., quality=q)`` passed as ``tracks=`` alone) through the engine and the
processor, on the seeded frames of tests/test_gpu_track_batch.py: four frames whose faces are pairwise disjoint (the premise of
every case about carrying, asserted) and the crowded frame, whose touching faces the guard never carries.  The contract: the
bank holds fit embeddings only; a face that turns unfit is carried on its track's held row - through the CURRENT call's scan -
while the associate launch does not ask for an embed and the row is younger than ``max_age``; otherwise it is rejected and
reported Unknown.  Thresholds of the rejecting cases come from the values the accept-all turn measured.

The engine without ``det_size`` runs on exactly those frames.  Under ``det_size=(640, 640)`` the synthetic detector finds a
mirrored "face" (mouth above the eyes) in four of that file's frames, the crowded one among them, and no threshold lets a
mirrored face through (include/frhip.h fr_face_quality_f16) - "accept all" would not accept all.  That engine therefore runs on
frames of the same generator, two sizes again, in which every face is disjoint from the others and accepted (asserted); the
guard's cases run on the first engine only."""
import warnings

import numpy as np
import pytest
import torch

from tests import test_gpu_track_batch as tb
from tests.test_gpu_quality_pipeline import ACCEPT

pytestmark = pytest.mark.gpu
CAMS = tb.CAMS
SENTINEL = 0x7FC5A5A5                           # a NaN with a payload: any arithmetic on it, or a 0 / 1 fill, would show
EMBED, CARRY, REJECT = 1, 2, 3
LONE, CROWD = (0, 1, 3, 4), 2                   # frame indices
SIZES = {"uniform": tb.SIZES["uniform"][:CROWD] + [tb.CROWDED] + tb.SIZES["uniform"][CROWD + 1:],
         "det_size": [(480, 640, 13), (240, 320, 12), (240, 320, 18), (240, 320, 25), (240, 320, 28)]}
SWAP_SEED = {"uniform": tb.SWAP_SEED["uniform"], "det_size": 50}


@pytest.fixture(scope="module")
def app():
    from facerecognition_infrenceengine_amd import FaceAnalysis
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = FaceAnalysis(name="buffalo_l").prepare(ctx_id=0)
    assert a.synthetic and a.det_size is None
    return a


@pytest.fixture(scope="module", params=["uniform", "det_size"])
def world(app, request):
    from facerecognition_infrenceengine_amd import FaceQuality
    from make_golden import synth_frame
    eng = app if request.param == "uniform" else app.clone_with(det_size=(640, 640))
    frames = [synth_frame(h, w, s) for h, w, s in SIZES[request.param]]
    swapped = list(frames)
    h, w, _ = SIZES[request.param][tb.SWAPPED]
    swapped[tb.SWAPPED] = synth_frame(h, w, SWAP_SEED[request.param])
    for k in LONE:                                               # the premise of every case about carrying
        n, bad = tb._touching(eng, frames[k])
        assert n >= 1 and bad == 0, (k, n, bad)
    n, touching = tb._touching(eng, frames[CROWD])
    assert touching >= 2 if request.param == "uniform" else touching == 0, (n, touching)   # the premise of the guard's cases
    n, bad = tb._touching(eng, swapped[tb.SWAPPED])
    assert n >= 1 and bad == 0, (n, bad)
    proc, _ = tb._processor(eng, frames)
    dev = torch.from_numpy(np.stack(frames)).to("cuda:0") if request.param == "uniform" else \
        [torch.from_numpy(f).to("cuda:0") for f in frames]
    accept = FaceQuality(**ACCEPT)
    judged = proc.recognize_batch(frames, "acme", quality=accept)                      # the values every threshold is taken from
    sharp = sorted(d["quality"]["sharp"] for res in judged for d in res)
    assert all(d["quality_ok"] for res in judged for d in res) and len(sharp) >= 6
    median = sharp[len(sharp) // 2]
    assert sharp[0] < median                                     # some face is below the median, and the median face is not
    return dict(kind=request.param, eng=eng, proc=proc, frames=frames, swapped=swapped, dev=dev, touching=touching,
                faces=len(sharp), accept=accept, half=FaceQuality(**dict(ACCEPT, sharp_min=median)),
                none=FaceQuality(**dict(ACCEPT, sharp_min=sharp[-1] + 1)), below=sum(s < median for s in sharp))


def _tracks(**kw):
    from facerecognition_infrenceengine_amd import FaceTracks
    return FaceTracks(slots=8, **kw)


def _held(r):
    n, cap = r["det_score"].shape
    return (torch.arange(cap, device="cuda:0")[None, :] < r["counts"][:, None]).reshape(-1)


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _holding(tracks):
    """live entries that hold a fit row for their current track"""
    ts, tq = tracks.tstate, tracks.tqual
    return int(((ts[:, :, 0] == 1) & (tq[:, :, 0] == 1) & (tq[:, :, 2] == ts[:, :, 3])).sum())


def _unknown(d):
    return d["person_id"] is None and d["person_info"] == {"name": "Unknown", "type": "unknown"} and d["recognition_score"] == 0


def test_accept_all_is_the_tracks_only_call_bit_for_bit(world):
    """(a) three turns: every tensor of the engine's dict and every face dict field shared with the tracks-only call, and tstate"""
    w = world
    plain, judging = _tracks(max_reuse=3), _tracks(max_reuse=3, quality=w["accept"])
    assert not hasattr(plain, "tqual") and "rejected" not in plain.stats          # no new state without quality
    for turn in range(3):
        a = w["eng"].detect_embed_slots(w["dev"], compact_embed=True, tracks=plain, camera_ids=CAMS)
        b = w["eng"].detect_embed_slots(w["dev"], compact_embed=True, tracks=judging, camera_ids=CAMS)
        assert set(b) == set(a) | {"track_action", "quality", "quality_f", "quality_verdict"}
        h = _held(a)
        assert torch.equal(a["counts"], b["counts"])
        for k in ("bbox", "kps", "det_score"):                   # the detector's rows of empty slots are not defined
            assert _bits_equal(a[k].reshape(h.numel(), -1)[h], b[k].reshape(h.numel(), -1)[h]), (turn, k)
        for k in ("embedding", "normed_embedding", "track_id", "carried"):
            assert _bits_equal(a[k], b[k]), (turn, k)
        assert torch.equal(plain.tstate, judging.tstate) and torch.equal(plain.tbox, judging.tbox), turn
        assert _bits_equal(plain.bank, judging.bank), turn
        act = b["track_action"].reshape(-1)
        assert ((act != 0) == h).all() and not (act == REJECT).any() and ((act == CARRY) == (b["carried"].reshape(-1) == 1)).all()
        assert (b["quality_verdict"].reshape(-1)[h] == 0).all()
    assert int(judging.tstate[:, :, 1].max()) == 2 and int(b["carried"].sum()) == w["faces"] - w["touching"]
    assert {k: v for k, v in judging.stats.items() if k != "rejected"} == plain.stats and judging.stats["rejected"] == 0
    plain, judging = _tracks(max_reuse=3), _tracks(max_reuse=3, quality=w["accept"])
    for turn in range(3):
        for call, kw in ((w["proc"].recognize_batch, {}), (w["proc"].identify_batch, {"k": 3})):
            a = call(w["frames"], "acme", tracks=plain, camera_ids=CAMS, **kw)
            b = call(w["frames"], "acme", tracks=judging, camera_ids=CAMS, **kw)
            for x, y in zip(a, b):
                assert tb._faces_equal(x, y, True) and len(x) == len(y)
                for p, q in zip(x, y):
                    assert set(q) == set(p) | {"quality", "quality_ok"} and q["quality_ok"] is True
                    assert (p["track_id"], p["tracked"]) == (q["track_id"], q["tracked"])
        assert torch.equal(plain.tstate, judging.tstate)


def test_max_reuse_zero_is_the_quality_only_call(world):
    """(b) nothing is ever carried: embed the fit, reject the unfit, face for face the call with ``quality=`` alone"""
    w = world
    tracks = _tracks(max_reuse=0, quality=w["half"])
    for call, kw in ((w["proc"].recognize_batch, {}), (w["proc"].identify_batch, {"k": 3})):
        want = call(w["frames"], "acme", quality=w["half"], **kw)
        for turn in range(2):
            got = call(w["frames"], "acme", tracks=tracks, camera_ids=CAMS, **kw)
            for x, y in zip(want, got):
                assert tb._faces_equal(x, y, True) and len(x) == len(y)
                for p, q in zip(x, y):
                    assert set(q) == set(p) | {"track_id", "tracked"} and q["tracked"] is False and q["track_id"] >= 0
                    assert p["quality"] == q["quality"] and p["quality_ok"] == q["quality_ok"]
                    if not q["quality_ok"]:
                        assert _unknown(q) if "person_id" in q else q["candidates"] == []
    unfit = sum(not d["quality_ok"] for res in want for d in res)
    assert unfit == w["below"] and 0 < unfit < w["faces"]
    assert tracks.stats == {"faces": 4 * w["faces"], "embedded": 4 * (w["faces"] - unfit), "carried": 0, "untracked": 0,
                            "rejected": 4 * unfit}


def test_fit_then_unfit_is_carried_on_the_held_row_until_max_age(world, monkeypatch):
    """(c) turn 1 fit; from turn 2 ``sharp_min`` lies above every face.  Lone faces answer with turn 1's person id and score
    bits, the touching faces of the crowded frame are Unknown, the bank keeps turn 1's bits, and after max_age turns all is Unknown"""
    w = world
    tracks = _tracks(max_reuse=3, quality=w["accept"], max_age=2)
    t1 = w["proc"].recognize_batch(w["frames"], "acme", tracks=tracks, camera_ids=CAMS)
    assert all(d["tracked"] is False and d["quality_ok"] for res in t1 for d in res)
    assert any(d["person_id"] for k in LONE for d in t1[k])
    bank, tqual = tracks.bank.clone(), tracks.tqual.clone()
    assert int(tqual[:, :, 0].sum()) == w["faces"]               # every face was fit and found an entry: each holds its row
    tracks.quality = w["none"]
    forwards = tb._count_forwards(monkeypatch, w["eng"])
    for turn in (2, 3):
        t = w["proc"].recognize_batch(w["frames"], "acme", tracks=tracks, camera_ids=CAMS)
        for k in LONE:
            assert len(t[k]) == len(t1[k])
            for p, q in zip(t1[k], t[k]):
                assert q["tracked"] is True and q["track_id"] == p["track_id"] and q["quality_ok"] is False
                assert q["quality"]["reasons"] == ["blurred"] and np.array_equal(p["bbox"], q["bbox"])
                assert q["person_id"] == p["person_id"] and tb._bits(q["recognition_score"]) == tb._bits(p["recognition_score"])
        crowd = t[CROWD]
        assert sum(_unknown(d) and not d["tracked"] for d in crowd) == w["touching"]        # the guard: rejected, not carried
        assert sum(d["tracked"] for d in crowd) == len(crowd) - w["touching"]
        assert _bits_equal(tracks.bank, bank), turn
    t4 = w["proc"].recognize_batch(w["frames"], "acme", tracks=tracks, camera_ids=CAMS)
    assert all(_unknown(d) and d["tracked"] is False and d["quality_ok"] is False for res in t4 for d in res)
    assert forwards == [] and _bits_equal(tracks.bank, bank) and _holding(tracks) == 0
    lone = sum(len(t1[k]) for k in LONE) + len(t1[CROWD]) - w["touching"]
    assert tracks.stats == {"faces": 4 * w["faces"], "embedded": w["faces"], "carried": 2 * lone, "untracked": 0,
                            "rejected": 3 * w["faces"] - 2 * lone}
    ident = w["proc"].identify_batch(w["frames"], "acme", k=3, tracks=tracks, camera_ids=CAMS)
    assert all(d["candidates"] == [] for res in ident for d in res)
    tracks.quality = w["accept"]                                 # fit again: embedded anew, under the ids the tracks kept
    t6 = w["proc"].recognize_batch(w["frames"], "acme", tracks=tracks, camera_ids=CAMS)
    assert forwards == [w["faces"]] and all(d["tracked"] is False for res in t6 for d in res)
    assert [d["track_id"] for k in LONE for d in t6[k]] == [d["track_id"] for k in LONE for d in t1[k]]
    assert all(tb._faces_equal(a, b, False) for a, b in zip(t6, t1))


def test_reject_all_embeds_nothing_and_leaves_the_bank_alone(world, monkeypatch):
    """(d)"""
    w = world
    tracks = _tracks(max_reuse=3, quality=w["none"])
    tracks.bank.view(torch.int32).fill_(SENTINEL)
    forwards = tb._count_forwards(monkeypatch, w["eng"])
    for turn in range(3):
        t = w["proc"].recognize_batch(w["frames"], "acme", tracks=tracks, camera_ids=CAMS)
        assert all(_unknown(d) and not d["tracked"] and not d["quality_ok"] for res in t for d in res)
    assert forwards == [] and tracks.stats["embedded"] == 0 and tracks.stats["carried"] == 0
    assert tracks.stats["rejected"] == tracks.stats["faces"] == 3 * w["faces"]
    assert (tracks.bank.view(torch.int32) == SENTINEL).all() and int(tracks.tqual[:, :, 0].sum()) == 0
    r = w["eng"].detect_embed_slots(w["dev"], compact_embed=True, tracks=tracks, camera_ids=CAMS)
    place = torch.zeros(512, device="cuda:0")
    place[0] = 1.0
    assert (r["embedding"] == place).all() and (r["normed_embedding"] == place).all()
    assert ((r["track_action"].reshape(-1) == REJECT) == _held(r)).all()


def test_an_unchanged_frame_moves_neither_tstate_nor_tqual(world):
    """(e)"""
    from facerecognition_infrenceengine_amd import ActivityGate
    from facerecognition_infrenceengine_amd.processor import UNCHANGED
    w = world
    tracks = _tracks(max_reuse=3, quality=w["accept"])
    gate = ActivityGate(slots=8, max_hw=(480, 640))

    def call(frames):
        return w["proc"].recognize_batch(frames, "acme", gate=gate, tracks=tracks, camera_ids=CAMS)
    t1 = call(w["frames"])
    assert all(r is not UNCHANGED for r in t1)
    s1, q1 = tracks.tstate.clone(), tracks.tqual.clone()
    assert int(q1[:, :, 0].sum()) >= 3
    t2 = call(w["swapped"])                                      # one frame active: only its camera's rows move
    assert [r is UNCHANGED for r in t2] == [k != tb.SWAPPED for k in range(5)]
    for k, cam in enumerate(CAMS):
        s = tracks.slot_of(cam)
        assert torch.equal(tracks.tqual[s], q1[s]) == (k != tb.SWAPPED), cam
        assert torch.equal(tracks.tstate[s], s1[s]) == (k != tb.SWAPPED), cam
    s2, q2 = tracks.tstate.clone(), tracks.tqual.clone()
    t3 = call(w["swapped"])                                      # nothing moved: no frame reaches the tracks
    assert all(r is UNCHANGED for r in t3)
    assert torch.equal(tracks.tstate, s2) and torch.equal(tracks.tqual, q2)


def test_the_two_argument_form_still_raises(world):
    """(f)"""
    w = world
    tracks = _tracks(quality=w["accept"])
    with pytest.raises(ValueError, match="quality together with tracks"):
        w["eng"].detect_embed_slots(w["dev"], compact_embed=True, tracks=tracks, camera_ids=CAMS, quality=w["accept"])
    for call in (w["proc"].recognize_batch, w["proc"].identify_batch):
        with pytest.raises(ValueError, match="quality together with tracks"):
            call(w["frames"], "acme", tracks=tracks, camera_ids=CAMS, quality=w["accept"])
    assert len(tracks) == 0 and int(tracks.tstate.abs().sum()) == 0 and int(tracks.tqual.abs().sum()) == 0
    with pytest.raises(ValueError, match="do not judge"):
        z = torch.zeros((5, 4), dtype=torch.int32, device="cuda:0")
        _tracks().resolve_device(z, z, z, z, torch.zeros(5, dtype=torch.int32, device="cuda:0"), CAMS)


@pytest.mark.parametrize("how", ["forget", "reset", "failed_embed"])
def test_dropped_tracks_never_answer_with_the_previous_rows(world, how, monkeypatch):
    """forget, reset and the failed embed pass zero ``live`` only; ``tqual`` keeps has = 1 under the old ids.  The faces come
    back under new ids, and an unfit face of the new tracks is rejected turn after turn - the id comparison, nothing else"""
    w = world
    tracks = _tracks(max_reuse=3, quality=w["accept"])
    t1 = w["proc"].recognize_batch(w["frames"], "acme", tracks=tracks, camera_ids=CAMS)
    assert _holding(tracks) == w["faces"]
    if how == "forget":
        for c in CAMS:
            tracks.forget(c)
    elif how == "reset":
        tracks.reset(CAMS)
    else:
        def failing(crops, *a, **kw):
            raise RuntimeError("the embedder is down")
        with monkeypatch.context() as m:
            m.setattr(w["eng"].rec, "forward", failing)
            with pytest.raises(RuntimeError, match="the embedder is down"):
                w["proc"].recognize_batch(w["swapped"], "acme", tracks=tracks, camera_ids=CAMS)
    assert int(tracks.tstate[:, :, 0].sum()) == 0 and int(tracks.tqual[:, :, 0].sum()) >= w["faces"]      # the rows are still marked
    tracks.quality, carried = w["none"], tracks.stats["carried"]
    old = {(k, d["track_id"]) for k, res in enumerate(t1) for d in res}
    for turn in (2, 3, 4):
        t = w["proc"].recognize_batch(w["frames"], "acme", tracks=tracks, camera_ids=CAMS)
        assert all(_unknown(d) and d["tracked"] is False for res in t for d in res), turn
        if how != "forget":                                      # (a forgotten camera takes another slot, whose counter is its own)
            assert not {(k, d["track_id"]) for k, res in enumerate(t) for d in res} & old
    assert tracks.stats["carried"] == carried                    # (the failed call counted its faces before it failed)
