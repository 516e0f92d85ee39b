"""GPU: the order of device work behind the detector in ``FaceAnalysis.detect_embed_slots(compact_embed=True)``, per pass, and its one
device-to-host copy.  Spies record the engine's steps by name; what a pass must show is written out below, and whether align and the
embed net run at all - and over how many faces - is read off the columns the call returns, never assumed.

  plain:    cpu -> [_warp_faces -> forward]
  tracks:   associate -> cpu -> [_warp_faces -> forward] -> commit -> [fuse]
  quality:  _warp_slots -> measure -> cpu -> [forward]
  judging:  associate -> _warp_slots -> measure -> resolve -> cpu -> [forward] -> commit -> [fuse]

[_warp_faces / forward]: only when a slot is selected; [fuse]: only with ``template``.  The call without ``compact_embed`` aligns
every slot, embeds every slot and copies nothing."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

INF = float("inf")
CAMS = ["lobby", ("gate", 3)]
VARIANTS = {"plain": {}, "tracks": {"tracks": 0}, "tracks_template": {"tracks": 3}, "quality": {"quality": True},
            "judging": {"tracks": 0, "judge": True}, "judging_template": {"tracks": 3, "judge": True}}


@pytest.fixture(scope="module")
def world():
    from facerecognition_infrenceengine_amd import FaceAnalysis, FaceQuality
    from make_golden import synth_frame
    from tests.helpers import quality_ref as qr
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        app = FaceAnalysis(name="buffalo_l").prepare(ctx_id=0)
    assert app.synthetic and app.det_size is None
    dev = torch.from_numpy(np.stack([synth_frame(240, 320, s) for s in (5, 2)])).cuda()
    accept = FaceQuality(min_eye=0, mean_lo=0, mean_hi=255, contrast_min=0, sharp_min=0, clip_max=qr.N, yaw_max=INF, pitch_lo=-INF,
                         pitch_hi=INF)
    return app, dev, accept


@pytest.fixture
def spies(world, monkeypatch):
    """the recorded step names of everything that runs while ``log`` is handed out; ``cpu`` only for device tensors"""
    from facerecognition_infrenceengine_amd import FaceAnalysis, FaceQuality, FaceTracks
    app = world[0]
    log = []

    def spy(owner, attr, name, note=None):
        real = getattr(owner, attr)

        def wrapped(*a, **kw):
            log.append(name if note is None else (name, note(*a, **kw)))
            return real(*a, **kw)
        monkeypatch.setattr(owner, attr, wrapped)

    spy(FaceAnalysis, "_warp_slots", "_warp_slots")
    spy(FaceAnalysis, "_warp_faces", "_warp_faces")
    spy(app.rec, "forward", "forward", note=lambda crops: int(crops.shape[0]))
    for attr in ("associate_device", "resolve_device", "commit_device", "fuse_device"):
        spy(FaceTracks, attr, attr.split("_")[0])
    spy(FaceQuality, "measure_device", "measure")
    real_cpu = torch.Tensor.cpu

    def cpu(self, *a, **kw):
        if self.is_cuda:
            log.append("cpu")
        return real_cpu(self, *a, **kw)
    monkeypatch.setattr(torch.Tensor, "cpu", cpu)
    return log


def _expected(r, judging, tracked, quality, template):
    """the sequence the pass must have recorded, and the slots it had to embed - both from the returned columns"""
    counts = r["counts"].cpu().numpy()
    cap = r["bbox"].shape[1]
    valid = np.arange(cap)[None, :] < counts[:, None]
    if judging:
        embed = valid & (r["track_action"].cpu().numpy() == 1)
    elif tracked:
        embed = valid & (r["carried"].cpu().numpy() == 0)
    elif quality:
        embed = valid & (r["quality_verdict"].cpu().numpy() == 0)
    else:
        embed = valid
    F = int(embed.sum())
    all_slots = judging or quality
    seq = ["associate"] if tracked else []
    seq += (["_warp_slots", "measure"] if all_slots else []) + (["resolve"] if judging else []) + ["cpu"]
    if F:
        seq += ([] if all_slots else ["_warp_faces"]) + [("forward", F)]
    if tracked:
        seq += ["commit"] + (["fuse"] if template else [])
    return seq, F


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_each_pass_runs_its_steps_in_order_with_one_copy(world, spies, variant):
    from facerecognition_infrenceengine_amd import FaceTracks
    app, dev, accept = world
    v = VARIANTS[variant]
    kw = {}
    if "tracks" in v:
        kw = {"tracks": FaceTracks(slots=8, template=v["tracks"], quality=accept if v.get("judge") else None), "camera_ids": CAMS}
    if v.get("quality"):
        kw["quality"] = accept
    embedded = []
    for turn in range(2):                                        # the same frames twice: the second turn has faces to carry
        del spies[:]
        r = app.detect_embed_slots(dev, compact_embed=True, **kw)
        seen = list(spies)                                       # what ran inside the call; the reads below copy as well
        seq, F = _expected(r, bool(v.get("judge")), "tracks" in v, bool(v.get("quality")), bool(v.get("tracks")))
        print(variant, turn, seen, F)
        assert seen == seq, (variant, turn)
        assert seen.count("cpu") == 1
        assert (("forward", F) in seen) == (F > 0)
        embedded.append(F)
    assert embedded[0] >= 2                                      # each frame holds a face: the first turn embeds


def test_the_call_without_compact_embed_copies_nothing(world, spies):
    app, dev, _ = world
    del spies[:]
    r = app.detect_embed_slots(dev)
    seen = list(spies)
    assert seen == ["_warp_slots", ("forward", r["bbox"].shape[0] * r["bbox"].shape[1])]
    assert set(r) == {"counts", "bbox", "kps", "det_score", "embedding", "normed_embedding"}
