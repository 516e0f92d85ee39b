"""A buffalo_s-shaped pack - a depthwise SCRFD detector and a MobileFaceNet recogniser, both read from ONNX - dropping into
FaceAnalysis whole on the MI355X: the detector's head maps against float64, then get_batch and the recognition processor.

Head tolerance: the SCRFD policy, 4 e with e = max |E16 - R64| per head kind measured on the CPU for
this graph and these frames (tests/helpers/mbf_cases.py E_DET).  Embedding tolerance: 4 e with e = max |E16 - R64| of
tests/helpers/mbf_ref.py on the very crops the engine aligned (computed here: the net is narrow)."""
import warnings

import numpy as np
import pytest
import torch

from facerecognition_infrenceengine_amd import onnx_import
from tests.helpers import mbf_cases as cases
from tests.helpers import mbf_ref
from tests.helpers.mbf_onnx import CFG_TINY, write_dw_scrfd_onnx, write_mbf_onnx
from tests.helpers.scrfd_onnx import lowpass_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pack(tmp_path_factory):
    root = tmp_path_factory.mktemp("packroot")
    d = root / "models" / "buffalo_s"
    d.mkdir(parents=True)
    write_dw_scrfd_onnx(d / "det_500m.onnx", seed=cases.DET_SEED, score_bias=cases.DET_BIAS)
    write_mbf_onnx(d / "w600k_mbf.onnx", CFG_TINY, seed=cases.GRAPH_SEED, fold_bn=False, fc="matmul")
    return root


@pytest.fixture(scope="module")
def frames():
    return lowpass_frames(cases.DET_FRAMES, 64, 64, seed=cases.DET_FRAME_SEED)


@pytest.fixture(scope="module")
def app(pack):
    from facerecognition_infrenceengine_amd import FaceAnalysis
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # no synthetic-weights warning of any kind
        return FaceAnalysis(name="buffalo_s", root=str(pack)).prepare(ctx_id=0, det_size=(64, 64))


def test_depthwise_heads_within_four_e_of_r64(pack, frames):
    from facerecognition_infrenceengine_amd.scrfd import SCRFDHIP
    path = str(pack / "models" / "buffalo_s" / "det_500m.onnx")
    det = SCRFDHIP(path)
    plan = det.plan((64, 64))
    assert sum(s["op"] == "dwconv" for s in plan.steps) >= 10
    want = mbf_ref.run_scrfd_plan(onnx_import.scrfd_plan_from_onnx(path, (64, 64)), frames)
    ar, heads = det.forward_heads(torch.from_numpy(frames).cuda())
    for (stride, sc, bb, kp), w in zip(heads, want):
        n = sc.shape[0]
        got = {"score": sc.cpu().numpy(), "bbox": bb.cpu().numpy().reshape(n, -1, 4), "kps": kp.cpu().numpy().reshape(n, -1, 10)}
        for kind in ("score", "bbox", "kps"):
            err = float(np.abs(got[kind] - w[kind]).max())
            print(f"stride {stride} {kind}: max |gpu - r64| = {err:.4e} (e = {cases.E_DET[kind]}, bound {4 * cases.E_DET[kind]})")
            assert got[kind].shape == w[kind].shape and err <= 4 * cases.E_DET[kind]


def test_pack_drops_in_whole(app, frames):
    from facerecognition_infrenceengine_amd.mbf import PlanRecogniserHIP
    from facerecognition_infrenceengine_amd.scrfd import SCRFDHIP
    assert isinstance(app.det, SCRFDHIP) and isinstance(app.rec, PlanRecogniserHIP) and app.synthetic is False
    assert app.arch == "mbf" and app.det_size == (64, 64)
    res = app.get_batch(frames)
    assert len(res) == len(frames) and all(len(r) >= 1 for r in res)
    for faces in res:
        for f in faces:
            assert f.bbox.shape == (4,) and f.kps.shape == (5, 2) and f.embedding.shape == f.normed_embedding.shape == (512,)
            assert f.bbox.dtype == f.kps.dtype == f.embedding.dtype == f.normed_embedding.dtype == np.float32
            assert isinstance(f.det_score, float) and 0.5 <= f.det_score <= 1.0
            assert abs(float(np.linalg.norm(f.normed_embedding)) - 1.0) < 1e-5
    # the same embeddings from the crops of the slot pipeline, bit for bit
    dev = torch.from_numpy(frames).cuda()
    cap = app.det.cap_out
    crops = torch.empty((len(frames) * cap, 112, 112, 8), dtype=torch.float16, device="cuda")
    r = app.detect_embed_slots(dev, crops_out=crops)
    counts = r["counts"].cpu().numpy()
    assert counts.tolist() == [len(x) for x in res]
    sel = [f * cap + j for f in range(len(frames)) for j in range(counts[f])]
    mine = crops[sel].contiguous()
    emb, normed = app.rec.forward(mine)
    flat = [f for faces in res for f in faces]
    assert np.array_equal(np.stack([f.embedding for f in flat]).view(np.uint32), emb.cpu().numpy().view(np.uint32))
    assert np.array_equal(np.stack([f.normed_embedding for f in flat]).view(np.uint32), normed.cpu().numpy().view(np.uint32))
    # and within 4 e of the float64 forward of those crops, e measured on them
    plan = app.rec.plan
    host = mine.cpu()
    assert not host[..., 3:].any()                               # the warp's format: zeros in channels 3..7
    r64, e16 = mbf_ref.run_plan(plan, host, "r64"), mbf_ref.run_plan(plan, host, "e16")
    e = float(np.abs(e16 - r64).max())
    err = float(np.abs(emb.cpu().numpy().astype(np.float64) - r64).max())
    print(f"{len(flat)} faces: max |gpu - r64| = {err:.4e}, e = {e:.4e}, bound {4 * e:.4e}")
    assert err <= 4 * e


def test_processor_recognises_the_planted_ids(app, frames):
    from facerecognition_infrenceengine_amd.processor import EmbeddingManager, FaceRecognitionProcessor, InMemoryStore
    two = [frames[0], frames[2]]
    faces = [app.get(f) for f in two]
    assert all(faces)
    store = InMemoryStore()
    rng = np.random.default_rng(0)
    for i in range(20):
        store.add_employee(f"n{i}", "acme", rng.standard_normal(512).astype(np.float32), name=f"N{i}")
    for k, fs in enumerate(faces):
        store.add_employee(f"face{k}", "acme", fs[0].embedding, name=f"F{k}")
    proc = FaceRecognitionProcessor(EmbeddingManager(store=store, device="cuda:0"), face_detector=app)
    res = proc.recognize_batch(two, "acme")
    for k, (got, want) in enumerate(zip(res, faces)):
        assert len(got) == len(want)
        assert got[0]["person_id"] == f"face{k}" and np.array_equal(got[0]["bbox"], want[0].bbox.astype(int))
