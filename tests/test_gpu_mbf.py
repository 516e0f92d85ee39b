"""The plan recogniser (MobileFaceNet read from ONNX, mbf.PlanRecogniserHIP) on the MI355X against the CPU restatement of
tests/helpers/mbf_ref.py.

Tolerance: the project's SCRFD policy (DESIGN.md sections 4.3b / 4.3c).  e = max |E16 - R64| over the embedding elements of
the test's own crops, measured on the CPU and recorded in tests/helpers/mbf_cases.py; every GPU element must lie within 4 e of
R64 (the 4 x covers summation order and the f32-versus-f64 epilogue), and 1 - cos(GPU, R64) within 4 x the same figure of
E16."""
import threading
import warnings

import numpy as np
import pytest
import torch

from facerecognition_infrenceengine_amd import _lib, onnx_import
from tests.helpers import mbf_cases as cases
from tests.helpers import mbf_ref
from tests.helpers.mbf_onnx import write_dw_scrfd_onnx
from tests.helpers.scrfd_onnx import lowpass_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nets(tmp_path_factory):
    d = tmp_path_factory.mktemp("mbf")
    out = {}
    for net in cases.NETS:
        p = str(d / f"{net}.onnx")
        cases.write_net(p, net)
        out[net] = p
    return out


@pytest.fixture(scope="module")
def small(nets):
    from facerecognition_infrenceengine_amd.mbf import PlanRecogniserHIP
    return PlanRecogniserHIP(nets["1111"])


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("net", list(cases.NETS))
def test_embedding_within_four_e_of_r64(nets, net):
    from facerecognition_infrenceengine_amd.mbf import PlanRecogniserHIP
    plan = onnx_import.recognition_plan_from_onnx(nets[net])
    rec = PlanRecogniserHIP(plan)
    assert rec.flops_per_face == plan.macs2 > 0
    x = cases.crops_of(net)
    want = mbf_ref.run_plan(plan, x, "r64")
    emb, normed = rec.forward(x.cuda())
    assert emb.shape == normed.shape == (len(x), 512) and emb.dtype == normed.dtype == torch.float32 and emb.is_cuda
    got = emb.cpu().numpy().astype(np.float64)
    err, cos = float(np.abs(got - want).max()), float(cases.cos_dist(got, want).max())
    print(f"{net}: max |gpu - r64| = {err:.4e} (e = {cases.E[net]}, bound {4 * cases.E[net]}); 1 - cos = {cos:.3e} "
          f"(E16: {cases.COS[net]}, bound {4 * cases.COS[net]})")
    assert err <= 4 * cases.E[net]
    assert cos <= 4 * cases.COS[net]
    n = normed.cpu().numpy().astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-6
    assert np.abs(n - got / np.linalg.norm(got, axis=1, keepdims=True)).max() < 1e-6


def test_batch_and_chunking_do_not_change_a_bit(nets, small):
    from facerecognition_infrenceengine_amd.mbf import PlanRecogniserHIP
    x = mbf_ref.seeded_crops(5, seed=31).cuda()
    emb, normed = small.forward(x)
    for i in range(5):
        e1, n1 = small.forward(x[i:i + 1].contiguous())
        assert np.array_equal(_bits(e1)[0], _bits(emb)[i]) and np.array_equal(_bits(n1)[0], _bits(normed)[i]), i
    chunked = PlanRecogniserHIP(nets["1111"], max_chunk=2)
    e2, n2 = chunked.forward(x)
    assert np.array_equal(_bits(e2), _bits(emb)) and np.array_equal(_bits(n2), _bits(normed))
    small.release_plans()                                   # arenas are rebuilt on demand: the same bits again
    e3, _ = small.forward(x)
    assert np.array_equal(_bits(e3), _bits(emb))


def test_two_threads_share_one_recogniser(small):
    xs = [mbf_ref.seeded_crops(3, seed=40 + i).cuda() for i in range(2)]
    want = [_bits(small.forward(x)[0]) for x in xs]
    got, errs = [None, None], []

    def work(i):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                for _ in range(4):
                    e, _n = small.forward(xs[i])
                torch.cuda.current_stream().synchronize()
                got[i] = _bits(e)
        except Exception as ex:                              # pragma: no cover - reported below
            errs.append(ex)
    torch.cuda.synchronize()
    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.fixture(scope="module")
def app(tmp_path_factory):
    from facerecognition_infrenceengine_amd import FaceAnalysis
    root = tmp_path_factory.mktemp("packroot")
    d = root / "models" / "buffalo_sc"
    d.mkdir(parents=True)
    write_dw_scrfd_onnx(d / "det_500m.onnx", seed=cases.DET_SEED, score_bias=cases.DET_BIAS)
    cases.write_net(str(d / "w600k_mbf.onnx"), "1111")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return FaceAnalysis(name="buffalo_sc", root=str(root)).prepare(ctx_id=0, det_size=(64, 64))


def test_graph_replay_equals_eager_through_get(nets, tmp_path):
    """FaceAnalysis replays graphs only without a detection canvas, so this pack pairs the recogniser with MTCNN weights: get()
    with graphs on (the detector graph, then the captured align + embed of the face slots) returns the eager bits."""
    import os
    import shutil
    import sys
    from facerecognition_infrenceengine_amd import FaceAnalysis, weights
    from facerecognition_infrenceengine_amd.mbf import PlanRecogniserHIP
    from facerecognition_infrenceengine_amd.mtcnn import MTCNNHIP
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from make_golden import synth_frame
    d = tmp_path / "models" / "mixed"
    d.mkdir(parents=True)
    for n, st in zip(("pnet", "rnet", "onet"), weights.synth_mtcnn_states()):
        torch.save(st, d / f"mtcnn_{n}.pt")
    shutil.copy(nets["1111"], d / "w600k_mbf.onnx")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        app = FaceAnalysis(name="mixed", root=str(tmp_path)).prepare(ctx_id=0)
    assert isinstance(app.det, MTCNNHIP) and isinstance(app.rec, PlanRecogniserHIP) and app.arch == "mbf" and app.synthetic is False
    frame = synth_frame(240, 320, 4)
    eager = app.get(frame)
    assert len(eager) >= 1
    app.enable_graphs(True)
    try:
        first, again = app.get(frame), app.get(frame)                  # capture, then a pure replay
    finally:
        app.enable_graphs(False)
    for got in (first, again):
        assert len(got) == len(eager)
        for a, b in zip(got, eager):
            assert np.array_equal(a.embedding.view(np.uint32), b.embedding.view(np.uint32))
            assert np.array_equal(a.normed_embedding.view(np.uint32), b.normed_embedding.view(np.uint32)) and np.array_equal(a.bbox, b.bbox)
    other = app.clone_with(cap_o=1)
    assert other.rec is app.rec and other.arch == "mbf"
    assert np.array_equal(other.get(frame)[0].embedding, eager[0].embedding)


def test_calibrate_fp8_is_refused(app):
    frames = lowpass_frames(2, 64, 64, seed=1)
    with pytest.raises(_lib.FrError, match="IResNet only"):
        app.calibrate_fp8(frames)
    with pytest.raises(_lib.FrError, match="IResNet only"):
        app.rec.enable_fp8(None)
