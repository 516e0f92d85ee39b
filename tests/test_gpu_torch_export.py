"""Networks exported by torch's own ONNX exporter (tests/helpers/torch_export.py, from the plain nn.Modules of
tests/helpers/torch_nets.py) through the engine on the MI355X, against the exported module itself in float64 - the path a real
model pack takes, with a writer that shares nothing with the readers of onnx_import.py.

  IResNet-18     default export -> iresnet_state_from_onnx -> IResNetHIP against module.double(): 1 - cos < 1e-3 per face, the
                 bound tests/test_gpu_embed.py::test_r50_variant_vs_oracle applies to this path; the export with constant
                 folding off (BatchNormalization kept as nodes) gives the embedding bits of the module's own state_dict()
  MobileFaceNet  PlanRecogniserHIP on the file against module.double(): the 4 e policy of tests/test_gpu_mbf.py
  detectors      SCRFDHIP on the file, 64 x 64 canvas: the nine head maps against module.double(), the 4 e policy of
                 tests/test_gpu_scrfd.py::test_heads_within_four_e_of_r64 (decode + NMS: the tests there)
  a pack         the exported files drop into FaceAnalysis without a warning

e = max |E16 - R64| is measured on the CPU for these modules and inputs and recorded in tests/helpers/torch_cases.py;
tests/test_onnx_torch_export.py re-measures it."""
import copy
import shutil
import warnings

import numpy as np
import pytest
import torch

from facerecognition_infrenceengine_amd import weights
from tests.helpers import mbf_ref, scrfd_ref
from tests.helpers import torch_cases as cases
from tests.helpers import torch_nets as tn
from tests.helpers.torch_export import export

pytestmark = pytest.mark.gpu


def _f64(module, x):
    with torch.no_grad():
        out = copy.deepcopy(module).double()(x)
    return [t.numpy() for t in out] if isinstance(out, tuple) else out.numpy()


def _nhwc8(x):
    """float32 [B,3,H,W] holding f16 numbers -> f16 [B,H,W,8] on the device (channels 0..2, rest zero)"""
    out = torch.zeros((x.shape[0], x.shape[2], x.shape[3], 8), dtype=torch.float16)
    out[..., :3] = x.permute(0, 2, 3, 1).to(torch.float16)
    return out.cuda()


@pytest.fixture(scope="module")
def r18(tmp_path_factory):
    d = tmp_path_factory.mktemp("r18")
    m = cases.iresnet18()
    example = torch.zeros(1, 3, 112, 112)
    folded = export(m, example, d / "w600k_r18.onnx")
    unfolded = export(m, example, d / "unfolded.onnx", opset_version=11, do_constant_folding=False)
    return m, folded, unfolded


def test_iresnet18_export_against_the_module(r18):
    from facerecognition_infrenceengine_amd.iresnet import IResNetHIP
    m, folded, unfolded = r18
    x = cases.iresnet_input(3)
    ref = _f64(m, x.double())
    st = weights.load_state(folded)
    assert "layer1.0.conv1.bias" in st and "layer1.0.bn2.weight" not in st            # BatchNorms folded by the exporter
    emb, normed = IResNetHIP(st, "r18", "cuda:0").forward(_nhwc8(x))
    emb = emb.cpu().numpy().astype(np.float64)
    cos = (emb * ref).sum(1) / (np.linalg.norm(emb, axis=1) * np.linalg.norm(ref, axis=1))
    print(f"r18, default export: 1 - cos per face = {(1 - cos).tolist()}, max |ref| = {float(np.abs(ref).max()):.4g}")
    assert emb.shape == ref.shape == (3, 512) and (1 - cos).max() < 1e-3, cos
    n = normed.cpu().numpy().astype(np.float64)
    assert np.abs(n - emb / np.linalg.norm(emb, axis=1, keepdims=True)).max() < 1e-6


def test_unfolded_iresnet18_export_gives_the_bits_of_the_state_dict(r18):
    from facerecognition_infrenceengine_amd.iresnet import IResNetHIP
    m, folded, unfolded = r18
    x = _nhwc8(cases.iresnet_input(3))
    own = {k: v.detach().clone() for k, v in m.state_dict().items() if not k.endswith("num_batches_tracked")}
    st = weights.load_state(unfolded)
    assert set(st) == set(own)
    a, an = IResNetHIP(st, "r18", "cuda:0").forward(x)
    b, bn = IResNetHIP(own, "r18", "cuda:0").forward(x)
    assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))
    assert np.array_equal(an.cpu().numpy().view(np.uint32), bn.cpu().numpy().view(np.uint32))
    assert np.isfinite(a.cpu().numpy()).all() and float(a.abs().max()) > 0.1


@pytest.fixture(scope="module")
def mbf(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("mbf") / "w600k_mbf.onnx")
    return cases.export_mbf(p), p


def test_mobilefacenet_export_within_four_e_of_the_module(mbf):
    from facerecognition_infrenceengine_amd.mbf import PlanRecogniserHIP
    m, path = mbf
    rec = PlanRecogniserHIP(path)
    assert len(rec.plan.steps) - 1 == len(tn.layer_list(m)) and rec.flops_per_face == rec.plan.macs2 > 0
    x = cases.mbf_crops()
    want = _f64(m, mbf_ref.blob(x))
    emb, normed = rec.forward(x.cuda())
    assert emb.shape == normed.shape == (cases.MBF_CROPS, 512) and emb.dtype == torch.float32
    got = emb.cpu().numpy().astype(np.float64)
    err, cos = float(np.abs(got - want).max()), float(cases.cos_dist(got, want).max())
    print(f"mobilefacenet: max |gpu - module| = {err:.4e} (e = {cases.E_MBF}, bound {4 * cases.E_MBF}); 1 - cos = {cos:.3e} "
          f"(E16: {cases.COS_MBF}, bound {4 * cases.COS_MBF}); max |module| = {float(np.abs(want).max()):.4g}")
    assert err <= 4 * cases.E_MBF
    assert cos <= 4 * cases.COS_MBF
    n = normed.cpu().numpy().astype(np.float64)
    assert np.abs(n - got / np.linalg.norm(got, axis=1, keepdims=True)).max() < 1e-6


@pytest.fixture(scope="module")
def detectors(tmp_path_factory):
    d = tmp_path_factory.mktemp("det")
    out = {}
    for dw in (False, True):
        p = str(d / f"det_{cases.det_name(dw)}.onnx")
        out[dw] = (cases.export_detector(p, dw), p)
    return out


@pytest.mark.parametrize("dw", [False, True], ids=["plain", "dw"])
def test_detector_export_heads_within_four_e_of_the_module(detectors, dw):
    from facerecognition_infrenceengine_amd.scrfd import SCRFDHIP
    m, path = detectors[dw]
    E = cases.E_DET[cases.det_name(dw)]
    det = SCRFDHIP(path)
    plan = det.plan(cases.DET_HW)
    assert plan.num_anchors == 2 and sum(s["op"] == "dwconv" for s in plan.steps) == (11 if dw else 0)
    frames = cases.det_frames()
    want = dict(zip(tn.OUTPUT_ORDER, _f64(m, scrfd_ref.blob(frames))))
    ar, heads = det.forward_heads(torch.from_numpy(frames).cuda())
    assert len(heads) == 3
    for li, (stride, sc, bb, kp) in enumerate(heads):
        n = sc.shape[0]
        got = {"score": sc.cpu().numpy().reshape(n, -1, 1), "bbox": bb.cpu().numpy().reshape(n, -1, 4), "kps": kp.cpu().numpy().reshape(n, -1, 10)}
        assert stride == (8, 16, 32)[li] and n == cases.DET_FRAMES
        for kind in ("score", "bbox", "kps"):
            w = want[(li, kind)]
            if kind == "score":                                         # the module gives probabilities, the engine keeps logits
                w = np.log(w) - np.log1p(-w)
            assert got[kind].shape == w.shape == (n, (64 // stride) ** 2 * 2, {"score": 1, "bbox": 4, "kps": 10}[kind])
            err = float(np.abs(got[kind] - w).max())
            print(f"{cases.det_name(dw)} stride {stride} {kind}: max |gpu - module| = {err:.4e} (e = {E[kind]}, bound {4 * E[kind]})")
            assert err <= 4 * E[kind]


@pytest.mark.parametrize("rec", ["mbf", "r18"])
def test_a_torch_exported_pack_drops_in(tmp_path, detectors, mbf, r18, rec):
    from facerecognition_infrenceengine_amd import FaceAnalysis
    from facerecognition_infrenceengine_amd.iresnet import IResNetHIP
    from facerecognition_infrenceengine_amd.mbf import PlanRecogniserHIP
    from facerecognition_infrenceengine_amd.scrfd import SCRFDHIP
    d = tmp_path / "models" / "exported"
    d.mkdir(parents=True)
    shutil.copy(detectors[rec == "mbf"][1], d / "det_500m.onnx")
    shutil.copy(mbf[1] if rec == "mbf" else r18[1], d / ("w600k_mbf.onnx" if rec == "mbf" else "w600k_r18.onnx"))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        app = FaceAnalysis(name="exported", root=str(tmp_path)).prepare(ctx_id=0, det_size=(64, 64))
    assert app.synthetic is False and app.arch == rec and app.det_size == (64, 64)
    assert isinstance(app.det, SCRFDHIP) and isinstance(app.rec, PlanRecogniserHIP if rec == "mbf" else IResNetHIP)
    res = app.get_batch(cases.det_frames())
    assert len(res) == cases.DET_FRAMES
    for faces in res:
        for f in faces:
            assert f.embedding.shape == (512,) and np.isfinite(f.embedding).all() and abs(float(np.linalg.norm(f.normed_embedding)) - 1.0) < 1e-5
