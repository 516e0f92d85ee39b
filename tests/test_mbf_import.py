"""Plan recogniser import (no GPU): onnx_import.recognition_plan_from_onnx on MobileFaceNet-shaped graphs written by
tests/helpers/mbf_onnx.py, the plan's folded weights against the raw graph in float64, the refusals, the depthwise SCRFD
plan, the model-pack search of FaceAnalysis, the ABI."""
import logging
import os
import re
import warnings

import numpy as np
import pytest

from facerecognition_infrenceengine_amd import _lib, onnx_import, weights
from tests.helpers import mbf_ref, scrfd_ref
from tests.helpers.mbf_onnx import (CFG_DW_SMALL, CFG_FULL, CFG_TINY, dw_scrfd_counts, n_steps, write_dw_scrfd_onnx,
                                    write_mbf_onnx)
from tests.helpers.onnx_write import write_iresnet_onnx
from tests.helpers.scrfd_onnx import CFG_SMALL, lowpass_frames, write_scrfd_onnx

STYLES = [(True, "gemm", "Flatten"), (False, "gemm", "Reshape"), (True, "matmul", "Flatten"), (False, "matmul", "Flatten"),
          (False, "gemm_nt", "Flatten")]                                 # (BN folded, fc spelling, flatten spelling)


def test_plan_of_the_full_net_has_the_expected_steps(tmp_path):
    path = tmp_path / "w600k_mbf.onnx"
    write_mbf_onnx(path, CFG_FULL, seed=1, fold_bn=False)
    plan = onnx_import.recognition_plan_from_onnx(str(path))
    convs = [s for s in plan.steps if s["op"] == "conv"]
    dws = [s for s in plan.steps if s["op"] == "dwconv"]
    assert (len(convs), len(dws)) == n_steps(CFG_FULL) == (33, 17) and plan.steps[0]["op"] == "input"
    assert len(plan.steps) == 1 + 33 + 17
    # stem 3x3 s2 PReLU on the crop; the fully connected layer is the last step, f32, linear
    assert (convs[0]["k"], convs[0]["stride"], convs[0]["act"], convs[0]["x"]) == (3, 2, 2, 0) and convs[0]["w"].shape == (64, 3, 3, 3)
    assert plan.steps[-1] is convs[-1] and convs[-1]["f32"] and convs[-1]["act"] == 0 and convs[-1]["w"].shape == (512, 512, 1, 1)
    assert sum(s["f32"] for s in plan.steps[1:]) == 1 and plan.output == convs[-1]["out"] and plan.dim == 512
    # blocks (1, 4, 6, 2): 12 skip connections, each the residual of a linear 1x1 project conv; 3 stride-2 blocks without
    assert sum(s["res"] is not None for s in convs) == 12 and all(s["act"] == 0 and s["k"] == 1 for s in convs if s["res"] is not None)
    assert [s["stride"] for s in dws].count(2) == 3 and all(s["res"] is None for s in dws)
    assert (dws[-1]["k"], dws[-1]["pad"], dws[-1]["act"]) == (7, 0, 0) and plan.shapes[dws[-1]["x"]] == (512, 7, 7)
    assert all(s["k"] == 3 and s["pad"] == 1 and s["act"] == 2 for s in dws[:-1])
    sizes = [plan.shapes[s["out"]][1] for s in dws]
    assert sizes == [56] + [28] * 5 + [14] * 7 + [7] * 3 + [1]
    for s in plan.steps[1:]:
        assert s["w"].dtype == np.float64 and s["b"].shape == (s["w"].shape[0],)
        assert (s["slope"] is not None and s["slope"].shape == (s["w"].shape[0],)) == (s["act"] == 2)
    assert plan.macs2 == sum(2 * plan.shapes[s["out"]][1] * plan.shapes[s["out"]][2] * s["w"].size for s in plan.steps[1:])
    assert 0.40e9 < plan.macs2 < 0.48e9                                 # MobileFaceNet: ~0.44 GFLOP (2 x MAC) per face


@pytest.mark.parametrize("fold_bn,fc,flatten", STYLES)
def test_folded_plan_is_the_raw_graph_in_float64(tmp_path, fold_bn, fc, flatten):
    path = tmp_path / "mbf.onnx"
    write_mbf_onnx(path, CFG_TINY, seed=2, fold_bn=fold_bn, fc=fc, flatten=flatten)
    crops = mbf_ref.seeded_crops(2, seed=3)
    plan = onnx_import.recognition_plan_from_onnx(str(path))
    assert (len([s for s in plan.steps if s["op"] == "conv"]), len([s for s in plan.steps if s["op"] == "dwconv"])) == n_steps(CFG_TINY)
    raw = mbf_ref.r64_graph(str(path), crops)
    have = mbf_ref.run_plan(plan, crops, "r64")
    assert raw.shape == have.shape == (2, 512) and np.abs(raw).max() > 0.1
    assert np.abs(raw - have).max() < 1e-12


@pytest.mark.parametrize("mutate,match", [("group2", r"node '\d+' \(Conv\): grouped conv \(group 2"),
                                          ("dilation", r"node '\d+' \(Conv\): dilations \[2, 2\]"),
                                          ("relu", r"node '\d+' \(Relu\): op Relu is not supported"),
                                          ("two_outputs", r"expected one graph output.*found 2.*node '\d+' \((Add|Conv)\)"),
                                          ("slope_len", r"node '\d+' \(PRelu\): PRelu slope of shape .* on 16 channels")])
def test_refusals_name_the_node(tmp_path, mutate, match):
    path = tmp_path / "bad.onnx"
    write_mbf_onnx(path, CFG_TINY, seed=5, mutate=mutate)
    with pytest.raises(ValueError, match=match):
        onnx_import.recognition_plan_from_onnx(str(path))


def test_a_detector_is_no_recogniser_and_an_iresnet_stays_an_iresnet(tmp_path):
    det = tmp_path / "det_10g.onnx"
    write_scrfd_onnx(det, CFG_SMALL, seed=5)
    with pytest.raises(ValueError, match=r"node '\d+' \(Relu\)"):
        onnx_import.recognition_plan_from_onnx(str(det))
    dwdet = tmp_path / "det_500m.onnx"
    write_dw_scrfd_onnx(dwdet, seed=5)
    with pytest.raises(ValueError, match=r"node '\d+' \(Relu\)"):
        onnx_import.recognition_plan_from_onnx(str(dwdet))
    # and the other way round: a MobileFaceNet is no detector (PRelu is still refused there) and no IResNet
    mbf = tmp_path / "w600k_mbf.onnx"
    write_mbf_onnx(mbf, CFG_TINY, seed=5)
    with pytest.raises(ValueError, match=r"\(PRelu\)"):
        onnx_import.scrfd_plan_from_onnx(str(mbf), (640, 640))
    with pytest.raises(ValueError):
        onnx_import.iresnet_state_from_onnx(str(mbf))
    st = weights.synth_iresnet_state("r18", seed=3)
    r18 = tmp_path / "w600k_r18.onnx"
    write_iresnet_onnx(r18, {k: v.numpy() for k, v in st.items()}, "r18", fold_bn=True)
    assert onnx_import.iresnet_state_from_onnx(str(r18))[1] == "r18"
    from facerecognition_infrenceengine_amd.face_analysis import FaceAnalysis
    d = tmp_path / "models" / "pack"
    d.mkdir(parents=True)
    write_dw_scrfd_onnx(d / "det_500m.onnx", seed=6)
    write_iresnet_onnx(d / "w600k_r18.onnx", {k: v.numpy() for k, v in st.items()}, "r18", fold_bn=True)
    app = FaceAnalysis(name="pack", root=str(tmp_path))
    rec, _ = app._load_states()
    assert app.arch == "r18" and isinstance(rec, dict) and app._scrfd_graph is not None


@pytest.mark.parametrize("fold_bn", [True, False])
def test_depthwise_scrfd_plan(tmp_path, fold_bn):
    path = tmp_path / "det_500m.onnx"
    names = write_dw_scrfd_onnx(path, seed=3, fold_bn=fold_bn, score_bias=-1.0)
    plan = onnx_import.scrfd_plan_from_onnx(str(path), (64, 96))
    convs = [s for s in plan.steps if s["op"] == "conv"]
    dws = [s for s in plan.steps if s["op"] == "dwconv"]
    assert (len(convs), len(dws)) == dw_scrfd_counts(CFG_DW_SMALL) and list(plan.outputs) == names
    assert all(s["k"] == 3 and s["pad"] == 1 and s["relu"] and s["res"] is None and not s["f32"] and s["w"].shape[1] == 1 for s in dws)
    assert sorted({s["stride"] for s in dws}) == [1, 2]
    assert plan.macs2 == sum(2 * plan.shapes[s["out"]][1] * plan.shapes[s["out"]][2] * s["w"].size for s in convs + dws)
    frames = lowpass_frames(2, 64, 96, seed=1)
    raw = scrfd_ref.r64_graph(str(path), frames)
    levels = mbf_ref.run_scrfd_plan(plan, frames)
    for t, (li, kind) in plan.outputs.items():
        want, have = raw[t], levels[li][kind]
        if kind == "score":
            have = 1.0 / (1.0 + np.exp(-have))
        assert np.abs(want.reshape(have.shape) - have).max() < 1e-12, (t, kind)


def test_pack_with_a_depthwise_scrfd_and_a_mobilefacenet_loads_without_any_warning(tmp_path, caplog):
    from facerecognition_infrenceengine_amd.face_analysis import FaceAnalysis
    d = tmp_path / "models" / "buffalo_s"
    d.mkdir(parents=True)
    write_dw_scrfd_onnx(d / "det_500m.onnx", seed=6)
    write_mbf_onnx(d / "w600k_mbf.onnx", CFG_TINY, seed=7, fold_bn=False)
    (d / "genderage.onnx").write_bytes(b"\x08")
    app = FaceAnalysis(name="buffalo_s", root=str(tmp_path))
    with warnings.catch_warnings(), caplog.at_level(logging.INFO):
        warnings.simplefilter("error")
        rec, det = app._load_states()
    assert det is None and app._scrfd_graph is not None and app.synthetic is False and app.arch == "mbf"
    assert isinstance(rec, onnx_import.RecognitionPlan) and rec.dim == 512
    assert any("genderage.onnx" in r.getMessage() for r in caplog.records)
    # the detector alone is still refused with the wording the other import tests pin
    (d / "w600k_mbf.onnx").unlink()
    with pytest.raises(_lib.FrError, match="none of its .onnx files"):
        app._load_states()


def test_new_entries_are_declared_exported_and_bound_under_abi_106():
    import ctypes as C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "frhip.h")).read()
    lib = _lib.load()
    assert int(re.search(r"#define FR_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == lib.fr_version() == 106
    cdll = C.CDLL(_lib.LIB_PATH)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, nargs in (("fr_dw_conv_f16", 16), ("fr_det_conv_act_f16", 22)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs and hasattr(cdll, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    one = C.c_void_p(16)                                              # never dereferenced: the arguments are refused first
    with pytest.raises(_lib.FrError, match="does not follow"):
        lib.fr_dw_conv_f16(one, one, one, None, one, 1, 8, 8, 8, 3, 2, 1, 5, 4, 0, None)
    with pytest.raises(_lib.FrError, match="multiple of 8"):
        lib.fr_dw_conv_f16(one, one, one, None, one, 1, 8, 8, 12, 3, 1, 1, 8, 8, 0, None)
    with pytest.raises(_lib.FrError, match="kernel 4"):
        lib.fr_dw_conv_f16(one, one, one, None, one, 1, 8, 8, 8, 4, 1, 1, 7, 7, 0, None)
    with pytest.raises(_lib.FrError, match="needs the slope"):
        lib.fr_dw_conv_f16(one, one, one, None, one, 1, 8, 8, 8, 3, 1, 1, 8, 8, 2, None)
    with pytest.raises(_lib.FrError, match="null pointer"):
        lib.fr_dw_conv_f16(None, one, one, None, one, 1, 8, 8, 8, 3, 1, 1, 8, 8, 0, None)
    with pytest.raises(_lib.FrError, match="needs the slope"):
        lib.fr_det_conv_act_f16(one, one, one, None, None, one, 1, 8, 8, 32, 32, 3, 1, 1, 8, 8, 32, 32, 2, 0, 0, None)
    with pytest.raises(_lib.FrError, match="fr_det_conv_act_f16: Cin 28 must be a positive multiple of 8"):
        lib.fr_det_conv_act_f16(one, one, one, one, None, one, 1, 8, 8, 28, 32, 3, 1, 1, 8, 8, 32, 32, 2, 0, 0, None)


def test_pack_dw_layout():
    from facerecognition_infrenceengine_amd.scrfd import pack_dw
    rng = np.random.default_rng(0)
    w = rng.standard_normal((12, 1, 3, 3))
    wt, bias, slope, cp = pack_dw(w, np.arange(12), np.arange(12) * 0.5)
    assert cp == 16 and wt.shape == (9, 16) and wt.dtype == np.float16 and bias.dtype == slope.dtype == np.float32
    for tap in range(9):
        assert np.array_equal(wt[tap, :12], w[:, 0, tap // 3, tap % 3].astype(np.float16)) and not wt[tap, 12:].any()
    assert np.array_equal(bias[:12], np.arange(12)) and not bias[12:].any() and slope[3] == 1.5 and not slope[12:].any()
    assert pack_dw(w, np.zeros(12))[2] is None
