"""SCRFD detector import (no GPU): onnx_import.scrfd_plan_from_onnx on graphs written by tests/helpers/scrfd_onnx.py, the
plan's folded weights against the raw graph in float64, the refusals, the model-pack search of FaceAnalysis, the ABI."""
import logging
import re
import warnings

import numpy as np
import pytest

from facerecognition_infrenceengine_amd import _lib, onnx_import, weights
from tests.helpers import scrfd_ref
from tests.helpers.onnx_write import write_iresnet_onnx
from tests.helpers.scrfd_onnx import CFG_10G, CFG_SMALL, lowpass_frames, write_scrfd_onnx

STYLES = [(True, False), (True, True), (False, False), (False, True)]          # (BN folded, dynamic shapes)


def n_convs(cfg):
    body = 3 + sum(2 * nb + (1 if (si > 0 or cfg["stem"][2] != w) else 0) for si, (nb, w) in enumerate(cfg["stages"]))
    return body + 3 + 3 + 2 + 2 + 3 * (cfg["head_convs"] + 3)          # laterals, fpn, downsample, pafpn, heads


@pytest.mark.parametrize("fold_bn,dynamic", STYLES)
@pytest.mark.parametrize("cfg", [CFG_SMALL, CFG_10G], ids=["small", "10g"])
def test_plan_matches_the_written_graph(tmp_path, cfg, fold_bn, dynamic):
    path = tmp_path / "det.onnx"
    names = write_scrfd_onnx(path, cfg, seed=3, fold_bn=fold_bn, dynamic=dynamic)
    for hw in ((640, 640), (96, 160)):
        plan = onnx_import.scrfd_plan_from_onnx(str(path), hw)
        assert plan.num_anchors == cfg["anchors"] and [lv["stride"] for lv in plan.levels] == [8, 16, 32]
        assert list(plan.outputs) == names
        assert [plan.outputs[t] for t in names] == [(li, k) for li in range(3) for k in ("score", "bbox", "kps")]
        convs = [s for s in plan.steps if s["op"] == "conv"]
        assert len(convs) == n_convs(cfg)
        assert [s["op"] for s in plan.steps if s["op"] != "conv"] == ["input", "pool"] + ["pool"] * 3 + ["upadd"] * 2
        assert sum(s["f32"] for s in convs) == 9 and not any(s["relu"] or s["res"] is not None for s in convs if s["f32"])
        # every block's second conv carries the identity and the ReLU; the PAFPN bottom-up convs a residual without ReLU
        assert sum(s["res"] is not None and s["relu"] for s in convs) == sum(nb for nb, _ in cfg["stages"])
        assert sum(s["res"] is not None and not s["relu"] for s in convs) == 2
        # heads shared across the strides: one packing key for the tower / cls / kps convs, the scaled bbox conv per stride
        assert len({s["wkey"] for s in convs}) == len(convs) - 2 * (cfg["head_convs"] + 2)
        for li, lv in enumerate(plan.levels):
            s = lv["stride"]
            for kind, k in (("score", 1), ("bbox", 4), ("kps", 10)):
                assert plan.shapes[lv[kind]] == (k * cfg["anchors"], hw[0] // s, hw[1] // s)
        assert plan.macs2 == sum(2 * plan.shapes[s["out"]][1] * plan.shapes[s["out"]][2] * s["w"].size for s in convs)


@pytest.mark.parametrize("fold_bn,dynamic", STYLES)
def test_folded_plan_is_the_raw_graph_in_float64(tmp_path, fold_bn, dynamic):
    path = tmp_path / "det.onnx"
    write_scrfd_onnx(path, CFG_SMALL, seed=4, fold_bn=fold_bn, dynamic=dynamic, score_bias=-1.0)
    frames = lowpass_frames(2, 64, 96, seed=1)
    plan = onnx_import.scrfd_plan_from_onnx(str(path), (64, 96))
    raw = scrfd_ref.r64_graph(str(path), frames)
    levels = scrfd_ref.run_plan(plan, frames)
    assert len(raw) == 9
    for t, (li, kind) in plan.outputs.items():
        want, have = raw[t], levels[li][kind]
        if kind == "score":
            have = 1.0 / (1.0 + np.exp(-have))
        assert np.abs(want.reshape(have.shape) - have).max() < 1e-12, (t, kind)


@pytest.mark.parametrize("mutate,match", [("prelu", r"node '\d+' \(PRelu\).*not supported"), ("group", r"node '\d+' \(Conv\): grouped conv"),
                                          ("resize3", r"node '\d+' \(Resize\).*x2"), ("nokps", "without keypoint outputs"),
                                          ("nosigmoid", "does not come out of a Sigmoid")])
def test_refusals_name_the_node(tmp_path, mutate, match):
    path = tmp_path / "bad.onnx"
    write_scrfd_onnx(path, CFG_SMALL, seed=5, mutate=mutate)
    with pytest.raises(ValueError, match=match):
        onnx_import.scrfd_plan_from_onnx(str(path), (64, 64))


def test_an_iresnet_is_not_a_detector_and_canvas_sides_are_checked(tmp_path):
    st = weights.synth_iresnet_state("r18", seed=3)
    path = tmp_path / "w600k_r18.onnx"
    write_iresnet_onnx(path, {k: v.numpy() for k, v in st.items()}, "r18", fold_bn=True)
    with pytest.raises(ValueError, match=r"\(PRelu\)"):
        onnx_import.scrfd_plan_from_onnx(str(path), (640, 640))
    det = tmp_path / "det.onnx"
    write_scrfd_onnx(det, CFG_SMALL, seed=5)
    with pytest.raises(ValueError, match="multiples of 32"):
        onnx_import.scrfd_plan_from_onnx(str(det), (640, 600))


def test_pack_with_a_scrfd_and_an_iresnet_loads_without_a_detector_warning(tmp_path, caplog):
    from facerecognition_infrenceengine_amd.face_analysis import FaceAnalysis
    d = tmp_path / "models" / "pack"
    d.mkdir(parents=True)
    write_scrfd_onnx(d / "det_10g.onnx", CFG_SMALL, seed=6)
    (d / "genderage.onnx").write_bytes(b"\x08")
    st = weights.synth_iresnet_state("r18", seed=3)
    write_iresnet_onnx(d / "w600k_r18.onnx", {k: v.numpy() for k, v in st.items()}, "r18", fold_bn=False)
    app = FaceAnalysis(name="pack", root=str(tmp_path))
    with warnings.catch_warnings(), caplog.at_level(logging.INFO):
        warnings.simplefilter("error")
        rec, det = app._load_states()
    assert det is None and app._scrfd_graph is not None and app.synthetic is False and app.arch == "r18"
    assert np.array_equal(rec["conv1.weight"].numpy(), st["conv1.weight"].numpy())
    assert any("genderage.onnx" in r.getMessage() for r in caplog.records)
    # a SCRFD file alone: a directory whose .onnx files hold no ArcFace IResNet is refused, as before - never synthetic
    # recognition weights behind a real detector
    (d / "w600k_r18.onnx").unlink()
    (d / "genderage.onnx").unlink()
    with pytest.raises(_lib.FrError, match="none of its .onnx files"):
        app._load_states()


def test_garbage_detector_file_still_means_synthetic_mtcnn(tmp_path):
    from facerecognition_infrenceengine_amd.face_analysis import FaceAnalysis
    d = tmp_path / "models" / "pack"
    d.mkdir(parents=True)
    (d / "det_10g.onnx").write_bytes(b"\x3a\x05\x0a\x03abc")
    st = weights.synth_iresnet_state("r18", seed=3)
    write_iresnet_onnx(d / "w600k_r18.onnx", {k: v.numpy() for k, v in st.items()}, "r18", fold_bn=False)
    app = FaceAnalysis(name="pack", root=str(tmp_path))
    with pytest.warns(UserWarning, match="MTCNN detector"):
        rec, det = app._load_states()
    assert app._scrfd_graph is None and app.synthetic and len(det) == 3


def test_new_entries_are_bound_and_the_abi_version_is_consistent():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "frhip.h")).read()
    lib = _lib.load()
    assert int(re.search(r"#define FR_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == lib.fr_version()
    for name in ("fr_det_conv_f16", "fr_det_conv_weight_halves", "fr_det_input_f16", "fr_det_pool_f16", "fr_det_upsample_add_f16",
                 "fr_scrfd_decode"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, text), name
    lib = _lib.load()
    import ctypes as C
    one = C.c_void_p(16)
    with pytest.raises(_lib.FrError, match="multiple of 8"):
        lib.fr_det_conv_f16(one, one, one, None, one, 1, 8, 8, 28, 32, 3, 1, 1, 8, 8, 32, 32, 1, 0, 0, None)
    with pytest.raises(_lib.FrError, match="does not follow"):
        lib.fr_det_conv_f16(one, one, one, None, one, 1, 8, 8, 32, 32, 3, 2, 1, 8, 8, 32, 32, 1, 0, 0, None)
    with pytest.raises(_lib.FrError, match="windows outside"):
        lib.fr_det_pool_f16(one, one, 1, 8, 8, 8, 6, 6, 0, 2, 2, 0, None)
    assert lib.fr_det_conv_weight_halves(8, 32, 3) == 3 * 32 * 32 and lib.fr_det_conv_weight_halves(88, 96, 1) == 3 * 96 * 32


def test_pack_conv_layout():
    """the packed element [s][co][q][j] is weight (co, tap, channel 8c + j) of group 4s + q = tap * (Cin / 8) + c"""
    from facerecognition_infrenceengine_amd.scrfd import pack_conv
    rng = np.random.default_rng(0)
    w = rng.standard_normal((28, 12, 3, 3))
    packed, bias, cin_p, cout_w = pack_conv(w, np.arange(28))
    assert (cin_p, cout_w) == (16, 32) and packed.shape == (5, 32, 4, 8) and packed.dtype == np.float16
    for g in range(20):
        tap, c = divmod(g, 2) if g < 18 else (None, None)
        for co in (0, 27, 28, 31):
            got = packed[g // 4, co, g % 4]
            want = np.zeros(8)
            if tap is not None and co < 28:
                ch = np.arange(8 * c, 8 * c + 8)
                want[ch < 12] = w[co, ch[ch < 12], tap // 3, tap % 3]
            assert np.array_equal(got, want.astype(np.float16)), (g, co)
    assert np.array_equal(bias[:28], np.arange(28)) and not bias[28:].any()
