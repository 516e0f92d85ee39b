"""The three ONNX readers of onnx_import.py on files written by torch's own TorchScript exporter (no GPU).

Every other import test reads graphs written by tests/helpers/onnx_write.py - a writer made by the same hand, from the same
reading of onnx.proto, as the reader.  Here the writer is torch's C++ serialiser (tests/helpers/torch_export.py) and the
networks are plain nn.Modules written from the published architectures (tests/helpers/torch_nets.py); the imported network
is compared with the module itself.

  files that keep BatchNormalization as nodes (constant folding off, or training=PRESERVE): the IResNet state dict that comes
      back has exactly the module's state_dict() keys (less num_batches_tracked) and every array bit for bit
  every file: the imported network run in float64 (oracle.nets.iresnet_forward on the state dict; mbf_ref.run_plan /
      scrfd_ref.run_plan on a plan) against module.double() on the same seeded input:  max |got - ref| <= 1e-5 max |ref|.
      The exporter folds a BatchNorm into its conv in f32 - one rounding of 2^-24 per weight - and the readers add none:
      reference against reference that is 1e-7 of the output's scale, and 1e-5 leaves two orders of magnitude over it, far
      below what a structural slip gives (a missed bias, a wrong transB, eps or flatten order: the output's own scale)
  refusals that must stay, by message: BN epsilon 1e-3, a grouped conv that is not depthwise, align_corners bilinear
      upsampling, an IResNet whose Linear is not 25088 -> 512

Export styles are chosen pairwise (an orthogonal array over the two-valued axes, the opsets spread over its rows), every
value of every axis at least once.  Largest measured ratio max |got - ref| / max |ref| per net (this file prints each):
  IResNet-18 1.0e-07 (files with folded BatchNorms; 0 where they stay nodes)    IResNet-50 1.3e-07
  MobileFaceNet 7.5e-08 (folded; 4.9e-13 unfolded)                              detector 1.7e-07 (plain), 3.0e-07 (depthwise)
"""
import copy
import os
import re

import numpy as np
import pytest
import torch
from torch.onnx import TrainingMode

from facerecognition_infrenceengine_amd import onnx_import
from oracle import nets
from tests.helpers import mbf_ref, scrfd_ref
from tests.helpers import torch_cases as cases
from tests.helpers import torch_nets as tn
from tests.helpers.scrfd_onnx import lowpass_frames
from tests.helpers.torch_export import export

REL = 1e-5


def ratio(got, ref, what):
    r = float(np.abs(np.asarray(got) - np.asarray(ref)).max() / np.abs(ref).max())
    print(f"{what}: max |got - ref| / max |ref| = {r:.3e} (max |ref| = {float(np.abs(ref).max()):.4g})")
    return r


# ------------------------------------------------------------------------------------------------ the helper itself
def test_export_restores_the_exporter_and_raises_on_failure(tmp_path):
    from torch.onnx._internal.torchscript_exporter import onnx_proto_utils as mod

    class Broken(torch.nn.Module):
        def forward(self, x):
            raise RuntimeError("no graph from this module")

    before = mod._add_onnxscript_fn
    with pytest.raises(RuntimeError, match="no graph from this module"):
        export(Broken(), torch.zeros(1, 3), tmp_path / "broken.onnx")
    assert mod._add_onnxscript_fn is before
    path = export(torch.nn.Conv2d(3, 4, 3), torch.zeros(1, 3, 8, 8), tmp_path / "conv.onnx", opset_version=11)
    assert mod._add_onnxscript_fn is before
    g = onnx_import.read_onnx(path)
    assert [n.op for n in g.nodes] == ["Conv"] and len(g.inputs) == 1 and len(g.outputs) == 1
    assert sorted(a.shape for a in g.initializers.values()) == [(4,), (4, 3, 3, 3)]
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "torch_export.py")).read()
    imported = re.findall(r"^\s*(?:import|from)\s+([\w.]+)", src, flags=re.M)
    assert "torch" in imported and not [m for m in imported if m.split(".")[0] in ("onnx", "onnxruntime", "onnxscript")]
    assert "dynamo=False" in src


# ------------------------------------------------------------------------------------------------ IResNet
# (fold, opset, dynamic batch, flatten, keep_initializers_as_inputs, head, training=PRESERVE, seeded slopes)
IRESNET_STYLES = {
    "default":   (True, 17, False, "flatten", False, "linear", False, True),
    "oa1":       (True, 11, False, "view", False, "matmul", True, False),
    "oa2":       (True, 13, True, "flatten", True, "linear", True, False),
    "oa3":       (True, 9, True, "view", True, "matmul", False, True),
    "oa4":       (False, 9, False, "flatten", True, "matmul", False, False),
    "oa5":       (False, 13, False, "view", True, "linear", True, True),
    "oa6":       (False, 11, True, "flatten", False, "matmul", True, True),
    "oa7":       (False, 17, True, "view", False, "linear", False, False),
    "unfolded":  (False, 11, False, "flatten", False, "linear", False, True),     # the PReLU slope behind an Unsqueeze
    "gemm_nt":   (True, 13, False, "flatten", False, "addmm_t", False, True),     # a Gemm with transB = 0
}
IRESNET_CASES = [("r18", s) for s in IRESNET_STYLES] + [("r50", "default"), ("r50", "unfolded")]


def test_the_iresnet_styles_cover_every_value_of_every_axis():
    rows = list(IRESNET_STYLES.values())
    for axis, values in enumerate([(True, False), (9, 11, 13, 17), (True, False), ("flatten", "view"), (True, False),
                                   ("linear", "matmul"), (True, False), (True, False)]):
        assert set(values) <= {r[axis] for r in rows}, axis
    two = {0: (True, False), 2: (True, False), 3: ("flatten", "view"), 4: (True, False), 5: ("linear", "matmul"), 6: (True, False),
           7: (True, False)}
    for a in two:                                                         # the two-valued axes: every pair of values of every two
        for b in two:
            if a < b:
                assert {(x, y) for x in two[a] for y in two[b]} <= {(r[a], r[b]) for r in rows}, (a, b)


@pytest.fixture(scope="module")
def iresnet_modules():
    """arch -> {seeded slopes: (module, x float64 [2,3,112,112], module.double()(x))}: built once, never changed but for the
    ``flatten`` / ``head`` spelling of the forward (the function is the same)"""
    out = {}
    for arch in ("r18", "r50"):
        out[arch] = {}
        for seeded in ((True, False) if arch == "r18" else (True,)):
            m = tn.seed_module(tn.IResNet(tn.IRESNET_BLOCKS[arch]), 3 + int(seeded), prelu=seeded)
            x = torch.rand((2, 3, 112, 112), generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 2 - 1
            with torch.no_grad():
                ref = copy.deepcopy(m).double()(x).numpy()
            out[arch][seeded] = (m, x, ref)
    return out


@pytest.fixture(scope="module", params=IRESNET_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def iresnet_file(request, iresnet_modules, tmp_path_factory):
    """one export per style; the file (96 MB for r18, 174 MB for r50) is removed when the style's tests are through"""
    arch, style = request.param
    fold, opset, dyn, flatten, kiai, head, preserve, seeded = IRESNET_STYLES[style]
    m, x, ref = iresnet_modules[arch][seeded]
    m.flatten, m.head = flatten, head
    if head == "addmm_t":
        tn.use_transposed_head(m)
    path = tmp_path_factory.mktemp("iresnet") / f"{arch}_{style}.onnx"
    kw = dict(opset_version=opset, do_constant_folding=fold, keep_initializers_as_inputs=kiai, input_names=["data"], output_names=["fc1"])
    if dyn:
        kw["dynamic_axes"] = {"data": {0: "N"}, "fc1": {0: "N"}}
    if preserve:
        kw["training"] = TrainingMode.PRESERVE
    export(m, torch.zeros(1, 3, 112, 112), path, **kw)
    yield arch, style, str(path), m, x, ref
    m.flatten, m.head = "flatten", "linear"
    os.unlink(path)


def test_iresnet_file_imports_as_the_module(iresnet_file):
    arch, style, path, m, x, ref = iresnet_file
    fold, opset, dyn, flatten, kiai, head, preserve, seeded = IRESNET_STYLES[style]
    g = onnx_import.read_onnx(path)
    ops = {n.op for n in g.nodes}
    bn_nodes = sum(n.op == "BatchNormalization" for n in g.nodes)
    blocks = sum(tn.IRESNET_BLOCKS[arch])
    kept = not fold or preserve                                           # BatchNormalization stays a node behind every conv
    assert bn_nodes == (3 * blocks + 4 + 3 if kept else blocks + 2)        # folded: each block's bn1, the head's bn2, the BatchNorm1d
    # what the styles are there for: a slope behind an Unsqueeze, equal slopes sharing one initialiser through Identity nodes
    # (the exporter shares only where initialisers are not graph inputs too), a Gemm that does not transpose its weight
    made = {t: n.op for n in g.nodes for t in n.outputs}
    slopes = [made.get(n.inputs[1]) for n in g.nodes if n.op == "PRelu"]
    assert len(slopes) == blocks + 1 and (set(slopes) == {"Unsqueeze"}) == (not fold)
    assert ("Identity" in ops) == (not seeded and not kiai)
    assert [n.attrs.get("transB", 0) for n in g.nodes if n.op == "Gemm"] == {"linear": [1], "addmm_t": [0]}.get(head, [])
    assert g.inputs == ["data"]
    st, got_arch = onnx_import.iresnet_state_from_onnx(g)
    assert got_arch == arch
    want = {k: v for k, v in m.state_dict().items() if not k.endswith("num_batches_tracked")}
    if kept:
        assert set(st) == set(want)
        for k, v in want.items():
            assert st[k].dtype == np.float32 and st[k].shape == tuple(v.shape) and np.array_equal(st[k], v.numpy()), k
    else:
        folded = {k for k in want if k.split(".")[-2] in ("bn2", "bn3", "1") and k.startswith("layer")} | {k for k in want if k.startswith("bn1.")}
        convs = {k[:-len("weight")] + "bias" for k in want if k.endswith("weight") and want[k].dim() == 4}
        assert set(st) == (set(want) - folded) | convs
    got = nets.iresnet_forward({k: torch.from_numpy(v).double() for k, v in st.items()}, x, list(tn.IRESNET_BLOCKS[arch])).numpy()
    r = ratio(got, ref, f"{arch} {style}")
    assert got.shape == ref.shape == (2, 512) and r <= REL


# ------------------------------------------------------------------------------------------------ MobileFaceNet
MBF_STYLES = {"fold-11-fixed": (True, 11, False, "linear"), "fold-13-dyn": (True, 13, True, "linear"),
              "nofold-13-fixed": (False, 13, False, "linear"), "nofold-11-dyn": (False, 11, True, "linear"),
              "gemm_nt": (True, 13, False, "addmm_t")}


@pytest.fixture(scope="module")
def mbf_module():
    m = tn.seed_module(tn.MobileFaceNet(tn.MBF_TINY), 11)
    crops = mbf_ref.seeded_crops(2, seed=3)
    with torch.no_grad():
        ref = copy.deepcopy(m).double()(mbf_ref.blob(crops)).numpy()
    return m, crops, ref


@pytest.mark.parametrize("style", list(MBF_STYLES))
def test_recognition_plan_is_the_module(tmp_path, mbf_module, style):
    fold, opset, dyn, head = MBF_STYLES[style]
    m, crops, ref = mbf_module
    if head == "addmm_t":
        tn.use_transposed_head(m)
    kw = dict(dynamic_axes={"data": {0: "N"}, "fc1": {0: "N"}}) if dyn else {}
    try:
        path = export(m, torch.zeros(1, 3, 112, 112), tmp_path / "mbf.onnx", opset_version=opset, do_constant_folding=fold,
                      input_names=["data"], output_names=["fc1"], **kw)
    finally:
        m.head = "linear"
    g = onnx_import.read_onnx(path)
    made = {t: n.op for n in g.nodes for t in n.outputs}
    assert ({made.get(n.inputs[1]) for n in g.nodes if n.op == "PRelu"} == {"Unsqueeze"}) == (not fold)
    if head == "addmm_t":
        assert [n.attrs.get("transB", 0) for n in g.nodes if n.op == "Gemm"] == [0]
    plan = onnx_import.recognition_plan_from_onnx(g)
    layers = tn.layer_list(m)
    steps = plan.steps[1:]
    assert plan.steps[0]["op"] == "input" and len(steps) == len(layers) and plan.dim == 512 and plan.output == steps[-1]["out"]
    for s, (kind, cout, cin, k, stride, pad, prelu, res) in zip(steps, layers):
        assert (s["op"], s["w"].shape, s["stride"], s["pad"]) == (kind, (cout, cin, k, k), stride, pad)
        assert (s["act"] == 2) == prelu and s["act"] in (0, 2) and (s["res"] is not None) == res
        assert (s["slope"] is not None and s["slope"].shape == (cout,)) == prelu and s["b"].shape == (cout,)
    assert [s["f32"] for s in steps] == [False] * (len(steps) - 1) + [True]
    sizes = [plan.shapes[s["out"]][1:] for s in steps]
    assert sizes[0] == (56, 56) and sizes[-3:] == [(7, 7), (1, 1), (1, 1)]
    got = mbf_ref.run_plan(plan, crops, "r64")
    r = ratio(got, ref, f"mobilefacenet {style}")
    assert got.shape == ref.shape == (2, 512) and r <= REL


def test_recorded_e_of_the_gpu_cases_is_what_the_cpu_computes(tmp_path):
    """tests/helpers/torch_cases.py records e = max |E16 - R64| for the nets tests/test_gpu_torch_export.py runs, rounded up to
    two digits.  E16's float32 sums follow the host's summation order, which moves e by a fraction of a percent: 10 % either
    way is held."""
    p = str(tmp_path / "mbf.onnx")
    cases.export_mbf(p)
    e, cos = cases.measure_mbf(p)
    print(f"mobilefacenet: e = {e:.6g} (recorded {cases.E_MBF}), 1 - cos = {cos:.4g} (recorded {cases.COS_MBF})")
    assert abs(e - cases.E_MBF) <= 0.1 * cases.E_MBF and abs(cos - cases.COS_MBF) <= 0.1 * cases.COS_MBF
    for dw in (False, True):
        p = str(tmp_path / f"det_{cases.det_name(dw)}.onnx")
        cases.export_detector(p, dw)
        got = cases.measure_detector(p)
        print(f"detector {cases.det_name(dw)}: e = {got} (recorded {cases.E_DET[cases.det_name(dw)]})")
        for kind, v in got.items():
            rec = cases.E_DET[cases.det_name(dw)][kind]
            assert abs(v - rec) <= 0.1 * rec, (dw, kind)


# ------------------------------------------------------------------------------------------------ detector
# an orthogonal array over (depthwise, interpolate spelling, dynamic H / W, opset, fold, canvas)
DET_STYLES = [(False, "scale", False, 11, True, (64, 64)), (False, "scale", True, 11, False, (64, 96)),
              (False, "size", False, 13, True, (64, 96)), (False, "size", True, 13, False, (64, 64)),
              (True, "scale", False, 13, False, (64, 64)), (True, "scale", True, 13, True, (64, 96)),
              (True, "size", False, 11, False, (64, 96)), (True, "size", True, 11, True, (64, 64))]


def test_the_detector_styles_cover_every_pair_of_values():
    for a in range(6):
        for b in range(a + 1, 6):
            assert len({(r[a], r[b]) for r in DET_STYLES}) == 4, (a, b)


@pytest.mark.parametrize("style", DET_STYLES, ids=lambda s: f"{'dw' if s[0] else 'plain'}-{s[1]}-{'dyn' if s[2] else 'fixed'}-{s[3]}-"
                                                            f"{'fold' if s[4] else 'nofold'}-{s[5][0]}x{s[5][1]}")
def test_detector_plan_is_the_module(tmp_path, style):
    dw, up, dyn, opset, fold, hw = style
    m = tn.seed_module(tn.SCRFDNet(depthwise=dw, upsample=up), 31 + int(dw), score_bias=-1.0)
    frames = lowpass_frames(2, hw[0], hw[1], seed=1)
    with torch.no_grad():
        ref = [t.numpy() for t in copy.deepcopy(m).double()(scrfd_ref.blob(frames))]
    kw = dict(dynamic_axes={"input.1": {0: "N", 2: "H", 3: "W"}}) if dyn else {}
    # a file with fixed H and W serves the canvas it was exported at; a dynamic one is exported at 64 x 64 whatever the canvas
    example = torch.zeros((1, 3, 64, 64) if dyn else (1, 3) + hw)
    path = export(m, example, tmp_path / "det.onnx", opset_version=opset, do_constant_folding=fold, input_names=["input.1"], **kw)
    g = onnx_import.read_onnx(path)
    assert len(g.outputs) == 9 and ("BatchNormalization" in {n.op for n in g.nodes}) == (not fold)
    plan = onnx_import.scrfd_plan_from_onnx(g, hw)
    assert plan.num_anchors == m.anchors == 2 and [lv["stride"] for lv in plan.levels] == [8, 16, 32] and plan.canvas_hw == hw
    assert list(plan.outputs) == g.outputs and [plan.outputs[t] for t in g.outputs] == tn.OUTPUT_ORDER
    n_dw = sum(s["op"] == "dwconv" for s in plan.steps)
    assert n_dw == (sum(c.groups > 1 for c in m.modules() if isinstance(c, torch.nn.Conv2d)) if dw else 0)
    assert sum(s["op"] in ("conv", "dwconv") for s in plan.steps) == sum(isinstance(c, torch.nn.Conv2d) for c in m.modules())
    assert [(s["op"], s["up"]) for s in plan.steps if s["op"] == "upadd"] == [("upadd", 2)] * 2
    levels = mbf_ref.run_scrfd_plan(plan, frames)
    worst = 0.0
    for t, want in zip(g.outputs, ref):
        li, kind = plan.outputs[t]
        have = levels[li][kind]
        if kind == "score":
            have = 1.0 / (1.0 + np.exp(-have))
        s = hw[0] // plan.levels[li]["stride"] * (hw[1] // plan.levels[li]["stride"]) * 2
        assert want.shape == (2, s, {"score": 1, "bbox": 4, "kps": 10}[kind])
        r = float(np.abs(have.reshape(want.shape) - want).max() / np.abs(want).max())
        worst = max(worst, r)
        assert r <= REL, (t, li, kind, r)
    print(f"detector {style}: largest max |got - ref| / max |ref| over the nine outputs = {worst:.3e}")


# ------------------------------------------------------------------------------------------------ refusals that must stay
def test_bn_epsilon_other_than_1e5_is_refused(tmp_path):
    m = tn.seed_module(tn.IResNet(tn.IRESNET_BLOCKS["r18"], eps=1e-3), 1)
    path = export(m, torch.zeros(1, 3, 112, 112), tmp_path / "eps.onnx", opset_version=11, do_constant_folding=False)
    with pytest.raises(ValueError, match=r"^bn1: BatchNormalization epsilon 0\.001"):
        onnx_import.iresnet_state_from_onnx(path)
    path = export(m, torch.zeros(1, 3, 112, 112), tmp_path / "eps.onnx", opset_version=11)
    with pytest.raises(ValueError, match=r"^layer1\.0\.bn1: BatchNormalization epsilon 0\.001"):       # the one BN no exporter can fold
        onnx_import.iresnet_state_from_onnx(path)


def test_an_iresnet_with_another_embedding_width_is_refused(tmp_path):
    m = tn.seed_module(tn.IResNet(tn.IRESNET_BLOCKS["r18"], features=256), 1)
    path = export(m, torch.zeros(1, 3, 112, 112), tmp_path / "fc256.onnx", opset_version=11)
    with pytest.raises(ValueError, match=r"fc weight \(256, 25088\), expected \(512, 25088\)"):
        onnx_import.iresnet_state_from_onnx(path)


def test_a_grouped_conv_that_is_not_depthwise_is_refused(tmp_path):
    m = tn.seed_module(tn.MobileFaceNet(tn.MBF_TINY, odd_groups=2), 1)
    path = export(m, torch.zeros(1, 3, 112, 112), tmp_path / "mbf.onnx", opset_version=11)
    with pytest.raises(ValueError, match=r"node '[^']*Conv[^']*' \(Conv\): grouped conv \(group 2 on 24 channels, weight \(24, 12, 3, 3\)\) is not depthwise"):
        onnx_import.recognition_plan_from_onnx(path)
    d = tn.seed_module(tn.SCRFDNet(depthwise=True, odd_groups=2), 1)
    path = export(d, torch.zeros(1, 3, 64, 64), tmp_path / "det.onnx", opset_version=11)
    with pytest.raises(ValueError, match=r"node '[^']*Conv[^']*' \(Conv\): grouped conv \(group 2\) is not supported"):
        onnx_import.scrfd_plan_from_onnx(path, (64, 64))


def test_align_corners_bilinear_upsampling_is_refused(tmp_path):
    d = tn.seed_module(tn.SCRFDNet(upsample="bilinear"), 1)
    path = export(d, torch.zeros(1, 3, 64, 64), tmp_path / "det.onnx", opset_version=11)
    with pytest.raises(ValueError, match=r"node '[^']*Resize[^']*' \(Resize\): resize mode linear / align_corners"):
        onnx_import.scrfd_plan_from_onnx(path, (64, 64))


# ------------------------------------------------------------------------------------------------ a pack
def test_a_torch_exported_pack_loads_without_any_warning(tmp_path):
    import warnings
    from facerecognition_infrenceengine_amd.face_analysis import FaceAnalysis
    d = tmp_path / "models" / "exported"
    d.mkdir(parents=True)
    cases.export_detector(str(d / "det_500m.onnx"), True)
    cases.export_mbf(str(d / "w600k_mbf.onnx"))
    app = FaceAnalysis(name="exported", root=str(tmp_path))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rec, det = app._load_states()
    assert det is None and app._scrfd_graph is not None and app.synthetic is False and app.arch == "mbf"
    assert isinstance(rec, onnx_import.RecognitionPlan) and rec.dim == 512
