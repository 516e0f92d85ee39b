"""What tests/test_gpu_torch_export.py and its CPU companion (tests/test_onnx_torch_export.py) share: the seeded modules of
tests/helpers/torch_nets.py that are exported, their inputs, and the measured error of the f16 emulation.

E_MBF      e = max |E16 - R64| over the embedding elements of the MobileFaceNet's crops (tests/helpers/mbf_ref.py on the plan
           imported from the torch-exported file: E16 is the CPU forward with weights and stored activations rounded to f16,
           R64 float64), measured on the CPU and rounded UP to two digits
COS_MBF    max over those crops of 1 - cos(E16, R64), rounded up the same way
E_DET      the same e per head kind (logit; distances and offsets in strides) for the two detectors on their 64 x 64 canvases

Regenerate with ``python -m tests.helpers.torch_cases`` from the repository root (prints the three dicts)."""
import math
import os
import tempfile

import numpy as np
import torch

IRESNET_SEED, IRESNET_INPUT_SEED = 5, 9
MBF_SEED, MBF_CROP_SEED, MBF_CROPS = 23, 12, 3
DET_SEED, DET_FRAME_SEED, DET_FRAMES, DET_HW = 17, 6, 2, (64, 64)
DET_BIAS = -0.5

E_MBF = 0.0012                       # measured 0.0011310
COS_MBF = 1.9e-07                    # measured 1.8215e-07
E_DET = {"plain": {"score": 0.00038, "bbox": 0.00011, "kps": 0.0002},          # measured 0.00037700, 0.00010947, 0.00019284
         "dw": {"score": 0.00037, "bbox": 0.00014, "kps": 0.00028}}            # measured 0.00036820, 0.00013633, 0.00027734


def iresnet18():
    from tests.helpers import torch_nets
    return torch_nets.seed_module(torch_nets.IResNet(torch_nets.IRESNET_BLOCKS["r18"]), IRESNET_SEED)


def iresnet_input(n=3):
    """float32 [n,3,112,112] in [-1, 1), every value an f16 number (the engine takes its crops as f16)"""
    x = torch.rand((n, 3, 112, 112), generator=torch.Generator().manual_seed(IRESNET_INPUT_SEED)) * 2 - 1
    return x.to(torch.float16).to(torch.float32)


def mobilefacenet():
    from tests.helpers import torch_nets
    return torch_nets.seed_module(torch_nets.MobileFaceNet(torch_nets.MBF_TINY), MBF_SEED)


def mbf_crops():
    from tests.helpers import mbf_ref
    return mbf_ref.seeded_crops(MBF_CROPS, seed=MBF_CROP_SEED)


def detector(depthwise):
    from tests.helpers import torch_nets
    return torch_nets.seed_module(torch_nets.SCRFDNet(depthwise=depthwise), DET_SEED + int(depthwise), score_bias=DET_BIAS)


def det_frames():
    from tests.helpers.scrfd_onnx import lowpass_frames
    return lowpass_frames(DET_FRAMES, DET_HW[0], DET_HW[1], seed=DET_FRAME_SEED)


def det_name(depthwise):
    return "dw" if depthwise else "plain"


def export_mbf(path):
    from tests.helpers.torch_export import export
    m = mobilefacenet()
    export(m, torch.zeros(1, 3, 112, 112), path, opset_version=11, input_names=["data"], output_names=["fc1"],
           dynamic_axes={"data": {0: "N"}, "fc1": {0: "N"}})
    return m


def export_detector(path, depthwise):
    from tests.helpers.torch_export import export
    m = detector(depthwise)
    export(m, torch.zeros(1, 3, 64, 64), path, opset_version=11, input_names=["input.1"],
           dynamic_axes={"input.1": {0: "N", 2: "H", 3: "W"}})
    return m


def cos_dist(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return 1.0 - (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


def measure_mbf(path):
    """-> (e, max 1 - cos) of the file at ``path`` (written by export_mbf) on mbf_crops()"""
    from facerecognition_infrenceengine_amd import onnx_import
    from tests.helpers import mbf_ref
    plan = onnx_import.recognition_plan_from_onnx(path)
    x = mbf_crops()
    r, h = mbf_ref.run_plan(plan, x, "r64"), mbf_ref.run_plan(plan, x, "e16")
    return float(np.abs(h - r).max()), float(cos_dist(h, r).max())


def measure_detector(path):
    """-> {kind: e} of the file at ``path`` (written by export_detector) on det_frames()"""
    from facerecognition_infrenceengine_amd import onnx_import
    from tests.helpers import mbf_ref
    plan = onnx_import.scrfd_plan_from_onnx(path, DET_HW)
    frames = det_frames()
    r, h = mbf_ref.run_scrfd_plan(plan, frames, "r64"), mbf_ref.run_scrfd_plan(plan, frames, "e16")
    return {k: max(float(np.abs(a[k] - b[k]).max()) for a, b in zip(h, r)) for k in ("score", "bbox", "kps")}


def round_up(v, digits=2):
    """v rounded up to ``digits`` significant digits"""
    q = 10.0 ** (math.floor(math.log10(v)) - digits + 1)
    return float(f"{math.ceil(v / q) * q:.{digits - 1}e}")


def measure():
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "mbf.onnx")
        export_mbf(p)
        e, cos = measure_mbf(p)
        print("measured: e", e, "1 - cos", cos)
        print("E_MBF =", round_up(e))
        print("COS_MBF =", round_up(cos))
        ed = {}
        for dw in (False, True):
            p = os.path.join(d, det_name(dw) + ".onnx")
            export_detector(p, dw)
            got = measure_detector(p)
            print("measured:", det_name(dw), got)
            ed[det_name(dw)] = {k: round_up(v) for k, v in got.items()}
        print("E_DET =", ed)


if __name__ == "__main__":
    measure()
