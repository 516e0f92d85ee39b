"""What the plan-recogniser GPU tests and their CPU companion share: seeds and the measured error of the f16 emulation.

E[net]     e = max |E16 - R64| over the embedding elements of the test's own crops (tests/helpers/mbf_ref.py: E16 is the CPU
           forward with weights and stored activations rounded to f16, R64 float64), measured on the CPU
COS[net]   max over those crops of 1 - cos(E16, R64)
E_DET      the same e per head kind for the depthwise SCRFD graph of tests/test_gpu_pack_s.py on its (64, 64) canvases

Regenerate with ``python -m tests.helpers.mbf_cases`` from the repository root (prints the three dicts)."""
import os
import tempfile

import numpy as np

GRAPH_SEED, CROP_SEED = 21, 8
NETS = {"1111": ("CFG_1111", 3), "full": ("CFG_FULL", 2)}        # net -> (config of mbf_onnx, crops)
DET_SEED, DET_FRAME_SEED, DET_FRAMES = 13, 4, 4
DET_BIAS = -0.225                                                # leaves a few anchors per 64 x 64 frame above 0.5 (measured below)

E = {"1111": 0.000945, "full": 0.001249}
COS = {"1111": 1.427e-07, "full": 2.199e-07}
E_DET = {"score": 0.000515, "bbox": 0.000222, "kps": 0.000358}


def write_net(path, net):
    from tests.helpers import mbf_onnx
    mbf_onnx.write_mbf_onnx(path, getattr(mbf_onnx, NETS[net][0]), seed=GRAPH_SEED, fold_bn=(net == "full"),
                            fc="gemm" if net == "full" else "matmul")


def crops_of(net):
    from tests.helpers import mbf_ref
    return mbf_ref.seeded_crops(NETS[net][1], seed=CROP_SEED)


def cos_dist(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return 1.0 - (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


def measure():
    from facerecognition_infrenceengine_amd import onnx_import
    from tests.helpers import mbf_onnx, mbf_ref
    from tests.helpers.scrfd_onnx import lowpass_frames
    e, cos = {}, {}
    with tempfile.TemporaryDirectory() as d:
        for net in NETS:
            p = os.path.join(d, net + ".onnx")
            write_net(p, net)
            plan = onnx_import.recognition_plan_from_onnx(p)
            x = crops_of(net)
            r, h = mbf_ref.run_plan(plan, x, "r64"), mbf_ref.run_plan(plan, x, "e16")
            e[net], cos[net] = float(np.abs(h - r).max()), float(cos_dist(h, r).max())
            print(net, "max |R64|", float(np.abs(r).max()), "norms", np.linalg.norm(r, axis=1))
        p = os.path.join(d, "det.onnx")
        mbf_onnx.write_dw_scrfd_onnx(p, seed=DET_SEED, score_bias=DET_BIAS)
        plan = onnx_import.scrfd_plan_from_onnx(p, (64, 64))
        frames = lowpass_frames(DET_FRAMES, 64, 64, seed=DET_FRAME_SEED)
        r, h = mbf_ref.run_scrfd_plan(plan, frames, "r64"), mbf_ref.run_scrfd_plan(plan, frames, "e16")
        ed = {k: max(float(np.abs(a[k] - b[k]).max()) for a, b in zip(h, r)) for k in ("score", "bbox", "kps")}
        print("anchors above 0.5 per frame:", [sum(int((lv["score"][f] >= 0).sum()) for lv in r) for f in range(DET_FRAMES)])
        print("closest logit to the threshold:", min(float(np.abs(lv["score"]).min()) for lv in r))
    print("E =", e)
    print("COS =", cos)
    print("E_DET =", ed)


if __name__ == "__main__":
    measure()
