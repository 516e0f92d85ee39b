"""The CPU restatement of the SCRFD detector against itself (no GPU): the f16 emulation E16 stays within the error e that
tests/test_gpu_scrfd.py's tolerances are built on, and the reference leaves enough end-to-end frames clear."""
import numpy as np

from facerecognition_infrenceengine_amd import onnx_import
from tests.helpers import scrfd_ref as ref
from tests.helpers.scrfd_cases import BIAS_FEW, E, E2E_SCALES, FRAME_SEED, GRAPH_SEED
from tests.helpers.scrfd_onnx import CFG_10G, lowpass_frames, write_scrfd_onnx


def test_e16_error_is_within_the_recorded_e(tmp_path):
    """e = max |E16 - R64| per output kind over 16 frames is recorded in helpers/scrfd_cases.E (and DESIGN.md 4.3b); two of those
    frames cannot exceed it."""
    p = tmp_path / "det.onnx"
    write_scrfd_onnx(p, CFG_10G, seed=GRAPH_SEED, fold_bn=True, dynamic=True, score_bias=BIAS_FEW)
    plan = onnx_import.scrfd_plan_from_onnx(str(p), (640, 640))
    frames = lowpass_frames(16, 640, 640, seed=FRAME_SEED)[:2]
    r64, e16 = ref.run_plan(plan, frames), ref.run_plan(plan, frames, "e16")
    for kind in ("score", "bbox", "kps"):
        e = max(float(np.abs(a[kind] - b[kind]).max()) for a, b in zip(r64, e16))
        print(kind, e)
        assert 0.05 * E[kind] < e <= E[kind]


def test_reference_leaves_half_the_end_to_end_frames_clear(tmp_path):
    """the condition of test_gpu_scrfd.test_end_to_end_against_r64, checked where no GPU is needed: of its 16 frames the
    reference sets 8 aside and leaves 8 to be compared"""
    p = tmp_path / "det.onnx"
    write_scrfd_onnx(p, CFG_10G, seed=GRAPH_SEED, fold_bn=True, dynamic=True, score_bias=BIAS_FEW)
    frames = lowpass_frames(16, 640, 640, seed=FRAME_SEED)
    r64 = ref.run_plan(onnx_import.scrfd_plan_from_onnx(str(p), (640, 640)), frames)
    scales = E2E_SCALES(16)
    clear = [ref.reference_decides(r64, f, 2, (640, 640), 0.5, 0.4, scales[f], 1024, 16, 4 * E["score"])[0] for f in range(16)]
    print("clear frames:", sum(clear), clear)
    assert sum(clear) >= 8

