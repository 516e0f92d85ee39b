"""What the SCRFD GPU tests and their CPU companions share: seeds, score biases and the measured error of the f16 emulation.

E: e = max |E16 - R64| per output kind in head units (logit; distances and offsets in strides), measured on the CPU over
the 16 frames of (GRAPH_SEED, FRAME_SEED) with the BIAS_FEW graph; tests/test_scrfd_reference.py re-measures a part."""
import numpy as np

E = {"score": 0.0170, "bbox": 0.0081, "kps": 0.0139}
GRAPH_SEED, FRAME_SEED = 11, 5
BIAS_MANY, BIAS_FEW = -7.5, -9.0          # a few tens of anchors above 0.5 per frame / a handful (end-to-end test: see its docstring)


def E2E_SCALES(n):
    return np.random.default_rng(2).uniform(0.3, 1.5, n).astype(np.float32)
