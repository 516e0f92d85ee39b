"""``det_size``: the detection canvas of insightface's ``FaceAnalysis.prepare(det_size=(dw, dh))``.

The reference calls ``prepare(ctx_id=0)`` (/root/reference/infrenceServer.py:416), which in insightface means a 640 x 640
canvas: the frame is resized to fit, placed top-left and zero padded, the detector runs on the canvas, boxes and landmarks
are divided by the scale, and alignment samples the ORIGINAL frame.  This module holds the one definition of that
geometry and the host side of the frame table the HIP kernels read (include/frhip.h ``fr_frame_ref``); the kernels are
csrc/letterbox.hip (canvas, unscale) and csrc/align.hip (warps over a frame table).  No GPU is needed to import it.
"""
import numpy as np


def letterbox_geometry(H, W, det_size):
    """Frame of H x W on a canvas ``det_size = (dw, dh)`` (insightface's order: width first) -> ``(nh, nw, det_scale)``:
    the frame is resized to nh x nw (aspect kept, one side filling the canvas) and detections on the canvas are divided
    by ``det_scale`` (float32).  Python doubles and ``int()`` truncation, as insightface computes it.  ValueError when a
    side would be 0."""
    dw, dh = (int(v) for v in det_size)
    H, W = int(H), int(W)
    if H <= 0 or W <= 0 or dw <= 0 or dh <= 0:
        raise ValueError(f"letterbox_geometry: frame {H} x {W} on canvas {dh} x {dw}")
    im_ratio, model_ratio = float(H) / W, float(dh) / dw
    if im_ratio > model_ratio:
        nh = dh
        nw = int(nh / im_ratio)
    else:
        nw = dw
        nh = int(nw * im_ratio)
    if nh <= 0 or nw <= 0:
        raise ValueError(f"letterbox_geometry: a {H} x {W} frame leaves no pixels on a {dh} x {dw} canvas ({nh} x {nw})")
    return nh, nw, np.float32(float(nh) / H)


def check_det_size(det_size):
    """``None`` or ``(dw, dh)`` of two positive ints (an int means a square canvas)."""
    if det_size is None:
        return None
    if isinstance(det_size, (int, np.integer)):
        det_size = (det_size, det_size)
    dw, dh = (int(v) for v in det_size)
    if dw <= 0 or dh <= 0:
        raise ValueError(f"det_size must be (width, height) of positive ints, got {det_size!r}")
    return dw, dh


def frame_table(pointers, shapes, det_size=None):
    """Host image of a device frame table: ``(uint8 array [N * 32], float32 det_scale [N])``.  ``pointers``: the frames'
    device addresses, ``shapes``: their (H, W).  Without ``det_size`` nh = nw = 0 and det_scale = 1 (a table for the
    warps alone)."""
    from ._lib import FrameRef
    n = len(pointers)
    refs = (FrameRef * n)()
    scale = np.ones(n, dtype=np.float32)
    for i, (p, (h, w)) in enumerate(zip(pointers, shapes)):
        if int(h) * int(w) * 3 >= 2 ** 31:
            raise ValueError(f"frame {i}: {h} x {w} is beyond 2 GiB")
        refs[i].data, refs[i].H, refs[i].W = int(p), int(h), int(w)
        if det_size is not None:
            refs[i].nh, refs[i].nw, scale[i] = letterbox_geometry(h, w, det_size)
    return np.frombuffer(bytes(memoryview(refs)), dtype=np.uint8).copy(), scale

