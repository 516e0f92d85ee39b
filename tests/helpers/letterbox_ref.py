"""CPU reference of the ``det_size`` path, composed from the oracle's own pieces (imported, not edited): the canvas is
``oracle.detect.resize_bilinear`` of the BGR bytes rounded as ``oracle.align.warp_affine_u8`` rounds, the cascade is
``oracle.detect.detect`` on the canvas, the way back is a float32 division, crops come from the ORIGINAL frame."""
import numpy as np
import torch

from facerecognition_infrenceengine_amd import weights
from facerecognition_infrenceengine_amd.letterbox import letterbox_geometry
from oracle import align as oalign, detect as odetect, nets as onets


def canvas_ref(frame, det_size):
    """uint8 [H,W,3] -> (canvas uint8 [dh,dw,3], det_scale float32): resized image top-left, zeros elsewhere."""
    dw, dh = det_size
    H, W = frame.shape[:2]
    nh, nw, det_scale = letterbox_geometry(H, W, det_size)
    v = odetect.resize_bilinear(frame.astype(np.float32), nh, nw)
    canvas = np.zeros((dh, dw, 3), np.uint8)
    canvas[:nh, :nw] = np.clip(np.floor(v.astype(np.float64) + 0.5), 0, 255).astype(np.uint8)
    return canvas, det_scale


def detect_ref(canvas, det_scale, cap_o=16):
    """The oracle cascade on a canvas -> (boxes, scores, kps on the canvas, boxes, kps in frame pixels)."""
    p, r, o = weights.synth_mtcnn_states()
    b, s, k = odetect.detect(canvas, p, r, o, cap_o=cap_o)
    b, k = np.asarray(b, np.float32), np.asarray(k, np.float32)
    return b, s, k, b / np.float32(det_scale), k / np.float32(det_scale)


def embed_ref(frame, kps_frame):
    """fp32 r100 embeddings of the faces whose landmarks (FRAME pixels) are given, crops taken from the original frame."""
    if len(kps_frame) == 0:
        return np.zeros((0, 512), np.float32)
    crops = [oalign.norm_crop(frame, kk)[0] for kk in kps_frame]
    x = torch.from_numpy(np.stack([oalign.crop_to_net(c) for c in crops]))
    return onets.iresnet_forward(weights.synth_iresnet_state("r100"), x, weights.IRESNET_LAYERS["r100"]).numpy()
