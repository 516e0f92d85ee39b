"""Host emulation of the P-Net's coarse pass (csrc/pnet_fused.hip pnet23_body<true>): conv2 -> PReLU -> conv3 -> PReLU -> heads
from a conv1 map with every operand - map, weights, both activations - rounded to f16 and the sums kept in f32, beside the
float64 evaluation of the same f32 operands (tests/test_pnet_coarse_host.py, tests/test_gpu_pnet_coarse.py).

Layers are tests/helpers/detect_ref.py Layer objects (pnet_layers: 1 = conv2, 2 = conv3 with the heads)."""
import torch
import torch.nn.functional as F


def _tail(x1, L2, L3, q, dtype):
    """x1 NCHW [N, 10, H1, W1]; q rounds an operand; -> logit1 - logit0 [N, H1 - 4, W1 - 4]"""
    def prelu(y, s):
        return torch.where(y >= 0, y, y * s.to(dtype)[None, :, None, None])
    def t(w):
        return q(w.to(dtype))
    x2 = prelu(F.conv2d(q(x1.to(dtype)), t(L2.w), L2.b.to(dtype)), L2.slope)
    x3 = prelu(F.conv2d(q(x2), t(L3.w), L3.b.to(dtype)), L3.slope)
    hw, hb = L3.head
    a = F.conv2d(q(x3), t(hw[:2, :, None, None]), hb[:2].to(dtype))
    return a[:, 1] - a[:, 0]


def dl_f64(x1, L2, L3):
    """the float64 logit difference of the f32 operands"""
    return _tail(x1, L2, L3, lambda z: z, torch.float64)


def dl_hi_only(x1, L2, L3):
    """the coarse pass's: f16 operands, f32 sums"""
    return _tail(x1, L2, L3, lambda z: z.half().float(), torch.float32)
