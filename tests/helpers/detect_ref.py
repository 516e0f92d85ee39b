"""Float64 references of the MTCNN layers, one kernel layer at a time (tests/test_gpu_detect_precision.py).

A layer here is what one HIP kernel layer id computes: conv (or dense), bias, PReLU, ceil-mode max pool, head, in the order
oracle/nets.py applies them.  Every function takes and returns float64 NCHW tensors that hold the kernel's f32 inputs, and
returns beside each output the magnitude A that bounds the f32 rounding error: |y - y64| <= c * A, with A = sum |w * x| + |b|
for a conv output, carried through PReLU (|slope| where it applies) and pool (the largest A of the window).

``split=True`` evaluates the split-precision arithmetic the batch-path kernels state: every f32 operand x = hi + lo with
hi = f16(x), lo = f16(x - hi), a product as wh*xh + wh*xl + wl*xh (lo*lo dropped), summed exactly here."""
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from oracle import nets as onets

D = torch.float64


def split_f16(x):
    """f32 tensor -> (hi, lo) as float64 values of the two f16 halves"""
    x = x.float()
    hi = x.half()
    lo = (x - hi.float()).half()
    return hi.double(), lo.double()


@dataclass
class Layer:
    w: torch.Tensor                    # float64 [cout, cin, kh, kw] (conv) or [cout, cin*k*k] (dense over the (w, h, c) flatten)
    b: torch.Tensor
    slope: torch.Tensor = None         # PReLU slopes or None
    pool: int = 0                      # ceil-mode max pool k x k / s2 after the PReLU
    head: tuple = None                 # (w [nh, cout], b [nh]): 1x1 head after the PReLU (P-Net conv3)

    def scaled(self, sw, sb, shw=1.0):
        """weights x sw, bias x sb, head weights x shw (powers of two: exact)"""
        h = None if self.head is None else (self.head[0] * shw, self.head[1])
        return Layer(self.w * sw, self.b * sb, self.slope, self.pool, h)


def _t(st, k):
    return st[k].detach().double().cpu()


def pnet_layers(p):
    hw = torch.cat([_t(p, "conv4_1.weight").reshape(2, -1), _t(p, "conv4_2.weight").reshape(4, -1)])
    hb = torch.cat([_t(p, "conv4_1.bias"), _t(p, "conv4_2.bias")])
    return {0: Layer(_t(p, "conv1.weight"), _t(p, "conv1.bias"), _t(p, "prelu1.weight"), 2),
            1: Layer(_t(p, "conv2.weight"), _t(p, "conv2.bias"), _t(p, "prelu2.weight")),
            2: Layer(_t(p, "conv3.weight"), _t(p, "conv3.bias"), _t(p, "prelu3.weight"), head=(hw, hb))}


def rnet_layers(r):
    return {10: Layer(_t(r, "conv1.weight"), _t(r, "conv1.bias"), _t(r, "prelu1.weight"), 3),
            11: Layer(_t(r, "conv2.weight"), _t(r, "conv2.bias"), _t(r, "prelu2.weight"), 3),
            12: Layer(_t(r, "conv3.weight"), _t(r, "conv3.bias"), _t(r, "prelu3.weight")),
            13: Layer(_t(r, "dense4.weight"), _t(r, "dense4.bias"), _t(r, "prelu4.weight")),
            14: Layer(torch.cat([_t(r, "dense5_1.weight"), _t(r, "dense5_2.weight")]),
                      torch.cat([_t(r, "dense5_1.bias"), _t(r, "dense5_2.bias")]))}


def onet_layers(o):
    return {20: Layer(_t(o, "conv1.weight"), _t(o, "conv1.bias"), _t(o, "prelu1.weight"), 3),
            21: Layer(_t(o, "conv2.weight"), _t(o, "conv2.bias"), _t(o, "prelu2.weight"), 3),
            22: Layer(_t(o, "conv3.weight"), _t(o, "conv3.bias"), _t(o, "prelu3.weight"), 2),
            23: Layer(_t(o, "conv4.weight"), _t(o, "conv4.bias"), _t(o, "prelu4.weight")),
            24: Layer(_t(o, "dense5.weight"), _t(o, "dense5.bias"), _t(o, "prelu5.weight")),
            25: Layer(torch.cat([_t(o, k + ".weight") for k in ("dense6_1", "dense6_2", "dense6_3")]),
                      torch.cat([_t(o, k + ".bias") for k in ("dense6_1", "dense6_2", "dense6_3")]))}


def _lin(x, w):
    """conv for 4-d weights, else the MTCNN dense layer over the (w, h, c) flatten; output NCHW"""
    if w.dim() == 4:
        return F.conv2d(x, w)
    return F.linear(onets._flatten_whc(x), w)[:, :, None, None]


def _prod(x, w, split):
    if not split:
        return _lin(x, w)
    xh, xl = split_f16(x)
    wh, wl = split_f16(w)
    return _lin(xh, wh) + _lin(xl, wh) + _lin(xh, wl)


def _prelu(y, A, s, c):
    """PReLU of y and its bound: A x |slope| where the slope applies, A x max(1, |slope|) where y is too close to 0 for
    its sign to be certain"""
    s4 = s[None, :, None, None]
    unsure = y.abs() <= c * A
    sa = s4.abs()
    A = torch.where(unsure, A * torch.clamp(sa, min=1.0), torch.where(y > 0, A, A * sa))
    return torch.where(y > 0, y, y * s4), A


def apply(layer, x, c, split=False, carry=None):
    """(y, A) of one kernel layer.  carry: the bound of x's own error, in units of c (a previous layer's A)."""
    y = _prod(x, layer.w, split) + layer.b[None, :, None, None]
    A = _lin(x.abs(), layer.w.abs()) + layer.b.abs()[None, :, None, None]
    if carry is not None:
        A = A + _lin(carry, layer.w.abs())
    if layer.slope is not None:
        y, A = _prelu(y, A, layer.slope, c)
    if layer.pool:
        y = F.max_pool2d(y, layer.pool, 2, ceil_mode=True)
        A = F.max_pool2d(A, layer.pool, 2, ceil_mode=True)
    if layer.head is not None:
        hw, hb = layer.head
        hw4 = hw[:, :, None, None]
        act = y
        y = _prod(act, hw4, split) + hb[None, :, None, None]
        A = F.conv2d((split_carry(act, A, c) if split else A) + act.abs(), hw4.abs()) + hb.abs()[None, :, None, None]
    return y, A


def forward(layers, ids, x):
    """the exact float64 layers `ids` in order from x; the last one's output (NCHW)"""
    for i in ids:
        x, _ = apply(layers[i], x, 0.0)
    return x


def split_carry(y, A, c):
    """what the next split layer sees of a split-layer output y (bound c * A): the kernel splits ITS f32 value, the
    reference splits f32(y).  Split representation error max(2^-22 |y|, 2^-25) on both sides, plus the f32 rounding:
    the carry in units of c."""
    return A + (3.0 * y.abs() + 2.0 ** -23 / c)


def ratio(got, want, A):
    """worst |got - want| / A (inf where A == 0 but the values differ)"""
    err = (got.double() - want).abs()
    r = torch.where(A > 0, err / torch.where(A > 0, A, torch.ones_like(A)), torch.where(err > 0, torch.full_like(err, float("inf")), err))
    return float(r.max()) if r.numel() else 0.0
