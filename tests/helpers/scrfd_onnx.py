"""Test helper: seeded SCRFD detector graphs as ONNX files, written with the protobuf writers of onnx_write.py.

The architecture is the public one of insightface's SCRFD-10GF with keypoints (ResNetV1e-style deep stem and BasicBlock
stages, PAFPN, three conv heads whose weights are shared across the strides, 2 anchors per cell); a narrow variant with a
few blocks serves the fast tests.  Export styles: BatchNormalization kept as nodes or folded into the convs; the FPN Resize
by a static ``scales`` input or by ``sizes`` computed with a Shape -> Gather / Slice -> ... -> Concat chain (then the head
Reshape targets are computed the same way)."""
import numpy as np

from tests.helpers import onnx_write as ow

CFG_10G = dict(stem=(28, 28, 56), stages=((3, 56), (4, 88), (2, 88), (3, 224)), fpn=56, head=80, head_convs=3, anchors=2)
CFG_SMALL = dict(stem=(8, 8, 16), stages=((1, 16), (2, 24), (1, 24), (1, 40)), fpn=16, head=24, head_convs=2, anchors=2)
EPS = 1e-5


def _tensor_i64(name, a):
    a = np.asarray(a, dtype=np.int64)                    # (a 0-d array stays 0-d: scalars as exporters write them)
    return b"".join(ow._vi(1, d) for d in a.shape) + ow._vi(2, 7) + ow._ld(8, name.encode()) + ow._ld(9, a.tobytes())


def _scalar_f32(name, v):
    return ow._vi(2, 1) + ow._ld(8, name.encode()) + ow._ld(9, np.float32(v).tobytes())


def _attr_str(name, v):
    return ow._ld(1, name.encode()) + ow._ld(4, v.encode()) + ow._vi(20, 3)


def _attr_tensor(name, t):
    return ow._ld(1, name.encode()) + ow._ld(5, t) + ow._vi(20, 4)


class _W(ow._Writer):
    def init_i64(self, a):
        nm = self.name()
        self.inits.append(_tensor_i64(nm, a))
        return nm

    def init_scalar(self, v):
        nm = self.name()
        self.inits.append(_scalar_f32(nm, v))
        return nm

    def const_i64(self, a):
        """an int64 constant as a Constant NODE (exporters emit both forms)"""
        return self.node("Constant", [], [_attr_tensor("value", _tensor_i64("", a))])


def write_scrfd_onnx(path, cfg=CFG_10G, seed=0, fold_bn=True, dynamic=False, score_bias=-4.0, mutate=None):
    """Writes the graph; returns the list of the nine output names in graph order (per stride: score, bbox, kps).
    ``mutate``: None, or one of 'prelu', 'group', 'resize3', 'nokps', 'nosigmoid' - a defect for the refusal tests."""
    rng = np.random.default_rng(seed)
    w = _W()
    shared = {}

    def conv(x, cin, cout, k, stride=1, bn=True, relu=True, gain=1.0, bias=None, key=None, group=1):
        """conv [+ BN] [+ relu]; ``key``: initialisers shared by every call with that key (the heads)"""
        if key is not None and key in shared:
            ini = shared[key]
        else:
            wt = rng.standard_normal((cout, cin // group, k, k)) * gain * np.sqrt(2.0 / (cin * k * k))
            ini = {"w": wt}
            if bn:
                ini["bn"] = [rng.uniform(0.8, 1.2, cout), rng.standard_normal(cout) * 0.1, rng.standard_normal(cout) * 0.1,
                             rng.uniform(0.8, 1.2, cout)]
                if fold_bn:
                    s = ini["bn"][0] / np.sqrt(ini["bn"][3] + EPS)
                    ini["names"] = [w.init(wt * s[:, None, None, None]), w.init(ini["bn"][1] - ini["bn"][2] * s)]
                else:
                    ini["names"] = [w.init(wt)]
                    ini["bn_names"] = [w.init(a) for a in ini["bn"]]
            else:
                b = rng.standard_normal(cout) * 0.05 if bias is None else np.broadcast_to(np.asarray(bias, dtype=np.float64), (cout,))
                ini["names"] = [w.init(wt), w.init(b)]
            if key is not None:
                shared[key] = ini
        attrs = [ow._attr_ints("kernel_shape", [k, k]), ow._attr_ints("strides", [stride, stride]),
                 ow._attr_ints("pads", [k // 2] * 4), ow._attr_ints("dilations", [1, 1]), ow._attr_int("group", group)]
        x = w.node("Conv", [x] + ini["names"], attrs)
        if bn and not fold_bn:
            x = w.node("BatchNormalization", [x] + ini["bn_names"], [ow._attr_float("epsilon", EPS)])
        return w.node("Relu", [x]) if relu else x

    def resize(x, like):
        if mutate == "resize3":
            return w.node("Resize", [x, "", w.init(np.array([1.0, 1.0, 3.0, 3.0]))], [_attr_str("mode", "nearest"),
                          _attr_str("coordinate_transformation_mode", "asymmetric"), _attr_str("nearest_mode", "floor")])
        if not dynamic:
            return w.node("Resize", [x, "", w.init(np.array([1.0, 1.0, 2.0, 2.0]))], [_attr_str("mode", "nearest"),
                          _attr_str("coordinate_transformation_mode", "asymmetric"), _attr_str("nearest_mode", "floor")])
        # sizes = concat(shape(x)[0:2], [floor(float(shape(x)[2]) * 2)], shape(like)[3:4])
        sx, sl = w.node("Shape", [x]), w.node("Shape", [like])
        nc = w.node("Slice", [sx, w.init_i64([0]), w.init_i64([2]), w.init_i64([0])])
        h = w.node("Gather", [sx, w.const_i64(np.array(2))], [ow._attr_int("axis", 0)])
        h = w.node("Cast", [h], [ow._attr_int("to", 1)])
        h = w.node("Floor", [w.node("Mul", [h, w.init_scalar(2.0)])])
        h = w.node("Unsqueeze", [w.node("Cast", [h], [ow._attr_int("to", 7)])], [ow._attr_ints("axes", [0])])
        wd = w.node("Slice", [sl, w.init_i64([3]), w.init_i64([4]), w.init_i64([0])])
        sizes = w.node("Concat", [nc, h, wd], [ow._attr_int("axis", 0)])
        return w.node("Resize", [x, "", "", sizes], [_attr_str("mode", "nearest"),
                      _attr_str("coordinate_transformation_mode", "half_pixel"), _attr_str("nearest_mode", "round_prefer_floor")])

    def flatten(x, src, k):
        t = w.node("Transpose", [x], [ow._attr_ints("perm", [0, 2, 3, 1])])
        if not dynamic:
            return w.node("Reshape", [t, w.init_i64([1, -1, k])])
        b = w.node("Unsqueeze", [w.node("Gather", [w.node("Shape", [src]), w.init_i64(np.array(0))], [ow._attr_int("axis", 0)])],
                   [ow._attr_ints("axes", [0])])
        return w.node("Reshape", [t, w.node("Concat", [b, w.init_i64([-1]), w.init_i64([k])], [ow._attr_int("axis", 0)])])

    x = "input.1"
    s0, s1, s2 = cfg["stem"]
    x = conv(x, 3, s0, 3, 2)
    x = conv(x, s0, s1, 3, group=2 if mutate == "group" else 1)
    x = conv(x, s1, s2, 3)
    x = w.node("MaxPool", [x], [ow._attr_ints("kernel_shape", [3, 3]), ow._attr_ints("strides", [2, 2]), ow._attr_ints("pads", [1] * 4),
                                ow._attr_int("ceil_mode", 0)])
    cin, feats = s2, []
    for si, (nb, width) in enumerate(cfg["stages"]):
        for bi in range(nb):
            stride = 2 if bi == 0 and si > 0 else 1
            t = conv(x, cin, width, 3, stride)
            t = conv(t, width, width, 3, relu=False, gain=0.5)
            sc = x
            if stride != 1 or cin != width:
                if stride != 1:
                    sc = w.node("AveragePool", [sc], [ow._attr_ints("kernel_shape", [2, 2]), ow._attr_ints("strides", [2, 2]),
                                                      ow._attr_ints("pads", [0] * 4), ow._attr_int("ceil_mode", 1),
                                                      ow._attr_int("count_include_pad", 0)])
                sc = conv(sc, cin, width, 1, relu=False)
            x = w.node("Relu", [w.node("Add", [t, sc])])
            if mutate == "prelu" and si == 0 and bi == 0:
                x = w.node("PRelu", [x, w.init(np.full((width, 1, 1), 0.25))])
            cin = width
        if si > 0:
            feats.append((x, width))
    f = cfg["fpn"]
    lat = [conv(t, c, f, 1, bn=False, relu=False) for t, c in feats]
    for i in (2, 1):
        lat[i - 1] = w.node("Add", [lat[i - 1], resize(lat[i], lat[i - 1])])
    inter = [conv(t, f, f, 3, bn=False, relu=False) for t in lat]
    for i in (0, 1):
        inter[i + 1] = w.node("Add", [inter[i + 1], conv(inter[i], f, f, 3, 2, bn=False, relu=False)])
    outs = [inter[0]] + [conv(inter[i], f, f, 3, bn=False, relu=False) for i in (1, 2)]
    hd, A, names = cfg["head"], cfg["anchors"], []
    for li, t in enumerate(outs):
        src, c = t, f
        for j in range(cfg["head_convs"]):
            t = conv(t, c, hd, 3, key=("head", j))
            c = hd
        cls = conv(t, hd, A, 3, bn=False, relu=False, gain=0.1, bias=score_bias, key="cls")
        reg = conv(t, hd, 4 * A, 3, bn=False, relu=False, gain=0.03, bias=1.5, key="reg")
        reg = w.node("Mul", [reg, w.init(np.array([1.0, 0.9, 1.1][li]))])
        cls = flatten(cls, src, 1)
        names.append(cls if mutate == "nosigmoid" and li == 1 else w.node("Sigmoid", [cls]))
        names.append(flatten(reg, src, 4))
        if mutate != "nokps":
            kps = conv(t, hd, 10 * A, 3, bn=False, relu=False, gain=0.05, bias=0.0, key="kps")
            names.append(flatten(kps, src, 10))
    graph = b"".join(ow._ld(1, n) for n in w.nodes) + ow._ld(2, b"scrfd") + b"".join(ow._ld(5, t) for t in w.inits)
    graph += ow._ld(11, ow._ld(1, b"input.1")) + b"".join(ow._ld(12, ow._ld(1, n.encode())) for n in names)
    model = ow._vi(1, 7) + ow._ld(2, b"tests/helpers/scrfd_onnx.py") + ow._ld(7, graph) + ow._ld(8, ow._ld(1, b"") + ow._vi(2, 11))
    with open(path, "wb") as fh:
        fh.write(model)
    return names


def lowpass_frames(n, h, w, seed=0):
    """seeded smooth BGR uint8 frames [n,h,w,3]: coarse noise, bilinearly enlarged"""
    import torch
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        z = torch.rand((1, 3, max(h // 32, 2), max(w // 32, 2)), generator=g, dtype=torch.float64)
        out.append(torch.nn.functional.interpolate(z, size=(h, w), mode="bilinear", align_corners=False)[0])
    x = torch.stack(out).permute(0, 2, 3, 1) * 255.0
    return x.round().clamp(0, 255).to(torch.uint8).numpy()
