"""Test helper: seeded MobileFaceNet-shaped recognition graphs (and a depthwise-backbone SCRFD) as ONNX files, written with
the protobuf writers of onnx_write.py.

The architecture is the public one of insightface's MobileFaceNet (``w600k_mbf``): 3x3 s2 stem + PReLU, a depthwise 3x3 +
PReLU, stages of depthwise-residual blocks (1x1 expand + PReLU, depthwise 3x3 + PReLU, 1x1 project linear; a stage opens with
a stride-2 block without a skip, its other blocks add their input), 1x1 to 512 + PReLU, depthwise 7x7 linear, flatten, Linear
512 -> 512, BatchNorm1d.  Weights are synthetic: He-normal convs, non-trivial BN, block-final gamma small,
PReLU slopes that mix negative, zero, (0, 1) and > 1.  Export styles: BatchNormalization kept as nodes or folded into the conv /
the Gemm; the fully connected layer as Gemm (transB 1 or 0) or MatMul + Add; the flatten as Flatten or Reshape."""
import numpy as np

from tests.helpers import onnx_write as ow
from tests.helpers.scrfd_onnx import _W, write_scrfd_onnx  # noqa: F401  (the SCRFD writer is re-used below)

EPS = 1e-5
# stem width, then per stage (expand width of the stride-2 block, stage width, residual blocks, their expand width), tail width
CFG_FULL = dict(stem=64, stages=((128, 64, 4, 128), (256, 128, 6, 256), (512, 128, 2, 256)), tail=512)       # blocks (1, 4, 6, 2)
CFG_1111 = dict(stem=64, stages=((128, 64, 1, 128), (256, 128, 1, 256), (512, 128, 1, 256)), tail=512)       # full width, one block each
CFG_TINY = dict(stem=16, stages=((24, 16, 1, 24), (40, 24, 2, 40), (48, 24, 1, 48)), tail=512)               # the CPU tests


def n_steps(cfg):
    """(convs, depthwise convs) a plan of ``cfg`` holds: the fully connected layer counts as a conv"""
    blocks = sum(1 + nb for _, _, nb, _ in cfg["stages"])
    return 1 + 2 * blocks + 1 + 1, 1 + blocks + 1


def _value_info(name, shape):
    dims = b"".join(ow._ld(1, ow._ld(2, b"N") if d is None else ow._vi(1, d)) for d in shape)
    return ow._ld(1, name.encode()) + ow._ld(2, ow._ld(1, ow._vi(1, 1) + ow._ld(2, dims)))


def write_mbf_onnx(path, cfg=CFG_FULL, seed=0, fold_bn=True, fc="gemm", flatten="Flatten", mutate=None):
    """Writes the graph; returns the output name.  ``fc``: 'gemm' (transB = 1), 'gemm_nt' (transB = 0) or 'matmul' (MatMul +
    Add).  ``mutate``: None or one of 'group2', 'dilation', 'relu', 'two_outputs', 'slope_len' - a defect for the refusal tests."""
    rng = np.random.default_rng(seed)
    w = _W()

    def slopes(c):
        s = rng.uniform(0.05, 0.95, c)
        k = rng.integers(0, 4, c)                                    # a quarter each: (0, 1), negative, zero, > 1
        return np.where(k == 1, -rng.uniform(0.1, 0.5, c), np.where(k == 2, 0.0, np.where(k == 3, rng.uniform(1.1, 1.6, c), s)))

    def conv(x, cin, cout, k, stride=1, pad=None, dw=False, prelu=True, final=False, group=None, dilation=1, slope_len=None):
        grp = group if group is not None else (cin if dw else 1)
        wt = rng.standard_normal((cout, cin // grp, k, k)) * np.sqrt(2.0 / (cin // grp * k * k))
        g = rng.uniform(0.1, 0.2, cout) if final else rng.uniform(0.8, 1.2, cout)
        bn = [g, rng.standard_normal(cout) * 0.1, rng.standard_normal(cout) * 0.1, rng.uniform(0.8, 1.2, cout)]
        attrs = [ow._attr_ints("kernel_shape", [k, k]), ow._attr_ints("strides", [stride, stride]),
                 ow._attr_ints("pads", [k // 2 if pad is None else pad] * 4), ow._attr_ints("dilations", [dilation] * 2), ow._attr_int("group", grp)]
        if fold_bn:
            s = bn[0] / np.sqrt(bn[3] + EPS)
            x = w.node("Conv", [x, w.init(wt * s[:, None, None, None]), w.init(bn[1] - bn[2] * s)], attrs)
        else:
            x = w.node("Conv", [x, w.init(wt)], attrs)
            x = w.node("BatchNormalization", [x] + [w.init(a) for a in bn], [ow._attr_float("epsilon", EPS)])
        if prelu:
            sl = slopes(cout if slope_len is None else slope_len)
            shape = [(-1,), (-1, 1, 1), (1, -1, 1, 1)][int(rng.integers(0, 3))]
            x = w.node("PRelu", [x, w.init(sl.reshape(shape))])
        return x

    def block(x, cin, cout, expand, stride, skip):
        t = conv(x, cin, expand, 1)
        t = conv(t, expand, expand, 3, stride, dw=True)
        t = conv(t, expand, cout, 1, prelu=False, final=True)
        return w.node("Add", [x, t]) if skip else t

    c = cfg["stem"]
    x = conv("input.1", 3, c, 3, 2, dilation=2 if mutate == "dilation" else 1, pad=2 if mutate == "dilation" else None)
    x = conv(x, c, c, 3, dw=True, slope_len=c + 1 if mutate == "slope_len" else None)
    if mutate == "relu":
        x = w.node("Relu", [x])
    extra = None
    for si, (dexp, width, nb, rexp) in enumerate(cfg["stages"]):
        if mutate == "group2" and si == 0:
            x = conv(x, c, c, 3, group=2)
        x = block(x, c, width, dexp, 2, False)
        c = width
        for _ in range(nb):
            x = block(x, c, c, rexp, 1, True)
        extra = extra or x
    hw = 112 // 2 ** (1 + len(cfg["stages"]))
    x = conv(x, c, cfg["tail"], 1)
    x = conv(x, cfg["tail"], cfg["tail"], hw, pad=0, dw=True, prelu=False)
    if flatten == "Flatten":
        x = w.node("Flatten", [x], [ow._attr_int("axis", 1)])
    else:
        x = w.node("Reshape", [x, w.init_i64([-1, cfg["tail"]])])
    d = cfg["tail"]
    fw, fb = rng.standard_normal((512, d)) * np.sqrt(1.0 / d), rng.standard_normal(512) * 0.05
    bn = [rng.uniform(0.8, 1.2, 512), rng.standard_normal(512) * 0.1, rng.standard_normal(512) * 0.1, rng.uniform(0.8, 1.2, 512)]
    if fold_bn:
        s = bn[0] / np.sqrt(bn[3] + EPS)
        fw, fb = fw * s[:, None], (fb - bn[2]) * s + bn[1]
    if fc == "matmul":
        x = w.node("Add", [w.node("MatMul", [x, w.init(fw.T)]), w.init(fb)])
    else:
        x = w.node("Gemm", [x, w.init(fw if fc == "gemm" else fw.T), w.init(fb)],
                   [ow._attr_float("alpha", 1.0), ow._attr_float("beta", 1.0), ow._attr_int("transB", 1 if fc == "gemm" else 0)])
    if not fold_bn:
        x = w.node("BatchNormalization", [x] + [w.init(a) for a in bn], [ow._attr_float("epsilon", EPS)])
    outs = [(x, [None, 512])]
    if mutate == "two_outputs":
        outs.append((extra, [None, cfg["stages"][0][1], 28, 28]))
    graph = b"".join(ow._ld(1, n) for n in w.nodes) + ow._ld(2, b"mbf") + b"".join(ow._ld(5, t) for t in w.inits)
    graph += ow._ld(11, _value_info("input.1", [None, 3, 112, 112])) + b"".join(ow._ld(12, _value_info(n, sh)) for n, sh in outs)
    model = ow._vi(1, 7) + ow._ld(2, b"tests/helpers/mbf_onnx.py") + ow._ld(7, graph) + ow._ld(8, ow._ld(1, b"") + ow._vi(2, 11))
    with open(path, "wb") as fh:
        fh.write(model)
    return x


# ---------------------------------------------------------------------------------------------- depthwise SCRFD
CFG_DW_SMALL = dict(stem=(8, 16), stages=((1, 16), (2, 24), (1, 24), (1, 40)), fpn=16, head=24, head_convs=2, anchors=2)


def write_dw_scrfd_onnx(path, cfg=CFG_DW_SMALL, seed=0, fold_bn=True, score_bias=-4.0):
    """The small SCRFD config with a MobileNet-style depthwise-separable backbone (the shape of insightface's det_500m /
    det_2.5g: 3x3 s2 stem, then depthwise 3x3 + BN + ReLU -> 1x1 + BN + ReLU units; strides 4, 8, 16, 32), the same PAFPN and
    shared heads as scrfd_onnx.write_scrfd_onnx with depthwise-separable head towers.  Returns the nine output names in graph
    order (per stride: score, bbox, kps)."""
    rng = np.random.default_rng(seed)
    w = _W()
    shared = {}

    def conv(x, cin, cout, k, stride=1, bn=True, relu=True, gain=1.0, bias=None, key=None, dw=False):
        if key is not None and key in shared:
            ini = shared[key]
        else:
            fan = k * k if dw else cin * k * k
            wt = rng.standard_normal((cout, 1 if dw else cin, k, k)) * gain * np.sqrt(2.0 / fan)
            ini = {}
            if bn:
                p = [rng.uniform(0.8, 1.2, cout), rng.standard_normal(cout) * 0.1, rng.standard_normal(cout) * 0.1, rng.uniform(0.8, 1.2, cout)]
                if fold_bn:
                    s = p[0] / np.sqrt(p[3] + EPS)
                    ini["names"] = [w.init(wt * s[:, None, None, None]), w.init(p[1] - p[2] * s)]
                else:
                    ini["names"], ini["bn_names"] = [w.init(wt)], [w.init(a) for a in p]
            else:
                b = rng.standard_normal(cout) * 0.05 if bias is None else np.broadcast_to(np.asarray(bias, dtype=np.float64), (cout,))
                ini["names"] = [w.init(wt), w.init(b)]
            if key is not None:
                shared[key] = ini
        attrs = [ow._attr_ints("kernel_shape", [k, k]), ow._attr_ints("strides", [stride, stride]), ow._attr_ints("pads", [k // 2] * 4),
                 ow._attr_ints("dilations", [1, 1]), ow._attr_int("group", cin if dw else 1)]
        x = w.node("Conv", [x] + ini["names"], attrs)
        if bn and not fold_bn:
            x = w.node("BatchNormalization", [x] + ini["bn_names"], [ow._attr_float("epsilon", EPS)])
        return w.node("Relu", [x]) if relu else x

    def sep(x, cin, cout, stride=1, key=None):
        x = conv(x, cin, cin, 3, stride, dw=True, key=None if key is None else (key, "dw"))
        return conv(x, cin, cout, 1, key=None if key is None else (key, "pw"))

    def flatten(x, k):
        t = w.node("Transpose", [x], [ow._attr_ints("perm", [0, 2, 3, 1])])
        return w.node("Reshape", [t, w.init_i64([1, -1, k])])

    s0, s1 = cfg["stem"]
    x = conv("input.1", 3, s0, 3, 2)
    x = sep(x, s0, s1)
    cin, feats = s1, []
    for si, (nb, width) in enumerate(cfg["stages"]):
        for bi in range(nb):
            x = sep(x, cin, width, 2 if bi == 0 else 1)
            cin = width
        if si > 0:
            feats.append((x, width))
    f = cfg["fpn"]
    lat = [conv(t, c, f, 1, bn=False, relu=False) for t, c in feats]
    for i in (2, 1):
        up = w.node("Resize", [lat[i], "", w.init(np.array([1.0, 1.0, 2.0, 2.0]))],
                    [ow._ld(1, b"mode") + ow._ld(4, b"nearest") + ow._vi(20, 3),
                     ow._ld(1, b"coordinate_transformation_mode") + ow._ld(4, b"asymmetric") + ow._vi(20, 3),
                     ow._ld(1, b"nearest_mode") + ow._ld(4, b"floor") + ow._vi(20, 3)])
        lat[i - 1] = w.node("Add", [lat[i - 1], up])
    inter = [conv(t, f, f, 3, bn=False, relu=False) for t in lat]
    for i in (0, 1):
        inter[i + 1] = w.node("Add", [inter[i + 1], conv(inter[i], f, f, 3, 2, bn=False, relu=False)])
    outs = [inter[0]] + [conv(inter[i], f, f, 3, bn=False, relu=False) for i in (1, 2)]
    hd, A, names = cfg["head"], cfg["anchors"], []
    for li, t in enumerate(outs):
        c = f
        for j in range(cfg["head_convs"]):
            t = sep(t, c, hd, key=("head", j))
            c = hd
        cls = conv(t, hd, A, 3, bn=False, relu=False, gain=0.1, bias=score_bias, key="cls")
        reg = conv(t, hd, 4 * A, 3, bn=False, relu=False, gain=0.03, bias=1.5, key="reg")
        reg = w.node("Mul", [reg, w.init(np.array([1.0, 0.9, 1.1][li]))])
        kps = conv(t, hd, 10 * A, 3, bn=False, relu=False, gain=0.05, bias=0.0, key="kps")
        names += [w.node("Sigmoid", [flatten(cls, 1)]), flatten(reg, 4), flatten(kps, 10)]
    graph = b"".join(ow._ld(1, n) for n in w.nodes) + ow._ld(2, b"scrfd_dw") + b"".join(ow._ld(5, t) for t in w.inits)
    graph += ow._ld(11, ow._ld(1, b"input.1")) + b"".join(ow._ld(12, ow._ld(1, n.encode())) for n in names)
    model = ow._vi(1, 7) + ow._ld(2, b"tests/helpers/mbf_onnx.py") + ow._ld(7, graph) + ow._ld(8, ow._ld(1, b"") + ow._vi(2, 11))
    with open(path, "wb") as fh:
        fh.write(model)
    return names


def dw_scrfd_counts(cfg=CFG_DW_SMALL):
    """(convs, depthwise convs) of the plan of ``write_dw_scrfd_onnx(cfg)``"""
    units = 1 + sum(nb for nb, _ in cfg["stages"]) + 3 * cfg["head_convs"]
    return 1 + units + 3 + 3 + 2 + 2 + 3 * 3, units
