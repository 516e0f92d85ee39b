"""Read the recognition network of an insightface model pack straight from its ONNX file.

The reference gets its networks as ONNX files resolved by name (``FaceAnalysis(name="buffalo_l")``,
/root/reference/infrenceServer.py:412-416: ``~/.insightface/models/buffalo_l/w600k_r50.onnx`` is the ArcFace
IResNet-50).  Neither ``onnx`` nor ``onnxruntime`` exists in this image, and only two things are needed
from such a file - the graph's node list and its initialisers - so this module decodes the protobuf wire format
itself (ONNX ``ModelProto`` / ``GraphProto`` / ``NodeProto`` / ``TensorProto`` field numbers from the public
onnx.proto) and maps an IResNet graph onto the state-dict naming of weights.py by FOLLOWING THE DATA FLOW (tensor
names in ONNX exports are arbitrary numbers), not by name.

Both export styles are understood: BatchNormalization kept as nodes, or folded into the preceding Conv / Gemm by
the exporter (then the conv carries a bias and the state dict gets ``<conv>.bias`` and no BN entry; iresnet.py and
the oracle treat a missing BN as the identity).  The pre-activation ``bn1`` of a block can never be folded by an
exporter (zero padding sits between it and the conv) and must be present.

No real pack exists in the image.  The mapping is tested on two independent writers: graphs written by
tests/helpers/onnx_write.py from seeded state dicts, and files written by torch's own TorchScript exporter (the exporter
family insightface's packs came from) from plain nn.Modules, over its export styles: tests/test_onnx_torch_export.py.
Constants that reach their reader through Identity / Unsqueeze / Squeeze / Reshape / Transpose / Cast nodes are resolved
once, in front of all three mappers (``_fold_constant_views``; the SCRFD mapper evaluates the same ops, ``_const_eval``,
while it walks the shape arithmetic of a dynamic-shape export).
"""
import struct

import numpy as np

# --------------------------------------------------------------------------- protobuf wire format (reader)


def _varint(buf, i):
    r = s = 0
    while True:
        b = buf[i]
        i += 1
        r |= (b & 0x7F) << s
        if not b & 0x80:
            return r, i
        s += 7


def _fields(buf):
    """Yield (field number, wire type, value) of one message; value = int (varint / fixed) or memoryview (bytes)."""
    i, n = 0, len(buf)
    while i < n:
        key, i = _varint(buf, i)
        f, wt = key >> 3, key & 7
        if wt == 0:
            v, i = _varint(buf, i)
        elif wt == 1:
            v = bytes(buf[i:i + 8]); i += 8
        elif wt == 2:
            ln, i = _varint(buf, i)
            v = buf[i:i + ln]; i += ln
        elif wt == 5:
            v = bytes(buf[i:i + 4]); i += 4
        else:
            raise ValueError(f"unsupported protobuf wire type {wt}")
        yield f, wt, v


def _packed_varints(v, wt):
    if wt == 0:
        return [v]
    out, i = [], 0
    while i < len(v):
        x, i = _varint(v, i)
        out.append(x)
    return out


def _signed(x):
    return x - (1 << 64) if x >= 1 << 63 else x


_DTYPES = {1: np.float32, 10: np.float16, 11: np.float64, 6: np.int32, 7: np.int64}


def _tensor(buf):
    dims, dtype, name, raw, floats, int64s, int32s, external = [], 1, "", None, [], [], [], False
    for f, wt, v in _fields(buf):
        if f == 1:
            dims += [_signed(x) for x in _packed_varints(v, wt)]
        elif f == 2:
            dtype = v
        elif f == 8:
            name = bytes(v).decode()
        elif f == 9:
            raw = bytes(v)
        elif f == 4:                                    # float_data, packed or one fixed32 per element
            floats.append(bytes(v))
        elif f == 5:                                    # int32_data: int32 payloads, and float16 as uint16 bit patterns
            int32s += [_signed(x) for x in _packed_varints(v, wt)]
        elif f == 7:
            int64s += [_signed(x) for x in _packed_varints(v, wt)]
        elif f == 14:                                   # data_location: 0 = DEFAULT (legal when written explicitly), 1 = EXTERNAL
            external = v == 1
    if external:
        raise ValueError(f"initializer {name!r} stores its data in an external file (not supported)")
    if dtype not in _DTYPES:
        raise ValueError(f"initializer {name!r}: unsupported ONNX data type {dtype}")
    if raw is not None:
        a = np.frombuffer(raw, dtype=np.dtype(_DTYPES[dtype]).newbyteorder("<"))
    elif floats:
        a = np.frombuffer(b"".join(floats), dtype="<f4")
    elif int32s:
        a = np.asarray(int32s, dtype=np.int64)
        a = a.astype(np.uint16).view(np.float16) if dtype == 10 else a.astype(np.int32)
    else:
        a = np.asarray(int64s, dtype=np.int64)
    return name, a.astype(_DTYPES[dtype]).reshape(dims)


def _attribute(buf):
    name, val = "", None
    ints, floats = [], []
    for f, wt, v in _fields(buf):
        if f == 1:
            name = bytes(v).decode()
        elif f == 2:
            val = struct.unpack("<f", v)[0]
        elif f == 3:
            val = _signed(v)
        elif f == 4:
            val = bytes(v)
        elif f == 5:
            val = _tensor(v)[1]
        elif f == 8:
            ints += [_signed(x) for x in _packed_varints(v, wt)]
        elif f == 7:
            floats += [struct.unpack("<f", v)[0]] if wt == 5 else list(np.frombuffer(bytes(v), "<f4"))
    if ints:
        val = ints
    elif floats:
        val = floats
    return name, val


class Node:
    __slots__ = ("op", "name", "inputs", "outputs", "attrs")

    def __init__(self):
        self.op, self.name, self.inputs, self.outputs, self.attrs = "", "", [], [], {}

    def __repr__(self):
        return f"{self.op}({', '.join(self.inputs)}) -> {', '.join(self.outputs)}"


def _node(buf):
    n = Node()
    for f, wt, v in _fields(buf):
        if f == 1:
            n.inputs.append(bytes(v).decode())
        elif f == 2:
            n.outputs.append(bytes(v).decode())
        elif f == 3:
            n.name = bytes(v).decode()
        elif f == 4:
            n.op = bytes(v).decode()
        elif f == 5:
            k, a = _attribute(v)
            n.attrs[k] = a
    return n


class OnnxGraph:
    """nodes (file order = topological), initialisers by name, graph input names that are not initialisers; ``outputs``: the
    declared graph output names (None when the file was not read here); ``value_shapes``: name -> declared shape of a graph
    input / output as a list (None for a symbolic dimension), only for those whose ValueInfo carries one."""

    def __init__(self, nodes, initializers, inputs, outputs=None, value_shapes=None):
        self.nodes, self.initializers, self.inputs = nodes, initializers, inputs
        self.outputs, self.value_shapes = outputs, value_shapes or {}


def _value_info(buf):
    """ValueInfoProto -> (name, shape or None): type (2) . tensor_type (1) . shape (2) . dim (1) . dim_value (1)"""
    name, shape = "", None
    for f, _, v in _fields(buf):
        if f == 1:
            name = bytes(v).decode()
        elif f == 2:
            for g, _, tt in _fields(v):
                if g == 1:
                    for h, _, sh in _fields(tt):
                        if h == 2:
                            shape = []
                            for d, _, dim in _fields(sh):
                                if d == 1:
                                    val = [x for e, wt, x in _fields(dim) if e == 1 and wt == 0]
                                    shape.append(_signed(val[0]) if val else None)
    return name, shape


def read_onnx(path):
    with open(path, "rb") as fh:
        buf = memoryview(fh.read())
    graph = None
    for f, wt, v in _fields(buf):
        if f == 7 and wt == 2:
            graph = v
    if graph is None:
        raise ValueError(f"{path}: no GraphProto (field 7) in the ModelProto")
    nodes, inits, inputs, outputs, vshapes = [], {}, [], [], {}
    for f, wt, v in _fields(graph):
        if f == 1:
            nodes.append(_node(v))
        elif f == 5:
            name, a = _tensor(v)
            inits[name] = a
        elif f in (11, 12):                             # graph inputs / outputs (ValueInfoProto)
            name, shape = _value_info(v)
            (inputs if f == 11 else outputs).append(name)
            if shape is not None:
                vshapes[name] = shape
    # Constant nodes are initialisers in all but name
    for n in nodes:
        if n.op == "Constant" and "value" in n.attrs and n.outputs:
            inits[n.outputs[0]] = n.attrs["value"]
    return OnnxGraph([n for n in nodes if n.op != "Constant"], inits, [i for i in inputs if i not in inits], outputs, vshapes)


# --------------------------------------------------------------------------- constants behind nodes

_CAST = {1: np.float32, 6: np.int32, 7: np.int64, 11: np.float64}


def _who(n):
    return f"node {n.name or (n.outputs[0] if n.outputs else '?')!r} ({n.op})"


def _const_eval(n, a):
    """The value of node n on the constant inputs a (None for an omitted one): the shape arithmetic of dynamic-shape
    exports, and the views (Identity, Unsqueeze, Squeeze, Reshape, Transpose, Cast) an exporter may leave between an
    initialiser and its reader.  Raises ValueError naming the node for any other op."""
    op = n.op
    if op == "Gather":
        return np.take(a[0], np.asarray(a[1]).astype(np.int64), axis=int(n.attrs.get("axis", 0)))
    if op == "Slice":
        data = np.asarray(a[0])
        if len(a) > 1:
            starts, ends = a[1], a[2]
            axes = a[3] if len(a) > 3 and a[3] is not None else np.arange(len(starts))
            stp = a[4] if len(a) > 4 and a[4] is not None else np.ones(len(starts), np.int64)
        else:
            starts, ends = n.attrs["starts"], n.attrs["ends"]
            axes, stp = n.attrs.get("axes", list(range(len(starts)))), [1] * len(starts)
        sl = [slice(None)] * data.ndim
        for s, e, ax, sp in zip(np.ravel(starts), np.ravel(ends), np.ravel(axes), np.ravel(stp)):
            sl[int(ax)] = slice(int(s), int(min(e, 2 ** 62)), int(sp))
        return data[tuple(sl)]
    if op == "Concat":
        return np.concatenate([np.atleast_1d(x) for x in a], axis=int(n.attrs.get("axis", 0)))
    if op in ("Unsqueeze", "Squeeze"):
        axes = n.attrs.get("axes")
        if axes is None and len(a) > 1 and a[1] is not None:
            axes = [int(x) for x in np.ravel(a[1])]
        x = np.asarray(a[0])
        if op == "Squeeze":
            return np.squeeze(x, axis=tuple(axes) if axes else None)
        if axes is None:
            raise ValueError(f"{_who(n)}: Unsqueeze without axes")
        rank = x.ndim + len(axes)
        for ax in sorted(ax + rank if ax < 0 else ax for ax in axes):
            x = np.expand_dims(x, ax)
        return x
    if op == "Reshape":
        x = np.asarray(a[0])
        tgt = [int(v) for v in (np.ravel(a[1]) if len(a) > 1 and a[1] is not None else n.attrs.get("shape", []))]
        if not n.attrs.get("allowzero", 0):
            if any(v == 0 and i >= x.ndim for i, v in enumerate(tgt)):
                raise ValueError(f"{_who(n)}: Reshape of a {x.shape} constant to {tgt}")
            tgt = [x.shape[i] if v == 0 else v for i, v in enumerate(tgt)]
        return x.reshape(tgt)
    if op == "Transpose":
        x = np.asarray(a[0])
        return np.transpose(x, n.attrs.get("perm", list(range(x.ndim))[::-1]))
    if op == "Cast":
        to = n.attrs.get("to")
        if to not in _CAST:
            raise ValueError(f"{_who(n)}: cast to ONNX data type {to} not supported")
        return np.asarray(a[0]).astype(_CAST[to])
    if op in ("Mul", "Add", "Sub"):
        return {"Mul": np.multiply, "Add": np.add, "Sub": np.subtract}[op](a[0], a[1])
    if op == "Div":
        x, y = np.asarray(a[0]), np.asarray(a[1])
        return x // y if x.dtype.kind in "iu" and y.dtype.kind in "iu" else x / y
    if op in ("Floor", "Ceil"):
        return (np.floor if op == "Floor" else np.ceil)(a[0])
    if op == "Identity":
        return a[0]
    raise ValueError(f"{_who(n)}: op {n.op} is not supported (on constant inputs)")


_CONST_VIEWS = ("Identity", "Unsqueeze", "Squeeze", "Reshape", "Transpose", "Cast")


def _fold_constant_views(g):
    """-> the graph with every Identity / Unsqueeze / Squeeze / Reshape / Transpose / Cast that reads constants only
    evaluated: its output becomes an initialiser and the node goes.  Exporters leave such chains between a parameter
    and its reader - a PReLU slope behind an Unsqueeze when constant folding is off, one initialiser shared by equal
    parameters through Identity nodes, the transposed weight of a matmul(x, W.t()) - and the mappers below then meet an
    initialiser like any other.  The values are views or casts of the stored ones: no arithmetic happens here."""
    init, nodes = dict(g.initializers), []
    for n in g.nodes:
        ins = [t for t in n.inputs if t]
        if n.op in _CONST_VIEWS and ins and n.outputs and all(t in init for t in ins):
            init[n.outputs[0]] = _const_eval(n, [init[t] if t else None for t in n.inputs])
        else:
            nodes.append(n)
    return OnnxGraph(nodes, init, g.inputs, g.outputs, g.value_shapes)


# --------------------------------------------------------------------------- IResNet graph -> state dict

_ARCH_BY_BLOCKS = {(2, 2, 2, 2): "r18", (3, 4, 6, 3): "r34", (3, 4, 14, 3): "r50", (3, 13, 30, 3): "r100"}


def iresnet_state_from_onnx(path_or_graph):
    """-> (state dict of numpy float32 arrays in the naming of weights.py, arch).  Raises ValueError with the node
    it stopped at when the graph is not an ArcFace IResNet (conv-bn-prelu stem, pre-activation residual blocks,
    bn-flatten-fc-bn head)."""
    g = _fold_constant_views(path_or_graph if isinstance(path_or_graph, OnnxGraph) else read_onnx(path_or_graph))
    init = g.initializers
    consumers = {}
    producer = {}
    for n in g.nodes:
        for t in n.inputs:
            consumers.setdefault(t, []).append(n)
        for t in n.outputs:
            producer[t] = n
    st = {}

    def f32(name):
        if name not in init:
            raise ValueError(f"tensor {name!r} is not an initialiser")
        return np.ascontiguousarray(init[name], dtype=np.float32)

    def only(t, op, what):
        c = [n for n in consumers.get(t, []) if n.op == op]
        if len(c) != 1:
            raise ValueError(f"expected one {op} reading {t!r} ({what}), found {[n.op for n in consumers.get(t, [])]}")
        return c[0]

    def maybe(t, op):
        c = [n for n in consumers.get(t, []) if n.op == op]
        return c[0] if len(c) == 1 else None

    def take_bn(n, prefix):
        eps = n.attrs.get("epsilon", 1e-5)
        if abs(eps - 1e-5) > 1e-9:
            raise ValueError(f"{prefix}: BatchNormalization epsilon {eps} (this engine folds with 1e-5)")
        for key, t in zip(("weight", "bias", "running_mean", "running_var"), n.inputs[1:5]):
            st[f"{prefix}.{key}"] = f32(t).reshape(-1)
        return n.outputs[0]

    def take_conv(n, prefix, k, stride):
        w = f32(n.inputs[1])
        ks = n.attrs.get("kernel_shape", list(w.shape[2:]))
        s = n.attrs.get("strides", [1, 1])
        p = n.attrs.get("pads", [0, 0, 0, 0])
        if list(ks) != [k, k] or list(s) != [stride, stride] or list(p) != [k // 2] * 4 or n.attrs.get("group", 1) != 1:
            raise ValueError(f"{prefix}: conv geometry kernel {ks} strides {s} pads {p} is not {k}x{k}/s{stride}/p{k // 2}")
        st[f"{prefix}.weight"] = w
        if len(n.inputs) > 2 and n.inputs[2]:
            st[f"{prefix}.bias"] = f32(n.inputs[2]).reshape(-1)         # a BatchNormalization folded in by the exporter
        return n.outputs[0]

    def conv_bn(t, conv_prefix, bn_prefix, k, stride, what):
        """Conv [+ BatchNormalization] reading tensor t -> output tensor."""
        c = only(t, "Conv", what)
        t = take_conv(c, conv_prefix, k, stride)
        b = maybe(t, "BatchNormalization")
        if b is not None:
            t = take_bn(b, bn_prefix)
        elif f"{conv_prefix}.bias" not in st:
            raise ValueError(f"{conv_prefix}: neither a BatchNormalization after it nor a folded bias")
        return t

    def take_prelu(t, key, what):
        n = only(t, "PRelu", what)
        st[key] = f32(n.inputs[1]).reshape(-1)
        return n.outputs[0]

    if len(g.inputs) != 1:
        raise ValueError(f"expected one graph input, found {g.inputs}")
    cur = g.inputs[0]
    cur = conv_bn(cur, "conv1", "bn1", 3, 1, "stem conv")
    cur = take_prelu(cur, "prelu.weight", "stem PReLU")
    stages, li, bi = [], 0, 0
    while True:
        bn = only(cur, "BatchNormalization", "block bn1 or the head's bn2")
        after = consumers.get(bn.outputs[0], [])
        if any(n.op in ("Flatten", "Reshape", "Gemm", "MatMul") for n in after):
            break                                                        # the head
        # a block whose shortcut is a conv opens a new stage
        has_sc = any(n.op == "Conv" and n is not None and n.attrs.get("kernel_shape", [0])[0] == 1
                     for n in consumers.get(cur, []))
        if has_sc or li == 0:
            if li:
                stages.append(bi)
            li, bi = li + 1, 0
        p = f"layer{li}.{bi}"
        stride = 2 if bi == 0 else 1
        t = take_bn(bn, p + ".bn1")
        t = conv_bn(t, p + ".conv1", p + ".bn2", 3, 1, p + ".conv1")
        t = take_prelu(t, p + ".prelu.weight", p + ".prelu")
        t = conv_bn(t, p + ".conv2", p + ".bn3", 3, stride, p + ".conv2")
        add = only(t, "Add", p + " residual add")
        other = [x for x in add.inputs if x != t]
        if len(other) != 1:
            raise ValueError(f"{p}: residual add {add!r} does not join two tensors")
        if other[0] != cur:
            sc = [n for n in consumers.get(cur, []) if n.op == "Conv"]
            if len(sc) != 1 or bi != 0:
                raise ValueError(f"{p}: the add's other input {other[0]!r} is neither the block input nor a shortcut conv of it")
            t2 = take_conv(sc[0], p + ".downsample.0", 1, stride)
            b = maybe(t2, "BatchNormalization")
            if b is not None:
                t2 = take_bn(b, p + ".downsample.1")
            if t2 != other[0]:
                raise ValueError(f"{p}: shortcut output {t2!r} is not the add's input {other[0]!r}")
        elif bi == 0:
            raise ValueError(f"{p}: first block of a stage without a shortcut conv")
        cur = add.outputs[0]
        bi += 1
    stages.append(bi)
    arch = _ARCH_BY_BLOCKS.get(tuple(stages))
    if arch is None:
        raise ValueError(f"blocks per stage {stages} match no known IResNet depth {sorted(_ARCH_BY_BLOCKS)}")
    # head: bn2 -> flatten -> fc (Gemm, or MatMul + Add) -> features BN (kept, or folded into the Gemm)
    t = take_bn(bn, "bn2")
    fl = [n for n in consumers.get(t, []) if n.op in ("Flatten", "Reshape")]
    if fl:
        t = fl[0].outputs[0]
    fc = [n for n in consumers.get(t, []) if n.op in ("Gemm", "MatMul")]
    if len(fc) != 1:
        raise ValueError(f"expected the fc Gemm / MatMul after the flatten, found {consumers.get(t, [])}")
    fc = fc[0]
    w = f32(fc.inputs[1])
    if fc.op == "Gemm":
        if fc.attrs.get("alpha", 1.0) != 1.0 or fc.attrs.get("beta", 1.0) != 1.0 or fc.attrs.get("transA", 0):
            raise ValueError("fc Gemm with alpha / beta / transA other than 1 / 1 / 0")
        if not fc.attrs.get("transB", 0):
            w = w.T
        bias = f32(fc.inputs[2]).reshape(-1) if len(fc.inputs) > 2 else np.zeros(w.shape[0], np.float32)
        t = fc.outputs[0]
    else:
        w = w.T
        t = fc.outputs[0]
        a = maybe(t, "Add")
        bias = np.zeros(w.shape[0], np.float32)
        if a is not None:
            bias = f32([x for x in a.inputs if x != t][0]).reshape(-1)
            t = a.outputs[0]
    if w.shape != (512, 512 * 49):
        raise ValueError(f"fc weight {w.shape}, expected (512, 25088)")
    st["fc.weight"], st["fc.bias"] = np.ascontiguousarray(w), bias
    b = maybe(t, "BatchNormalization")
    if b is not None:
        take_bn(b, "features")
    return st, arch


# --------------------------------------------------------------------------- SCRFD graph -> device plan

class ScrfdPlan:
    """What ``scrfd_plan_from_onnx`` returns for one canvas size.

    steps    device steps in execution order, dicts with ``op`` in
             ``input``  (out)                                       the canvas as tensor 0
             ``conv``   (x, out, w, b, wkey, k, stride, pad, relu, res, f32)   w [Cout,Cin,k,k] / b [Cout] float64, BN / Mul folded
             ``dwconv`` (the same keys; res None, f32 False)        depthwise 3x3, pad 1: w [C,1,3,3]
             ``pool``   (x, out, kind, k, stride, pad)              kind 0 max, 1 average
             ``upadd``  (coarse, lateral, out, up)                  lateral + nearest x up of coarse
    shapes   tensor id -> (C, H, W), the channel count unpadded
    levels   three dicts (stride, score, bbox, kps: tensor ids of f32 head maps read flat as [H*W*A, 1 | 4 | 10]), strides 8, 16, 32
    outputs  the nine graph output names in graph order -> (level index, kind)
    """

    def __init__(self, canvas_hw, steps, shapes, levels, num_anchors, outputs):
        self.canvas_hw, self.steps, self.shapes, self.levels = tuple(canvas_hw), steps, shapes, levels
        self.num_anchors, self.outputs = num_anchors, outputs
        self.macs2 = sum(2 * shapes[s["out"]][1] * shapes[s["out"]][2] * int(np.prod(s["w"].shape))
                         for s in steps if s["op"] in ("conv", "dwconv"))


_NEAREST_OK = {("asymmetric", "floor"), ("asymmetric", "round_prefer_floor"), ("half_pixel", "round_prefer_floor"),
               ("pytorch_half_pixel", "round_prefer_floor")}


def _text(v, default):
    return default if v is None else (bytes(v).decode() if not isinstance(v, str) else v)


def scrfd_plan_from_onnx(path_or_graph, canvas_hw=(640, 640)):
    """Map a SCRFD detector graph (insightface's ``det_*.onnx``: conv backbone, FPN, three strides of score / bbox / kps
    heads) onto device steps by following the data flow.  ``canvas_hw`` = (height, width), multiples of 32: shape
    arithmetic of dynamic-shape exports is evaluated on the host for it.  Raises ValueError naming the node and op it cannot
    map; a graph is mapped whole or not at all."""
    g = path_or_graph if isinstance(path_or_graph, OnnxGraph) else read_onnx(path_or_graph)
    ch, cw = int(canvas_hw[0]), int(canvas_hw[1])
    if ch <= 0 or cw <= 0 or ch % 32 or cw % 32:
        raise ValueError(f"canvas {ch} x {cw}: sides must be positive multiples of 32")
    if len(g.inputs) != 1:
        raise ValueError(f"expected one graph input, found {g.inputs}")
    consumers = {}
    for n in g.nodes:
        for t in n.inputs:
            if t:
                consumers.setdefault(t, []).append(n)
    host = dict(g.initializers)          # tensor name -> numpy value known on the host
    dev = {g.inputs[0]: 0}               # tensor name -> device tensor id
    shapes = {0: (3, ch, cw)}
    steps = [{"op": "input", "out": 0}]
    producer = {}                        # tensor id -> its conv step (only while more may be folded into it)
    resized = {}                         # tensor name -> (source tensor id, factor): a Resize waiting for its Add
    nhwc, flat, sigm = {}, {}, {}        # tail views: name -> tensor id / (tensor id, K) / (tensor id, K)

    who = _who

    def new(shape):
        tid = len(shapes)
        shapes[tid] = shape
        return tid

    def sole(n, t):
        return len(consumers.get(t, [])) == 1 and consumers[t][0] is n

    def open_conv(n, t):
        """the conv step that produced device tensor name t, when n is its only reader"""
        st = producer.get(dev.get(t))
        return st if st is not None and sole(n, t) else None

    def sym(n, key, k):
        p = list(n.attrs.get(key, [0, 0, 0, 0]))
        if len(p) != 4 or len(set(p)) != 1:
            raise ValueError(f"{who(n)}: pads {p} are not symmetric")
        return int(p[0])

    def square(n, key, default=None):
        v = n.attrs.get(key, default)
        if v is None or len(v) != 2 or v[0] != v[1]:
            raise ValueError(f"{who(n)}: {key} {v} is not square")
        return int(v[0])

    for n in g.nodes:
        ins = [t for t in n.inputs if t]
        if not n.outputs:
            raise ValueError(f"{who(n)}: node without outputs")
        out = n.outputs[0]
        if n.op == "Shape" and ins and ins[0] in dev:
            c, h, w = shapes[dev[ins[0]]]
            host[out] = np.array([1, c, h, w], dtype=np.int64)
            continue
        if ins and all(t in host for t in ins):
            host[out] = _const_eval(n, [host[t] if t else None for t in n.inputs])
            continue
        if n.op == "Conv":
            if ins[0] not in dev or ins[1] not in host:
                raise ValueError(f"{who(n)}: conv input / weight is not a feature map / an initialiser")
            w = np.asarray(host[ins[1]], dtype=np.float64)
            c, h, wd = shapes[dev[ins[0]]]
            grp = n.attrs.get("group", 1)
            # the one grouped form there is a kernel for: depthwise 3x3, pad 1 (the small SCRFDs' separable convs)
            dw = grp != 1 and w.ndim == 4 and grp == c == w.shape[0] and w.shape[1] == 1 and list(w.shape[2:]) == [3, 3] \
                and list(n.attrs.get("kernel_shape", [3, 3])) == [3, 3] and list(n.attrs.get("pads", [0] * 4)) == [1] * 4 \
                and list(n.attrs.get("strides", [1, 1])) in ([1, 1], [2, 2]) and list(n.attrs.get("dilations", [1, 1])) == [1, 1]
            if grp != 1 and not dw:
                raise ValueError(f"{who(n)}: grouped conv (group {n.attrs['group']}) is not supported")
            k = square(n, "kernel_shape", list(w.shape[2:]))
            s = square(n, "strides", [1, 1])
            p = sym(n, "pads", k)
            if w.ndim != 4 or w.shape[1] != (1 if dw else c) or w.shape[2] != k or w.shape[3] != k or k not in (1, 3) or s not in (1, 2) \
                    or p >= k or list(n.attrs.get("dilations", [1, 1])) != [1, 1]:
                raise ValueError(f"{who(n)}: conv weight {w.shape} kernel {k} stride {s} pad {p} on {c} channels is not a "
                                 "1x1 / 3x3, stride 1 / 2, undilated conv of its input")
            b = np.asarray(host[ins[2]], dtype=np.float64).reshape(-1) if len(ins) > 2 else np.zeros(w.shape[0])
            if len(ins) > 2 and ins[2] not in host:
                raise ValueError(f"{who(n)}: conv bias is not an initialiser")
            tid = new((w.shape[0], (h + 2 * p - k) // s + 1, (wd + 2 * p - k) // s + 1))
            st = {"op": "dwconv" if dw else "conv", "x": dev[ins[0]], "out": tid, "w": w, "b": b,
                  "wkey": (ins[1], ins[2] if len(ins) > 2 else None), "k": k, "stride": s, "pad": p, "relu": False, "res": None, "f32": False}
            steps.append(st)
            producer[tid] = st
            dev[out] = tid
        elif n.op == "BatchNormalization":
            st = open_conv(n, ins[0])
            if st is None or st["relu"] or st["res"] is not None:
                raise ValueError(f"{who(n)}: BatchNormalization that does not directly follow a Conv")
            sc, bi, mu, var = (np.asarray(host[t], dtype=np.float64).reshape(-1) for t in ins[1:5])
            f = sc / np.sqrt(var + float(n.attrs.get("epsilon", 1e-5)))
            st["w"], st["b"] = st["w"] * f[:, None, None, None], (st["b"] - mu) * f + bi
            st["wkey"] += ("bn",) + tuple(ins[1:5])
            dev[out] = st["out"]
        elif n.op == "Mul":
            c = [t for t in ins if t in host]
            d = [t for t in ins if t in dev]
            st = open_conv(n, d[0]) if len(d) == 1 and len(c) == 1 else None
            if st is None or np.size(host[c[0]]) != 1 or st["relu"] or st["res"] is not None:
                raise ValueError(f"{who(n)}: Mul that is not a constant scalar scale of a Conv output")
            f = float(np.ravel(host[c[0]])[0])
            st["w"], st["b"] = st["w"] * f, st["b"] * f
            st["wkey"] += ("mul", c[0], f)
            dev[out] = st["out"]
        elif n.op == "Relu":
            st = open_conv(n, ins[0]) if ins[0] in dev else None
            if st is None or st["relu"]:
                raise ValueError(f"{who(n)}: Relu that does not follow a Conv or a Conv + Add")
            st["relu"] = True
            dev[out] = st["out"]
        elif n.op == "Add":
            if len(ins) != 2:
                raise ValueError(f"{who(n)}: Add of {len(ins)} tensors")
            rs = [t for t in ins if t in resized]
            if rs:
                other = [t for t in ins if t not in resized]
                if len(rs) != 1 or len(other) != 1 or other[0] not in dev or not sole(n, rs[0]):
                    raise ValueError(f"{who(n)}: Add of a Resize output with something that is not a feature map")
                src, up = resized[rs[0]]
                lat = dev[other[0]]
                if shapes[lat] != (shapes[src][0], shapes[src][1] * up, shapes[src][2] * up):
                    raise ValueError(f"{who(n)}: Add of a {shapes[lat]} map with a x{up} resize of a {shapes[src]} map")
                tid = new(shapes[lat])
                steps.append({"op": "upadd", "coarse": src, "lateral": lat, "out": tid, "up": up})
                producer.pop(lat, None)
                dev[out] = tid
                continue
            if not all(t in dev for t in ins):
                raise ValueError(f"{who(n)}: Add of something that is not a feature map")
            a, b = dev[ins[0]], dev[ins[1]]
            if shapes[a] != shapes[b]:
                raise ValueError(f"{who(n)}: Add of maps of shapes {shapes[a]} and {shapes[b]}")
            # the conv that runs LAST takes the other map as its residual (relu(acc + bias + residual))
            made = {s["out"]: i for i, s in enumerate(steps)}
            cand = [(made[st["out"]], st, o) for t, o in ((ins[0], b), (ins[1], a))
                    for st in [open_conv(n, t)] if st is not None and st["op"] == "conv" and not st["relu"] and st["res"] is None
                    and made[st["out"]] > made[o]]
            if cand and a != b:
                _, st, o = max(cand, key=lambda c: c[0])
                st["res"] = o
                producer.pop(o, None)
                dev[out] = st["out"]
            else:
                tid = new(shapes[a])
                steps.append({"op": "upadd", "coarse": a, "lateral": b, "out": tid, "up": 1})
                producer.pop(a, None), producer.pop(b, None)
                dev[out] = tid
        elif n.op in ("MaxPool", "AveragePool"):
            if ins[0] not in dev:
                raise ValueError(f"{who(n)}: pool of something that is not a feature map")
            c, h, wd = shapes[dev[ins[0]]]
            k, s = square(n, "kernel_shape"), square(n, "strides", [1, 1])
            p = sym(n, "pads", k)
            ceil = int(n.attrs.get("ceil_mode", 0))
            cip = int(n.attrs.get("count_include_pad", 0))
            if k > 3 or s > 2 or p >= k or list(n.attrs.get("dilations", [1, 1])) != [1, 1] or n.attrs.get("storage_order", 0):
                raise ValueError(f"{who(n)}: pool kernel {k} stride {s} pad {p} is not implemented (kernel <= 3, stride <= 2)")

            def osz(x):
                o = -((x + 2 * p - k) // -s) + 1 if ceil else (x + 2 * p - k) // s + 1
                return o - 1 if ceil and (o - 1) * s >= x + p else o
            ho, wo = osz(h), osz(wd)
            over = p > 0 or (ho - 1) * s + k > h or (wo - 1) * s + k > wd
            if n.op == "AveragePool" and cip and over:
                raise ValueError(f"{who(n)}: AveragePool with count_include_pad over padded or overhanging windows is not implemented")
            tid = new((c, ho, wo))
            steps.append({"op": "pool", "x": dev[ins[0]], "out": tid, "kind": 0 if n.op == "MaxPool" else 1, "k": k, "stride": s,
                          "pad": p})
            producer.pop(dev[ins[0]], None)
            dev[out] = tid
        elif n.op in ("Resize", "Upsample"):
            if ins[0] not in dev:
                raise ValueError(f"{who(n)}: resize of something that is not a feature map")
            c, h, wd = shapes[dev[ins[0]]]
            mode = _text(n.attrs.get("mode"), "nearest")
            ctm = _text(n.attrs.get("coordinate_transformation_mode"), "half_pixel" if n.op == "Resize" else "asymmetric")
            nm = _text(n.attrs.get("nearest_mode"), "round_prefer_floor" if n.op == "Resize" else "floor")
            if mode != "nearest" or (ctm, nm) not in _NEAREST_OK:
                raise ValueError(f"{who(n)}: resize mode {mode} / {ctm} / {nm} is not a nearest-neighbour copy")
            rest = [t for t in n.inputs[1:]]
            if any(t and t not in host for t in rest):
                raise ValueError(f"{who(n)}: resize scales / sizes do not follow from the input size")
            vals = [np.ravel(host[t]) for t in rest if t and np.size(host[t])]
            if n.op == "Resize" and len(n.inputs) > 3 and n.inputs[3]:
                tgt = [int(v) for v in np.ravel(host[n.inputs[3]])]
                ok = len(tgt) == 4 and tgt[2] == 2 * h and tgt[3] == 2 * wd and tgt[1] == c
            else:
                sc = vals[-1] if vals else np.ravel(n.attrs.get("scales", []))
                ok = len(sc) == 4 and float(sc[0]) == 1 and float(sc[1]) == 1 and float(sc[2]) == 2 and float(sc[3]) == 2
            if not ok:
                raise ValueError(f"{who(n)}: resize is not a x2 nearest-neighbour upsample of its {h} x {wd} input")
            resized[out] = (dev[ins[0]], 2)
            producer.pop(dev[ins[0]], None)
        elif n.op == "Transpose":
            if ins[0] not in dev or list(n.attrs.get("perm", [])) != [0, 2, 3, 1] or not sole(n, ins[0]):
                raise ValueError(f"{who(n)}: Transpose that is not the (0, 2, 3, 1) of a head map")
            nhwc[out] = dev[ins[0]]
        elif n.op == "Reshape":
            if ins[0] not in nhwc or len(ins) < 2 or ins[1] not in host:
                raise ValueError(f"{who(n)}: Reshape that does not flatten a transposed head map to a constant last dimension")
            tgt = [int(v) for v in np.ravel(host[ins[1]])]
            tid = nhwc[ins[0]]
            c, h, wd = shapes[tid]
            if (len(tgt) < 2 or tgt[-1] <= 0 or c % tgt[-1] or tgt[-2] not in (-1, c * h * wd // tgt[-1])
                    or any(v > 0 and v != 1 for v in tgt[:-2])):
                raise ValueError(f"{who(n)}: Reshape target {tgt} does not flatten a {shapes[tid]} head map")
            flat[out] = (tid, tgt[-1])
        elif n.op == "Sigmoid":
            if ins[0] not in flat:
                raise ValueError(f"{who(n)}: Sigmoid that is not on a flattened head map")
            sigm[out] = flat[ins[0]]
        else:
            raise ValueError(f"{who(n)}: op {n.op} is not supported")

    produced = [t for n in g.nodes for t in n.outputs]
    outs = [t for t in produced if t not in consumers and t not in host]
    if len(outs) != 9:
        kinds = "" if len(outs) != 6 else " (a detector without keypoint outputs: alignment needs them)"
        raise ValueError(f"expected 9 graph outputs (3 strides x score, bbox, kps), found {len(outs)}{kinds}: not a SCRFD detector with keypoints")
    by_stride = {}
    for t in outs:
        if t in sigm:
            tid, kk, sg = sigm[t] + (True,)
        elif t in flat:
            tid, kk, sg = flat[t] + (False,)
        else:
            raise ValueError(f"graph output {t!r} is not a flattened head map")
        st = producer.get(tid)
        c, h, w = shapes[tid]
        if st is None or st["op"] != "conv" or st["relu"] or st["res"] is not None or ch % h or cw % w or ch // h != cw // w:
            raise ValueError(f"graph output {t!r} does not come straight out of a head conv")
        by_stride.setdefault(ch // h, []).append((t, tid, c, kk, sg, st))
    if sorted(by_stride) != [8, 16, 32] or any(len(v) != 3 for v in by_stride.values()):
        raise ValueError(f"head maps at strides {sorted(by_stride)} with {[len(v) for v in by_stride.values()]} outputs each: "
                         "expected score, bbox and kps at strides 8, 16, 32")
    levels, outputs, A = [], {}, None
    for li, s in enumerate((8, 16, 32)):
        ent = sorted(by_stride[s], key=lambda e: e[2])
        a = ent[0][2]
        A = a if A is None else A
        if a != A or [e[2] for e in ent] != [a, 4 * a, 10 * a] or [e[3] for e in ent] != [1, 4, 10]:
            raise ValueError(f"stride {s}: head channels {[e[2] for e in ent]} flattened to {[e[3] for e in ent]} are not "
                             f"(A, 4A, 10A) to (1, 4, 10) with A = {A}")
        if not ent[0][4]:
            raise ValueError(f"stride {s}: score output {ent[0][0]!r} does not come out of a Sigmoid")
        if ent[1][4] or ent[2][4]:
            raise ValueError(f"stride {s}: a Sigmoid on a bbox / kps output")
        for e, kind in zip(ent, ("score", "bbox", "kps")):
            e[5]["f32"] = True
            outputs[e[0]] = (li, kind)
        levels.append({"stride": s, "score": ent[0][1], "bbox": ent[1][1], "kps": ent[2][1]})
    # graph order: the declared outputs' where the file declares them (an exporter lists them as the module returned them,
    # which need not be the order of the nodes), else the nodes'
    declared = g.outputs if g.outputs and sorted(g.outputs) == sorted(outs) else outs
    outputs = {t: outputs[t] for t in declared}
    used = {s[k] for s in steps for k in ("x", "res", "coarse", "lateral") if s.get(k) is not None}
    used |= {lv[k] for lv in levels for k in ("score", "bbox", "kps")}
    for s in steps:
        if s["out"] not in used:
            raise ValueError(f"a {s['op']} step's result (tensor {s['out']}, shape {shapes[s['out']]}) feeds nothing: not a SCRFD detector")
    return ScrfdPlan((ch, cw), steps, shapes, levels, A, outputs)


# --------------------------------------------------------------------------- recognition graph -> device plan

class RecognitionPlan:
    """What ``recognition_plan_from_onnx`` returns: a recognition network as device steps on a 112 x 112 aligned crop.

    steps    in execution order, dicts with ``op`` in
             ``input``   (out)                                       the crop as tensor 0, (3, 112, 112)
             ``conv``    (x, out, w, b, k, stride, pad, act, slope, res, f32)   w [Cout,Cin,k,k] / b [Cout] float64, BN folded;
                         act 0 none / 1 ReLU (never produced here) / 2 PReLU with ``slope`` [Cout]; ``res``: tensor id added
                         in front of the activation; ``f32``: the output is the embedding (the fully connected layer, k 1 on a 1 x 1 map)
             ``dwconv``  (the same keys; res None, f32 False)         depthwise: w [C,1,k,k]
    shapes   tensor id -> (C, H, W)
    output   tensor id of the embedding, shape (dim, 1, 1)
    macs2    2 x multiply-accumulates per face
    """

    def __init__(self, steps, shapes, output):
        self.steps, self.shapes, self.output = steps, shapes, output
        self.dim = shapes[output][0]
        self.macs2 = sum(2 * shapes[s["out"]][1] * shapes[s["out"]][2] * int(np.prod(s["w"].shape))
                         for s in steps if s["op"] in ("conv", "dwconv"))


def recognition_plan_from_onnx(path_or_graph):
    """Map a recognition graph built from convs, depthwise convs, PReLU and residual adds - insightface's MobileFaceNet
    (``w600k_mbf.onnx``) is the shape this is written for - onto device steps by following the data flow: widths and block
    counts are the graph's own.  One input [*,3,112,112], one output [*,512].  Raises ValueError naming the node and op it
    cannot map; a graph is mapped whole or not at all."""
    g = _fold_constant_views(path_or_graph if isinstance(path_or_graph, OnnxGraph) else read_onnx(path_or_graph))
    if len(g.inputs) != 1:
        raise ValueError(f"expected one graph input, found {g.inputs}")
    ishape = g.value_shapes.get(g.inputs[0])
    if ishape is not None and (len(ishape) != 4 or list(ishape[1:]) != [3, 112, 112]):
        raise ValueError(f"graph input {g.inputs[0]!r} of shape {ishape}: expected [*, 3, 112, 112]")
    consumers = {}
    for n in g.nodes:
        for t in n.inputs:
            if t:
                consumers.setdefault(t, []).append(n)
    host = g.initializers
    dev = {g.inputs[0]: 0}
    shapes = {0: (3, 112, 112)}
    steps = [{"op": "input", "out": 0}]
    producer = {}                        # tensor id -> its conv / dwconv step while more may be folded into it
    flat = {}                            # tensor name -> tensor id of the 1 x 1 map it flattens
    made_by = {}                         # tensor name -> node

    who = _who

    def sole(n, t):
        return len(consumers.get(t, [])) == 1 and consumers[t][0] is n

    def open_step(n, t):
        st = producer.get(dev.get(t))
        return st if st is not None and sole(n, t) else None

    def const(n, t, what):
        if t not in host:
            raise ValueError(f"{who(n)}: {what} is not an initialiser")
        return np.asarray(host[t], dtype=np.float64)

    def add_step(op, x, w, b, k, s, p, hw, f32=False):
        tid = len(shapes)
        shapes[tid] = (w.shape[0],) + hw
        st = {"op": op, "x": x, "out": tid, "w": w, "b": b, "k": k, "stride": s, "pad": p, "act": 0, "slope": None, "res": None,
              "f32": f32}
        steps.append(st)
        producer[tid] = st
        return st

    for n in g.nodes:
        ins = [t for t in n.inputs if t]
        if not n.outputs or not ins:
            raise ValueError(f"{who(n)}: node without inputs or outputs")
        out = n.outputs[0]
        for t in n.outputs:
            made_by[t] = n
        if n.op == "Conv":
            if ins[0] not in dev or len(ins) < 2:
                raise ValueError(f"{who(n)}: conv input is not a feature map")
            w = const(n, ins[1], "conv weight")
            c, h, wd = shapes[dev[ins[0]]]
            grp = n.attrs.get("group", 1)
            ks = list(n.attrs.get("kernel_shape", list(w.shape[2:])))
            st_, pd, dl = list(n.attrs.get("strides", [1, 1])), list(n.attrs.get("pads", [0, 0, 0, 0])), list(n.attrs.get("dilations", [1, 1]))
            if dl != [1, 1]:
                raise ValueError(f"{who(n)}: dilations {dl} are not supported")
            if len(pd) != 4 or len(set(pd)) != 1:
                raise ValueError(f"{who(n)}: pads {pd} are not symmetric")
            if w.ndim != 4 or len(ks) != 2 or ks[0] != ks[1] or list(w.shape[2:]) != ks or len(st_) != 2 or st_[0] != st_[1]:
                raise ValueError(f"{who(n)}: conv weight {w.shape} kernel {ks} strides {st_} is not a square 2-d conv")
            k, s, p = int(ks[0]), int(st_[0]), int(pd[0])
            if grp == 1:
                if w.shape[1] != c or k not in (1, 3) or s not in (1, 2) or p != k // 2:
                    raise ValueError(f"{who(n)}: conv weight {w.shape} kernel {k} stride {s} pad {p} on {c} channels is not a "
                                     "1x1 / 3x3, stride 1 / 2, pad k/2 conv of its input")
                op = "conv"
            else:
                if not (grp == c == w.shape[0] and w.shape[1] == 1):
                    raise ValueError(f"{who(n)}: grouped conv (group {grp} on {c} channels, weight {w.shape}) is not depthwise: not supported")
                if not ((k == 3 and p == 1 and s in (1, 2)) or (k == h == wd and p == 0 and k % 2 == 1 and k <= 7 and s in (1, 2))):
                    raise ValueError(f"{who(n)}: depthwise conv kernel {k} stride {s} pad {p} on a {h} x {wd} map is neither 3x3 / pad 1 / "
                                     "stride 1 | 2 nor the global form (kernel = map size <= 7, pad 0)")
                op = "dwconv"
            b = const(n, ins[2], "conv bias").reshape(-1) if len(ins) > 2 else np.zeros(w.shape[0])
            if b.shape != (w.shape[0],):
                raise ValueError(f"{who(n)}: conv bias of shape {b.shape} on {w.shape[0]} channels")
            dev[out] = add_step(op, dev[ins[0]], w, b, k, s, p, ((h + 2 * p - k) // s + 1, (wd + 2 * p - k) // s + 1))["out"]
        elif n.op == "BatchNormalization":
            st = open_step(n, ins[0]) if ins[0] in dev else None
            if st is None or st["act"] or st["res"] is not None or len(ins) != 5:
                raise ValueError(f"{who(n)}: BatchNormalization that does not directly follow a Conv or the fully connected layer")
            sc, bi, mu, var = (const(n, t, "BatchNormalization parameter").reshape(-1) for t in ins[1:5])
            if any(a.shape != (st["w"].shape[0],) for a in (sc, bi, mu, var)):
                raise ValueError(f"{who(n)}: BatchNormalization parameters of {sc.shape[0]} channels on {st['w'].shape[0]}")
            f = sc / np.sqrt(var + float(n.attrs.get("epsilon", 1e-5)))
            st["w"], st["b"] = st["w"] * f[:, None, None, None], (st["b"] - mu) * f + bi
            dev[out] = st["out"]
        elif n.op == "PRelu":
            st = open_step(n, ins[0]) if ins[0] in dev else None
            if st is None or st["act"] or st["f32"] or len(ins) != 2:
                raise ValueError(f"{who(n)}: PRelu that does not follow a Conv or a Conv + Add")
            sl = const(n, ins[1], "PRelu slope")
            C = st["w"].shape[0]
            if sl.shape not in ((C,), (C, 1, 1), (1, C, 1, 1)):
                raise ValueError(f"{who(n)}: PRelu slope of shape {sl.shape} on {C} channels (expected [C], [C,1,1] or [1,C,1,1])")
            if st["op"] == "dwconv" and st["res"] is not None:
                raise ValueError(f"{who(n)}: PRelu behind a residual add onto a depthwise conv")
            st["act"], st["slope"] = 2, sl.reshape(-1)
            dev[out] = st["out"]
        elif n.op == "Add":
            if len(ins) != 2:
                raise ValueError(f"{who(n)}: Add of {len(ins)} tensors")
            hs, ds = [t for t in ins if t in host], [t for t in ins if t in dev]
            if len(hs) == 1 and len(ds) == 1:                          # MatMul + Add: the fully connected layer's bias
                st = open_step(n, ds[0])
                bv = np.asarray(host[hs[0]], dtype=np.float64).reshape(-1)
                if st is None or not st["f32"] or st.get("gemm") != "MatMul" or bv.shape != st["b"].shape:
                    raise ValueError(f"{who(n)}: Add of a constant that is not the bias of a MatMul")
                st["b"], st["gemm"] = st["b"] + bv, "MatMul+Add"
                dev[out] = st["out"]
                continue
            if len(ds) != 2:
                raise ValueError(f"{who(n)}: Add of something that is not a feature map")
            a, b = dev[ins[0]], dev[ins[1]]
            if shapes[a] != shapes[b] or a == b:
                raise ValueError(f"{who(n)}: Add of maps of shapes {shapes[a]} and {shapes[b]}" + (" (one map with itself)" if a == b else ""))
            # the conv that runs LAST takes the other map as its residual, in front of its activation
            made = {s["out"]: i for i, s in enumerate(steps)}
            cand = [(made[st["out"]], st, o) for t, o in ((ins[0], b), (ins[1], a))
                    for st in [open_step(n, t)] if st is not None and st["op"] == "conv" and not st["act"] and st["res"] is None
                    and not st["f32"] and made[st["out"]] > made[o]]
            if not cand:
                raise ValueError(f"{who(n)}: Add whose later input does not come straight out of a linear 1x1 / 3x3 conv (no residual to fuse)")
            _, st, o = max(cand, key=lambda c: c[0])
            st["res"] = o
            producer.pop(o, None)
            dev[out] = st["out"]
        elif n.op in ("Flatten", "Reshape"):
            tid = dev.get(ins[0])
            if tid is None or shapes[tid][1:] != (1, 1):
                raise ValueError(f"{who(n)}: {n.op} of something that is not a 1 x 1 map")
            if n.op == "Flatten" and n.attrs.get("axis", 1) != 1:
                raise ValueError(f"{who(n)}: Flatten along axis {n.attrs['axis']}")
            if n.op == "Reshape":
                tgt = [int(v) for v in np.ravel(const(n, ins[1], "Reshape target"))] if len(ins) > 1 else []
                if len(tgt) != 2 or tgt[1] not in (-1, shapes[tid][0]) or tgt[0] not in (-1, 0, 1) or tgt == [-1, -1]:
                    raise ValueError(f"{who(n)}: Reshape target {tgt} does not flatten a {shapes[tid]} map to [N, {shapes[tid][0]}]")
            producer.pop(tid, None)
            flat[out] = tid
        elif n.op in ("Gemm", "MatMul"):
            tid = flat.get(ins[0])
            if tid is None or len(ins) < 2:
                raise ValueError(f"{who(n)}: {n.op} that does not read a flattened 1 x 1 map")
            w = const(n, ins[1], "fully connected weight")
            if n.op == "Gemm":
                if n.attrs.get("alpha", 1.0) != 1.0 or n.attrs.get("beta", 1.0) != 1.0 or n.attrs.get("transA", 0):
                    raise ValueError(f"{who(n)}: Gemm with alpha / beta / transA other than 1 / 1 / 0")
                if not n.attrs.get("transB", 0):
                    w = w.T
            else:
                w = w.T
            c = shapes[tid][0]
            if w.ndim != 2 or w.shape[1] != c:
                raise ValueError(f"{who(n)}: fully connected weight {w.shape} on {c} features")
            b = const(n, ins[2], "Gemm bias").reshape(-1) if n.op == "Gemm" and len(ins) > 2 else np.zeros(w.shape[0])
            if b.shape != (w.shape[0],):
                raise ValueError(f"{who(n)}: Gemm bias of shape {b.shape} on {w.shape[0]} outputs")
            st = add_step("conv", tid, np.ascontiguousarray(w)[:, :, None, None], b, 1, 1, 0, (1, 1), f32=True)
            st["gemm"] = n.op
            dev[out] = st["out"]
        else:
            raise ValueError(f"{who(n)}: op {n.op} is not supported")

    produced = [t for n in g.nodes for t in n.outputs]
    outs = list(g.outputs) if g.outputs else [t for t in produced if t not in consumers]
    if len(outs) != 1:
        desc = ", ".join(f"{t!r} of {who(made_by[t])}" if t in made_by else repr(t) for t in outs)
        raise ValueError(f"expected one graph output (the embedding), found {len(outs)}: {desc}")
    tid = dev.get(outs[0])
    st = producer.get(tid)
    if st is None or not st["f32"] or st["res"] is not None:
        raise ValueError(f"graph output {outs[0]!r} does not come out of the fully connected layer")
    oshape = g.value_shapes.get(outs[0])
    if shapes[tid][0] != 512 or (oshape is not None and (len(oshape) != 2 or oshape[1] != 512)):
        raise ValueError(f"graph output {outs[0]!r}: embedding of {shapes[tid][0]} dimensions (declared {oshape}), expected [*, 512]")
    used = {s[k] for s in steps for k in ("x", "res") if s.get(k) is not None} | {tid}
    for s in steps:
        if s["out"] not in used:
            raise ValueError(f"a {s['op']} step's result (tensor {s['out']}, shape {shapes[s['out']]}) feeds nothing: not a recognition network")
    return RecognitionPlan(steps, shapes, tid)
