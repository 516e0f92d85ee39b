"""CPU restatement of the SCRFD detector, written from the ONNX operator semantics: the definition the HIP kernels and
scrfd.py are tested against (it imports neither).

  r64_graph   float64 forward of the RAW graph (every node interpreted, shape arithmetic included)
  run_plan    forward of an import plan (folded weights, fused steps): mode 'r64' float64; mode 'e16' float32 with the
              weights and every stored activation rounded to f16 and the nine head maps left in f32
  decode_nms  decode + NMS in NumPy float32, one IEEE rounding per operation, as the issue / DESIGN.md 4.3b state it
"""
import numpy as np
import torch
import torch.nn.functional as F

from facerecognition_infrenceengine_amd import onnx_import


def blob(canvas):
    """uint8 [N,H,W,3] BGR -> float64 NCHW RGB, (x - 127.5) / 128"""
    x = torch.from_numpy(np.ascontiguousarray(canvas[..., ::-1])).to(torch.float64)
    return ((x - 127.5) / 128.0).permute(0, 3, 1, 2).contiguous()


def _t(v):
    return torch.from_numpy(np.asarray(v, dtype=np.float64))


def r64_graph(graph, canvas):
    """-> {output name: float64 array [N, H*W*A, K]} (scores as PROBABILITIES, as the graph computes them)"""
    g = graph if isinstance(graph, onnx_import.OnnxGraph) else onnx_import.read_onnx(graph)
    val = {k: v for k, v in g.initializers.items()}
    val[g.inputs[0]] = blob(canvas)
    used = set()
    for n in g.nodes:
        used.update(n.inputs)
        a = [val[t] if t else None for t in n.inputs]
        at, op = n.attrs, n.op
        if op == "Conv":
            r = F.conv2d(a[0], _t(a[1]), _t(a[2]) if len(a) > 2 else None, stride=at.get("strides", [1, 1]),
                         padding=at["pads"][:2], groups=at.get("group", 1))
        elif op == "BatchNormalization":
            s, b, m, v = (_t(x).reshape(1, -1, 1, 1) for x in a[1:5])
            r = (a[0] - m) / torch.sqrt(v + at.get("epsilon", 1e-5)) * s + b
        elif op == "Relu":
            r = torch.relu(a[0])
        elif op == "Sigmoid":
            r = torch.sigmoid(a[0])
        elif op in ("Add", "Mul") and any(torch.is_tensor(x) for x in a):
            x, y = (x if torch.is_tensor(x) else _t(x) for x in a)
            r = x + y if op == "Add" else x * y
        elif op == "MaxPool":
            r = F.max_pool2d(a[0], at["kernel_shape"], at["strides"], at["pads"][:2], ceil_mode=bool(at.get("ceil_mode", 0)))
        elif op == "AveragePool":
            r = F.avg_pool2d(a[0], at["kernel_shape"], at["strides"], at["pads"][:2], ceil_mode=bool(at.get("ceil_mode", 0)),
                             count_include_pad=bool(at.get("count_include_pad", 0)))
        elif op == "Resize":
            if len(a) > 3 and a[3] is not None:
                size = [int(v) for v in np.ravel(a[3])][2:]
            else:
                size = [int(a[0].shape[2] * float(np.ravel(a[2])[2])), int(a[0].shape[3] * float(np.ravel(a[2])[3]))]
            iy = torch.arange(size[0]) * a[0].shape[2] // size[0]        # nearest, asymmetric / floor (= half_pixel / round_prefer_floor at x2)
            ix = torch.arange(size[1]) * a[0].shape[3] // size[1]
            r = a[0][:, :, iy][:, :, :, ix]
        elif op == "Transpose":
            r = a[0].permute(*at["perm"]).contiguous()
        elif op == "Reshape":
            r = a[0].reshape([int(v) if v != 1 or i else a[0].shape[0] for i, v in enumerate(np.ravel(a[1]))])
        elif op == "Shape":
            r = np.array(a[0].shape, dtype=np.int64)
            r[0] = 1
        elif op == "Gather":
            r = np.take(a[0], np.asarray(a[1]).astype(np.int64), axis=at.get("axis", 0))
        elif op == "Slice":
            r = np.asarray(a[0])[int(np.ravel(a[1])[0]):int(np.ravel(a[2])[0])]
        elif op == "Concat":
            r = np.concatenate([np.atleast_1d(x) for x in a], axis=at.get("axis", 0))
        elif op == "Unsqueeze":
            r = np.expand_dims(np.asarray(a[0]), at["axes"][0])
        elif op == "Cast":
            r = np.asarray(a[0]).astype({1: np.float32, 7: np.int64}[at["to"]])
        elif op == "Floor":
            r = np.floor(a[0])
        elif op in ("Add", "Mul"):
            r = np.add(*a) if op == "Add" else np.multiply(*a)
        else:
            raise NotImplementedError(op)
        val[n.outputs[0]] = r
    outs = [t for n in g.nodes for t in n.outputs if t not in used]
    return {t: val[t].numpy() for t in outs if torch.is_tensor(val[t])}


def _f16(x):
    return x.to(torch.float16).to(x.dtype)


def run_plan(plan, canvas, mode="r64"):
    """-> three dicts (stride, score = LOGITS [N,H*W*A], bbox [N,H*W*A,4], kps [N,H*W*A,10]), float64 ('r64') or float32 ('e16')"""
    e16 = mode == "e16"
    dt = torch.float32 if e16 else torch.float64
    t = {}
    for s in plan.steps:
        if s["op"] == "input":
            t[s["out"]] = blob(canvas).to(dt)                                 # exact in f16
        elif s["op"] == "conv":
            w, b = torch.from_numpy(s["w"]).to(dt), torch.from_numpy(s["b"]).to(dt)
            y = F.conv2d(t[s["x"]], _f16(w) if e16 else w, None, stride=s["stride"], padding=s["pad"]) + b.reshape(1, -1, 1, 1)
            if s["res"] is not None:
                y = y + t[s["res"]]
            if s["relu"]:
                y = torch.relu(y)
            t[s["out"]] = _f16(y) if e16 and not s["f32"] else y
        elif s["op"] == "pool":
            x = t[s["x"]].to(torch.float64)
            h, w = plan.shapes[s["out"]][1:]
            # taps outside the input do not count: pad by hand so that ceil-mode overhang is covered too
            ph = (h - 1) * s["stride"] + s["k"] - x.shape[2] - s["pad"]
            pw = (w - 1) * s["stride"] + s["k"] - x.shape[3] - s["pad"]
            if s["kind"] == 0:
                y = F.max_pool2d(F.pad(x, (s["pad"], max(pw, 0), s["pad"], max(ph, 0)), value=-float("inf")), s["k"], s["stride"])
            else:
                one = F.pad(torch.ones_like(x), (s["pad"], max(pw, 0), s["pad"], max(ph, 0)))
                xs = F.pad(x, (s["pad"], max(pw, 0), s["pad"], max(ph, 0)))
                y = F.avg_pool2d(xs, s["k"], s["stride"]) / F.avg_pool2d(one, s["k"], s["stride"])
            y = y[:, :, :h, :w].to(dt)
            t[s["out"]] = _f16(y) if e16 else y
        elif s["op"] == "upadd":
            c = t[s["coarse"]]
            if s["up"] == 2:
                c = c.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
            y = t[s["lateral"]] + c
            t[s["out"]] = _f16(y) if e16 else y
    levels = []
    for lv in plan.levels:
        d = {"stride": lv["stride"]}
        for kind, k in (("score", 1), ("bbox", 4), ("kps", 10)):
            m = t[lv[kind]].permute(0, 2, 3, 1).contiguous().numpy()
            d[kind] = m.reshape(m.shape[0], -1) if k == 1 else m.reshape(m.shape[0], -1, k)
        levels.append(d)
    return levels


def logit_threshold(t):
    """f32 of log(t / (1 - t)) computed in float64"""
    return np.float32(np.log(np.float64(t) / (1.0 - np.float64(t))))


def decode_level(score, bbox, kps, hw, A, stride, logit_thr, det_scale, cap):
    """One frame, one level, NumPy float32: anchors with logit >= logit_thr in raster / anchor order, first ``cap``."""
    f = np.float32
    score, bbox, kps = score.astype(f), bbox.astype(f), kps.astype(f)
    idx = np.nonzero(score >= f(logit_thr))[0][:cap]
    cell = idx // A
    cx = ((cell % hw[1]) * stride).astype(f)
    cy = ((cell // hw[1]) * stride).astype(f)
    s, ds = f(stride), f(det_scale)
    d, k = bbox[idx], kps[idx]
    boxes = np.stack([(cx - d[:, 0] * s) / ds, (cy - d[:, 1] * s) / ds, (cx + d[:, 2] * s) / ds, (cy + d[:, 3] * s) / ds], axis=1)
    pts = np.empty((len(idx), 10), dtype=f)
    for i in range(5):
        pts[:, 2 * i] = (cx + k[:, 2 * i] * s) / ds
        pts[:, 2 * i + 1] = (cy + k[:, 2 * i + 1] * s) / ds
    sc = f(1.0) / (f(1.0) + np.exp(-score[idx]).astype(f))
    return boxes.astype(f), sc.astype(f), pts


def iou_plus1(a, b):
    """IoU of two float32 boxes with the +1 area convention, float32 operation by operation"""
    f = np.float32
    aa = (a[2] - a[0] + f(1)) * (a[3] - a[1] + f(1))
    ab = (b[2] - b[0] + f(1)) * (b[3] - b[1] + f(1))
    w = max(f(0), min(a[2], b[2]) - max(a[0], b[0]) + f(1))
    h = max(f(0), min(a[3], b[3]) - max(a[1], b[1]) + f(1))
    inter = f(w) * f(h)
    return inter / (aa + ab - inter)


def decode_nms(levels, frame, A, canvas_hw, det_thresh, nms_thresh, det_scale, cap, cap_out, pairs=None, strides=None):
    """levels: run_plan's result (or the GPU's head maps in that form).  -> boxes [n,4], scores [n], kps [n,5,2], float32,
    in score order (ties by slot: level, then position in the level's list).  ``pairs``: a list that receives every IoU the
    greedy pass evaluated; ``strides``: a list that receives, per kept detection, the stride of the level it came from."""
    f = np.float32
    thr = logit_threshold(det_thresh)
    B, S, K, L = [], [], [], []
    for lv in levels:
        s = lv["stride"]
        b, sc, k = decode_level(lv["score"][frame], lv["bbox"][frame], lv["kps"][frame], (canvas_hw[0] // s, canvas_hw[1] // s), A,
                                s, thr, det_scale, cap)
        B.append(b), S.append(sc), K.append(k), L.append(np.full(len(sc), s, dtype=np.int64))
    B, S, K, L = np.concatenate(B), np.concatenate(S), np.concatenate(K), np.concatenate(L)
    order = np.argsort(-S.astype(np.float64), kind="stable")
    keep, alive = [], np.ones(len(order), dtype=bool)
    for oi, i in enumerate(order):
        if not alive[oi]:
            continue
        keep.append(i)
        if len(keep) == cap_out:
            break
        for oj in range(oi + 1, len(order)):
            if alive[oj]:
                v = iou_plus1(B[i], B[order[oj]])
                if pairs is not None:
                    pairs.append(float(v))
                if v > f(nms_thresh):
                    alive[oj] = False
    keep = np.asarray(keep, dtype=np.int64)
    if strides is not None:
        strides.extend(L[keep].tolist())
    return B[keep], S[keep], K[keep].reshape(-1, 5, 2)


def reference_decides(levels, frame, A, canvas_hw, det_thresh, nms_thresh, det_scale, cap, cap_out, logit_tol, iou_tol=1e-3):
    """-> (clear, boxes, scores, kps, strides): strides int64 [n], each detection's level; ``clear`` is False when, in these reference head maps alone, an anchor's logit lies
    within ``logit_tol`` of the threshold or an IoU the greedy pass evaluated lies within ``iou_tol`` of ``nms_thresh`` - a
    frame whose detections a rounding-sized difference could change."""
    thr = np.float64(logit_threshold(det_thresh))
    near = any((np.abs(lv["score"][frame] - thr) <= logit_tol).any() for lv in levels)
    pairs, strides = [], []
    b, s, k = decode_nms(levels, frame, A, canvas_hw, det_thresh, nms_thresh, det_scale, cap, cap_out, pairs=pairs, strides=strides)
    return not near and not any(abs(p - nms_thresh) <= iou_tol for p in pairs), b, s, k, np.asarray(strides, dtype=np.int64)
