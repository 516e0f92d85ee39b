"""CPU restatement of a plan recogniser (MobileFaceNet), written from the ONNX operator semantics: the definition
fr_dw_conv_f16, fr_det_conv_act_f16 and mbf.py are tested against (it imports none of them).

  r64_graph   float64 forward of the RAW graph, node by node
  run_plan    forward of an import plan (folded weights, fused steps): mode 'r64' float64; mode 'e16' float32 with the weights
              and every stored activation rounded to f16 and the embedding left in f32
  run_scrfd_plan   scrfd_ref.run_plan for a detector plan that holds depthwise steps
  dw_ref      one depthwise layer in float64 with the sum of |products| beside it (the kernel test's tolerance)
"""
import numpy as np
import torch
import torch.nn.functional as F

from facerecognition_infrenceengine_amd import onnx_import


def seeded_crops(n, seed=0):
    """f16 [n,112,112,8] in the warp's format: smooth RGB (v - 127.5) / 127.5 in channels 0..2, zeros in 3..7"""
    g = torch.Generator().manual_seed(seed)
    z = torch.rand((n, 3, 7, 7), generator=g, dtype=torch.float64)
    x = F.interpolate(z, size=(112, 112), mode="bilinear", align_corners=False) + 0.05 * torch.rand((n, 3, 112, 112), generator=g, dtype=torch.float64)
    x = ((x.clamp(0, 1) * 255.0).round() - 127.5) / 127.5
    out = torch.zeros((n, 112, 112, 8), dtype=torch.float16)
    out[..., :3] = x.permute(0, 2, 3, 1).to(torch.float16)
    return out


def blob(crops):
    """f16 [N,112,112,8] (tensor or array) -> float64 NCHW [N,3,112,112]"""
    x = crops if torch.is_tensor(crops) else torch.from_numpy(np.asarray(crops))
    return x[..., :3].to(torch.float64).permute(0, 3, 1, 2).contiguous()


def _t(v):
    return torch.from_numpy(np.asarray(v, dtype=np.float64))


def r64_graph(graph, crops):
    """-> float64 array [N, 512]"""
    g = graph if isinstance(graph, onnx_import.OnnxGraph) else onnx_import.read_onnx(graph)
    val = {g.inputs[0]: blob(crops)}
    out = None
    for n in g.nodes:
        a = [val[t] if t in val else _t(g.initializers[t]) for t in n.inputs]
        at, op = n.attrs, n.op
        if op == "Conv":
            r = F.conv2d(a[0], a[1], a[2] if len(a) > 2 else None, stride=at.get("strides", [1, 1]), padding=at["pads"][:2],
                         dilation=at.get("dilations", [1, 1]), groups=at.get("group", 1))
        elif op == "BatchNormalization":
            shp = (1, -1, 1, 1) if a[0].dim() == 4 else (1, -1)
            s, b, m, v = (x.reshape(shp) for x in a[1:5])
            r = (a[0] - m) / torch.sqrt(v + at.get("epsilon", 1e-5)) * s + b
        elif op == "PRelu":
            sl = a[1].reshape(1, -1, 1, 1)
            r = torch.where(a[0] < 0, a[0] * sl, a[0])
        elif op == "Add":
            r = a[0] + a[1]
        elif op in ("Flatten", "Reshape"):
            r = a[0].reshape(a[0].shape[0], -1)
        elif op == "Gemm":
            r = a[0] @ (a[1].T if at.get("transB", 0) else a[1]) + a[2]
        elif op == "MatMul":
            r = a[0] @ a[1]
        else:
            raise NotImplementedError(op)
        val[n.outputs[0]] = out = r
    return out.numpy()


def _f16(x):
    return x.to(torch.float16).to(x.dtype)


def run_plan(plan, crops, mode="r64"):
    """-> the embedding [N,512], float64 ('r64') or float32 ('e16')"""
    e16 = mode == "e16"
    dt = torch.float32 if e16 else torch.float64
    t = {}
    for s in plan.steps:
        if s["op"] == "input":
            t[s["out"]] = blob(crops).to(dt)                                   # the crop is f16 already
            continue
        w, b = torch.from_numpy(s["w"]).to(dt), torch.from_numpy(s["b"]).to(dt)
        y = F.conv2d(t[s["x"]], _f16(w) if e16 else w, None, stride=s["stride"], padding=s["pad"],
                     groups=w.shape[0] if s["op"] == "dwconv" else 1) + b.reshape(1, -1, 1, 1)
        if s["res"] is not None:
            y = y + t[s["res"]]
        if s["act"] == 2:
            y = torch.where(y < 0, y * torch.from_numpy(s["slope"]).to(dt).reshape(1, -1, 1, 1), y)
        elif s["act"] == 1:
            y = torch.relu(y)
        t[s["out"]] = _f16(y) if e16 and not s["f32"] else y
    return t[plan.output].reshape(-1, plan.dim).numpy()


def dw_ref(x, w, bias, slope, K, stride, pad, act):
    """x f16 [N,H,W,C], w f16 [K*K,C], bias / slope f32 [C] -> (y float64 [N,Ho,Wo,C] before the f16 rounding,
    A = sum |x * w| + |bias| float64, same shape), zero padding"""
    xd = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2)
    C = x.shape[3]
    wd = torch.from_numpy(w.astype(np.float64)).T.reshape(C, 1, K, K)
    bd = torch.from_numpy(bias.astype(np.float64))
    y = F.conv2d(xd, wd, bd, stride=stride, padding=pad, groups=C)
    A = F.conv2d(xd.abs(), wd.abs(), bd.abs(), stride=stride, padding=pad, groups=C)
    if act == 1:
        y = torch.relu(y)
    elif act == 2:
        y = torch.where(y < 0, y * torch.from_numpy(slope.astype(np.float64)).reshape(1, -1, 1, 1), y)
    return y.permute(0, 2, 3, 1).contiguous().numpy(), A.permute(0, 2, 3, 1).contiguous().numpy()


def conv_ref(x, w, bias, slope, res, stride, pad, act):
    """x f16 [N,H,W,Cin], w [Cout,Cin,k,k] holding f16 values, bias / slope [Cout], res f16 [N,Ho,Wo,Cout] or None ->
    (y float64 [N,Ho,Wo,Cout] before the output rounding, A = sum |x * w| + |bias| + |res|)"""
    xd = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2)
    wd = torch.from_numpy(np.asarray(w, dtype=np.float64))
    bd = torch.from_numpy(np.asarray(bias, dtype=np.float64))
    y = F.conv2d(xd, wd, bd, stride=stride, padding=pad)
    A = F.conv2d(xd.abs(), wd.abs(), bd.abs(), stride=stride, padding=pad)
    if res is not None:
        r = torch.from_numpy(res.astype(np.float64)).permute(0, 3, 1, 2)
        y, A = y + r, A + r.abs()
    if act == 1:
        y = torch.relu(y)
    elif act == 2:
        y = torch.where(y < 0, y * torch.from_numpy(np.asarray(slope, dtype=np.float64)).reshape(1, -1, 1, 1), y)
    return y.permute(0, 2, 3, 1).contiguous().numpy(), A.permute(0, 2, 3, 1).contiguous().numpy()


def run_scrfd_plan(plan, canvas, mode="r64"):
    """scrfd_ref.run_plan on a plan with ``dwconv`` steps: each is handed over as the dense conv with the same value (weight
    [C,C,3,3], zero off the diagonal - the added products are exact zeros)."""
    import copy
    from tests.helpers import scrfd_ref
    dense = copy.copy(plan)
    dense.steps = []
    for s in plan.steps:
        if s["op"] == "dwconv":
            C = s["w"].shape[0]
            w = np.zeros((C, C) + s["w"].shape[2:], dtype=np.float64)
            w[np.arange(C), np.arange(C)] = s["w"][:, 0]
            s = dict(s, op="conv", w=w)
        dense.steps.append(s)
    return scrfd_ref.run_plan(dense, canvas, mode)
