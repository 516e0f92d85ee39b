"""SCRFD detector on HIP: the ``det_10g.onnx`` of an insightface model pack as ``FaceAnalysis``'s detector.

``onnx_import.scrfd_plan_from_onnx`` turns the graph into device steps for one canvas size; ``SCRFDHIP`` packs the
folded weights once (head weights the graph shares across strides are packed once), keeps one activation arena per
(thread, stream, batch size, canvas size) - the ``MAX_ARENAS`` most recently used of a thread - and walks the steps with the fr_det_* kernels, then fr_scrfd_decode per level and
fr_sort_nms per frame - all on the current stream, no host synchronisation.
"""
import threading

import numpy as np
import torch

from . import _lib
from .onnx_import import OnnxGraph, read_onnx, scrfd_plan_from_onnx


MAX_ARENAS = 8          # activation arenas kept per thread: the most recently used (batch size, canvas size, stream) keys


def _ceil(x, m):
    return (x + m - 1) // m * m


def logit_threshold(t):
    """f32 of log(t / (1 - t)), computed in float64: score >= t as a comparison of logits"""
    t = np.float64(t)
    if not 0.0 < t < 1.0:
        raise ValueError(f"det_thresh {t} must lie strictly between 0 and 1")
    return float(np.float32(np.log(t / (1.0 - t))))


def pack_conv(w, b):
    """w [Cout,Cin,k,k], b [Cout] (any float dtype) -> (f16 array in fr_det_conv_f16's layout [steps][cout_packed][4][8],
    f32 bias [cout_packed], Cin padded to 8, cout_packed)."""
    w = np.asarray(w, dtype=np.float64)
    cout, cin, k, _ = w.shape
    cin_p, cout_w = _ceil(cin, 8), _ceil(cout, 16)
    wp = np.zeros((cout_w, k * k, cin_p), dtype=np.float64)
    wp[:cout, :, :cin] = w.transpose(0, 2, 3, 1).reshape(cout, k * k, cin)
    G = k * k * cin_p // 8
    steps = (G + 3) // 4
    grp = np.zeros((steps * 4, cout_w, 8), dtype=np.float64)
    grp[:G] = wp.reshape(cout_w, G, 8).transpose(1, 0, 2)
    packed = np.ascontiguousarray(grp.reshape(steps, 4, cout_w, 8).transpose(0, 2, 1, 3)).astype(np.float16)
    bias = np.zeros(cout_w, dtype=np.float32)
    bias[:cout] = np.asarray(b, dtype=np.float64).reshape(-1)
    return packed, bias, cin_p, cout_w


def pack_dw(w, b, slope=None):
    """w [C,1,k,k], b [C], slope [C] or None -> (f16 [k*k][Cp] tap-major as fr_dw_conv_f16 reads it, f32 bias [Cp], f32 slope
    [Cp] or None, Cp = C padded to 8 with zeros)"""
    w = np.asarray(w, dtype=np.float64)
    c, _, k, _ = w.shape
    cp = _ceil(c, 8)
    wp = np.zeros((k * k, cp), dtype=np.float64)
    wp[:, :c] = w.reshape(c, k * k).T
    bias = np.zeros(cp, dtype=np.float32)
    bias[:c] = np.asarray(b, dtype=np.float64).reshape(-1)
    sl = None
    if slope is not None:
        sl = np.zeros(cp, dtype=np.float32)
        sl[:c] = np.asarray(slope, dtype=np.float64).reshape(-1)
    return wp.astype(np.float16), bias, sl, cp


class _Arena:
    """The activation buffers of one plan at one batch size, and the launch list that fills them."""

    def __init__(self, det, plan, N):
        dev, lib = det.device, det.lib
        self.N, self.plan = N, plan
        last = {}
        for i, s in enumerate(plan.steps):
            for key in ("x", "res", "coarse", "lateral"):
                if s.get(key) is not None:
                    last[s[key]] = i
        heads = {lv[k] for lv in plan.levels for k in ("score", "bbox", "kps")}
        f32 = {s["out"] for s in plan.steps if s.get("f32")}
        free, self.buf, self.blocks = [], {}, []

        def take(tid):
            c, h, w = plan.shapes[tid]
            nbytes = N * h * w * (c * 4 if tid in f32 else _ceil(c, 8) * 2)
            fit = [j for j, b in enumerate(free) if b.numel() >= nbytes]
            if fit:
                b = free.pop(min(fit, key=lambda j: free[j].numel()))
            else:
                b = torch.empty(_ceil(nbytes, 256), dtype=torch.uint8, device=dev)
                self.blocks.append(b)
            self.buf[tid] = b

        self.calls = []
        for i, s in enumerate(plan.steps):
            take(s["out"])
            out = self.buf[s["out"]]
            c, h, w = plan.shapes[s["out"]]
            if s["op"] == "input":
                self.input = out
            elif s["op"] == "conv":
                ci, hi, wi = plan.shapes[s["x"]]
                wt, bias, cin_p, cout_w = det.packed[s["wkey"]]
                assert cin_p == _ceil(ci, 8)
                cs, ldo = (c, c) if s["f32"] else (_ceil(c, 8), _ceil(c, 8))
                res = self.buf[s["res"]] if s["res"] is not None else None
                self.calls.append((lib.fr_det_conv_f16, (_lib.ptr(self.buf[s["x"]]), _lib.ptr(wt), _lib.ptr(bias), _lib.ptr(res), _lib.ptr(out),
                                                         N, hi, wi, cin_p, cout_w, s["k"], s["stride"], s["pad"], h, w, cs, ldo,
                                                         int(s["relu"]), int(s["f32"]), 0)))
            elif s["op"] == "dwconv":
                ci, hi, wi = plan.shapes[s["x"]]
                wt, bias, cp = det.packed[s["wkey"]]
                assert cp == _ceil(ci, 8) == _ceil(c, 8)
                self.calls.append((lib.fr_dw_conv_f16, (_lib.ptr(self.buf[s["x"]]), _lib.ptr(wt), _lib.ptr(bias), None, _lib.ptr(out), N, hi, wi,
                                                        cp, s["k"], s["stride"], s["pad"], h, w, int(s["relu"]))))
            elif s["op"] == "pool":
                ci, hi, wi = plan.shapes[s["x"]]
                self.calls.append((lib.fr_det_pool_f16, (_lib.ptr(self.buf[s["x"]]), _lib.ptr(out), N, hi, wi, _ceil(ci, 8), h, w, s["kind"],
                                                         s["k"], s["stride"], s["pad"])))
            elif s["op"] == "upadd":
                self.calls.append((lib.fr_det_upsample_add_f16, (_lib.ptr(self.buf[s["coarse"]]), _lib.ptr(self.buf[s["lateral"]]),
                                                                 _lib.ptr(out), N, h, w, _ceil(c, 8), s["up"])))
            for key in ("x", "res", "coarse", "lateral"):
                t = s.get(key)
                if t is not None and last.get(t) == i and t not in heads and all(b is not self.buf[t] for b in free):
                    free.append(self.buf[t])
        cap = det.cap
        self.cb = torch.empty((N, 3, cap, 4), dtype=torch.float32, device=dev)
        self.cs = torch.empty((N, 3, cap), dtype=torch.float32, device=dev)
        self.ca = torch.empty((N, 3, cap, 10), dtype=torch.float32, device=dev)
        self.cc = torch.empty((N * 3,), dtype=torch.int32, device=dev)

    def head(self, tid):
        """a head map as an f32 tensor [N, H*W*C] (a view of the arena: valid until the next call on this arena)"""
        c, h, w = self.plan.shapes[tid]
        return self.buf[tid][:self.N * h * w * c * 4].view(torch.float32).view(self.N, h * w * c)


class SCRFDHIP:
    """``detect_batch(canvas u8 [N,dh,dw,3] BGR, det_scale f32 [N]) -> boxes [N,cap_out,4], scores [N,cap_out],
    kps [N,cap_out,5,2], counts i32 [N]``: FRAME pixels (canvas pixels / det_scale), descending score, device tensors on
    the current stream, no host sync.  ``cap``: candidates kept per level and frame in front of NMS (raster order; 3 * cap <=
    4096); ``cap_out``: faces per frame.  ``share``: another SCRFDHIP of the same graph and device whose packed weights
    are used (``FaceAnalysis.clone_with``).

    Memory: one activation arena is kept per (thread, stream, batch size N, canvas size), the ``MAX_ARENAS`` most recently
    used of each thread (a gated camera turn brings any N from 1 to the camera count: DESIGN.md 4.5c); an arena grows with
    N - several hundred MB at N = 64 on 640 x 640.  A dropped arena's blocks return to torch's allocator, which hands them
    out again only behind the work already queued on them; no path of this package captures ``detect_batch`` in a graph (an
    engine with a detection canvas runs eagerly), and a caller that does keeps the capture's own memory pool alive."""

    def __init__(self, path_or_graph, device="cuda:0", det_thresh=0.5, nms_thresh=0.4, cap=1024, cap_out=16, share=None):
        _lib.require_gpu()
        self.lib = _lib.load()
        self.device = torch.device(device)
        if not (0 < cap and 3 * cap <= 4096 and 0 < cap_out <= 1024):
            raise ValueError(f"SCRFDHIP: cap {cap} must lie in 1 .. 1365 (3 * cap <= 4096: one fr_sort_nms segment per level) and "
                             f"cap_out {cap_out} in 1 .. 1024")
        self.graph = path_or_graph if isinstance(path_or_graph, OnnxGraph) else read_onnx(path_or_graph)
        self.det_thresh, self.nms_thresh, self.cap, self.cap_out = float(det_thresh), float(nms_thresh), int(cap), int(cap_out)
        self.cap_o = self.cap_out                       # the name FaceAnalysis's graph replay reads
        self.logit_thr = logit_threshold(det_thresh)
        # plans and packed weights depend on the graph alone: detectors that share them share the lock that guards them
        self._plans, self.packed, self._plan_lock = ({}, {}, threading.Lock()) if share is None else (share._plans, share.packed, share._plan_lock)
        self._tls = threading.local()                   # per-thread arenas: detect_batch is re-entrant across threads
        self.plan((640, 640))                           # refuses a graph that is no SCRFD detector here, not at the first frame

    def plan(self, canvas_hw):
        """the plan for a canvas size (height, width), built once; its weights packed and uploaded once per distinct conv"""
        key = (int(canvas_hw[0]), int(canvas_hw[1]))
        with self._plan_lock:
            p = self._plans.get(key)
            if p is None:
                p = scrfd_plan_from_onnx(self.graph, key)
                for s in p.steps:
                    if s["op"] == "conv" and s["wkey"] not in self.packed:
                        wt, bias, cin_p, cout_w = pack_conv(s["w"], s["b"])
                        self.packed[s["wkey"]] = (torch.from_numpy(wt).to(self.device), torch.from_numpy(bias).to(self.device), cin_p, cout_w)
                    elif s["op"] == "dwconv" and s["wkey"] not in self.packed:
                        wt, bias, _, cp = pack_dw(s["w"], s["b"])
                        self.packed[s["wkey"]] = (torch.from_numpy(wt).to(self.device), torch.from_numpy(bias).to(self.device), cp)
                self._plans[key] = p
            return p

    def _arena(self, N, hw):
        arenas = self._tls.__dict__.setdefault("arenas", {})
        key = (N, hw, torch.cuda.current_stream(self.device).cuda_stream)
        a = arenas.pop(key, None)
        if a is None:
            # a gated camera turn (activity.ActivityGate) brings any frame count from 1 to the camera count: keep the
            # MAX_ARENAS most recently used (a dropped arena's blocks go back to the allocator behind the work queued on them)
            while len(arenas) >= MAX_ARENAS:
                arenas.pop(next(iter(arenas)))
            a = _Arena(self, self.plan(hw), N)
        arenas[key] = a                                 # most recently used last
        return a

    def forward_heads(self, canvas):
        """The nine head maps of ``canvas``: (arena, [(stride, score [N,HW*A], bbox [N,HW*A*4], kps [N,HW*A*10]) per level]),
        f32 views of the arena (logits, distances and offsets in units of the stride)."""
        if not (torch.is_tensor(canvas) and canvas.dtype == torch.uint8 and canvas.dim() == 4 and canvas.shape[3] == 3):
            raise ValueError("canvas must be a uint8 [N,dh,dw,3] BGR device tensor")
        canvas = canvas.contiguous()
        N, dh, dw, _ = canvas.shape
        if dh % 32 or dw % 32:
            raise ValueError(f"canvas {dh} x {dw}: sides must be multiples of 32")
        ar = self._arena(N, (dh, dw))
        st = _lib.stream_ptr()
        self.lib.fr_det_input_f16(_lib.ptr(canvas), _lib.ptr(ar.input), N, dh, dw, st)
        for fn, args in ar.calls:
            fn(*args, st)
        return ar, [(lv["stride"], ar.head(lv["score"]), ar.head(lv["bbox"]), ar.head(lv["kps"])) for lv in ar.plan.levels]

    def detect_batch(self, canvas, det_scale=None):
        with torch.cuda.device(self.device):
            ar, heads = self.forward_heads(canvas)
            N, dh, dw = canvas.shape[0], canvas.shape[1], canvas.shape[2]
            if det_scale is None:
                det_scale = torch.ones(N, dtype=torch.float32, device=self.device)
            if not (det_scale.dtype == torch.float32 and det_scale.numel() == N and det_scale.is_contiguous()):
                raise ValueError("det_scale must be a contiguous f32 [N] device tensor")
            st, lib, A = _lib.stream_ptr(), self.lib, ar.plan.num_anchors
            for li, (stride, sc, bb, kp) in enumerate(heads):
                lib.fr_scrfd_decode(_lib.ptr(sc), _lib.ptr(bb), _lib.ptr(kp), N, dh // stride, dw // stride, A, stride, li, self.logit_thr,
                                    _lib.ptr(det_scale), self.cap, _lib.ptr(ar.cb), _lib.ptr(ar.cs), _lib.ptr(ar.ca), _lib.ptr(ar.cc), st)
            boxes = torch.zeros((N, self.cap_out, 4), dtype=torch.float32, device=self.device)
            scores = torch.zeros((N, self.cap_out), dtype=torch.float32, device=self.device)
            kps = torch.zeros((N, self.cap_out, 10), dtype=torch.float32, device=self.device)
            counts = torch.empty((N,), dtype=torch.int32, device=self.device)
            lib.fr_sort_nms(_lib.ptr(ar.cb), _lib.ptr(ar.cs), _lib.ptr(ar.ca), 10, _lib.ptr(ar.cc), N, 3, self.cap, 0, self.nms_thresh, 0,
                            self.cap_out, _lib.ptr(boxes), _lib.ptr(scores), _lib.ptr(kps), _lib.ptr(counts), self.cap_out, st)
        return boxes, scores, kps.view(N, self.cap_out, 5, 2), counts
