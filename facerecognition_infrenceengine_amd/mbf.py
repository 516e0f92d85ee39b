"""A recognition network read as a plan, on HIP: the MobileFaceNet (``w600k_mbf.onnx``) of insightface's buffalo_s /
buffalo_sc packs as ``FaceAnalysis``'s embed network.

``onnx_import.recognition_plan_from_onnx`` turns the graph into device steps; ``PlanRecogniserHIP`` packs the folded
weights once, keeps one activation arena per (thread, stream, batch size) and walks the steps with fr_det_conv_act_f16 (stem,
1x1 expand / project, the fully connected layer as a 1x1 conv on the 1x1 map) and fr_dw_conv_f16 (depthwise 3x3 and the
global 7x7), then fr_l2norm_rows_f32 - all on the current stream, no host synchronisation.
f16 storage, f32 accumulation; there is no fp8 path.
"""
import ctypes
import threading

import numpy as np
import torch

from . import _lib
from .onnx_import import RecognitionPlan, recognition_plan_from_onnx
from .scrfd import _ceil, pack_conv, pack_dw


class _Arena:
    """The activation buffers of the plan at one batch size and the launch list that fills them.  The first step's input is
    the caller's crops and the last step's output the caller's embedding: those two slots are patched per call."""

    def __init__(self, rec, N):
        plan, lib, dev = rec.plan, rec.lib, rec.device
        self.N = N
        last = {}
        for i, s in enumerate(plan.steps):
            for key in ("x", "res"):
                if s.get(key) is not None:
                    last[s[key]] = i
        free, buf, self.blocks, self.calls = [], {}, [], []

        def take(tid):
            c, h, w = plan.shapes[tid]
            nbytes = N * h * w * _ceil(c, 8) * 2
            fit = [j for j, b in enumerate(free) if b.numel() >= nbytes]
            if fit:
                b = free.pop(min(fit, key=lambda j: free[j].numel()))
            else:
                b = torch.empty(_ceil(nbytes, 256), dtype=torch.uint8, device=dev)
                self.blocks.append(b)
            buf[tid] = b

        def ptr(tid):
            return None if tid in (0, plan.output) else _lib.ptr(buf[tid])

        for i, s in enumerate(plan.steps):
            if s["op"] == "input":
                continue
            if s["out"] != plan.output:
                take(s["out"])
            c, h, w = plan.shapes[s["out"]]
            ci, hi, wi = plan.shapes[s["x"]]
            wt, bias, slope, cin_p, cout_w = rec.packed[i]
            assert cin_p == _ceil(ci, 8)
            if s["op"] == "conv":
                cs, ldo = (c, c) if s["f32"] else (_ceil(c, 8), _ceil(c, 8))
                args = [ptr(s["x"]), _lib.ptr(wt), _lib.ptr(bias), _lib.ptr(slope), ptr(s["res"]) if s["res"] is not None else None,
                        ptr(s["out"]), N, hi, wi, cin_p, cout_w, s["k"], s["stride"], s["pad"], h, w, cs, ldo, s["act"], int(s["f32"]), 0]
                fn, xi, yi = lib.fr_det_conv_act_f16, 0, 5
            else:
                args = [ptr(s["x"]), _lib.ptr(wt), _lib.ptr(bias), _lib.ptr(slope), ptr(s["out"]), N, hi, wi, cin_p, s["k"], s["stride"],
                        s["pad"], h, w, s["act"]]
                fn, xi, yi = lib.fr_dw_conv_f16, 0, 4
            self.calls.append((fn, args, xi if s["x"] == 0 else None, yi if s["out"] == plan.output else None))
            for key in ("x", "res"):
                t = s.get(key)
                if t is not None and t != 0 and last.get(t) == i and all(b is not buf[t] for b in free):
                    free.append(buf[t])
        self.buf = buf


class PlanRecogniserHIP:
    """``forward(x f16 [B,112,112,8]) -> (embedding, normed_embedding)`` f32 [B,512] device tensors, the surface
    ``FaceAnalysis`` uses of ``IResNetHIP``.  ``plan_or_path``: an ``onnx_import.RecognitionPlan``, an ``OnnxGraph`` or a path.
    ``x`` is what fr_warp_affine_5pt writes: RGB (v - 127.5) / 127.5 in channels 0..2, zeros in 3..7.  B is cut into pieces of
    ``max_chunk`` faces; an element's bits do not depend on B, the chunking or the face's place in the batch.

    Memory: one arena per (thread, stream, chunk size) that has been seen, kept until ``release_plans()`` (a captured graph
    may hold its addresses): about 4 MB per face for MobileFaceNet."""

    def __init__(self, plan_or_path, device="cuda:0", max_chunk=256):
        _lib.require_gpu()
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.plan = plan_or_path if isinstance(plan_or_path, RecognitionPlan) else recognition_plan_from_onnx(plan_or_path)
        if self.plan.dim != 512:
            raise ValueError(f"PlanRecogniserHIP: embedding of {self.plan.dim} dimensions, expected 512")
        if max_chunk < 1:
            raise ValueError(f"PlanRecogniserHIP: max_chunk {max_chunk} must be positive")
        self.max_chunk = int(max_chunk)
        self.arch = "mbf"
        self.flops_per_face = self.plan.macs2
        self.fp8_on = False
        self.packed = {}                                # step index -> (weights, bias, slope, Cin padded, Cout packed): device tensors
        dev = self.device

        def up(a):
            return None if a is None else torch.from_numpy(a).to(dev)
        for i, s in enumerate(self.plan.steps):
            if s["op"] == "conv":
                wt, bias, cin_p, cout_w = pack_conv(s["w"], s["b"])
                slope = None
                if s["act"] == 2:
                    slope = np.zeros(cout_w, dtype=np.float32)
                    slope[:len(s["slope"])] = s["slope"]
                self.packed[i] = (up(wt), up(bias), up(slope), cin_p, cout_w)
            elif s["op"] == "dwconv":
                wt, bias, slope, cp = pack_dw(s["w"], s["b"], s["slope"] if s["act"] == 2 else None)
                self.packed[i] = (up(wt), up(bias), up(slope), cp, cp)
        self._tls = threading.local()                   # per-thread arenas: forward is re-entrant across threads
        self._gen = 0                                   # release_plans() makes every thread drop its arenas at its next call

    def _arena(self, N):
        tls = self._tls.__dict__
        if tls.get("gen") != self._gen:
            tls["gen"], tls["arenas"] = self._gen, {}
        key = (N, torch.cuda.current_stream(self.device).cuda_stream)
        a = tls["arenas"].get(key)
        if a is None:
            a = tls["arenas"][key] = _Arena(self, N)
        return a

    def release_plans(self):
        """Drop the activation arenas (this thread's now, every other thread's at its next call).  Call only when no
        captured graph of this network is alive - ``FaceAnalysis.enable_graphs(False)`` does, after dropping its graphs."""
        self._gen += 1
        self._tls.__dict__.pop("arenas", None)

    def enable_fp8(self, *args, **kwargs):
        raise _lib.FrError("PlanRecogniserHIP: the fp8 path exists for IResNet only (this network runs in f16)")

    def forward(self, x):
        assert x.dtype == torch.float16 and x.shape[1:] == (112, 112, 8) and x.is_contiguous()
        B = x.shape[0]
        emb = torch.empty((B, 512), dtype=torch.float32, device=self.device)
        normed = torch.empty_like(emb)
        if not B:
            return emb, normed
        with torch.cuda.device(self.device):
            st = _lib.stream_ptr()
            xp, ep = x.data_ptr(), emb.data_ptr()
            for b0 in range(0, B, self.max_chunk):
                n = min(B, b0 + self.max_chunk) - b0
                xc, ec = ctypes.c_void_p(xp + b0 * 112 * 112 * 8 * 2), ctypes.c_void_p(ep + b0 * 512 * 4)
                for fn, args, xi, yi in self._arena(n).calls:
                    if xi is not None:
                        args[xi] = xc
                    if yi is not None:
                        args[yi] = ec
                    fn(*args, st)
            self.lib.fr_l2norm_rows_f32(_lib.ptr(emb), _lib.ptr(normed), B, 512, st)
        return emb, normed
