"""``FaceAnalysis``-shaped engine: the drop-in for the object the reference builds at
/root/reference/infrenceServer.py:412-416 (``FaceAnalysis(name=..., providers=...)``,
``.prepare(ctx_id=0)``) and calls at :528 (``.get(frame) -> [Face]``).

The reference reads three Face fields only: ``bbox`` (:531), ``normed_embedding`` (:532) and
``det_score`` (:557); ``kps`` and ``embedding`` are provided as insightface does.

detect (MTCNN, HIP) -> align (5-point warp, HIP) -> embed (IResNet on MFMA, HIP); the match
step lives in ``gallery.GalleryMatcher``.  There is no CPU path: construction succeeds
anywhere, ``prepare`` raises without a HIP device.
"""
import contextlib
import logging
import os
import threading
import warnings

import numpy as np
import torch

from . import _lib, weights
from .letterbox import check_det_size, frame_table


class Face(dict):
    """Attribute-style record like insightface's Face (``face.bbox`` and ``face['bbox']``)."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name)

    def __setattr__(self, name, value):
        self[name] = value


def _model_dir(name, root):
    return os.path.join(os.path.expanduser(root), "models", name)


@contextlib.contextmanager
def _reset_on_failure(tracks, camera_ids):
    """Round everything a pass runs behind ``tracks.associate_device`` (``tracks`` None: round nothing).  The associate launch
    has moved the state: should anything behind it fail, the bank misses this turn's rows, and no track of these cameras may be
    carried from it."""
    try:
        yield
    except BaseException:
        if tracks is not None:
            tracks.reset(camera_ids)
        raise


class _Ragged:
    """A batch handed to the kernels as a frame table (include/frhip.h fr_frame_ref): frames of differing sizes, or a uniform
    stack under ``det_size``.  table: device u8 [N*32]; det_scale: device f32 [N]; keep: what the table points into."""

    def __init__(self, n, table, det_scale, keep):
        self.n, self.table, self.det_scale, self.keep = n, table, det_scale, keep


class FaceAnalysis:
    """Same constructor / prepare / get surface as insightface.app.FaceAnalysis.

    ``name`` selects a model directory ``<root>/models/<name>/`` holding ``arcface_<arch>.pt|.safetensors``
    and ``mtcnn_{pnet,rnet,onet}.pt`` state dicts (public PyTorch naming, see weights.py).  A recognition network
    shipped as ONNX - the ``w600k_r50.onnx`` of the reference's own buffalo_l pack - is read too (onnx_import.py: the
    first ``*.onnx`` of the directory whose graph is an ArcFace IResNet; ``arch`` then follows the file), and so is a
    MobileFaceNet-style one built from depthwise convs (the ``w600k_mbf.onnx`` of buffalo_s / buffalo_sc: ``arch`` becomes
    ``"mbf"`` and ``mbf.PlanRecogniserHIP`` runs the plan ``onnx_import.recognition_plan_from_onnx`` reads; f16 only).  The pack's
    detector (``det_10g.onnx``, SCRFD) is read too when the directory holds no ``mtcnn_*.pt`` files: the first ``*.onnx``
    that ``onnx_import.scrfd_plan_from_onnx`` accepts becomes a ``scrfd.SCRFDHIP`` detector on a 640 x 640 canvas unless
    ``prepare`` is given another ``det_size``; with neither, MTCNN runs on synthetic weights.  The detector keywords of the
    constructor (``minsize``, ``factor``, ``thresholds``, ``cap_scale``, ``keep_scale``, ``cap_p``, ``cap_r``, ``cap_o``) are
    MTCNN's.  Under a SCRFD detector ``cap_p`` is its ``cap`` (candidates kept per level and frame in front of NMS, at most
    1365: 3 * cap <= 4096, a larger value raises ValueError) and ``cap_o`` its ``cap_out`` (faces per frame); the others have
    no counterpart and are ignored with a warning - the score threshold is ``prepare(det_thresh=...)``.  When the directory is absent the engine falls back to SEEDED SYNTHETIC weights and says so loudly:
    the pipeline is then numerically exact w.r.t. its oracle but recognises nothing.
    ``providers`` is accepted for signature compatibility and ignored (HIP only).
    """

    def __init__(self, name="buffalo_l", root="~/.insightface", allowed_modules=None, providers=None,
                 arch="r100", **kwargs):
        self.name, self.root, self.providers, self.arch = name, root, providers, arch
        self.det = self.rec = None
        self._lock = threading.Lock()         # one engine may be shared by threads (trainingServer.py:115,227)
        self.det_kwargs = {k: kwargs[k] for k in ("minsize", "factor", "thresholds", "cap_scale", "keep_scale",
                                                  "cap_p", "cap_r", "cap_o") if k in kwargs}
        self.synthetic = None
        self.det_size = None
        self._scrfd_graph = None              # the pack's SCRFD detector graph, when _load_states found one and no mtcnn_*.pt

    def _load_states(self):
        d = _model_dir(self.name, self.root)
        rec = det = None
        for ext in (".safetensors", ".pt", ".pth"):
            p = os.path.join(d, f"arcface_{self.arch}{ext}")
            if rec is None and os.path.exists(p):
                rec = weights.load_state(p)
            ps = [os.path.join(d, f"mtcnn_{n}{ext}") for n in ("pnet", "rnet", "onet")]
            if det is None and all(os.path.exists(q) for q in ps):
                det = tuple(weights.load_state(q) for q in ps)
        parsed = {}                                        # file name -> graph (or None: the recognition network's), read once
        if rec is None and os.path.isdir(d):              # insightface packs ship the recognition network as ONNX
            from .onnx_import import iresnet_state_from_onnx, read_onnx, recognition_plan_from_onnx
            skipped = []
            for fn in sorted(os.listdir(d)):
                if fn.endswith(".onnx"):
                    try:
                        parsed[fn] = read_onnx(os.path.join(d, fn))
                        st, arch = iresnet_state_from_onnx(parsed[fn])
                        rec, self.arch = {k: torch.from_numpy(v) for k, v in st.items()}, arch
                    except Exception as e:                 # no IResNet: a MobileFaceNet-style recogniser (buffalo_s / _sc)?
                        try:
                            if fn not in parsed:
                                raise
                            rec, self.arch = recognition_plan_from_onnx(parsed[fn]), "mbf"
                        except Exception as e2:            # the pack's detector / landmark / attribute models, or a
                            why = f"{fn}: {type(e).__name__}: {e}"            # graph this reader cannot map
                            skipped.append(why if e2 is e else f"{why}; as a depthwise recogniser: {type(e2).__name__}: {e2}")
                            continue
                    parsed[fn] = None
                    break
            for why in skipped:
                logging.getLogger(__name__).info("model pack '%s': skipped %s", self.name, why)
            if rec is None and skipped:
                # the directory HOLDS .onnx files but none maps onto an ArcFace IResNet: falling back to synthetic
                # recognition weights here would silently recognise nobody
                raise _lib.FrError(f"model pack '{self.name}' under {d}: none of its .onnx files is a readable ArcFace "
                                   "IResNet or depthwise (MobileFaceNet-style) recogniser (" + "; ".join(skipped) + ")")
        self._scrfd_graph = self._find_scrfd(d, parsed) if det is None and os.path.isdir(d) else None
        if self._scrfd_graph is not None:
            # rec is never None here: a directory that holds .onnx files of which none is an ArcFace IResNet raised above,
            # and one without .onnx files holds no SCRFD graph
            self.synthetic = False
            return (rec, None)
        self.synthetic = rec is None or det is None
        if self.synthetic:
            missing = " and ".join(w for w, x in (("recognition", rec), ("MTCNN detector", det)) if x is None)
            warnings.warn(f"model pack '{self.name}' under {d}: no {missing} weights found: using SEEDED SYNTHETIC "
                          f"weights for them (numerically exact pipeline, meaningless identities)")
        return (rec if rec is not None else weights.synth_iresnet_state(self.arch), det or weights.synth_mtcnn_states())

    def _find_scrfd(self, d, parsed):
        """The graph of the first ``*.onnx`` under d that is a SCRFD detector with keypoints, or None; the others are
        skipped with their reason at INFO.  ``parsed``: the graphs _load_states has read already (None: the file it took as
        the recognition network, which is not looked at again)."""
        from .onnx_import import read_onnx, scrfd_plan_from_onnx
        for fn in sorted(os.listdir(d)):
            if fn.endswith(".onnx") and parsed.get(fn, fn) is not None:
                try:
                    g = parsed.get(fn) or read_onnx(os.path.join(d, fn))
                    scrfd_plan_from_onnx(g, (640, 640))
                    return g
                except Exception as e:
                    logging.getLogger(__name__).info("model pack '%s': %s is no SCRFD detector: %s: %s", self.name, fn,
                                                     type(e).__name__, e)
        return None

    def _make_detector(self, det_kwargs, det_thresh=None, share=None):
        from .mtcnn import MTCNNHIP
        if self._scrfd_graph is None:
            return MTCNNHIP(*self._det_states, device=self.device, **det_kwargs)
        from .scrfd import SCRFDHIP
        # the detector keywords are MTCNN's; two have a SCRFD meaning (class docstring), the others none
        kw = {new: det_kwargs[old] for old, new in (("cap_p", "cap"), ("cap_o", "cap_out")) if old in det_kwargs}
        ignored = sorted(k for k in det_kwargs if k not in ("cap_p", "cap_o"))
        if ignored:
            warnings.warn(f"model pack '{self.name}': its detector is SCRFD, which ignores the MTCNN keyword(s) {', '.join(ignored)} "
                          "(the score threshold is prepare(det_thresh=...))")
        return SCRFDHIP(self._scrfd_graph, device=self.device, det_thresh=0.5 if det_thresh is None else det_thresh, share=share, **kw)

    def prepare(self, ctx_id=0, det_thresh=None, det_size=None):
        """``ctx_id`` = HIP device ordinal (infrenceServer.py:416).

        ``det_size=(dw, dh)`` (insightface's order, width first; the reference's ``prepare(ctx_id=0)`` means (640, 640)):
        every frame is resized on the device to fit a dw x dh detection canvas (aspect kept, top-left, zero padded, bilinear
        without antialiasing like ``cv2.resize``'s default: ``letterbox_geometry``, csrc/letterbox.hip), the detector runs on
        the canvas, boxes and landmarks are divided by the frame's scale and alignment samples the ORIGINAL frame.
        ``minsize`` and the pyramid then apply to CANVAS pixels: a 20-pixel minimum face on the 640 x 360 image of a 1080p
        frame is 60 pixels in the frame.  Detector cost no longer grows with the camera's resolution, and frames of
        differing sizes go through one call (``get_batch`` / ``detect_embed_*`` take a list of them).
        ``det_size=None`` (default): MTCNN walks the full pyramid of the full frame, and a batch is frames of one size.

        A pack whose detector is a SCRFD ONNX file (no ``mtcnn_*.pt``): ``det_size=None`` means (640, 640), insightface's
        default, both sides multiples of 32; ``det_thresh`` (default 0.5) is the score threshold.  MTCNN takes its
        thresholds from the constructor and ignores ``det_thresh``, as before."""
        from .iresnet import IResNetHIP
        _lib.require_gpu()
        self.det_size = check_det_size(det_size)
        self.device = torch.device(f"cuda:{max(int(ctx_id), 0)}")
        rec, det = self._load_states()
        self._det_states = det
        if self._scrfd_graph is not None:
            self.det_size = self.det_size or (640, 640)
            if self.det_size[0] % 32 or self.det_size[1] % 32:
                raise ValueError(f"det_size {self.det_size}: the SCRFD detector needs both sides in multiples of 32")
        self._det_thresh = det_thresh
        if self.arch == "mbf":                          # _load_states read a recognition PLAN (onnx_import.RecognitionPlan)
            from .mbf import PlanRecogniserHIP
            self.rec = PlanRecogniserHIP(rec, self.device)
        else:
            self.rec = IResNetHIP(rec, self.arch, self.device)
        self.det = self._make_detector(self.det_kwargs, det_thresh)
        self.lib = _lib.load()
        self._use_graphs, self._graphs = False, {}
        return self

    def calibrate_fp8(self, frames, max_faces=64):
        """Switch the embed network's eligible body convs to the fp8 matrix cores (BASELINE config C5).  ``frames``
        (uint8 [N,H,W,3] BGR, device tensor or array) are run through detect + align; the aligned crops of up to
        ``max_faces`` detected faces are the calibration batch of ``IResNetHIP.enable_fp8`` (static per-tensor
        activation scales).  Returns the number of convs switched."""
        if self.det is None:
            raise _lib.FrError("FaceAnalysis.prepare() has not been called")
        if self.arch == "mbf":
            raise _lib.FrError(f"model pack '{self.name}': its recogniser is a depthwise (MobileFaceNet-style) network; the fp8 path "
                               "exists for IResNet only")
        frames = self._to_device(frames)
        with self._lock, torch.cuda.device(self.device):
            frames, src = self._source(frames)
            N = src.n if src is not None else frames.shape[0]
            boxes, scores, kps, counts = self._detect(frames, src)
            cap = boxes.shape[1]
            crops = torch.empty((N * cap, 112, 112, 8), dtype=torch.float16, device=self.device)
            self._warp_slots(frames, src, kps, counts, cap, crops)
            valid = (torch.arange(cap, device=self.device)[None, :] < counts[:, None]).reshape(-1).nonzero().squeeze(1)
            if valid.numel() == 0:
                raise _lib.FrError("calibrate_fp8: no face detected in the calibration frames")
            n = self.rec.enable_fp8(crops[valid[:max_faces]].contiguous())
            self._graphs = {}                     # captured graphs hold the f16 launch sequence
        return n

    def clone_with(self, det_size="same", **det_kwargs):
        """A second engine on the same device that SHARES this one's embed network (weights resident once) and
        has its own detector with other capacities / thresholds (e.g. ``cap_o=1`` for single-face frames).  It keeps this
        engine's ``det_size`` unless one is given (``None``: no detection canvas)."""
        if self.det is None:
            raise _lib.FrError("FaceAnalysis.prepare() has not been called")
        other = FaceAnalysis(self.name, self.root, providers=self.providers, arch=self.arch)
        other.device, other.rec, other.lib, other.synthetic = self.device, self.rec, self.lib, self.synthetic
        other._det_states = self._det_states
        other.det_size = self.det_size if isinstance(det_size, str) and det_size == "same" else check_det_size(det_size)
        other.det_kwargs = {**self.det_kwargs, **det_kwargs}
        other._scrfd_graph, other._det_thresh = self._scrfd_graph, getattr(self, "_det_thresh", None)
        if self._scrfd_graph is not None:
            if other.det_size is None or other.det_size[0] % 32 or other.det_size[1] % 32:
                raise ValueError(f"det_size {other.det_size}: the SCRFD detector needs a canvas with both sides in multiples of 32")
            other.det = other._make_detector(other.det_kwargs, other._det_thresh, share=self.det)      # packed weights resident once
        else:
            other.det = other._make_detector(other.det_kwargs)
        other._use_graphs, other._graphs = False, {}
        other._shares_rec = self._shares_rec = True          # neither engine may free the shared network's plans
        return other

    # ------------------------------------------------------------------ det_size / ragged batches
    def _to_device(self, frames):
        """host array(s) -> device tensor(s): a [N,H,W,3] array / tensor stays one tensor, a list stays a list"""
        def one(f):
            if not torch.is_tensor(f):
                f = torch.from_numpy(np.ascontiguousarray(np.asarray(f)))
            return f.to(self.device).contiguous()
        return [one(f) for f in frames] if isinstance(frames, (list, tuple)) else one(frames)

    def _source(self, frames, table=None, det_scale=None):
        """What a pipeline call was given -> ``(frames, src)``.  src None: a uniform [N,H,W,3] stack and no ``det_size`` -
        the kernels take (frames, N, H, W) as always.  Otherwise a ``_Ragged``: a list of [Hi,Wi,3] device frames or a
        stack, as a frame table written on the host (no device work is waited for).  ``table`` / ``det_scale``: already
        on the device (``RaggedIngest.upload``)."""
        if table is not None:
            if self.det_size is not None and det_scale is None:
                raise ValueError("a frame table under det_size comes with its det_scale (RaggedIngest.det_scale)")
            return frames, _Ragged(table.numel() // 32, table, det_scale, frames)
        if isinstance(frames, (list, tuple)):
            if not frames:
                raise ValueError("no frames")
            for f in frames:
                if not (torch.is_tensor(f) and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3 and f.is_contiguous()):
                    raise ValueError("frames must be contiguous uint8 [H,W,3] BGR device tensors")
            if self.det_size is None:
                if any(f.shape != frames[0].shape for f in frames):
                    raise ValueError("frames of differing sizes need a detection canvas: prepare(det_size=(w, h))")
                return torch.stack(list(frames)), None
            ptrs, shapes = [f.data_ptr() for f in frames], [tuple(f.shape[:2]) for f in frames]
        else:
            if not (frames.dim() == 4 and frames.shape[3] == 3 and frames.dtype == torch.uint8):
                raise ValueError("frames must be uint8 [N,H,W,3] BGR")
            if self.det_size is None:
                return frames, None
            frames = frames.contiguous()
            N, H, W, _ = frames.shape
            ptrs, shapes = [frames.data_ptr() + i * H * W * 3 for i in range(N)], [(H, W)] * N
        tab, scale = frame_table(ptrs, shapes, self.det_size)
        # pinned staging from torch's caching host allocator (it holds a block back until the copy that read it is done):
        # the two small copies are asynchronous and ordered on the current stream in front of the kernels that read them
        table = torch.from_numpy(tab).pin_memory().to(self.device, non_blocking=True)
        det_scale = torch.from_numpy(scale).pin_memory().to(self.device, non_blocking=True)
        return frames, _Ragged(len(ptrs), table, det_scale, frames)

    def _canvas(self, src):
        dw, dh = self.det_size
        canvas = torch.empty((src.n, dh, dw, 3), dtype=torch.uint8, device=self.device)
        self.lib.fr_letterbox_u8(_lib.ptr(src.table), src.n, _lib.ptr(canvas), dh, dw, _lib.stream_ptr())
        return canvas

    def letterbox(self, frames):
        """The detection canvases of ``frames`` ([N,H,W,3], or a list of [Hi,Wi,3] frames of any sizes; host arrays or
        device tensors) under this engine's ``det_size``: ``(canvas u8 [N,dh,dw,3], det_scale f32 [N])``, device tensors.
        Canvas coordinates divided by ``det_scale[f]`` are frame pixels."""
        if self.det is None:
            raise _lib.FrError("FaceAnalysis.prepare() has not been called")
        if self.det_size is None:
            raise ValueError("letterbox() needs prepare(det_size=(w, h))")
        with torch.cuda.device(self.device):
            frames, src = self._source(self._to_device(frames))
            canvas = self._canvas(src)
        return canvas, src.det_scale

    def _detect(self, frames, src, contiguous_kps=True):
        """The detector on the current stream -> boxes, scores, kps, counts in FRAME pixels.  Under ``det_size``: canvas,
        cascade on the canvas, division by det_scale on the device - no host sync."""
        if src is None or self.det_size is None:
            if src is not None:
                raise ValueError("frames of differing sizes need a detection canvas: prepare(det_size=(w, h))")
            boxes, scores, kps, counts = self.det.detect_batch(frames)
            return boxes, scores, kps.contiguous() if contiguous_kps else kps, counts
        if self._scrfd_graph is not None:               # SCRFD divides by det_scale in its decode, in front of NMS (frame pixels)
            with torch.cuda.device(self.device):
                return self.det.detect_batch(self._canvas(src), src.det_scale)
        with torch.cuda.device(self.device):
            boxes, scores, kps, counts = self.det.detect_batch(self._canvas(src))
            boxes, kps = boxes.contiguous(), kps.contiguous()
            self.lib.fr_detections_unscale(_lib.ptr(boxes), _lib.ptr(kps), _lib.ptr(counts), _lib.ptr(src.det_scale),
                                           src.n, boxes.shape[1], _lib.stream_ptr())
        return boxes, scores, kps, counts

    def _warp_slots(self, frames, src, kps, counts, cap, crops):
        if src is None:
            N, H, W, _ = frames.shape
            self.lib.fr_warp_affine_5pt_slots(_lib.ptr(frames), N, H, W, _lib.ptr(kps), _lib.ptr(counts), cap, 112,
                                              _lib.ptr(crops), _lib.stream_ptr())
        else:
            self.lib.fr_warp_affine_5pt_slots_refs(_lib.ptr(src.table), src.n, _lib.ptr(kps), _lib.ptr(counts), cap, 112,
                                                   _lib.ptr(crops), _lib.stream_ptr())

    def _warp_faces(self, frames, src, kps, frame_idx, F, crops):
        if src is None:
            N, H, W, _ = frames.shape
            self.lib.fr_warp_affine_5pt(_lib.ptr(frames), N, H, W, _lib.ptr(kps), _lib.ptr(frame_idx), None,
                                        F, 112, _lib.ptr(crops), None, None, _lib.stream_ptr())
        else:
            self.lib.fr_warp_affine_5pt_refs(_lib.ptr(src.table), src.n, _lib.ptr(kps), _lib.ptr(frame_idx), None,
                                             F, 112, _lib.ptr(crops), None, None, _lib.stream_ptr())

    # ------------------------------------------------------------------ device-side pipeline
    def detect_embed_device(self, frames, quality=None):
        """frames: uint8 [N,H,W,3] BGR on the device, or - with ``det_size`` - a list of [Hi,Wi,3] device frames of any
        sizes.  One host sync (face counts).

        quality: a ``quality.FaceQuality`` - one launch more measures the F aligned crops (no sync more) and the dict gains
        ``quality`` i32 [F,8], ``quality_f`` f32 [F,4] and ``quality_verdict`` i32 [F] (0: fit).  EVERY face is still embedded:
        enrolment wants the embedding whatever the verdict.

        Returns dict of device tensors for the F detected faces (frame-major, descending score
        within a frame): frame_idx i32 [F], bbox f32 [F,4], kps f32 [F,5,2], det_score f32 [F],
        embedding f32 [F,512], normed_embedding f32 [F,512]; plus counts (host list)."""
        if self.det is None:
            raise _lib.FrError("FaceAnalysis.prepare() has not been called")
        frames, src = self._source(frames)
        N = src.n if src is not None else frames.shape[0]
        boxes, scores, kps, counts = self._detect(frames, src, contiguous_kps=False)
        cap = boxes.shape[1]
        cnt = counts.cpu()                                            # the one sync of the pipeline
        if N == 1:                                                    # a single frame: its valid slots are a prefix - views, no gathers
            F = int(cnt[0])
            frame_idx = torch.zeros(F, dtype=torch.int32, device=self.device)
            out = {"counts": [F], "frame_idx": frame_idx, "bbox": boxes[0, :F], "kps": kps[0, :F].contiguous(),
                   "det_score": scores[0, :F]}
        else:
            mask = torch.arange(cap)[None, :] < cnt[:, None]
            sel = mask.reshape(-1).nonzero().squeeze(1).to(self.device)   # frame-major valid slots
            F = sel.numel()
            frame_idx = (sel // cap).to(torch.int32)
            out = {"counts": cnt.tolist(), "frame_idx": frame_idx,
                   "bbox": boxes.reshape(-1, 4)[sel], "kps": kps.reshape(-1, 5, 2)[sel].contiguous(),
                   "det_score": scores.reshape(-1)[sel]}
        emb = torch.empty((F, 512), dtype=torch.float32, device=self.device)
        normed = torch.empty_like(emb)
        if F:
            with torch.cuda.device(self.device):
                crops = torch.empty((F, 112, 112, 8), dtype=torch.float16, device=self.device)
                self._warp_faces(frames, src, out["kps"], frame_idx, F, crops)
                if quality is not None:
                    out["quality"], out["quality_f"], out["quality_verdict"] = quality.measure_device(crops, out["kps"])
                emb, normed = self.rec.forward(crops)
        elif quality is not None:
            out["quality"] = torch.empty((0, 8), dtype=torch.int32, device=self.device)
            out["quality_f"] = torch.empty((0, 4), dtype=torch.float32, device=self.device)
            out["quality_verdict"] = torch.empty(0, dtype=torch.int32, device=self.device)
        out["embedding"], out["normed_embedding"] = emb, normed
        return out

    def detect_embed_slots(self, frames, det_stream=None, ready_event=None, compact_embed=False, crops_out=None,
                           table=None, det_scale=None, tracks=None, camera_ids=None, quality=None):
        """Sync-free form for streaming/serving: every frame owns ``cap_o`` face slots.

        frames: uint8 [N,H,W,3] BGR on the device; with ``det_size`` also a list of [Hi,Wi,3] device frames of any sizes,
        or the arena, ``table`` and ``det_scale`` of a ``RaggedIngest``.  Returns device tensors only (no host sync):
        counts i32 [N]; bbox f32 [N,cap,4]; kps f32 [N,cap,5,2]; det_score f32 [N,cap];
        embedding / normed_embedding f32 [N*cap,512] (rows of empty slots are meaningless: mask with counts).

        det_stream: optional second HIP stream for the detector.  Align + embed stay on the current stream and
        wait for the detector through an event, but the detector does NOT wait for work already queued on the
        current stream, so batch i+1's cascade (latency-bound, leaves CU slots idle) runs beside batch i's embed
        convs (MFMA-bound).  The caller guarantees ``frames`` is complete before this call is made (it is when the
        frames were produced on ``det_stream`` or synchronised earlier) or passes ``ready_event`` (e.g. the event of
        ``FrameIngest.upload``), which the detector's stream waits for.

        compact_embed: embed only the slots that hold a face (ONE host sync on the face counts after the detector),
        the outputs keep the slot layout.  For callers that read the results on the host anyway (the camera batcher):
        8 cameras x 16 slots with a face or two each would otherwise pay for 128 embeddings.

        crops_out: f16 [N*cap,112,112,8] (a slice of a larger buffer): detect + align only - the aligned crops land there, the
        returned dict holds the detector outputs, and the caller runs ``embed_slots`` over the whole buffer.

        tracks: a ``tracks.FaceTracks`` with ``camera_ids`` (one per frame, none repeated), only with ``compact_embed``: behind
        the detector one launch decides which detections are faces the camera's tracks hold an embedding for, the copy of the
        face counts carries that verdict along (no second sync), align and embed run for the others only, and a second launch
        fills the carried rows from the bank and stores the new ones.  The dict gains ``track_id`` and ``carried`` i32 [N,cap].

        quality: a ``quality.FaceQuality``, only with ``compact_embed`` and without ``crops_out`` (ValueError otherwise): every
        slot is aligned (sync-free, empty slots skipped by their counts), ONE launch judges the aligned crops, the copy of the
        face counts carries the verdicts along (no second sync), and the embed net runs over the slots that hold a face AND are
        fit.  A rejected slot keeps the unit-vector placeholder of an empty one.  The dict gains ``quality`` i32 [N,cap,8],
        ``quality_f`` f32 [N,cap,4] and ``quality_verdict`` i32 [N,cap] (0: fit, -1: no face, else the reason bits of
        include/frhip.h fr_face_quality_f16).  ``quality`` beside ``tracks`` raises ValueError; the two combine through the tracks
        object instead: ``tracks=FaceTracks(..., quality=q)`` with ``quality=None``.  Such tracks judge:
        associate, align of every slot, the quality launch and one launch that decides embed / carry / reject per face run
        ahead of the one copy, which carries counts, actions, entries and verdicts; the embed net runs for the faces to embed
        and the commit launch stores their rows and fills the carried ones, so the bank holds fit embeddings only.  The dict then
        carries ``track_id``, ``carried``, ``track_action`` i32 [N,cap] (0 no face, 1 embedded, 2 carried, 3 rejected) and the
        three quality tensors; a rejected slot keeps the unit-vector placeholder.

        Tracks that fuse (``FaceTracks(..., template=K)``, plain or judging) add one launch right behind the
        commit launch and three keys: ``query`` f32 [N*cap,512], the row to scan with - the unit mean of the track's last shots
        where the face's track holds a template, else its ``normed_embedding`` row - and ``template_shots`` /
        ``template_event`` i32 [N,cap] (shots in the template, 0: none; 0 none, 1 started, 2 joined, 3 restarted, 4 read).
        ``embedding`` and ``normed_embedding`` stay this frame's row, or the carried one."""
        if self.det is None:
            raise _lib.FrError("FaceAnalysis.prepare() has not been called")
        if tracks is not None:
            if not compact_embed or crops_out is not None:
                raise ValueError("tracks need compact_embed=True: the carried faces are left out of the embed pass on the host")
            if camera_ids is None:
                raise ValueError("tracks need camera_ids: one camera id per frame")
            camera_ids = list(camera_ids)
            if len(set(camera_ids)) != len(camera_ids):
                raise ValueError("a camera id is repeated in one call")
        elif camera_ids is not None:
            raise ValueError("camera_ids come with tracks (tracks=FaceTracks(...))")
        if quality is not None:
            if not compact_embed or crops_out is not None:
                raise ValueError("quality needs compact_embed=True and no crops_out: the rejected faces are left out of the "
                                 "embed pass on the host")
            if tracks is not None:
                raise ValueError("quality together with tracks is not supported yet")
        cur = torch.cuda.current_stream(self.device)
        if ready_event is not None:
            (det_stream if det_stream is not None else cur).wait_event(ready_event)
        if det_stream is None:
            frames, src = self._source(frames, table, det_scale)
            boxes, scores, kps, counts = self._detect(frames, src)
        else:
            with torch.cuda.stream(det_stream):
                frames, src = self._source(frames, table, det_scale)           # (a table made here is uploaded on det_stream)
                boxes, scores, kps, counts = self._detect(frames, src)         # overlapped with the embedder
            cur.wait_stream(det_stream)
            for t in (boxes, scores, kps, counts) + ((src.table,) if src is not None and table is None else ()):
                t.record_stream(cur)
        N = src.n if src is not None else frames.shape[0]
        cap = boxes.shape[1]
        if compact_embed:
            return self._embed_compact(frames, src, boxes, scores, kps, counts, tracks, camera_ids, quality)
        with torch.cuda.device(self.device):
            if crops_out is not None:                  # the caller embeds several calls' slots in ONE forward (embed_slots)
                assert crops_out.shape == (N * cap, 112, 112, 8) and crops_out.dtype == torch.float16 and crops_out.is_contiguous()
            crops = crops_out if crops_out is not None else torch.empty((N * cap, 112, 112, 8), dtype=torch.float16, device=self.device)
            self._warp_slots(frames, src, kps, counts, cap, crops)
            if crops_out is not None:
                return {"counts": counts, "bbox": boxes, "kps": kps, "det_score": scores}
            emb, normed = self.rec.forward(crops)
        return {"counts": counts, "bbox": boxes, "kps": kps, "det_score": scores, "embedding": emb,
                "normed_embedding": normed}

    def _embed_compact(self, frames, src, boxes, scores, kps, counts, tracks, camera_ids, quality):
        """The ``compact_embed`` pass of ``detect_embed_slots`` behind the detector.  Its four forms are one sequence, of which
        each runs its own steps ([]: only when a slot is selected; fuse: only tracks with a ``template``):

          plain     copy -> [align the selected -> embed]
          tracks    associate -> copy -> [align the selected -> embed] -> commit -> fuse
          quality   align all -> judge -> copy -> [embed]
          judging   associate -> align all -> judge -> resolve -> copy -> [embed] -> commit -> fuse      (tracks that judge)

        The ONE copy is the sync on the face counts; its row widens to carry what selects the slots to embed: ``need`` and
        ``entry`` (tracks), the verdicts (quality), or actions, entries and verdicts (tracks that judge)."""
        N, cap = boxes.shape[:2]
        judging = tracks is not None and getattr(tracks, "quality", None) is not None
        if judging:
            quality = tracks.quality
        if tracks is not None and len(camera_ids) != N:
            raise ValueError(f"one camera id per frame: {N} frames, {len(camera_ids)} ids")
        crops, trk, qual, fused = None, {}, {}, {}
        with torch.cuda.device(self.device):
            if tracks is not None:
                entry, need, tid = tracks.associate_device(boxes, counts, camera_ids)
            with _reset_on_failure(tracks, camera_ids):
                row = [counts.reshape(N, 1)]
                if quality is not None:                                   # every slot aligned, sync-free, and judged
                    kps = kps.contiguous()
                    crops = torch.empty((N * cap, 112, 112, 8), dtype=torch.float16, device=self.device)
                    self._warp_slots(frames, src, kps, counts, cap, crops)
                    qi, qf, verdict = quality.measure_device(crops, kps, counts, cap)
                    verdict = verdict.view(N, cap)
                    qual = {"quality": qi.view(N, cap, 8), "quality_f": qf.view(N, cap, 4), "quality_verdict": verdict}
                if judging:                                               # embed / carry / reject per face; the pair to commit
                    action, need2, entry2 = tracks.resolve_device(entry, need, tid, verdict, counts, camera_ids)
                    row += [action, entry, verdict]
                elif tracks is not None:
                    need2, entry2 = need, entry
                    row += [need, entry]
                elif quality is not None:
                    row.append(verdict)
                both = (torch.cat(row, dim=1) if len(row) > 1 else row[0]).cpu()   # the one sync, a wider row than the counts
                cnt, first = both[:, 0], both[:, 1:1 + cap]
                if judging:
                    tracks.count(cnt.numpy(), None, both[:, 1 + cap:1 + 2 * cap].numpy(), first.numpy())
                    mask = first == 1                                     # action: embed
                elif tracks is not None:
                    tracks.count(cnt.numpy(), first.numpy(), both[:, 1 + cap:].numpy())
                    mask = first != 0                                     # need
                else:
                    mask = first == 0 if quality is not None else None    # verdict: fit
                emb, normed = self._embed_selected(frames, src, kps, self._select(cnt, cap, mask), N, cap, crops)
                if tracks is not None:
                    tracks.commit_device(entry2, need2, counts, camera_ids, emb, normed)
                    carried = action == 2 if judging else (need == 0) & (entry >= 0)   # a slot past the count has entry -1
                    trk = {"track_id": tid, "carried": carried.to(torch.int32)}
                    if judging:
                        trk["track_action"] = action
                    fused = self._fuse(tracks, entry2, need2, tid, counts, camera_ids, normed)
        return dict({"counts": counts, "bbox": boxes, "kps": kps, "det_score": scores, "embedding": emb,
                     "normed_embedding": normed}, **trk, **qual, **fused)

    def _select(self, cnt, cap, mask=None):
        """The slots to embed as a device index, frame-major: below the frame's host count ``cnt`` [N] and, with a host
        ``mask`` [N,cap], set in it."""
        held = torch.arange(cap)[None, :] < cnt[:, None]
        if mask is not None:
            held = held & mask
        return held.reshape(-1).nonzero().squeeze(1).to(self.device)

    def _embed_selected(self, frames, src, kps, sel, N, cap, crops=None):
        """Slot-layout (embedding, normed_embedding) f32 [N*cap,512] with the embed net's rows for the slots ``sel`` (a device
        index) and unit vectors - never NaN downstream - in every other row: empty, carried or rejected.  ``crops``: the
        aligned crops of all N*cap slots where the pass has them (``_warp_slots``); without, the selected slots are aligned
        here."""
        emb = torch.zeros((N * cap, 512), dtype=torch.float32, device=self.device)
        emb[:, 0] = 1.0
        normed = emb.clone()
        if sel.numel():
            with torch.cuda.device(self.device):
                # named, not inline: a temporary dies as soon as its pointer is taken and the next temporary
                # may be handed the same block before the kernel has read it
                if crops is not None:
                    faces = crops.index_select(0, sel)
                else:
                    F = sel.numel()
                    faces = torch.empty((F, 112, 112, 8), dtype=torch.float16, device=self.device)
                    kps_sel = kps.reshape(-1, 5, 2)[sel].contiguous()
                    frame_idx = (sel // cap).to(torch.int32)
                    self._warp_faces(frames, src, kps_sel, frame_idx, F, faces)
                e, nm = self.rec.forward(faces)
                emb[sel], normed[sel] = e, nm
        return emb, normed

    @staticmethod
    def _fuse(tracks, entry, need, tid, counts, camera_ids, normed):
        """The keys that tracks which fuse (``FaceTracks(..., template=K)``) add to the slot dict, right behind the commit launch
        and over its (entry, need) pair; {} for tracks that do not: no launch, no tensor."""
        if not getattr(tracks, "template", 0):
            return {}
        query, shots, event = tracks.fuse_device(entry, need, tid, counts, camera_ids, normed)
        return {"query": query, "template_shots": shots, "template_event": event}

    def embed_slots(self, crops):
        """Second half of ``detect_embed_slots(..., crops_out=...)``: ONE embed forward over the aligned crops of several
        detector calls (f16 [S,112,112,8], slot-major as those calls filled it) -> (embedding, normed_embedding) f32 [S,512].
        A 4K camera group of 8 frames x 16 slots is 128 faces - half of the 256 CUs for the one-workgroup-per-face stage
        kernels; two groups' crops side by side fill them (bench.py --workload C3)."""
        if self.rec is None:
            raise _lib.FrError("FaceAnalysis.prepare() has not been called")
        with torch.cuda.device(self.device):
            return self.rec.forward(crops)

    # ------------------------------------------------------------------ HIP-graph replay of the launch sequence
    def enable_graphs(self, on=True):
        """Single-frame calls are launch-bound (~250 kernel launches for a 640x480 frame): with graphs on, ``get`` /
        ``get_batch`` capture the sync-free slot pipeline once per input shape into a HIP graph (pinned staging buffers
        on both sides) and replay it.  Results are bit-identical to the eager path (same kernels, same order).
        Not under ``det_size``: an engine with a detection canvas runs every call eagerly, graphs on or off."""
        self._use_graphs = bool(on)
        if not on:
            self._graphs = {}
            if self.rec is not None and not getattr(self, "_shares_rec", False):
                torch.cuda.synchronize(self.device)          # replays in flight still read the plan buffers
                self.rec.release_plans()                     # ~90 MB per stream that the dropped graphs kept alive
        return self

    def _graph_for(self, shape):
        g = self._graphs.get(shape)
        if g is None:
            g = self._graphs[shape] = _GraphedPipeline(self, shape)
        return g

    # ------------------------------------------------------------------ reference-shaped API
    def get_batch(self, frames, quality=None):
        """list/array of BGR uint8 frames -> list (per frame) of lists of Face.  The frames are of one size; under
        ``det_size`` a list may mix sizes (bbox / kps are in each frame's own pixels).

        ``quality`` (a ``quality.FaceQuality``): every Face gains ``quality`` (the dict of ``FaceQuality.describe``) and
        ``quality_ok``; every face is embedded whatever its verdict.  Such a call runs eagerly, also under ``enable_graphs``."""
        if not isinstance(frames, np.ndarray):
            frames = [np.ascontiguousarray(np.asarray(f)) for f in frames]
            if any(f.ndim != 3 or f.shape[2] != 3 or f.dtype != np.uint8 for f in frames):
                raise ValueError("frames must be uint8 [H,W,3] BGR")
            if len(frames) and any(f.shape != frames[0].shape for f in frames):
                if self.det_size is None:
                    raise ValueError("frames of differing sizes need a detection canvas: prepare(det_size=(w, h))")
                with self._lock:
                    return self._faces_of(self.detect_embed_device(self._to_device(frames), quality))
            frames = np.stack(frames)
        arr = np.ascontiguousarray(frames)
        if arr.ndim != 4 or arr.shape[3] != 3 or arr.dtype != np.uint8:
            raise ValueError("frames must be uint8 [N,H,W,3] BGR")
        if getattr(self, "_use_graphs", False) and self.det_size is None and quality is None:
            with self._lock:
                counts, host = self._graph_for(tuple(arr.shape)).run(arr)
            return _faces_from_slots(counts, host)
        with self._lock:
            dev = torch.from_numpy(arr).to(self.device)
            return self._faces_of(self.detect_embed_device(dev, quality))

    @staticmethod
    def _faces_of(r):
        """``detect_embed_device``'s result -> per-frame lists of Face"""
        # ONE device-to-host copy (and sync) for the five result tensors instead of five
        F = r["bbox"].shape[0]
        judged = "quality" in r                    # its integers ride in the same copy: all below 2^24, exact in float32
        extra = [r["quality"].to(torch.float32), r["quality_f"], r["quality_verdict"].reshape(F, 1).to(torch.float32)] if judged else []
        pack = torch.cat([r["bbox"].reshape(F, 4), r["kps"].reshape(F, 10), r["det_score"].reshape(F, 1),
                          r["embedding"], r["normed_embedding"]] + extra, dim=1).cpu().numpy()
        host = {"bbox": pack[:, 0:4], "kps": pack[:, 4:14].reshape(F, 5, 2), "det_score": pack[:, 14],
                "embedding": pack[:, 15:527], "normed_embedding": pack[:, 527:1039]}
        res, i = [], 0
        for n in r["counts"]:
            faces = []
            for _ in range(n):
                faces.append(Face(bbox=host["bbox"][i].copy(), kps=host["kps"][i].copy(),
                                  det_score=float(host["det_score"][i]), embedding=host["embedding"][i].copy(),
                                  normed_embedding=host["normed_embedding"][i].copy()))
                if judged:
                    from .quality import FaceQuality
                    q = FaceQuality.describe(pack[i, 1039:1047], pack[i, 1047:1051], pack[i, 1051])
                    faces[-1]["quality"], faces[-1]["quality_ok"] = q, q["ok"]
                i += 1
            res.append(faces)
        return res

    def get(self, img, max_num=0, quality=None):
        """One BGR uint8 HWC frame -> list of Face (descending det_score), as infrenceServer.py:528.  ``quality``: as
        ``get_batch``."""
        faces = self.get_batch(np.asarray(img)[None], quality)[0]
        return faces[:max_num] if max_num else faces

    def get_batch_yuv(self, frames, pixel_format="nv12", matrix="bt601"):
        """``get_batch`` for YUV 4:2:0 frames, as a video decoder produces them: ``frames`` is a ``uint8 [N, H*3/2, W]`` array
        or device tensor, or a list of ``[H*3/2, W]`` frames (host arrays or device tensors) - of one size, or under
        ``det_size`` of any sizes, as ``get_batch`` allows.  ``pixel_format``: ``"nv12"`` / ``"i420"``; ``matrix``: ``"bt601"``
        (default), ``"bt709"``, ``"jpeg"`` (colour.py).  H and W must be even.  Host frames cross the link as YUV (half of BGR's
        bytes) and are converted on the device (csrc/yuv_to_bgr.hip); from there on the call IS ``get_batch`` on the
        converted frames: the same kernels on the same bytes, the same faces bit for bit.  Runs eagerly: ``enable_graphs``
        does not cover this entry point."""
        from .colour import check_yuv_shape, yuv420_to_bgr
        if self.det is None:
            raise _lib.FrError("FaceAnalysis.prepare() has not been called")

        def one(f):
            if not torch.is_tensor(f):
                f = torch.from_numpy(np.ascontiguousarray(np.asarray(f)))
            if f.dtype != torch.uint8:
                raise ValueError("YUV frames must be uint8")
            return f.to(self.device).contiguous()
        if isinstance(frames, (list, tuple)):
            if not frames:
                return []
            yuv = [one(f) for f in frames]
            shapes = [check_yuv_shape(f.shape) for f in yuv]
            if any(s != shapes[0] for s in shapes):
                if self.det_size is None:
                    raise ValueError("frames of differing sizes need a detection canvas: prepare(det_size=(w, h))")
            else:
                yuv = torch.stack(yuv)
        else:
            yuv = one(frames)
            if yuv.dim() != 3:
                raise ValueError("frames must be uint8 [N, H*3/2, W] (or a list of [H*3/2, W] frames)")
            check_yuv_shape(yuv.shape[1:])
        with self._lock, torch.cuda.device(self.device):
            return self._faces_of(self.detect_embed_device(yuv420_to_bgr(yuv, pixel_format, matrix)))

    def get_batch_jpeg(self, blobs, decoder=None, orient=False):
        """``get_batch`` for JPEG files (one ``bytes`` per frame: an MJPEG camera's frames, enrolment photos): the files cross
        the link as they are and are decoded on the device (csrc/jpeg_decode.hip); from there on the call IS ``get_batch`` on
        the decoded frames - which are libjpeg's pixels, byte for byte - so the faces are those of
        ``get_batch`` on the host-decoded pictures, bit for bit.  Pictures of one size, or under ``det_size`` of any sizes.  A
        file the device decoder does not take (progressive, CMYK, not a JPEG at all ...) is decoded by ``ingest.decode_image``
        on the host; a blob that does not decode either way is a frame without faces.  ``decoder``: a
        ``jpeg_decode.JpegDecoder`` on this device (default: the engine's own).  ``orient=True``: every picture is turned as
        its EXIF orientation says (a phone's upright photo; what ``cv2.imdecode`` gives the reference), on the device in the
        decoder's last launch, and the faces' coordinates are the turned picture's; a ``decoder`` passed in must have been built
        with the same ``orient`` (ValueError).  Runs eagerly: ``enable_graphs`` does not cover this entry point."""
        if self.det is None:
            raise _lib.FrError("FaceAnalysis.prepare() has not been called")
        blobs = list(blobs)
        if decoder is None:
            name = "_jpeg_decoder_oriented" if orient else "_jpeg_decoder"
            decoder = self.__dict__.get(name)
            if decoder is None:
                from .jpeg_decode import JpegDecoder
                decoder = JpegDecoder(self.device, orient=bool(orient))
                setattr(self, name, decoder)
        elif bool(getattr(decoder, "orient", False)) != bool(orient):
            raise ValueError(f"get_batch_jpeg(orient={bool(orient)}) with a decoder built with orient={decoder.orient}")
        with self._lock, torch.cuda.device(self.device):
            frames = decoder.decode_frames(blobs)
            live = [k for k, f in enumerate(frames) if f is not None]
            res = [[] for _ in frames]
            if live:
                batch = [frames[k] for k in live]
                if all(f.shape == batch[0].shape for f in batch):
                    batch = torch.stack(batch)
                elif self.det_size is None:
                    raise ValueError("frames of differing sizes need a detection canvas: prepare(det_size=(w, h))")
                for k, faces in zip(live, self._faces_of(self.detect_embed_device(batch))):
                    res[k] = faces
        return res

    def get_yuv(self, frame, pixel_format="nv12", matrix="bt601", max_num=0):
        """``get`` for one YUV 4:2:0 frame (``uint8 [H*3/2, W]``, host array or device tensor): see ``get_batch_yuv``.  Runs
        eagerly, whatever ``enable_graphs`` says."""
        if not torch.is_tensor(frame):
            frame = np.asarray(frame)
        if frame.ndim != 2:
            raise ValueError("frame must be uint8 [H*3/2, W]")
        faces = self.get_batch_yuv(frame[None], pixel_format, matrix)[0]
        return faces[:max_num] if max_num else faces


_GRAPH_KEYS = ("bbox", "kps", "det_score", "embedding", "normed_embedding")


def _faces_from_slots(counts, host):
    cap = host["bbox"].shape[1]
    res = []
    for f, n in enumerate(counts):
        faces = []
        for j in range(int(n)):
            i = f * cap + j
            faces.append(Face(bbox=host["bbox"][f, j].copy(), kps=host["kps"][f, j].copy(),
                              det_score=float(host["det_score"][f, j]), embedding=host["embedding"][i].copy(),
                              normed_embedding=host["normed_embedding"][i].copy()))
        res.append(faces)
    return res


class _GraphedPipeline:
    """frames (pinned) -> H2D -> [captured: detect -> align -> embed, fixed slots] -> D2H (pinned), one shape.

    A single frame with more than one face slot (``cap_o`` > 1) is captured in TWO parts: the detector, then - behind one read
    of the face count - align + embed for 1, 2, 4, 8 ... slots, one graph per size, captured when first needed.  One
    graph over all ``cap_o`` slots (the only form for several frames, and for one slot) embeds every slot whatever the
    frame holds: with the default 16 slots a one-face frame paid a 16-face forward (2.1 ms against 0.9)."""

    def __init__(self, app, shape):
        self.app, dev = app, app.device
        self.h_in = torch.empty(shape, dtype=torch.uint8).pin_memory()
        self.d_in = torch.empty(shape, dtype=torch.uint8, device=dev)
        self.stream = torch.cuda.Stream(device=dev)
        self.split = shape[0] == 1 and app.det.cap_o > 1
        with torch.cuda.device(dev):
            self.stream.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(self.stream):
                for _ in range(2):                       # first-launch work (attribute calls, lazy streams) outside capture
                    app.detect_embed_slots(self.d_in)
            self.stream.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=self.stream):
                if self.split:
                    boxes, scores, kps, counts = app.det.detect_batch(self.d_in)
                    self.out = {"counts": counts, "bbox": boxes, "kps": kps.contiguous(), "det_score": scores}
                else:
                    self.out = app.detect_embed_slots(self.d_in)
        keys = ("bbox", "kps", "det_score", "counts") if self.split else _GRAPH_KEYS + ("counts",)
        self.h_out = {k: torch.empty(self.out[k].shape, dtype=self.out[k].dtype).pin_memory() for k in keys}
        self.embed = {}                                   # slots -> (graph, embedding, normed, pinned host copies)
        if self.split:
            self.fidx = torch.zeros(app.det.cap_o, dtype=torch.int32, device=dev)

    def _embed_graph(self, n):
        g = self.embed.get(n)
        if g is None:
            app, dev = self.app, self.app.device
            _, H, W, _ = self.d_in.shape
            crops = torch.empty((n, 112, 112, 8), dtype=torch.float16, device=dev)
            kps = self.out["kps"][0, :n]                  # the frame's first n slots: a contiguous prefix

            def body():
                # slots at or past the face count are zero-filled by the kernel (count read on the device)
                app.lib.fr_warp_affine_5pt(_lib.ptr(self.d_in), 1, H, W, _lib.ptr(kps), _lib.ptr(self.fidx), _lib.ptr(self.out["counts"]),
                                           n, 112, _lib.ptr(crops), None, None, _lib.stream_ptr())
                return app.rec.forward(crops)
            with torch.cuda.device(dev), torch.cuda.stream(self.stream):
                body()
                self.stream.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=self.stream):
                    emb, normed = body()
            g = self.embed[n] = (graph, emb, normed, torch.empty((n, 512), dtype=torch.float32).pin_memory(),
                                 torch.empty((n, 512), dtype=torch.float32).pin_memory(), crops, kps)
        return g

    def run(self, arr):
        self.h_in.numpy()[...] = arr
        with torch.cuda.stream(self.stream):
            self.d_in.copy_(self.h_in, non_blocking=True)
            self.graph.replay()
            for k, h in self.h_out.items():
                h.copy_(self.out[k], non_blocking=True)
        self.stream.synchronize()
        counts = self.h_out["counts"].numpy().copy()
        if not self.split:
            return counts, {k: self.h_out[k].numpy() for k in _GRAPH_KEYS}
        host = {k: self.h_out[k].numpy() for k in ("bbox", "kps", "det_score")}
        F = int(counts[0])
        cap = self.app.det.cap_o
        host["embedding"] = host["normed_embedding"] = np.zeros((0, 512), dtype=np.float32)
        if F:
            n = 1
            while n < F:
                n *= 2
            graph, emb, normed, h_e, h_n = self._embed_graph(min(n, cap))[:5]
            with torch.cuda.stream(self.stream):
                graph.replay()
                h_e.copy_(emb, non_blocking=True)
                h_n.copy_(normed, non_blocking=True)
            self.stream.synchronize()
            host["embedding"], host["normed_embedding"] = h_e.numpy(), h_n.numpy()
        return counts, host


FaceEngine = FaceAnalysis
