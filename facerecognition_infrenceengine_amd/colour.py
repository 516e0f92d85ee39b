"""YUV 4:2:0 frames (NV12 / I420) -> the BGR frames the engine reads, converted on the device (csrc/yuv_to_bgr.hip).

The reference's live path is RTSP and webcam capture (/root/reference/infrenceServer.py:573-601): H.264 / H.265, which every
decoder - ``cv2.VideoCapture`` included - decodes to YUV 4:2:0 and then converts to BGR on the CPU.  A caller that decodes with
ffmpeg, PyAV or a hardware decoder holds NV12 or I420 buffers: 1.5 bytes per pixel against BGR's 3.  This module holds the
one table of conversion constants, the shape rule and the device entry point; ``ingest.FrameIngest`` / ``RaggedIngest`` use it
behind their copy, ``FaceAnalysis.get_yuv`` in front of the pipeline.  No GPU is needed to import it.

Arithmetic (include/frhip.h ``fr_yuv420_to_bgr_u8``): nearest chroma - a 2x2 pixel block shares its (U, V) pair - and per
pixel, in 32-bit integers::

    y = max(0, Y - y_off) * CY;   u = U - 128;   v = V - 128
    B = sat8((y + (1 << 19) + CUB u) >> 20)
    G = sat8((y + (1 << 19) + CUG u + CVG v) >> 20)
    R = sat8((y + (1 << 19) + CVR v) >> 20)             # arithmetic shift (floor), sat8 = clamp to [0, 255]
"""
import ctypes as C

import numpy as np

from . import _lib

# matrix -> (y_off, CY, CUB, CUG, CVG, CVR), 20 fractional bits.
#   bt601  limited-range BT.601, round(c * 2^20) of (1.164, 2.018, -0.391, -0.813, 1.596): the fixed-point form OpenCV uses for
#          COLOR_YUV2BGR_NV12 / _I420 [EXT] - external knowledge in the sense of SURVEY.md Appendix A; OpenCV is not in the
#          image, so tests/helpers/yuv_ref.py is the definition
#   bt709  limited-range BT.709 at 20 fractional bits: 255/219 for Y, 2.112402, -0.213249, -0.532909, 1.792741 for the chroma terms
#   jpeg   full-range BT.601 (JFIF, ffmpeg's yuvj420p): round(c * 2^20) of (1, 1.772, -0.344136, -0.714136, 1.402)
# With every row the largest intermediate is 5.7e8: inside int32 (the entry points check 255 CY + 2^19 + 128 max|chroma term|).
MATRICES = {
    "bt601": (16, 1220542, 2116026, -409993, -852492, 1673527),
    "bt709": (16, 1220945, 2215014, -223608, -558796, 1879825),
    "jpeg": (0, 1048576, 1858077, -360853, -748826, 1470104),
}
LAYOUTS = {"nv12": 0, "i420": 1}                     # include/frhip.h FR_YUV_NV12 / FR_YUV_I420
PIXEL_FORMATS = ("bgr",) + tuple(LAYOUTS)            # what the ingest rings and the processor take


def check_pixel_format(pixel_format, matrix="bt601", allow_bgr=True):
    """``(layout id or None for "bgr", constants)``; ValueError for a name this module does not know."""
    if pixel_format == "bgr" and allow_bgr:
        return None, None
    if pixel_format not in LAYOUTS:
        known = ", ".join(repr(p) for p in (PIXEL_FORMATS if allow_bgr else tuple(LAYOUTS)))
        raise ValueError(f"unknown pixel_format {pixel_format!r} (one of {known})")
    if matrix not in MATRICES:
        raise ValueError(f"unknown matrix {matrix!r} (one of {', '.join(repr(m) for m in MATRICES)})")
    return LAYOUTS[pixel_format], MATRICES[matrix]


def check_yuv_shape(shape):
    """Shape of one YUV 4:2:0 frame, ``(H * 3 / 2, W)`` -> ``(H, W)``.  H and W must be even - 4:2:0 has one chroma sample
    per 2x2 block; odd sizes are refused, not padded - and the BGR frame below 2 GiB."""
    if len(shape) != 2:
        raise ValueError(f"a YUV 4:2:0 frame is uint8 [H*3/2, W], got shape {tuple(shape)}")
    rows, w = int(shape[0]), int(shape[1])
    if rows <= 0 or rows % 3:
        raise ValueError(f"a YUV 4:2:0 frame is uint8 [H*3/2, W] with H and W even, got {rows} x {w}")
    return check_yuv_size(rows // 3 * 2, w)


def check_yuv_size(h, w):
    """``(H, W)`` of a frame that is to be held as YUV 4:2:0: both even and positive, the BGR frame below 2 GiB."""
    h, w = int(h), int(w)
    if h <= 0 or w <= 0 or h % 2 or w % 2:
        raise ValueError(f"YUV 4:2:0 needs H and W even (one chroma sample per 2x2 block; odd sizes are not padded), got {h} x {w}")
    if h * w * 3 >= 2 ** 31:
        raise ValueError(f"a {h} x {w} frame is beyond 2 GiB")
    return h, w


def yuv_nbytes(h, w):
    """bytes of one H x W YUV 4:2:0 frame"""
    return h * w * 3 // 2


def convert_batch(lib, src, dst, n, h, w, layout, consts):
    """One launch on the current stream: ``n`` frames of h x w back to back at ``src`` -> BGR at ``dst`` (device tensors)."""
    lib.fr_yuv420_to_bgr_u8(_lib.ptr(src), _lib.ptr(dst), n, h, w, layout, *consts, _lib.stream_ptr())


def convert_table(lib, table, src_ptrs, n, layout, consts):
    """One launch on the current stream: destination frame table (device u8 [n*32], ``letterbox.frame_table``) and device
    int64 [n] source addresses."""
    lib.fr_yuv420_to_bgr_refs_u8(_lib.ptr(table), _lib.ptr(src_ptrs), n, layout, *consts, _lib.stream_ptr())


def yuv420_to_bgr(frames, pixel_format="nv12", matrix="bt601", out=None):
    """YUV 4:2:0 device frames -> BGR device frames, on the current stream, one launch, no host synchronisation.

    frames: a uint8 device tensor ``[N, H*3/2, W]`` (or ``[H*3/2, W]``: one frame), or a list of ``[Hi*3/2, Wi]`` device
    tensors of any sizes.  Returns ``[N,H,W,3]`` (``[H,W,3]``), or a list of ``[Hi,Wi,3]`` tensors - views of ONE arena, the
    frames at 16-byte-aligned offsets.  ``out``: where to write instead of allocating - a contiguous tensor of the result's
    shape, or a list of such tensors.  ``pixel_format``: ``"nv12"`` / ``"i420"``; ``matrix``: ``"bt601"`` (default), ``"bt709"``,
    ``"jpeg"`` (module docstring).  H and W even; odd sizes raise ValueError."""
    import torch
    from .letterbox import frame_table
    layout, consts = check_pixel_format(pixel_format, matrix, allow_bgr=False)
    lib = _lib.load()

    def check(f):
        if not (torch.is_tensor(f) and f.is_cuda and f.dtype == torch.uint8 and f.is_contiguous()):
            raise ValueError("YUV frames must be contiguous uint8 device tensors")

    if not isinstance(frames, (list, tuple)):
        check(frames)
        if frames.dim() not in (2, 3):
            raise ValueError("YUV frames must be uint8 [N, H*3/2, W] (or one [H*3/2, W] frame)")
        h, w = check_yuv_shape(frames.shape[-2:])
        n = frames.shape[0] if frames.dim() == 3 else 1
        shape = (n, h, w, 3) if frames.dim() == 3 else (h, w, 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=frames.device)
        elif not (torch.is_tensor(out) and out.shape == shape and out.dtype == torch.uint8 and out.is_contiguous()
                  and out.device == frames.device):
            raise ValueError(f"out must be a contiguous uint8 tensor {shape} on the frames' device")
        with torch.cuda.device(frames.device):
            convert_batch(lib, frames, out, n, h, w, layout, consts)
        return out
    if not frames:
        raise ValueError("no frames")
    for f in frames:
        check(f)
    shapes = [check_yuv_shape(f.shape) for f in frames]
    dev = frames[0].device
    if out is None:
        offs, off = [], 0
        for h, w in shapes:
            offs.append(off)
            off += (h * w * 3 + 15) // 16 * 16
        arena = torch.empty(off, dtype=torch.uint8, device=dev)
        out = [arena[o:o + h * w * 3].view(h, w, 3) for o, (h, w) in zip(offs, shapes)]
    elif not (len(out) == len(frames) and all(
            torch.is_tensor(o) and o.shape == (h, w, 3) and o.dtype == torch.uint8 and o.is_contiguous() and o.device == dev
            for o, (h, w) in zip(out, shapes))):
        raise ValueError("out must be a list of contiguous uint8 [Hi,Wi,3] tensors on the frames' device, one per frame")
    tab, _ = frame_table([o.data_ptr() for o in out], shapes)
    srcs = np.array([f.data_ptr() for f in frames], dtype=np.int64)
    with torch.cuda.device(dev):
        # pinned staging from torch's caching host allocator, as FaceAnalysis._source uploads its tables: asynchronous, ordered
        # on the current stream in front of the launch that reads them
        table = torch.from_numpy(tab).pin_memory().to(dev, non_blocking=True)
        src_ptrs = torch.from_numpy(srcs).pin_memory().to(dev, non_blocking=True)
        convert_table(lib, table, src_ptrs, len(frames), layout, consts)
        for t in (table, src_ptrs):
            t.record_stream(torch.cuda.current_stream(dev))
    return list(out)
