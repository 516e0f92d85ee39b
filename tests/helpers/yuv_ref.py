"""YUV 4:2:0 -> BGR in NumPy: the definition the device conversion (csrc/yuv_to_bgr.hip) is pinned to, bit for bit.

Written from the specification, not from the kernel.  A frame is ``uint8 [H*3/2, W]`` (cv2's convention), H and W even:

* ``"nv12"``: Y plane ``H x W``, then ``H/2`` rows of ``W`` bytes of interleaved U, V;
* ``"i420"``: Y plane ``H x W``, then the U plane ``H/2 x W/2``, then the V plane.

Nearest chroma: each 2x2 pixel block shares its one (U, V) pair.  Per pixel, in exact integers (int64 here; every
intermediate fits int32)::

    y = max(0, Y - y_off) * CY;   u = U - 128;   v = V - 128
    B = sat8((y + (1 << 19) + CUB*u)          >> 20)
    G = sat8((y + (1 << 19) + CUG*u + CVG*v)  >> 20)
    R = sat8((y + (1 << 19) + CVR*v)          >> 20)        # >> is the arithmetic (floor) shift, sat8 clips to [0, 255]

``bt601`` is the fixed-point form OpenCV uses for ``COLOR_YUV2BGR_NV12`` / ``_I420`` [EXT]; the other rows are the standard
coefficients at 20 fractional bits.
"""
import numpy as np

# matrix -> (y_off, CY, CUB, CUG, CVG, CVR)
CONSTANTS = {
    "bt601": (16, 1220542, 2116026, -409993, -852492, 1673527),
    "bt709": (16, 1220945, 2215014, -223608, -558796, 1879825),
    "jpeg": (0, 1048576, 1858077, -360853, -748826, 1470104),
}
LAYOUTS = ("nv12", "i420")


def frame_hw(shape):
    """``(H*3/2, W)`` -> ``(H, W)``; ValueError unless H and W are even and positive."""
    if len(shape) != 2:
        raise ValueError(f"a YUV 4:2:0 frame is [H*3/2, W], got {tuple(shape)}")
    rows, w = int(shape[0]), int(shape[1])
    if rows <= 0 or w <= 0 or rows % 3 or w % 2:
        raise ValueError(f"odd size: [H*3/2, W] = {rows} x {w}")
    return rows // 3 * 2, w


def planes(frame, layout):
    """``(Y [H,W], U [H/2,W/2], V [H/2,W/2])`` of one frame, uint8 views / copies"""
    frame = np.asarray(frame)
    if frame.dtype != np.uint8:
        raise ValueError("uint8 frames only")
    h, w = frame_hw(frame.shape)
    y = frame[:h]
    c = frame[h:].reshape(-1)
    if layout == "nv12":
        uv = c.reshape(h // 2, w // 2, 2)
        return y, uv[..., 0], uv[..., 1]
    if layout == "i420":
        n = (h // 2) * (w // 2)
        return y, c[:n].reshape(h // 2, w // 2), c[n:2 * n].reshape(h // 2, w // 2)
    raise ValueError(f"unknown layout {layout!r}")


def pack(y, u, v, layout):
    """planes -> one ``[H*3/2, W]`` frame"""
    h, w = y.shape
    if h % 2 or w % 2 or u.shape != (h // 2, w // 2) or v.shape != u.shape:
        raise ValueError(f"odd size or mismatched planes: Y {y.shape}, U {u.shape}, V {v.shape}")
    out = np.empty((h * 3 // 2, w), np.uint8)
    out[:h] = y
    c = out[h:].reshape(-1)
    if layout == "nv12":
        c.reshape(h // 2, w // 2, 2)[..., 0] = u
        c.reshape(h // 2, w // 2, 2)[..., 1] = v
    elif layout == "i420":
        n = (h // 2) * (w // 2)
        c[:n] = u.reshape(-1)
        c[n:] = v.reshape(-1)
    else:
        raise ValueError(f"unknown layout {layout!r}")
    return out


def convert_triples(Y, U, V, matrix="bt601"):
    """The per-pixel formula on broadcastable integer arrays -> (B, G, R) uint8"""
    y_off, cy, cub, cug, cvg, cvr = CONSTANTS[matrix]
    y = np.maximum(np.asarray(Y, np.int64) - y_off, 0) * cy + (1 << 19)
    u = np.asarray(U, np.int64) - 128
    v = np.asarray(V, np.int64) - 128
    b = np.clip((y + cub * u) >> 20, 0, 255)
    g = np.clip((y + cug * u + cvg * v) >> 20, 0, 255)
    r = np.clip((y + cvr * v) >> 20, 0, 255)
    return b.astype(np.uint8), g.astype(np.uint8), r.astype(np.uint8)


def yuv420_to_bgr(frame, layout="nv12", matrix="bt601"):
    """One ``uint8 [H*3/2, W]`` frame -> ``uint8 [H,W,3]`` BGR"""
    y, u, v = planes(frame, layout)
    up = lambda c: np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)          # nearest: a 2x2 block shares its sample
    return np.stack(convert_triples(y, up(u), up(v), matrix), axis=2)


def float_bt601(Y, U, V):
    """Rounded float limited-range BT.601 (the coefficients the ``bt601`` row quantises) -> (B, G, R) uint8"""
    y = 1.164 * (np.maximum(np.asarray(Y, np.float64) - 16, 0))
    u, v = np.asarray(U, np.float64) - 128, np.asarray(V, np.float64) - 128
    f = lambda x: np.clip(np.floor(x + 0.5), 0, 255).astype(np.uint8)
    return f(y + 2.018 * u), f(y - 0.391 * u - 0.813 * v), f(y + 1.596 * v)


def bgr_to_yuv420(bgr, layout="nv12"):
    """Forward helper, used ONLY to manufacture realistic inputs: float limited-range BT.601, chroma = mean of the 2x2 block.
    ``uint8 [H,W,3]`` (H, W even) -> ``uint8 [H*3/2, W]``."""
    bgr = np.asarray(bgr)
    h, w = bgr.shape[:2]
    if h % 2 or w % 2:
        raise ValueError(f"odd size {h} x {w}")
    b, g, r = (bgr[..., i].astype(np.float64) for i in range(3))
    y = 16 + (65.481 * r + 128.553 * g + 24.966 * b) / 255
    u = 128 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255
    v = 128 + (112.0 * r - 93.786 * g - 18.214 * b) / 255
    mean = lambda c: c.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3))
    q = lambda c: np.clip(np.floor(c + 0.5), 0, 255).astype(np.uint8)
    return pack(q(y), q(mean(u)), q(mean(v)), layout)
