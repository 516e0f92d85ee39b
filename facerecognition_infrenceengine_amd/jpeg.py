"""JPEG out: the drawn frames of the live path encoded on the device (csrc/jpeg_encode.hip), so that what crosses the link and
lands in a camera's queue is a JPEG file - a few hundred KB at 1080p instead of 6.2 MB of BGR.

The bytes are DEFINED by tests/helpers/jpeg_ref.py (integers only) and the kernel reproduces them byte for byte:
baseline, 4:2:0, the Annex K Huffman tables (jpeg_tables.py, the one copy), one restart interval per MCU row.  Any JPEG decoder
reads them; they are not libjpeg's bytes for the same picture and quality.
"""
import collections
import logging
import struct

import numpy as np

from . import jpeg_tables as T

logger = logging.getLogger(__name__)

OK, OVERFLOW, SKIPPED = 0, 1, 2          # include/frhip.h FR_JPEG_OK / _OVERFLOW / _SKIPPED
HEADER_BYTES = 629                       # FR_JPEG_HEADER_BYTES
AT_H, AT_W, AT_DRI = 163, 165, 613       # FR_JPEG_AT_*: where the kernel patches SOF0's H / W and DRI's interval
MAX_SIDE = 65535


def default_row_budget(w):
    """bytes a coded MCU row may take by default: the raw BGR size of the padded strip"""
    return 16 * 16 * ((int(w) + 15) // 16) * 3


class JpegEncoder:
    """``quality``: 1 .. 95 (libjpeg's scaling of the Annex K tables).  ``row_budget``: bytes a coded MCU row may take in
    the workspace (None: the raw size of the strip, which nothing short of adversarial input fills: uniform noise at quality
    95 takes 0.4 of it); a frame with a row that does not fit comes back as None."""

    def __init__(self, quality=80, row_budget=None):
        self.quality = int(quality)
        self.qtables = T.quant_tables(self.quality)              # raises on a quality outside 1 .. 95
        if row_budget is not None and int(row_budget) < 1:
            raise ValueError(f"row_budget must be at least 1 (got {row_budget})")
        self.row_budget = None if row_budget is None else int(row_budget)
        self._header = self._build_header()
        self._consts = {}                                        # device -> (header, codes, qtables) there
        self._work = collections.OrderedDict()                   # (device, n, H, W, budget, capacity) -> buffers

    # ---- host half
    def _build_header(self):
        out = [b"\xff\xd8", b"\xff\xe0" + struct.pack(">H5sBBBHHBB", 16, b"JFIF\0", 1, 1, 0, 1, 1, 0, 0)]
        for tid in (0, 1):
            out.append(b"\xff\xdb" + struct.pack(">HB", 67, tid) + self.qtables[tid][T.ZIGZAG].astype(np.uint8).tobytes())
        out.append(b"\xff\xc0" + struct.pack(">HBHHB", 17, 8, 0, 0, 3) + bytes((1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1)))
        for tc_th, (bits, vals) in T.HUFFMAN.items():
            out.append(b"\xff\xc4" + struct.pack(">HB", 19 + len(vals), tc_th) + bytes(bits) + bytes(vals))
        out.append(b"\xff\xdd" + struct.pack(">HH", 4, 0))
        out.append(b"\xff\xda" + struct.pack(">HB", 12, 3) + bytes((1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))
        head = b"".join(out)
        assert len(head) == HEADER_BYTES and head[AT_H - 5:AT_H - 3] == b"\xff\xc0" and head[AT_DRI - 4:AT_DRI - 2] == b"\xff\xdd"
        return head

    def header(self, h, w):
        """SOI .. SOS of an h x w picture at this quality: the device header with H, W and the restart interval filled in"""
        h, w = int(h), int(w)
        if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
            raise ValueError(f"H and W must be 1..{MAX_SIDE} (got {h} x {w})")
        head = bytearray(self._header)
        head[AT_H:AT_H + 4] = struct.pack(">HH", h, w)
        head[AT_DRI:AT_DRI + 2] = struct.pack(">H", (w + 15) // 16)
        return bytes(head)

    def frame_bound(self, h, w, row_budget=None):
        """bytes a frame's file can take at most under the row budget"""
        mh = (int(h) + 15) // 16
        return HEADER_BYTES + mh * ((row_budget or self.row_budget or default_row_budget(w)) + 2)

    # ---- device half
    def _consts_on(self, device):
        import torch
        key = str(device)
        if key not in self._consts:
            izz = np.empty(64, np.int32)
            izz[T.ZIGZAG] = np.arange(64, dtype=np.int32)
            qt = np.concatenate([self.qtables.reshape(-1), izz]).astype(np.int32)
            self._consts[key] = (torch.from_numpy(np.frombuffer(self._header, np.uint8).copy()).to(device),
                                 torch.from_numpy(T.code_table().view(np.int32).reshape(-1).copy()).to(device),
                                 torch.from_numpy(qt).to(device))
        return self._consts[key]

    def _buffers(self, lib, device, n, h, w, budget, capacity):
        """workspace, stream and meta (offsets i64 [n + 1], then status i32 [n]) for a batch shape, cached (the oldest of 4 dropped)"""
        import torch
        key = (str(device), n, h, w, budget, capacity)
        hit = self._work.get(key)
        if hit is None:
            while len(self._work) >= 4:
                self._work.popitem(last=False)
            ws_bytes = int(lib.fr_jpeg_workspace(n, h, w, budget))
            hit = (torch.empty(ws_bytes, dtype=torch.uint8, device=device), ws_bytes,
                   torch.empty(max(capacity, 1), dtype=torch.uint8, device=device),
                   torch.zeros(8 * (n + 1) + 4 * n, dtype=torch.uint8, device=device))
            self._work[key] = hit
        else:
            self._work.move_to_end(key)
        return hit

    def encode_device(self, frames, shapes=None, out_capacity=None):
        """Encodes every frame, on the current stream, without a synchronisation, and returns device tensors ``(stream uint8,
        offsets int64 [n + 1], status int32 [n])``: frame f's file is ``stream[offsets[f]:offsets[f + 1]]``; a frame whose
        status is not ``OK`` has length 0.  The tensors are this encoder's, valid until its next call for the same batch shape.

        ``frames``: a device ``uint8 [n,H,W,3]`` BGR batch, or ``(arena, table)`` - a device arena holding frames of differing
        sizes and their frame table (include/frhip.h fr_frame_ref, what ``RaggedIngest.upload`` returns and ``Hud.draw`` hands
        back) - with ``shapes``, the frames' (H, W) in table order.  ``out_capacity``: bytes of the stream (None: what the row
        budgets allow at most, so that no frame is ever turned away for the stream's sake)."""
        import torch
        from . import _lib
        lib = _lib.load()
        ragged = isinstance(frames, (tuple, list))
        if ragged:
            arena, table = frames
            if shapes is None:
                raise ValueError("a frame table needs shapes: the (H, W) of its frames")
            shapes = [(int(h), int(w)) for h, w in shapes]
            device = arena.device
        else:
            if frames.dim() != 4 or frames.shape[3] != 3 or frames.dtype != torch.uint8 or not frames.is_contiguous():
                raise ValueError("frames must be a contiguous device uint8 [n,H,W,3]")
            arena, table = frames, None
            shapes = [(int(frames.shape[1]), int(frames.shape[2]))] * int(frames.shape[0])
            device = frames.device
        n = len(shapes)
        if n == 0:
            return (torch.empty(0, dtype=torch.uint8, device=device), torch.zeros(1, dtype=torch.int64, device=device),
                    torch.empty(0, dtype=torch.int32, device=device))
        for h, w in shapes:
            if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
                raise ValueError(f"H and W must be 1..{MAX_SIDE} (got {h} x {w})")
        h, w = max(s[0] for s in shapes), max(s[1] for s in shapes)
        budget = self.row_budget or default_row_budget(w)
        capacity = sum(self.frame_bound(fh, fw, budget) for fh, fw in shapes) if out_capacity is None else int(out_capacity)
        with torch.cuda.device(device):
            ws, ws_bytes, out, meta = self._buffers(lib, device, n, h, w, budget, capacity)
            offsets, status = meta[:8 * (n + 1)].view(torch.int64), meta[8 * (n + 1):].view(torch.int32)
            head, codes, qt = self._consts_on(device)
            tail = (_lib.ptr(head), HEADER_BYTES, _lib.ptr(codes), _lib.ptr(qt), budget, _lib.ptr(out), capacity,
                    _lib.ptr(offsets), _lib.ptr(status), _lib.ptr(ws), ws_bytes, _lib.stream_ptr())
            if ragged:
                lib.fr_jpeg_encode_refs_u8(_lib.ptr(table), n, h, w, *tail)
            else:
                lib.fr_jpeg_encode_u8(_lib.ptr(arena), n, h, w, *tail)
        return out, offsets, status

    @staticmethod
    def split(stream, offsets, status):
        """host bytes of the stream, the n + 1 offsets and the n flags -> one ``bytes`` per frame, None (and a logged warning)
        for a frame that was flagged"""
        out = []
        for f, st in enumerate(status):
            if int(st) != OK:
                logger.warning("JPEG: frame %d was not encoded (%s)", f,
                               "a row or the stream overflowed its budget" if int(st) == OVERFLOW else "bad table entry")
                out.append(None)
            else:
                out.append(bytes(stream[int(offsets[f]):int(offsets[f + 1])]))
        return out

    def _pinned(self, nbytes):
        """a pinned host buffer of at least ``nbytes`` (one per encoder, grown in powers of two)"""
        import torch
        have = getattr(self, "_stage", None)
        if have is None or have.numel() < nbytes:
            have = self._stage = torch.empty(1 << max(int(nbytes) - 1, 4095).bit_length(), dtype=torch.uint8).pin_memory()
        return have

    def read_back(self, stream, offsets, status):
        """What ``encode_device`` returned -> one ``bytes`` per frame, None (and a logged warning) for a flagged frame.  The
        pinned stage receives the n + 1 offsets with the flags, and then exactly ``offsets[n]`` bytes of the stream: two
        copies on the current stream, a synchronisation behind each."""
        import torch
        n = int(status.numel())
        if n == 0:
            return []
        with torch.cuda.device(stream.device):
            queue = torch.cuda.current_stream(stream.device)
            stage = self._pinned(8 * (n + 1) + 4 * n)
            host_off, host_st = stage[:8 * (n + 1)].view(torch.int64), stage[8 * (n + 1):8 * (n + 1) + 4 * n].view(torch.int32)
            host_off.copy_(offsets, non_blocking=True)
            host_st.copy_(status, non_blocking=True)
            queue.synchronize()
            offs, flags = host_off.numpy().copy(), host_st.numpy().copy()
            total = int(offs[n])
            stage = self._pinned(total)
            stage[:total].copy_(stream[:total], non_blocking=True)
            queue.synchronize()
        return self.split(memoryview(stage.numpy())[:total], offs, flags)

    def encode(self, frames, shapes=None, out_capacity=None):
        """``encode_device``, then ``read_back``: the files on the host, one ``bytes`` per frame, None (and a logged warning)
        for a frame that overflowed."""
        return self.read_back(*self.encode_device(frames, shapes, out_capacity))
