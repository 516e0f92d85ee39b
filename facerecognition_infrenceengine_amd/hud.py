"""The HUD of the live path, drawn on the device: detect -> align -> embed -> match -> DRAW.

The reference's ``recognize_faces(frame, company_id)`` returns the frame with a HUD on every face - a blended box, corner
ticks, two confidence bars and an info panel (infrenceServer.py:418-513) - drawn with OpenCV on the host, one
process per camera.  Here the BGR frames of a batch are on the device already (the ingest ring put or converted them there),
so the HUD is drawn there, in one launch for the whole batch (csrc/hud_draw.hip), and only what the viewer needs is read back:
the frames, or - with ``out_size`` - previews resized on the device by the pinned letterbox resize.

The picture is DEFINED by tests/helpers/hud_ref.py (integers only) and the kernel reproduces it byte for byte.
``Hud.records`` is the host half: result dicts -> the fixed records the kernel reads (include/frhip.h fr_hud_draw_u8).
"""
import collections
import logging
import math

import numpy as np

from .hud_font import FONT

logger = logging.getLogger(__name__)

K = 16                       # ints of a face record (include/frhip.h FR_HUD_K)
MAX_CAP = 64                 # FR_HUD_MAX_CAP: faces drawn per frame
MAX_CHARS = 64               # FR_HUD_MAX_CHARS
MAX_LINES = 4
COORD_LIMIT = 1 << 20
COLOURS = {"employee": (0, 255, 0), "visitor": (0, 255, 255)}          # as FaceRecognitionProcessor.annotate picks them
UNKNOWN_COLOUR = (0, 0, 255)


def _ascii(s, max_chars):
    """one byte per character, cut to ``max_chars``; whatever is not printable ASCII becomes '?'"""
    return bytes(ord(ch) if 0x20 <= ord(ch) <= 0x7E else 0x3F for ch in str(s)[:max_chars])


def _bar(span, score):
    """rows of a confidence bar: int(span * min(score, 1.0)) in Python floats, clamped to [0, span]; NaN gives 0"""
    score = float(score)
    if math.isnan(score):
        return 0
    return max(0, min(int(span * min(score, 1.0)), span))


def info_lines(result):
    """The panel's lines for one result dict, by the person's type (infrenceServer.py:457-475)."""
    info = result["person_info"]
    kind = info.get("type")
    if kind == "employee":
        return [f"Name: {info.get('name', '')}", f"ID: {info.get('employeeId', '')}", "Type: Employee",
                "Score: %.2f" % float(result["recognition_score"])]
    if kind == "visitor":
        return [f"Name: {info.get('name', '')}", "Type: Visitor", "Score: %.2f" % float(result["recognition_score"])]
    return ["Unknown Person", "Detection: %.2f" % float(result["det_score"])]


class Hud:
    """``scale``: an integer 1 .. 8 that multiplies every length of the HUD (2 suits 1080p).  ``out_size=(w, h)``: draw on
    previews of that size instead of the frames themselves (the frame resized to fit, top-left, zero padded).  ``max_chars``:
    where a text line is cut (1 .. 64).  ``font``: a ``uint8 [95, 7]`` table in place of hud_font.FONT."""

    def __init__(self, scale=1, out_size=None, max_chars=40, font=None):
        from .letterbox import check_det_size
        self.scale, self.max_chars = int(scale), int(max_chars)
        if not 1 <= self.scale <= 8:
            raise ValueError(f"scale must be 1..8 (got {scale})")
        if not 1 <= self.max_chars <= MAX_CHARS:
            raise ValueError(f"max_chars must be 1..{MAX_CHARS} (got {max_chars})")
        self.out_size = check_det_size(out_size)
        self.font = np.ascontiguousarray(FONT if font is None else font, dtype=np.uint8)
        if self.font.shape != FONT.shape:
            raise ValueError(f"font must be uint8 {FONT.shape}, got {self.font.shape}")
        self._font_dev = {}                              # device -> the font there
        self._tables = collections.OrderedDict()         # preview frame tables, by what they were made for

    # ---- host half: result dicts -> records
    def out_hw(self, frame_hw):
        """(nh, nw): the size a frame's picture takes on a preview; None without ``out_size``."""
        if self.out_size is None:
            return None
        from .letterbox import letterbox_geometry
        return letterbox_geometry(frame_hw[0], frame_hw[1], self.out_size)[:2]

    def records(self, results, frame_hw, out_hw=None):
        """One frame's result dicts (what ``recognize_batch`` returns for it) -> ``(faces int32 [m, K], text uint8
        [m, 4, max_chars])``: box (coordinates ordered), colour, bar heights, line count, line lengths; the lines' bytes.
        With ``out_hw = (nh, nw)`` the frame's picture is nh x nw (a preview) and a corner maps to floor(x nw / W),
        floor(y nh / H), in exact integers."""
        results = list(results or ())
        faces = np.zeros((len(results), K), np.int32)
        text = np.zeros((len(results), MAX_LINES, self.max_chars), np.uint8)
        H, W = (int(v) for v in frame_hw)
        for j, r in enumerate(results):
            xa, ya, xb, yb = (int(v) for v in r["bbox"])
            if out_hw is not None:
                nh, nw = (int(v) for v in out_hw)
                xa, xb, ya, yb = xa * nw // W, xb * nw // W, ya * nh // H, yb * nh // H
            x1, y1, x2, y2 = (max(-COORD_LIMIT, min(COORD_LIMIT, v)) for v in (min(xa, xb), min(ya, yb), max(xa, xb), max(ya, yb)))
            lines = [_ascii(s, self.max_chars) for s in info_lines(r)]
            faces[j, 0:4] = x1, y1, x2, y2
            faces[j, 4:7] = COLOURS.get(r["person_info"].get("type"), UNKNOWN_COLOUR)
            faces[j, 7], faces[j, 8] = _bar(y2 - y1, r["det_score"]), _bar(y2 - y1, r["recognition_score"])
            faces[j, 9] = len(lines)
            for i, b in enumerate(lines):
                faces[j, 10 + i] = len(b)
                text[j, i, :len(b)] = np.frombuffer(b, np.uint8)
        return faces, text

    def pack(self, results_per_frame, shapes):
        """The records of a batch as ONE host buffer and its layout: ``(uint8 buffer, cap, offset of faces, offset of text)``;
        counts ``int32 [n]`` come first.  A frame whose results are None or empty has count 0; a frame with more than 64 faces
        gets its first 64 drawn."""
        n = len(shapes)
        recs = [self.records(res if isinstance(res, (list, tuple)) else None, hw, self.out_hw(hw))
                for res, hw in zip(results_per_frame, shapes)]
        most = max((len(f) for f, _ in recs), default=0)
        if most > MAX_CAP:
            logger.warning("HUD: a frame has %d faces, the first %d are drawn", most, MAX_CAP)
        cap = max(1, min(most, MAX_CAP))
        at_faces = 4 * n
        at_text = at_faces + 4 * n * cap * K
        buf = np.zeros(at_text + n * cap * MAX_LINES * self.max_chars, np.uint8)
        counts = buf[:at_faces].view(np.int32)
        faces = buf[at_faces:at_text].view(np.int32).reshape(n, cap, K)
        text = buf[at_text:].reshape(n, cap, MAX_LINES, self.max_chars)
        for f, (fa, tx) in enumerate(recs):
            m = min(len(fa), cap)
            counts[f] = m
            faces[f, :m], text[f, :m] = fa[:m], tx[:m]
        return buf, cap, at_faces, at_text

    # ---- device half
    def _font_on(self, device):
        import torch
        key = str(device)
        if key not in self._font_dev:
            self._font_dev[key] = torch.from_numpy(self.font.copy()).to(device)
        return self._font_dev[key]

    def _preview_table(self, frames, table, shapes):
        """The frame table of the letterbox into ``out_size``: the given table's rows with nh / nw of the preview (device
        arithmetic on the table, no pointer crosses the link), or a table of its own for a dense batch."""
        import torch
        from .letterbox import frame_table
        dense = table is None
        key = (frames.data_ptr(), tuple(shapes), self.out_size) if dense else (table.data_ptr(), tuple(shapes), self.out_size)
        hit = self._tables.get(key)
        if hit is not None:
            return hit
        if dense:
            h, w = shapes[0]
            tab, _ = frame_table([frames.data_ptr() + i * h * w * 3 for i in range(len(shapes))], shapes, self.out_size)
            dev_tab = torch.from_numpy(tab).to(frames.device)
        else:
            geo = torch.tensor([self.out_hw(hw) for hw in shapes], dtype=torch.int32).to(table.device)
            rows = table.view(torch.int32).view(-1, 8).clone()           # fr_frame_ref: pointer (2 ints), H, W, nh, nw, reserved
            rows[:, 4:6] = geo
            dev_tab = rows.view(torch.uint8).reshape(-1)
        while len(self._tables) >= 16:
            self._tables.popitem(last=False)
        self._tables[key] = dev_tab
        return dev_tab

    def _frames(self, frames, shapes):
        """``frames`` as ``draw`` takes them -> (arena, table or None, shapes, device)"""
        import torch
        if isinstance(frames, (tuple, list)):
            arena, table = frames
            if shapes is None:
                raise ValueError("a frame table needs shapes: the (H, W) of its frames")
            return arena, table, [(int(h), int(w)) for h, w in shapes], arena.device
        if frames.dim() != 4 or frames.shape[3] != 3 or frames.dtype != torch.uint8 or not frames.is_contiguous():
            raise ValueError("frames must be a contiguous device uint8 [n,H,W,3]")
        return frames, None, [(int(frames.shape[1]), int(frames.shape[2]))] * int(frames.shape[0]), frames.device

    def canvas(self, frames, shapes=None):
        """The first step of ``draw`` on its own: with ``out_size=(w, h)`` the frames resized into a new ``uint8 [n,h,w,3]``
        (fr_letterbox_u8: top-left, zero padded) on the current stream; None without ``out_size`` or without frames.  What it
        returns goes to ``draw(..., canvas=...)``, so that something else - the redaction - can work on the previews between
        the two launches."""
        import torch
        from . import _lib
        arena, table, shapes, device = self._frames(frames, shapes)
        if self.out_size is None or not shapes:
            return None
        n, (w, h) = len(shapes), self.out_size
        with torch.cuda.device(device):
            refs = self._preview_table(arena, table, shapes)
            canvas = torch.empty((n, h, w, 3), dtype=torch.uint8, device=device)
            _lib.load().fr_letterbox_u8(_lib.ptr(refs), n, _lib.ptr(canvas), h, w, _lib.stream_ptr())
        return canvas

    def draw(self, frames, results_per_frame, shapes=None, canvas=None):
        """Draws the HUD of every frame's results, on the current stream, and returns the drawn frames on the device.

        ``frames``: a device ``uint8 [n,H,W,3]`` BGR batch, or ``(arena, table)`` - a device arena holding frames of differing
        sizes and their frame table (include/frhip.h fr_frame_ref, what ``RaggedIngest.upload`` returns) - with ``shapes``, the
        frames' (H, W) in table order.  ``results_per_frame``: per frame what ``recognize_batch`` returns for it; a frame whose
        entry is None or empty (or no list at all) comes back undrawn.

        Without ``out_size`` the frames are drawn IN PLACE and returned (the batch tensor, or the arena).  With
        ``out_size=(w, h)`` the frames are first resized into a new ``uint8 [n,h,w,3]`` (fr_letterbox_u8: top-left, zero
        padded), the HUD is drawn on that, boxes mapped by ``records``, and the frames given stay as they were.  ``canvas``:
        the previews ``canvas(frames, shapes)`` made of these frames; they are drawn on instead of a resize of their own."""
        import torch
        from . import _lib
        lib = _lib.load()
        arena, table, shapes, device = self._frames(frames, shapes)
        ragged = table is not None
        n = len(shapes)
        if len(results_per_frame) != n:
            raise ValueError(f"one results entry per frame: {n} frames, {len(results_per_frame)} entries")
        if n == 0:
            return arena
        if canvas is not None and (self.out_size is None or tuple(canvas.shape) != (n, self.out_size[1], self.out_size[0], 3)):
            raise ValueError("canvas must be what canvas(frames, shapes) returns for these frames")
        with torch.cuda.device(device):
            stream = _lib.stream_ptr()
            if self.out_size is not None and canvas is None:
                canvas = self.canvas(frames, shapes)
            if not any(isinstance(r, (list, tuple)) and len(r) for r in results_per_frame):
                return canvas if canvas is not None else arena
            buf, cap, at_faces, at_text = self.pack(results_per_frame, shapes)
            dev = torch.from_numpy(buf).to(device)
            counts, faces, text = dev[:at_faces], dev[at_faces:at_text], dev[at_text:]
            font = self._font_on(device)
            tail = (_lib.ptr(counts), cap, _lib.ptr(faces), _lib.ptr(text), self.max_chars, _lib.ptr(font), self.scale, stream)
            if canvas is not None:
                lib.fr_hud_draw_u8(_lib.ptr(canvas), n, canvas.shape[1], canvas.shape[2], *tail)
                return canvas
            if ragged:
                lib.fr_hud_draw_refs_u8(_lib.ptr(table), n, *tail)
            else:
                lib.fr_hud_draw_u8(_lib.ptr(arena), n, shapes[0][0], shapes[0][1], *tail)
            return arena
