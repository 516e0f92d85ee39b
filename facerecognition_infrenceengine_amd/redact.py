"""Face redaction of the live path, on the device: detect -> align -> embed -> match -> REDACT -> draw -> encode.

The engine publishes camera pictures - drawn frames, previews, JPEG snapshots and streams.  A deployment that shows them on a
dashboard is expected to mask faces: visitors who never consented, employees a works council protects, or everybody but a watch
list.  The only place that can be done for every camera is where the pictures are: on the device, behind the engine pass (which
sees the unmasked pixels) and in front of the HUD draw and the JPEG encoder, so that no unmasked picture of a masked face ever
crosses the link.  One launch for the whole batch (csrc/redact.hip) pixelates or fills the regions IN PLACE.

The picture is DEFINED by tests/helpers/redact_ref.py (integers only) and the kernel reproduces it byte for byte.
``Redactor.regions`` is the host half: result dicts -> the rectangles the kernel reads (include/frhip.h fr_redact_u8).
"""
import collections
import logging
import threading

import numpy as np

logger = logging.getLogger(__name__)

MAX_CAP = 64                 # FR_REDACT_MAX_CAP: regions of a frame
COORD_LIMIT = 1 << 20
MODES = {"pixelate": 0, "fill": 1}
KNOWN_TYPES = ("employee", "visitor")


def map_outward(lo, hi, n_out, n_in):
    """The inclusive range [lo, hi] of a side of ``n_in`` pixels on a preview of ``n_out``: floor(lo n_out / n_in) and
    ceil((hi + 1) n_out / n_in) - 1, in exact integers - every preview pixel that a source pixel of the range touches."""
    return lo * n_out // n_in, ((hi + 1) * n_out + n_in - 1) // n_in - 1


class Redactor:
    """``mode``: ``"pixelate"`` (a mosaic of ``block x block`` cells anchored at the picture's origin, each the rounded mean of
    its pixels) or ``"fill"`` (``colour``, B G R).  ``block``: 2 .. 64, in pixels of the picture that is redacted - the preview's
    with ``hud.out_size``.  ``margin``: a face's box is grown on each side by that many percent of its width and height.

    ``who``: the faces that are masked - a collection of ``person_info["type"]`` values out of ``"employee"``, ``"visitor"``,
    ``"unknown"`` (every other type counts as unknown), or a callable ``result dict -> bool``.  The default masks everybody;
    ``who=("unknown",)`` masks strangers only; a callable can spare a watch list.

    Fail-safe rules.  A frame whose results entry is None - nothing ran for it: no gallery, or it was answered ``UNCHANGED``
    with nothing held - is masked as a WHOLE with ``unprocessed="whole"`` (``"pass"`` leaves it as it is); an empty list means
    the engine ran and found no face, and the frame stays untouched.  A frame that would need more than 64 regions is masked as
    a whole, with a logged warning.  ``linger`` (0 .. 8): the regions of a key's last ``linger`` processed frames are added to
    its current frame's, so a face the detector misses for a frame or two stays masked; it needs ``keys`` (camera ids).  A
    frame without results neither adds to a key's history nor ages it.  ``forget(key)`` and ``reset()`` drop the history."""

    def __init__(self, mode="pixelate", block=16, colour=(0, 0, 0), margin=25, who=("employee", "visitor", "unknown"), linger=0,
                 unprocessed="whole"):
        if mode not in MODES:
            raise ValueError(f"mode must be 'pixelate' or 'fill' (got {mode!r})")
        self.mode, self.block, self.margin, self.linger = mode, int(block), int(margin), int(linger)
        if not 2 <= self.block <= 64:
            raise ValueError(f"block must be 2..64 (got {block})")
        if not 0 <= self.margin <= 400:
            raise ValueError(f"margin must be 0..400 percent (got {margin})")
        if not 0 <= self.linger <= 8:
            raise ValueError(f"linger must be 0..8 (got {linger})")
        if unprocessed not in ("whole", "pass"):
            raise ValueError(f"unprocessed must be 'whole' or 'pass' (got {unprocessed!r})")
        self.unprocessed = unprocessed
        self.colour = tuple(int(v) for v in colour)
        if len(self.colour) != 3 or not all(0 <= v <= 255 for v in self.colour):
            raise ValueError(f"colour must be three bytes, B G R (got {colour!r})")
        if callable(who):
            self.who = who
        else:
            self.who = frozenset([who] if isinstance(who, str) else who)
            odd = self.who - set(KNOWN_TYPES) - {"unknown"}
            if odd:
                raise ValueError(f"who holds {sorted(odd)}: a type is 'employee', 'visitor' or 'unknown'")
        self._lock = threading.Lock()
        self._history = {}                               # key -> deque(maxlen=linger) of region lists

    # ---- host half: result dicts -> regions
    def selects(self, result):
        """is this face masked?"""
        if callable(self.who):
            return bool(self.who(result))
        kind = (result.get("person_info") or {}).get("type")
        return (kind if kind in KNOWN_TYPES else "unknown") in self.who

    def face_region(self, result, frame_hw, out_hw=None):
        """One face's region ``(x1, y1, x2, y2)``, inclusive, on a ``frame_hw`` frame or on its ``out_hw = (nh, nw)`` preview:
        the box as ``Hud.records`` orders it, grown by the margin, clamped to +-2^20, mapped outward."""
        xa, ya, xb, yb = (int(v) for v in result["bbox"])
        x1, y1, x2, y2 = min(xa, xb), min(ya, yb), max(xa, xb), max(ya, yb)
        dx, dy = (x2 - x1 + 1) * self.margin // 100, (y2 - y1 + 1) * self.margin // 100
        x1, y1, x2, y2 = (max(-COORD_LIMIT, min(COORD_LIMIT, v)) for v in (x1 - dx, y1 - dy, x2 + dx, y2 + dy))
        if out_hw is not None:
            (H, W), (nh, nw) = (int(v) for v in frame_hw), (int(v) for v in out_hw)
            (x1, x2), (y1, y2) = map_outward(x1, x2, nw, W), map_outward(y1, y2, nh, H)
            x1, y1, x2, y2 = (max(-COORD_LIMIT, min(COORD_LIMIT, v)) for v in (x1, y1, x2, y2))
        return x1, y1, x2, y2

    def regions(self, results_per_frame, shapes, out_hws=None, keys=None):
        """The regions of a batch: ``(counts int32 [n], regions int32 [n, cap, 4], cap)``.  ``results_per_frame``: per frame what
        ``recognize_batch`` returns for it (a list, empty when no face was found; anything else: nothing ran).  ``shapes``: the
        frames' (H, W).  ``out_hws``: per frame the (nh, nw) its picture takes on a preview, when previews are redacted.
        ``keys``: one hashable id per frame (a camera id), what ``linger`` keeps its history under."""
        n = len(shapes)
        if len(results_per_frame) != n:
            raise ValueError(f"one results entry per frame: {n} frames, {len(results_per_frame)} entries")
        if out_hws is not None and len(out_hws) != n:
            raise ValueError(f"one preview size per frame: {n} frames, {len(out_hws)} sizes")
        if self.linger and keys is None:
            raise ValueError("linger needs keys: one id per frame (camera_ids) to hold a camera's history under")
        if keys is not None and len(keys) != n:
            raise ValueError(f"one key per frame: {n} frames, {len(keys)} keys")
        lists = []
        for f in range(n):
            hw = tuple(int(v) for v in shapes[f])
            out_hw = None if out_hws is None or out_hws[f] is None else tuple(int(v) for v in out_hws[f])
            ph, pw = out_hw if out_hw is not None else hw
            whole = (0, 0, pw - 1, ph - 1)
            res = results_per_frame[f]
            if not isinstance(res, (list, tuple)):                       # nothing ran for this frame
                lists.append([whole] if self.unprocessed == "whole" else [])
                continue
            fresh = list(dict.fromkeys(self.face_region(r, hw, out_hw) for r in res if self.selects(r)))
            regs = fresh
            if self.linger:
                with self._lock:
                    past = self._history.setdefault(keys[f], collections.deque(maxlen=self.linger))
                    regs = list(dict.fromkeys(fresh + [r for old in past for r in old]))
                    past.append(fresh if len(fresh) <= MAX_CAP else [whole])
            if len(regs) > MAX_CAP:
                logger.warning("redaction: a frame needs %d regions, more than %d: the whole picture is masked", len(regs), MAX_CAP)
                regs = [whole]
            lists.append(regs)
        cap = max(1, max((len(r) for r in lists), default=0))
        counts = np.zeros(n, np.int32)
        out = np.zeros((n, cap, 4), np.int32)
        for f, regs in enumerate(lists):
            counts[f] = len(regs)
            if regs:
                out[f, :len(regs)] = regs
        return counts, out, cap

    def forget(self, key):
        """a camera that is gone: its history is dropped"""
        with self._lock:
            self._history.pop(key, None)

    def reset(self):
        with self._lock:
            self._history.clear()

    # ---- device half
    @property
    def bgr_word(self):
        b, g, r = self.colour
        return b | (g << 8) | (r << 16)

    def apply(self, frames, results_per_frame, shapes=None, out_hws=None, keys=None):
        """Redacts every frame's regions IN PLACE, on the current stream, and returns the frames (``Hud.draw``'s twin): one host
        buffer, one copy, one launch.

        ``frames``: a device ``uint8 [n,H,W,3]`` BGR batch, or ``(arena, table)`` - a device arena of frames of differing sizes
        and their frame table (include/frhip.h fr_frame_ref) - with ``shapes``, the frames' (H, W) in table order.  With
        ``out_hws`` the batch given is a batch of PREVIEWS (``Hud.canvas``): ``shapes`` are the sizes of the frames they were made
        from, ``out_hws`` the (nh, nw) of each picture on its preview, and the regions are mapped outward onto it."""
        import torch
        from . import _lib
        lib = _lib.load()
        ragged = isinstance(frames, (tuple, list))
        if ragged:
            arena, table = frames
            if shapes is None:
                raise ValueError("a frame table needs shapes: the (H, W) of its frames")
            if out_hws is not None:
                raise ValueError("previews are a dense batch: out_hws does not go with a frame table")
            device = arena.device
        else:
            if frames.dim() != 4 or frames.shape[3] != 3 or frames.dtype != torch.uint8 or not frames.is_contiguous():
                raise ValueError("frames must be a contiguous device uint8 [n,H,W,3]")
            arena, table, device = frames, None, frames.device
            if shapes is None:
                if out_hws is not None:
                    raise ValueError("previews need shapes: the (H, W) of the frames they were made from")
                shapes = [(int(frames.shape[1]), int(frames.shape[2]))] * int(frames.shape[0])
            if len(shapes) != int(frames.shape[0]):
                raise ValueError(f"one shape per frame: {int(frames.shape[0])} frames, {len(shapes)} shapes")
        shapes = [(int(h), int(w)) for h, w in shapes]
        n = len(shapes)
        counts, regs, cap = self.regions(results_per_frame, shapes, out_hws, keys)
        if n == 0 or not counts.any():
            return arena
        buf = np.concatenate([counts, regs.reshape(-1)])
        with torch.cuda.device(device):
            dev = torch.from_numpy(buf).to(device)
            tail = (_lib.ptr(dev), cap, _lib.ptr(dev[n:]), self.block, MODES[self.mode], self.bgr_word, _lib.stream_ptr())
            if ragged:
                lib.fr_redact_refs_u8(_lib.ptr(table), n, *tail)
            else:
                lib.fr_redact_u8(_lib.ptr(arena), n, int(arena.shape[1]), int(arena.shape[2]), *tail)
        return arena
