"""Face chips of the live path, on the device: detect -> align -> embed -> match -> CHIPS -> previews -> redact -> draw -> encode.

The engine knows where every face is and who it is; a consumer that has to show the face itself - the thumbnail of an
unknown-person event, the shot beside a recognition log line, the watch list beside a masked stream - needs the pixels.  The
frames live in the ring on the device (a YUV or JPEG call's host never holds a BGR picture at all), so that is where the chips are
cut: one launch (csrc/face_chips.hip) cuts a square around every selected face out of the full-size, unmasked, undrawn frames and
resamples it to ``size x size`` with an exact area filter, and the device JPEG encoder takes the batch of chips as it is.

The picture is DEFINED by tests/helpers/chip_ref.py (integers only) and the kernel reproduces it byte for byte.
``FaceChips.records`` is the host half: result dicts -> the records the kernel reads (include/frhip.h fr_face_chips_u8).
"""
import collections

import numpy as np

MAX_SIDE = 4096              # FR_CHIP_MAX_SIDE
MIN_SIZE, MAX_SIZE = 16, 256
COORD_LIMIT = 1 << 20
MIN_BATCH = 16               # records are padded to a power of two, at least this
KNOWN_TYPES = ("employee", "visitor")
DEFAULT = object()           # encode=DEFAULT: a JpegEncoder(quality=85) of the instance's own

# what ``FaceChips.begin`` queued and ``finish`` reads back: the device chips, the faces they belong to, what the encoder returned
_Pending = collections.namedtuple("_Pending", "chips owners coded results")


class FaceChips:
    """``size``: the chip's side S in pixels, 16 .. 256.  ``margin``: the square is the larger side of the face's box grown on
    each side by that many percent (0 .. 400).  ``who``: the faces that are chipped - a collection of ``person_info["type"]``
    values out of ``"employee"``, ``"visitor"``, ``"unknown"`` (every other type counts as unknown), or a callable
    ``result dict -> bool``, exactly as ``Redactor``'s.  It is the rate limiter as well: ``who=lambda r: not r.get("tracked")``
    chips a face only in the frames in which it was embedded afresh.

    ``encode``: a ``jpeg.JpegEncoder`` (by default one of quality 85, this object's own) - a chip is then the JPEG ``bytes`` of
    the ``S x S`` picture, encoded on the device -, or None: a chip is a ``uint8 [S, S, 3]`` BGR array.  ``fill``: the colour
    (B G R) of what lies outside the frame.

    ``masked=False`` is the fail-safe: in a call that also has a redactor, a face the redactor masks gets no chip - an unmasked
    picture of a masked face does not leave the device by the side door.  ``masked=True`` is the explicit opt-out (a watch-list
    dashboard beside a fully masked stream)."""

    def __init__(self, size=112, margin=30, who=("employee", "visitor", "unknown"), encode=DEFAULT, fill=(0, 0, 0), masked=False):
        self.size, self.margin, self.masked = int(size), int(margin), bool(masked)
        if not MIN_SIZE <= self.size <= MAX_SIZE:
            raise ValueError(f"size must be {MIN_SIZE}..{MAX_SIZE} (got {size})")
        if not 0 <= self.margin <= 400:
            raise ValueError(f"margin must be 0..400 percent (got {margin})")
        self.fill = tuple(int(v) for v in fill)
        if len(self.fill) != 3 or not all(0 <= v <= 255 for v in self.fill):
            raise ValueError(f"fill must be three bytes, B G R (got {fill!r})")
        if callable(who):
            self.who = who
        else:
            self.who = frozenset([who] if isinstance(who, str) else who)
            odd = self.who - set(KNOWN_TYPES) - {"unknown"}
            if odd:
                raise ValueError(f"who holds {sorted(odd)}: a type is 'employee', 'visitor' or 'unknown'")
        if encode is DEFAULT:
            from .jpeg import JpegEncoder
            encode = JpegEncoder(quality=85)
        if encode is not None and not (hasattr(encode, "encode_device") and hasattr(encode, "read_back")):
            raise ValueError("encode must be a jpeg.JpegEncoder or None")
        self.encode = encode

    # ---- host half: result dicts -> records
    def selects(self, result):
        """is this face chipped?"""
        if callable(self.who):
            return bool(self.who(result))
        kind = (result.get("person_info") or {}).get("type")
        return (kind if kind in KNOWN_TYPES else "unknown") in self.who

    def square(self, result):
        """One face's square ``(x0, y0, side)``: the box ordered as ``Redactor.face_region`` orders it, the larger of its sides
        grown by the margin and clamped to 1 .. 4096, centred on the box (floor divisions: also left of and above the frame)."""
        xa, ya, xb, yb = (int(v) for v in result["bbox"])
        x1, y1, x2, y2 = min(xa, xb), min(ya, yb), max(xa, xb), max(ya, yb)
        s0 = max(x2 - x1 + 1, y2 - y1 + 1)
        side = max(1, min(MAX_SIDE, s0 + 2 * (s0 * self.margin // 100)))
        return (x1 + x2 + 1 - side) // 2, (y1 + y2 + 1 - side) // 2, side

    def records(self, results_per_frame, redact=None):
        """The records of a batch: ``(int32 [F, 4], owners)``.  ``results_per_frame``: per frame what ``recognize_batch`` returns
        for it; an entry that is not a list (None, ``UNCHANGED``) contributes nothing.  ``owners``: the ``(frame, face)`` each of
        the first ``len(owners)`` records belongs to; F is ``len(owners)`` padded up to a power of two, at least 16, with records
        that name no frame (``frame = -1``), so that the buffers behind a call are keyed by a handful of shapes.  ``redact``: the
        call's redactor - a face it masks is left out unless ``masked``."""
        owners, rows = [], []
        for f, res in enumerate(results_per_frame):
            if not isinstance(res, (list, tuple)):
                continue
            for k, r in enumerate(res):
                if not self.selects(r) or (redact is not None and not self.masked and redact.selects(r)):
                    continue
                x0, y0, side = self.square(r)
                owners.append((f, k))                                  # a coordinate beyond the limit: the kernel answers fill
                rows.append((f, max(-COORD_LIMIT - 1, min(COORD_LIMIT + 1, x0)), max(-COORD_LIMIT - 1, min(COORD_LIMIT + 1, y0)), side))
        F = max(MIN_BATCH, 1 << max(len(rows) - 1, 0).bit_length())
        out = np.zeros((F, 4), np.int32)
        out[:, 0] = -1
        if rows:
            out[:len(rows)] = rows
        return out, owners

    # ---- device half
    @property
    def bgr_word(self):
        b, g, r = self.fill
        return b | (g << 8) | (r << 16)

    def cut_device(self, src, records, n=None):
        """The chips of ``records`` (host ``int32 [F, 4]`` or a device tensor of that shape) as a device ``uint8 [F, S, S, 3]``: one
        copy of the records and one launch on the current stream, no synchronisation.  ``src``: a device ``uint8 [n,H,W,3]`` BGR
        batch, or ``(arena, table)`` - a device arena of frames of differing sizes and their frame table (include/frhip.h
        fr_frame_ref) - with ``n``, the number of frames the table holds."""
        import torch
        from . import _lib
        lib = _lib.load()
        ragged = isinstance(src, (tuple, list))
        if ragged:
            arena, table = src
            if n is None:
                raise ValueError("a frame table needs n: the number of its frames")
            device = arena.device
        else:
            if src.dim() != 4 or src.shape[3] != 3 or src.dtype != torch.uint8 or not src.is_contiguous():
                raise ValueError("frames must be a contiguous device uint8 [n,H,W,3]")
            arena, table, device = src, None, src.device
            if n is not None and int(n) != int(src.shape[0]):
                raise ValueError(f"n = {n} but the batch holds {int(src.shape[0])} frames")
            n = int(src.shape[0])
        if not isinstance(records, torch.Tensor):
            records = np.ascontiguousarray(records, np.int32)
            if records.ndim != 2 or records.shape[1] != 4:
                raise ValueError("records must be int32 [F, 4]: frame, x0, y0, side")
            records = torch.from_numpy(records)
        if records.dim() != 2 or records.shape[1] != 4 or records.dtype != torch.int32:
            raise ValueError("records must be int32 [F, 4]: frame, x0, y0, side")
        F, S = int(records.shape[0]), self.size
        with torch.cuda.device(device):
            dev = records.to(device, non_blocking=True).contiguous()
            out = torch.empty((F, S, S, 3), dtype=torch.uint8, device=device)
            tail = (_lib.ptr(dev), F, S, self.bgr_word, _lib.ptr(out), _lib.stream_ptr())
            if ragged:
                lib.fr_face_chips_refs_u8(_lib.ptr(table), int(n), *tail)
            else:
                lib.fr_face_chips_u8(_lib.ptr(arena), n, int(arena.shape[1]), int(arena.shape[2]), *tail)
        return out

    def begin(self, src, results_per_frame, n=None, redact=None):
        """Queues the cut (and the encoder's launches) for a batch's results on the current stream and returns what ``finish``
        reads back; nothing is synchronised, so a caller can queue more work on the same frames behind it."""
        records, owners = self.records(results_per_frame, redact)
        if not owners:
            return _Pending(None, owners, None, results_per_frame)
        chips = self.cut_device(src, records, n)
        coded = None if self.encode is None else self.encode.encode_device(chips)
        return _Pending(chips, owners, coded, results_per_frame)

    def finish(self, pending):
        """Reads the chips back and writes ``"chip"`` into every face dict of the results ``begin`` was given: the JPEG
        ``bytes`` (None for a chip the encoder turned away) or the ``uint8 [S, S, 3]`` array of a selected face, None for every
        other.  Returns the results."""
        for res in pending.results:
            if isinstance(res, (list, tuple)):
                for r in res:
                    r["chip"] = None
        if pending.owners:
            k = len(pending.owners)                                      # the padding chips are dropped here
            if pending.coded is not None:
                got = self.encode.read_back(*pending.coded)[:k]
            else:
                host = pending.chips[:k].cpu().numpy()
                got = [host[i].copy() for i in range(k)]
            for (f, face), chip in zip(pending.owners, got):
                pending.results[f][face]["chip"] = chip
        return pending.results

    def cut(self, src, results_per_frame, n=None, redact=None):
        """``begin`` and ``finish`` in one: every face dict of ``results_per_frame`` gains ``"chip"``."""
        return self.finish(self.begin(src, results_per_frame, n, redact))
