"""JPEG in: the files of an MJPEG camera and of enrolment uploads decoded on the device (csrc/jpeg_decode.hip), so that what
crosses the link is the file - a few hundred KB at 1080p instead of 6.2 MB of BGR - and the host thread that feeds the GPU
never decodes.

The pixels are DEFINED by tests/helpers/jpeg_decode_ref.py (integers only) and the kernels reproduce them byte
for byte; the definition is libjpeg's arithmetic, so they are also the pixels ``ingest.decode_image`` (Pillow) gives for the same
file.  The host reads SOI .. SOS only (``parse``: a walk over segment lengths); the entropy data is never touched here.

Supported: baseline sequential (SOF0), 8 bit, one interleaved scan, 3 components at 4:4:4 / 4:2:2 / 4:2:0 or 1 component, any
DQT / DHT contents, any restart interval or none.  Everything else - progressive, arithmetic coding, 16-bit DQT, CMYK, other
sampling factors, several scans - ``parse`` names as a reason string without a launch, and the caller falls back to
``decode_image``.

EXIF orientation (``exif_orientation``, ``orient``; ``JpegDecoder(..., orient=True)``): a phone held upright writes the sensor's
landscape picture and says in an Exif tag how to turn it.  ``cv2.imdecode`` applies the tag; with ``orient=True`` so does the
device decoder, in the launch that writes the pixels.  Off by default: the pixels as coded."""
import collections
import logging
import struct

import numpy as np

from . import jpeg_tables as T

logger = logging.getLogger(__name__)

OK, BAD_STREAM, SKIPPED = 0, 1, 2                       # include/frhip.h FR_JPEGD_OK / _BAD_STREAM / _SKIPPED
S444, S422, S420, GRAY = 0, 1, 2, 3                     # FR_JPEGD_444 / _422 / _420 / _GRAY
HUFF_ROW = 804                                          # FR_JPEGD_HUFF_ROW
MAX_SIDE = 65535
MAX_SCAN = 1 << 28
# include/frhip.h fr_jpeg_frame
FRAME = np.dtype([("scan_off", "<i8"), ("scan_len", "<i4"), ("H", "<i4"), ("W", "<i4"), ("sampling", "<i4"), ("restart", "<i4"),
                  ("qsel", "<i4", 3), ("dcsel", "<i4", 3), ("acsel", "<i4", 3)])
assert FRAME.itemsize == 64
_SAMPLING = {(0x11, 0x11, 0x11): S444, (0x21, 0x11, 0x11): S422, (0x22, 0x11, 0x11): S420}
_MCU = {S444: (8, 8), S422: (16, 8), S420: (16, 16), GRAY: (8, 8)}

Header = collections.namedtuple("Header", "H W sampling restart scan qtables huffman segments")
Header.__doc__ = """What ``parse`` reads from SOI .. SOS.  ``scan``: offset of the entropy data; ``qtables``: per component the 64
bytes of its DQT table (zigzag order, as in the file); ``huffman``: per component ``(dc, ac)``, each the BITS + HUFFVAL bytes of
its DHT table; ``segments``: the restart intervals the scan holds."""


def _huffman_ok(table):
    """BITS + HUFFVAL bytes describe a prefix code (T.81 Annex C): no length holds more codes than fit"""
    code = 0
    for length in range(1, 17):
        code += table[length - 1]
        if code > 1 << length:
            return False
        code <<= 1
    return True


def parse(data):
    """The header of a JPEG file: a ``Header``, or a string that says why the device decoder does not take the file (not a
    JPEG, cut short, or a kind of JPEG it does not decode).  Never raises, never reads the entropy data."""
    try:
        data = memoryview(data).cast("B")
    except TypeError:
        return "not bytes"
    n = len(data)
    if n < 2 or data[0] != 0xFF or data[1] != 0xD8:
        return "not a JPEG file (no SOI)"
    pos, quant, huff, restart, frame = 2, {}, {}, 0, None
    while True:
        if pos + 4 > n:
            return "header cut short"
        if data[pos] != 0xFF:
            return "no marker where one is due"
        marker = data[pos + 1]
        if marker == 0xFF:                               # a fill byte
            pos += 1
            continue
        if marker == 0xD9 or 0xD0 <= marker <= 0xD7 or marker == 0x01:
            return "marker 0x%02X before SOS" % marker
        length = data[pos + 2] << 8 | data[pos + 3]
        if length < 2 or pos + 2 + length > n:
            return "segment cut short"
        seg = bytes(data[pos + 4:pos + 2 + length])
        pos += 2 + length
        if marker == 0xDB:
            while seg:
                if seg[0] >> 4:
                    return "unsupported: 16-bit quantisation table"
                if len(seg) < 65 or seg[0] > 3:
                    return "broken DQT"
                quant[seg[0]] = seg[1:65]
                seg = seg[65:]
        elif marker == 0xC4:
            while seg:
                if len(seg) < 17 or (seg[0] & 0xEF) > 3:
                    return "broken DHT"
                count = sum(seg[1:17])
                if count > 256 or len(seg) < 17 + count or not _huffman_ok(seg[1:17]):
                    return "broken DHT"
                huff[seg[0]] = seg[1:17 + count]
                seg = seg[17 + count:]
        elif marker == 0xC0:
            if frame is not None or len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
                return "broken SOF0"
            frame = seg
        elif 0xC1 <= marker <= 0xCF and marker not in (0xC4, 0xC8, 0xCC):
            return "unsupported: SOF%d (%s)" % (marker - 0xC0, {2: "progressive", 1: "extended sequential"}.get(
                marker - 0xC0, "lossless, differential or arithmetic coding"))
        elif marker == 0xCC:
            return "unsupported: arithmetic coding"
        elif marker == 0xDD:
            if len(seg) != 2:
                return "broken DRI"
            restart = seg[0] << 8 | seg[1]
        elif marker == 0xDA:
            break
    if frame is None:
        return "SOS before SOF0"
    prec, h, w, nc = struct.unpack(">BHHB", frame[:6])
    comps = [tuple(frame[6 + 3 * i:9 + 3 * i]) for i in range(nc)]
    if prec != 8:
        return "unsupported: %d-bit samples" % prec
    if nc not in (1, 3):
        return "unsupported: %d components" % nc
    if h == 0:
        return "unsupported: height 0 (DNL)"
    if w == 0:
        return "broken SOF0"
    sampling = GRAY if nc == 1 else _SAMPLING.get(tuple(c[1] for c in comps))
    if sampling is None:
        return "unsupported: sampling factors " + " ".join("%02x" % c[1] for c in comps)
    if len(seg) != 4 + 2 * nc or seg[0] != nc:
        return "unsupported: a scan of %d of %d components" % (seg[0] if seg else 0, nc)
    if tuple(seg[1 + 2 * nc:]) != (0, 63, 0):
        return "unsupported: not a baseline scan"
    qtables, huffman = [], []
    for i, (cid, _, tq) in enumerate(comps):
        if seg[1 + 2 * i] != cid:
            return "unsupported: scan order"
        td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
        if tq not in quant or td not in huff or 0x10 | ta not in huff:
            return "a table the scan names is missing"
        qtables.append(quant[tq])
        huffman.append((huff[td], huff[0x10 | ta]))
    if n - pos >= MAX_SCAN:
        return "unsupported: a scan of 2^28 bytes and more"
    mw, mh = _MCU[sampling]
    mcus = ((w + mw - 1) // mw) * ((h + mh - 1) // mh)
    return Header(h, w, sampling, restart, pos, tuple(qtables), tuple(huffman), (mcus + restart - 1) // restart if restart else 1)


def exif_orientation(data):
    """The EXIF orientation a JPEG file carries, 1 .. 8; 1 (as coded) for a file without one.  Walks SOI .. SOS by segment
    lengths as ``parse`` does and takes the FIRST ``APP1`` segment whose payload begins ``Exif\\0\\0``: the TIFF header (``II`` /
    ``MM``, 42, the offset of IFD0), then IFD0's entries up to tag 0x0112, of type SHORT (count 1 or 2) or LONG (count 1); its
    first value when that is 1 .. 8.  Everything else is 1: no such segment or tag, another type or count, another value, an
    offset or entry count that leaves the segment, a file cut short.  Never raises, never reads the entropy data."""
    try:
        data = memoryview(data).cast("B")
    except TypeError:
        return 1
    n = len(data)
    if n < 2 or data[0] != 0xFF or data[1] != 0xD8:
        return 1
    pos = 2
    while pos + 4 <= n and data[pos] == 0xFF:
        marker = data[pos + 1]
        if marker == 0xFF:                               # a fill byte
            pos += 1
            continue
        if marker in (0xDA, 0xD9, 0x01) or 0xD0 <= marker <= 0xD7:
            return 1
        length = data[pos + 2] << 8 | data[pos + 3]
        if length < 2 or pos + 2 + length > n:
            return 1
        if marker == 0xE1 and length >= 8 and bytes(data[pos + 4:pos + 10]) == b"Exif\0\0":
            return _tiff_orientation(bytes(data[pos + 10:pos + 2 + length]))
        pos += 2 + length
    return 1


def _tiff_orientation(tiff):
    """tag 0x0112 of IFD0 of a TIFF structure (the payload of an Exif segment behind its six-byte name), or 1"""
    if len(tiff) < 8 or tiff[:2] not in (b"II", b"MM"):
        return 1
    order = "<" if tiff[:2] == b"II" else ">"
    magic, ifd = struct.unpack(order + "HI", tiff[2:8])
    if magic != 42 or ifd + 2 > len(tiff):
        return 1
    count, = struct.unpack_from(order + "H", tiff, ifd)
    if ifd + 2 + 12 * count > len(tiff):
        return 1
    for e in range(count):
        tag, kind, values = struct.unpack_from(order + "HHI", tiff, ifd + 2 + 12 * e)
        if tag != 0x0112:
            continue
        if kind == 3 and values in (1, 2):
            value, = struct.unpack_from(order + "H", tiff, ifd + 10 + 12 * e)
        elif kind == 4 and values == 1:
            value, = struct.unpack_from(order + "I", tiff, ifd + 10 + 12 * e)
        else:
            return 1
        return value if 1 <= value <= 8 else 1
    return 1


def orient(img, o):
    """``[H,W,C]`` array -> the picture EXIF orientation ``o`` (1 .. 8) asks for, as a view: ``[H,W,C]`` for 1 .. 4, ``[W,H,C]``
    for 5 .. 8.  What ``PIL.ImageOps.exif_transpose`` does, and ``cv2.imdecode``; tests/helpers/orient_ref.py is its twin."""
    if o in (2, 3, 7, 8):
        img = img[:, ::-1]
    if o in (3, 4, 6, 7):
        img = img[::-1]
    return img.transpose(1, 0, 2) if o > 4 else img


def oriented_shape(shape, o):
    """(H, W) of a coded picture -> (H, W) of the picture orientation ``o`` turns it into"""
    return (shape[1], shape[0]) if o > 4 else tuple(shape)


def _view(blob):
    try:
        return memoryview(blob).cast("B")
    except TypeError:                                    # not bytes: parse says so
        return memoryview(b"")


def quant_row(table):
    """the 64 bytes of a DQT table (zigzag order) -> ``int32 [64]``, natural order"""
    out = np.empty(64, np.int32)
    out[T.ZIGZAG] = np.frombuffer(table, np.uint8)
    return out


def huffman_row(table):
    """BITS + HUFFVAL bytes -> ``int32 [HUFF_ROW]``, what the kernel reads (include/frhip.h fr_jpeg_decode_refs_u8): [0, 512) the
    next 9 bits -> ``length << 8 | symbol`` (0: a longer code or none), [512, 530) the largest code of each length (-1: none),
    [530, 548) ``valptr - mincode`` of each length, [548, 804) HUFFVAL."""
    bits, vals = table[:16], table[16:]
    row = np.zeros(HUFF_ROW, np.int32)
    row[512:530] = -1
    code, k = 0, 0
    for length in range(1, 17):
        count = bits[length - 1]
        if count:
            row[530 + length] = k - code
            if length <= 9:
                for j in range(count):
                    row[(code + j) << (9 - length):(code + j + 1) << (9 - length)] = length << 8 | vals[k + j]
            code, k = code + count, k + count
            row[512 + length] = code - 1
        code <<= 1
    row[548:548 + len(vals)] = np.frombuffer(bytes(vals), np.uint8)
    return row


class JpegDecoder:
    """Decodes batches of JPEG files on ``device``.  The quantisation and Huffman tables go to the device once per distinct
    table, cached by the bytes of their DQT / DHT segments: a camera sends the same ones in every frame.

    ``orient=True``: every file is written as its EXIF orientation turns it (``exif_orientation``; what ``cv2.imdecode`` returns),
    so ``shapes`` and the frames are the ORIENTED ones - W x H for orientations 5 .. 8 - and ``last_orientations`` says what each
    file of the last call carried.  The turn happens in the launch that writes the pixels (jpegd_colour_oriented): no second
    pass, no second buffer; a batch without a turned file takes the path of ``orient=False``, launch for launch."""

    MAX_TABLES = 1024                                    # of either kind; past it the cache starts again
    STAGES = 3                                           # pinned staging buffers in rotation

    def __init__(self, device="cuda:0", orient=False):
        import torch
        self.device = torch.device(device)
        self.orient = bool(orient)
        self.last_orientations = []                      # per blob of the last call: 1 .. 8 (all 1 without ``orient``)
        self.last_fallbacks = {}                         # frame index -> why the device did not take it (the last call's)
        self._quant, self._huff = {}, {}                 # table bytes -> row
        self._qrows, self._hrows = [], []
        self._tables = None                              # (qtables, htables) on the device, None when rows were added
        self._natural = None
        self._stages = [None] * self.STAGES              # [pinned tensor, event of its last copy]
        self._turn = 0
        self._work = collections.OrderedDict()           # (n, H, W, segments) -> workspace

    # ---- host half
    def _row(self, cache, rows, table, build):
        at = cache.get(table)
        if at is None:
            at = cache[table] = len(rows)
            rows.append(build(table))
        return at

    def trim_tables(self):
        """the cache starts again once it holds more than ``MAX_TABLES`` rows of either kind (files with per-file tables over a
        long run); only between calls: descriptors already filled name rows by their index"""
        if len(self._qrows) > self.MAX_TABLES or len(self._hrows) > self.MAX_TABLES:
            self._quant, self._huff, self._qrows, self._hrows, self._tables = {}, {}, [], [], None

    def describe_into(self, rec, hd, scan_len):
        """fills one ``FRAME`` record (``scan_off`` is the caller's) from a header; new tables enter the cache"""
        rec["scan_len"], rec["H"], rec["W"], rec["sampling"], rec["restart"] = scan_len, hd.H, hd.W, hd.sampling, hd.restart
        for c in range(len(hd.qtables)):
            rec["qsel"][c] = self._row(self._quant, self._qrows, hd.qtables[c], quant_row)
            rec["dcsel"][c] = self._row(self._huff, self._hrows, hd.huffman[c][0], huffman_row)
            rec["acsel"][c] = self._row(self._huff, self._hrows, hd.huffman[c][1], huffman_row)

    def describe(self, blobs):
        """``parse`` of every blob -> ``(frames, headers)``: a ``FRAME`` record array (``scan_off`` still 0, ``scan_len`` the
        bytes behind SOS) and the list of headers, None where the device does not take the blob (``last_fallbacks`` says
        why; its record stays zero, which the kernel skips).  With ``orient`` also ``exif_orientation`` of every blob, into
        ``last_orientations``."""
        self.trim_tables()
        self.last_orientations = [exif_orientation(b) for b in blobs] if self.orient else [1] * len(blobs)
        frames = np.zeros(len(blobs), FRAME)
        headers, self.last_fallbacks = [], {}
        for f, blob in enumerate(blobs):
            hd = parse(blob)
            if isinstance(hd, str):
                self.last_fallbacks[f] = hd
                headers.append(None)
                continue
            headers.append(hd)
            self.describe_into(frames[f], hd, len(blob) - hd.scan)
        return frames, headers

    # ---- device half
    def _tables_on_device(self):
        """``(qtables, htables)`` on the device, on the current stream.  The tensors have room to spare and only the rows that
        are new since the last call go up; they are replaced (and their rows copied on the device) when the room runs out."""
        import torch
        if self._natural is None:
            self._natural = torch.from_numpy(T.ZIGZAG.astype(np.int32)).to(self.device)
        if self._tables is None:                         # first use, or the cache started again
            self._tables, self._up = [None, None], [0, 0]
        for i, (rows, width) in enumerate(((self._qrows, 64), (self._hrows, HUFF_ROW))):
            dev = self._tables[i]
            if dev is None or len(rows) > dev.shape[0]:
                grown = torch.zeros((max(32, 2 * len(rows)), width), dtype=torch.int32, device=self.device)
                if dev is not None:
                    grown[:self._up[i]].copy_(dev[:self._up[i]])
                dev = self._tables[i] = grown
            if self._up[i] < len(rows):
                dev[self._up[i]:len(rows)].copy_(torch.from_numpy(np.stack(rows[self._up[i]:])))
                self._up[i] = len(rows)
        return self._tables

    def _stage(self, nbytes):
        """the next pinned staging buffer of at least ``nbytes``, free of its last copy"""
        import torch
        k = self._turn = (self._turn + 1) % self.STAGES
        slot = self._stages[k]
        if slot is not None and slot[1] is not None:
            slot[1].synchronize()                        # the copy of STAGES calls ago: long done
        if slot is None or slot[0].numel() < nbytes:
            slot = self._stages[k] = [torch.empty(1 << max(int(nbytes) - 1, 4095).bit_length(), dtype=torch.uint8).pin_memory(), None]
        return slot

    def _workspace(self, lib, n, h, w, segments):
        import torch
        key = (n, h, w, segments)
        hit = self._work.get(key)
        if hit is None:
            while len(self._work) >= 4:
                self._work.popitem(last=False)
            nbytes = int(lib.fr_jpeg_decode_workspace(n, h, w, segments))
            hit = self._work[key] = (torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.device), nbytes)
        else:
            self._work.move_to_end(key)
        return hit

    def decode_device(self, blobs, out=None):
        """Decodes every blob on the current stream, without a synchronisation: one pinned staging copy of the concatenated
        scans with their descriptors, then the launches.  Returns ``(frames, shapes, status)``:

        - all blobs the device takes have one size (or ``out``, a contiguous device ``uint8 [n,H,W,3]``, is given): ``frames``
          is a device ``uint8 [n,H,W,3]`` BGR batch;
        - otherwise ``frames`` is ``(arena, table)``: a device arena holding the frames back to back at 16-byte-aligned
          offsets and their frame table (include/frhip.h fr_frame_ref, what ``RaggedIngest.upload`` returns);
        - ``shapes``: the (H, W) of every frame, None for a blob ``parse`` turned away (``last_fallbacks`` says why); with
          ``orient`` the ORIENTED (H, W), which is also the shape ``out`` must have and the destinations get;
        - ``status``: device ``int32 [n]``, ``OK`` / ``BAD_STREAM`` / ``SKIPPED``; a frame that is not ``OK`` was not written.

        The one-shot form: every call allocates its device staging, its status words and (without ``out``) its frames, and may
        wait on the event of the pinned staging buffer it reuses.  The live path keeps all of that in a ring instead:
        ``FrameIngest`` / ``RaggedIngest(..., pixel_format="jpeg")`` (ingest.py) allocate once and decode behind their copy."""
        import torch
        from . import _lib
        from .letterbox import frame_table
        lib = _lib.load()
        n = len(blobs)
        if n == 0:
            return torch.empty((0, 0, 0, 3), dtype=torch.uint8, device=self.device), [], torch.empty(0, dtype=torch.int32, device=self.device)
        views = [_view(b) for b in blobs]
        frames, headers = self.describe(views)
        coded = [(hd.H, hd.W) for hd in headers if hd is not None]
        turns = self.last_orientations
        turned = any(o != 1 for o, hd in zip(turns, headers) if hd is not None)
        shapes = [None if hd is None else oriented_shape((hd.H, hd.W), o) for hd, o in zip(headers, turns)]
        real = [s for s in shapes if s is not None]
        if out is not None:
            if out.dim() != 4 or out.shape[0] != n or out.shape[3] != 3 or out.dtype != torch.uint8 or not out.is_contiguous():
                raise ValueError("out must be a contiguous device uint8 [n,H,W,3]")
            dense = (int(out.shape[1]), int(out.shape[2]))
        else:
            dense = real[0] if real and all(s == real[0] for s in real) else None
        with torch.cuda.device(self.device):
            if dense is not None:
                if out is None:
                    out = torch.empty((n,) + dense + (3,), dtype=torch.uint8, device=self.device)
                step = dense[0] * dense[1] * 3
                # a blob that was turned away keeps a null entry: its frame of the batch is not written
                refs, _ = frame_table([out.data_ptr() + f * step if shapes[f] else 0 for f in range(n)],
                                      [dense if shapes[f] else (0, 0) for f in range(n)])
            else:
                offsets, off = [], 0
                for s in shapes:
                    offsets.append(off)
                    off += ((s[0] * s[1] * 3 if s else 0) + 15) // 16 * 16
                arena = torch.empty(max(off, 16), dtype=torch.uint8, device=self.device)
                refs, _ = frame_table([arena.data_ptr() + o if s else 0 for o, s in zip(offsets, shapes)],
                                      [s or (0, 0) for s in shapes])
            # staging: the descriptors, the frame table, the orientation words of a batch that has a turned file, then the
            # scans at 16-byte-aligned offsets
            at = (100 * n + 15) // 16 * 16 if turned else 96 * n
            for f, hd in enumerate(headers):
                if hd is not None:
                    frames["scan_off"][f] = at
                    at += (int(frames["scan_len"][f]) + 15) // 16 * 16
            total = max(at, 16)
            slot = self._stage(total)
            host = slot[0].numpy()
            host[:64 * n] = frames.view(np.uint8)
            host[64 * n:96 * n] = refs
            if turned:
                host[96 * n:100 * n] = np.asarray(turns, "<i4").view(np.uint8)
            for f, hd in enumerate(headers):
                if hd is not None:
                    o, ln = int(frames["scan_off"][f]), int(frames["scan_len"][f])
                    host[o:o + ln] = np.frombuffer(views[f], np.uint8)[hd.scan:]
            dev = torch.empty(total, dtype=torch.uint8, device=self.device)
            dev.copy_(slot[0][:total], non_blocking=True)
            slot[1] = torch.cuda.Event()
            slot[1].record()
            status = torch.empty(n, dtype=torch.int32, device=self.device)
            max_h, max_w = max([s[0] for s in coded] + [1]), max([s[1] for s in coded] + [1])    # the launches' geometry: coded
            segments = max([hd.segments for hd in headers if hd is not None] + [1])
            qt, ht = self._tables_on_device()
            ws, ws_bytes = self._workspace(lib, n, max_h, max_w, segments)
            base = dev.data_ptr()
            if turned:
                lib.fr_jpeg_decode_oriented_refs_u8(base, total, base, n, max_h, max_w, segments, _lib.ptr(qt), int(qt.shape[0]),
                                                    _lib.ptr(ht), int(ht.shape[0]), _lib.ptr(self._natural), base + 64 * n,
                                                    base + 96 * n, _lib.ptr(status), _lib.ptr(ws), ws_bytes, _lib.stream_ptr())
            else:
                lib.fr_jpeg_decode_refs_u8(base, total, base, n, max_h, max_w, segments, _lib.ptr(qt), int(qt.shape[0]), _lib.ptr(ht),
                                           int(ht.shape[0]), _lib.ptr(self._natural), base + 64 * n, _lib.ptr(status), _lib.ptr(ws),
                                           ws_bytes, _lib.stream_ptr())
        return (out if dense is not None else (arena, dev[64 * n:96 * n])), shapes, status

    def decode_frames(self, blobs, fallback=True):
        """``decode_device`` and one synchronisation for the flags: one device ``uint8 [H,W,3]`` BGR tensor per blob.  A blob the
        device did not take (``last_fallbacks[f]`` says why) is decoded by ``ingest.decode_image`` and copied up when
        ``fallback`` (with this decoder's ``orient``); None for what does not decode either way."""
        import torch
        blobs = list(blobs)
        if not blobs:
            self.last_fallbacks = {}
            return []
        frames, shapes, status = self.decode_device(blobs)
        flags = status.cpu().numpy()                     # synchronises
        out, off = [], 0
        for f, s in enumerate(shapes):
            size = s[0] * s[1] * 3 if s else 0
            if s is not None and flags[f] == OK:
                out.append(frames[0][off:off + size].view(s + (3,)) if isinstance(frames, tuple) else frames[f])
            else:
                if s is not None:
                    self.last_fallbacks[f] = "broken entropy data" if flags[f] == BAD_STREAM else "skipped by the device"
                logger.info("JPEG decode: frame %d goes to the host decoder: %s", f, self.last_fallbacks[f])
                img = None
                if fallback:
                    from .ingest import decode_image
                    img = decode_image(bytes(_view(blobs[f])), orient=self.orient)
                out.append(None if img is None else torch.from_numpy(img).to(self.device))
            off += (size + 15) // 16 * 16
        return out

    def decode(self, blobs):
        """``decode_device`` and the read-back: one ``uint8 [H,W,3]`` BGR array per blob, None (and ``last_fallbacks[f]`` says
        why) for a blob the device did not decode: the caller's to hand to ``ingest.decode_image``."""
        if len(blobs) == 0:
            self.last_fallbacks = {}
            return []
        frames, shapes, status = self.decode_device(blobs)
        flags = status.cpu().numpy()                     # synchronises
        out = []
        if isinstance(frames, tuple):
            host, off = frames[0].cpu().numpy(), 0
        else:
            host = frames.cpu().numpy()
        for f, s in enumerate(shapes):
            size = s[0] * s[1] * 3 if s else 0
            if s is not None and flags[f] == OK:
                out.append(host[off:off + size].reshape(s + (3,)).copy() if isinstance(frames, tuple) else host[f].copy())
            else:
                if s is not None:
                    self.last_fallbacks[f] = "broken entropy data" if flags[f] == BAD_STREAM else "skipped by the device"
                    logger.warning("JPEG decode: frame %d: %s", f, self.last_fallbacks[f])
                out.append(None)
            if isinstance(frames, tuple):
                off += (size + 15) // 16 * 16
        return out
