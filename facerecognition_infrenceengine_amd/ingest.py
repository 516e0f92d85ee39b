"""Frame ingest: pinned host ring -> device, overlapped with compute.

The reference hands every camera frame to ``FaceAnalysis.get`` as a pageable NumPy array
(/root/reference/infrenceServer.py:573-601: ``cap.read()`` -> ``recognize_faces(frame, ...)``), i.e. one
synchronous host-to-device copy per frame.  Here the capture/decoder side writes BGR frames straight into
page-locked ring slots (``host_buffer``), ``upload`` starts an asynchronous copy of a whole batch on a
dedicated HIP copy stream and returns an event; the detector stream waits for that event only, so the copy of
batch i+1 runs under the kernels of batch i.  The HUD is drawn into the ring's device frames (hud.py).

``pixel_format="nv12"`` / ``"i420"``: the ring's pinned slots hold YUV 4:2:0 frames (``uint8 [H*3/2, W]``, what a video decoder
produces: colour.py) - half the bytes on the link and in the pinned ring.  ``upload`` copies them to a device staging arena and
launches the conversion (csrc/yuv_to_bgr.hip) behind the copy on the copy stream; what it returns is what it returns for BGR.
"""
import io

import numpy as np
import torch

from . import _lib


def decode_image(data, orient=False):
    """Encoded image bytes (JPEG / PNG ...) -> ``uint8 [H,W,3]`` BGR, or None when the bytes do not decode: the
    ``cv2.imdecode(np.frombuffer(blob, np.uint8), cv2.IMREAD_COLOR)`` of the enrolment worker
    (/root/reference/trainingServer.py:219-224), with Pillow standing in for OpenCV (absent from the image).  Host
    side by design (decode stays on the CPU); JPEG decoders differ in their IDCT rounding, so
    pixel values can differ from OpenCV's by a unit - the lossless formats decode identically.

    ``orient=True``: the picture as its EXIF orientation turns it, which is what ``cv2.imdecode`` returns (OpenCV applies the
    tag unless told IMREAD_IGNORE_ORIENTATION): a JPEG's through ``jpeg_decode.exif_orientation`` - so a file decoded here and
    one decoded on the device give the same array -, another format's through Pillow's ``getexif``.  Default: as coded."""
    turn = 1
    try:
        from PIL import Image
        data = bytes(data)
        with Image.open(io.BytesIO(data)) as im:
            rgb = np.asarray(im.convert("RGB"), dtype=np.uint8)
            if orient:
                from .jpeg_decode import exif_orientation
                turn = exif_orientation(data) if im.format in ("JPEG", "MPO") else im.getexif().get(0x0112, 1)
    except Exception:                        # the reference logs "Failed to decode" and skips the image
        return None
    bgr = rgb[:, :, ::-1]
    if turn in (2, 3, 4, 5, 6, 7, 8):
        from .jpeg_decode import orient as turned
        bgr = turned(bgr, turn)
    return np.ascontiguousarray(bgr)


class _JpegSlots:
    """The JPEG half of a ring (``pixel_format="jpeg"``; csrc/jpeg_decode.hip): the pinned slots hold ENCODED
    bytes - the frame descriptors, then the scans of the files ``put`` so far, back to back - and ``queue`` copies exactly the
    bytes used into ONE device staging buffer and decodes them into the slot's BGR frames behind the copy.  Everything on the
    device is allocated here, once: staging, status words, the decoder's workspace.  A blob the device cannot take (``parse``
    turned it away, another size than its frame, longer than the slot has room for) is decoded by ``decode_image`` into a pinned
    BGR side buffer (made on first need) and copied into its device frame behind the decode launches; a blob that does not
    decode at all is a black frame.

    The rings (``FrameIngest`` / ``RaggedIngest`` with ``pixel_format="jpeg"``) IGNORE an EXIF orientation tag: their frames
    have fixed sizes and they serve cameras, which write none.  Photos that carry one go through
    ``JpegDecoder(..., orient=True)`` (enrolment, ``get_batch_jpeg``)."""

    def __init__(self, device, depth, shapes, offsets, nbytes, max_frame_bytes):
        from .jpeg_decode import FRAME, JpegDecoder
        self.device, self.depth, self.shapes, self.offsets, self.nbytes = device, depth, shapes, offsets, nbytes
        n = self.n = len(shapes)
        if max_frame_bytes is not None and int(max_frame_bytes) < 1:
            raise ValueError(f"max_frame_bytes must be at least 1 (got {max_frame_bytes})")
        # room for a frame's scan: half of its BGR bytes unless told - an NV12 slot's size; quality-95 4:4:4 files pass a quarter
        self.room = [int(max_frame_bytes) if max_frame_bytes is not None else max(h * w * 3 // 2, 4096) for h, w in shapes]
        self.head = 64 * n
        self.capacity = sum((r + 15) // 16 * 16 for r in self.room)
        self.decoder = JpegDecoder(device)
        self._lib = _lib.load()
        self._frame = FRAME
        self._host = [torch.zeros(self.head + self.capacity, dtype=torch.uint8).pin_memory() for _ in range(depth)]
        self._enc = torch.empty(self.head + self.capacity, dtype=torch.uint8, device=device)
        self.status = [torch.zeros(n, dtype=torch.int32, device=device) for _ in range(depth)]
        max_h, max_w = max(s[0] for s in shapes), max(s[1] for s in shapes)
        self._max = (max_h, max_w)
        self._seg_room = ((max_h + 7) // 8) * ((max_w + 7) // 8)      # a restart interval per 8 x 8 MCU: no file has more
        self._ws_bytes = int(self._lib.fr_jpeg_decode_workspace(n, max_h, max_w, self._seg_room))
        self._ws = torch.empty(max(self._ws_bytes, 16), dtype=torch.uint8, device=device)
        self._side = [None] * depth                                   # pinned BGR arenas for the host-decoded frames
        self._turn = [self._fresh() for _ in range(depth)]
        self._stale = [False] * depth                                 # the slot's records are those of an uploaded turn
        self.fallbacks = [dict() for _ in range(depth)]               # per slot: frame index -> why the host decoded it

    def _fresh(self):
        return {"cursor": 0, "segments": 1, "host": set()}

    def put(self, k, index, data, header=None, decoded=None):
        """True: the blob's scan is in the slot and the device will decode it.  False: the host decoded it (``fallbacks[k]``
        says why).  None: it does not decode at all - a black frame."""
        from .jpeg_decode import Header, parse
        st, h, w = self._turn[k], *self.shapes[index]
        records = self._host[k].numpy()[:self.head].view(self._frame)
        if self._stale[k]:                                            # the first put of a turn
            records[:] = np.zeros((), self._frame)
            self.fallbacks[k].clear()
            self.decoder.trim_tables()
            self._stale[k] = False
        records[index] = np.zeros((), self._frame)                    # a null entry: the launches skip it
        st["host"].discard(index)
        self.fallbacks[k].pop(index, None)
        hd = header if header is not None else parse(data)
        why = hd if isinstance(hd, str) else None
        if why is None and (hd.H, hd.W) != (h, w):
            why = f"a {hd.H} x {hd.W} picture in a {h} x {w} frame"
        if why is None:
            view = memoryview(data).cast("B")
            ln = len(view) - hd.scan
            if ln > self.room[index] or st["cursor"] + ln > self.capacity:
                why = f"a scan of {ln} bytes, the slot has room for {self.room[index]}"
        if why is None:
            one = np.zeros(1, self._frame)
            self.decoder.describe_into(one[0], hd, ln)
            one["scan_off"][0] = self.head + st["cursor"]
            records[index] = one[0]
            self._host[k].numpy()[self.head + st["cursor"]:self.head + st["cursor"] + ln] = np.frombuffer(view, np.uint8)[hd.scan:]
            st["cursor"] += (ln + 15) // 16 * 16
            st["segments"] = max(st["segments"], hd.segments)
            return True
        self.fallbacks[k][index] = why
        img = decoded if decoded is not None else decode_image(bytes(memoryview(data).cast("B")) if not isinstance(data, str) else b"")
        if self._side[k] is None:
            self._side[k] = torch.empty(self.nbytes, dtype=torch.uint8).pin_memory()
        side = self._side[k].numpy()[self.offsets[index]:self.offsets[index] + h * w * 3].reshape(h, w, 3)
        st["host"].add(index)
        if img is None or img.shape != (h, w, 3):
            side[...] = 0
            return None
        side[...] = img
        return False

    def queue(self, k, dev, table):
        """on the current (copy) stream: the bytes used up, the decode launches, the host-decoded frames behind them"""
        st = self._turn[k]
        used = self.head + st["cursor"]
        self._enc[:used].copy_(self._host[k][:used], non_blocking=True)
        qt, ht = self.decoder._tables_on_device()
        base = self._enc.data_ptr()
        self._lib.fr_jpeg_decode_refs_u8(base, used, base, self.n, self._max[0], self._max[1], min(st["segments"], self._seg_room),
                                         _lib.ptr(qt), int(qt.shape[0]), _lib.ptr(ht), int(ht.shape[0]), _lib.ptr(self.decoder._natural),
                                         _lib.ptr(table), _lib.ptr(self.status[k]), _lib.ptr(self._ws), self._ws_bytes, _lib.stream_ptr())
        # a scan that broke off: the launches flagged the frame and left its pixels alone - what the slot held some turns ago.
        # It becomes the black frame every other undecodable blob is
        self._lib.fr_jpeg_blank_bad_refs_u8(_lib.ptr(table), _lib.ptr(self.status[k]), self.n, _lib.stream_ptr())
        flat = dev.view(-1)
        for index in sorted(st["host"]):
            o, size = self.offsets[index], self.shapes[index][0] * self.shapes[index][1] * 3
            flat[o:o + size].copy_(self._side[k][o:o + size], non_blocking=True)
        self.link_bytes = used + sum(self.shapes[i][0] * self.shapes[i][1] * 3 for i in st["host"])
        self._turn[k] = self._fresh()
        # the next turn starts from null entries (its first put writes them): an index it does not put is skipped, not decoded
        # from this turn's descriptor
        self._stale[k] = True


class FrameIngest:
    """Ring of ``depth`` batch slots: pinned ``uint8 [N,H,W,3]`` host buffers + matching device buffers.  With a YUV
    ``pixel_format`` the pinned buffers are ``uint8 [N,H*3/2,W]`` and the device buffers are still BGR ``[N,H,W,3]``."""

    def __init__(self, n, h, w, device="cuda:0", depth=3, pixel_format="bgr", matrix="bt601", max_frame_bytes=None):
        """One asynchronous copy of the whole batch per slot on one copy stream (round 4 measured frame groups and a second copy
        stream: no gain / -5 %, profiles/r04_ingest_ab.txt; the knobs are gone).  ``pixel_format`` ``"nv12"`` / ``"i420"`` with
        ``matrix`` (colour.MATRICES): YUV 4:2:0 slots, H and W even, converted on the device by ``upload``.  ``pixel_format="jpeg"``
        (``max_frame_bytes``: room for one file's scan, default H * W * 3 / 2): the slots hold encoded bytes, written with ``put``,
        and ``upload`` decodes them on the device behind the copy (``_JpegSlots``); an EXIF orientation tag is ignored (the
        frames have one fixed size, and cameras write none)."""
        from .colour import check_pixel_format, check_yuv_size
        _lib.require_gpu()
        self.device = torch.device(device)
        self.shape, self.depth = (int(n), int(h), int(w), 3), int(depth)
        self.pixel_format = pixel_format
        self._jpeg = None
        if pixel_format == "jpeg":
            from .letterbox import frame_table
            n, h, w = self.shape[:3]
            self._layout = self._consts = None
            self._dev = [torch.empty(self.shape, dtype=torch.uint8, device=self.device) for _ in range(self.depth)]
            step = h * w * 3
            self._jpeg = _JpegSlots(self.device, self.depth, [(h, w)] * n, [i * step for i in range(n)], n * step, max_frame_bytes)
            self.tables = [torch.from_numpy(frame_table([d.data_ptr() + i * step for i in range(n)], [(h, w)] * n)[0]).to(self.device)
                           for d in self._dev]
            self._host = []
            self._stream = torch.cuda.Stream(device=self.device)
            self._busy = [None] * self.depth
            torch.cuda.synchronize(self.device)
            return
        self._layout, self._consts = check_pixel_format(pixel_format, matrix)
        host_shape = self.shape
        if self._layout is not None:
            check_yuv_size(self.shape[1], self.shape[2])
            host_shape = (self.shape[0], self.shape[1] * 3 // 2, self.shape[2])
            # ONE staging arena serves every slot: copy and conversion of a slot are queued on the one copy stream, so the next
            # slot's copy starts after this slot's conversion has read the arena
            self._yuv = torch.empty(host_shape, dtype=torch.uint8, device=self.device)
            self._lib = _lib.load()
        self._host = [torch.empty(host_shape, dtype=torch.uint8).pin_memory() for _ in range(self.depth)]
        self._dev = [torch.empty(self.shape, dtype=torch.uint8, device=self.device) for _ in range(self.depth)]
        self._stream = torch.cuda.Stream(device=self.device)
        self._busy = [None] * self.depth          # event: last consumer of the slot's device buffer

    def host_buffer(self, slot):
        """NumPy view of the slot's pinned buffer: the decoder / capture thread writes frames here (BGR ``[N,H,W,3]``, or
        the ring's YUV format ``[N,H*3/2,W]``)."""
        return self._host[slot % self.depth].numpy()

    def decode_into(self, slot, index, data):
        """Decode image bytes straight into frame ``index`` of the slot's pinned buffer (no intermediate pageable
        copy).  False when the bytes do not decode or the picture is not the ring's H x W - and always on a YUV ring: the
        decoder here produces BGR, and a still image that is to enter a YUV ring is the caller's to convert."""
        if self._layout is not None or self._jpeg is not None:
            return False
        img = decode_image(data)
        if img is None or img.shape != self.shape[1:]:
            return False
        self.host_buffer(slot)[index] = img
        return True

    def put(self, slot, index, data, **known):
        """A JPEG ring: file ``data`` (bytes) becomes frame ``index`` of the slot.  True: the device decodes it; False: the host
        did (``fallbacks(slot)`` says why); None: it does not decode - a black frame."""
        if self._jpeg is None:
            raise ValueError("put is for pixel_format=\"jpeg\" rings: write BGR / YUV frames into host_buffer(slot)")
        return self._jpeg.put(slot % self.depth, index, data, **known)

    def fallbacks(self, slot):
        """JPEG ring: frame index -> why the host decoded it, for the frames last ``put`` into the slot"""
        return self._jpeg.fallbacks[slot % self.depth]

    def upload(self, slot):
        """Start the H2D copy of the slot; returns (device frames, event that fires when they have landed).
        The copy waits for the slot's previous consumer (see ``release``).  A YUV ring copies the YUV bytes and converts them
        behind the copy on the same stream; the frames returned are BGR and the event fires after the conversion.  A JPEG ring
        copies the encoded bytes used and decodes them behind the copy; the event fires after the decode."""
        k = slot % self.depth
        with torch.cuda.stream(self._stream):
            if self._busy[k] is not None:
                self._stream.wait_event(self._busy[k])
            if self._jpeg is not None:
                self._jpeg.queue(k, self._dev[k], self.tables[k])
            elif self._layout is None:
                self._dev[k].copy_(self._host[k], non_blocking=True)
            else:
                from .colour import convert_batch
                self._yuv.copy_(self._host[k], non_blocking=True)
                convert_batch(self._lib, self._yuv, self._dev[k], self.shape[0], self.shape[1], self.shape[2], self._layout,
                              self._consts)
        ev = torch.cuda.Event()
        ev.record(self._stream)
        return self._dev[k], ev

    def release(self, slot, stream=None):
        """Mark the slot's device buffer free once the work queued so far on ``stream`` (default: current) is done."""
        ev = torch.cuda.Event()
        ev.record(stream if stream is not None else torch.cuda.current_stream(self.device))
        self._busy[slot % self.depth] = ev


class RaggedIngest:
    """``FrameIngest`` for frames of DIFFERING sizes (cameras of several resolutions in one batch): keyed by the tuple of frame
    shapes.  A slot is ONE pinned host arena holding the frames back to back at 16-byte-aligned offsets and a device arena
    of the same layout: one H2D copy per batch, the same ``upload`` / ``release`` protocol.  The frame table the kernels
    read (include/frhip.h fr_frame_ref: pointers into the slot's device arena, sizes, and - with ``det_size`` - the sizes on
    the detection canvas) and ``det_scale`` depend on the shapes alone: they are written on the host and uploaded once,
    here, so a batch adds no copy and no synchronisation for them.

    ``pixel_format="nv12"`` / ``"i420"`` (``shapes`` stay the frames' (H, W), both even): the pinned arena holds the YUV 4:2:0
    frames (``[H*3/2, W]`` each, at 16-byte-aligned offsets of their own), ``upload`` copies it to ONE device staging arena
    and converts the whole table in one launch behind the copy; the device arena, the tables and ``det_scale`` are those of
    the BGR ring.  ``pixel_format="jpeg"``: as ``FrameIngest``'s (``_JpegSlots``); an EXIF orientation tag is ignored, the frames
    keep the sizes given here."""

    def __init__(self, shapes, det_size=None, device="cuda:0", depth=3, pixel_format="bgr", matrix="bt601", max_frame_bytes=None):
        from .colour import check_pixel_format, check_yuv_size
        from .letterbox import check_det_size, frame_table
        _lib.require_gpu()
        self.device = torch.device(device)
        self.shapes = tuple((int(s[0]), int(s[1])) for s in shapes)
        self.det_size, self.depth = check_det_size(det_size), int(depth)
        self.pixel_format = pixel_format
        self._jpeg = None
        self._layout, self._consts = (None, None) if pixel_format == "jpeg" else check_pixel_format(pixel_format, matrix)
        self.offsets, off = [], 0
        for h, w in self.shapes:
            self.offsets.append(off)
            off += (h * w * 3 + 15) // 16 * 16
        self.nbytes = max(off, 16)
        host_bytes = self.nbytes
        if self._layout is not None:
            self.yuv_offsets, off = [], 0
            for h, w in self.shapes:
                check_yuv_size(h, w)
                self.yuv_offsets.append(off)
                off += (h * w * 3 // 2 + 15) // 16 * 16
            host_bytes = max(off, 16)
            # one staging arena for every slot: a slot's copy and conversion are queued on the one copy stream
            self._yuv = torch.empty(host_bytes, dtype=torch.uint8, device=self.device)
            self._src_ptrs = torch.tensor([self._yuv.data_ptr() + o for o in self.yuv_offsets], dtype=torch.int64).to(self.device)
            self._lib = _lib.load()
        if pixel_format == "jpeg":                       # the pinned slots hold encoded bytes (``put``), decoded behind the copy
            self._jpeg = _JpegSlots(self.device, self.depth, self.shapes, self.offsets, self.nbytes, max_frame_bytes)
            self._host = []
        else:
            self._host = [torch.empty(host_bytes, dtype=torch.uint8).pin_memory() for _ in range(self.depth)]
        self._dev = [torch.empty(self.nbytes, dtype=torch.uint8, device=self.device) for _ in range(self.depth)]
        self._stream = torch.cuda.Stream(device=self.device)
        self._busy = [None] * self.depth
        self.tables = []
        for d in self._dev:
            tab, scale = frame_table([d.data_ptr() + o for o in self.offsets], self.shapes, self.det_size)
            self.tables.append(torch.from_numpy(tab).to(self.device))
        self.det_scale = torch.from_numpy(scale).to(self.device)
        torch.cuda.synchronize(self.device)              # construction time: the tables are in place before the first upload

    def host_frame(self, slot, index):
        """NumPy view ``uint8 [H,W,3]`` of frame ``index`` in the slot's pinned arena: the capture side writes here.  On a
        YUV ring the view is the YUV frame, ``uint8 [H*3/2, W]``."""
        h, w = self.shapes[index]
        if self._layout is not None:
            o = self.yuv_offsets[index]
            return self._host[slot % self.depth].numpy()[o:o + h * w * 3 // 2].reshape(h * 3 // 2, w)
        o = self.offsets[index]
        return self._host[slot % self.depth].numpy()[o:o + h * w * 3].reshape(h, w, 3)

    def device_frame(self, slot, index):
        """The same frame in the slot's device arena (a view): BGR ``[H,W,3]`` whatever the ring's pixel format."""
        h, w = self.shapes[index]
        o = self.offsets[index]
        return self._dev[slot % self.depth][o:o + h * w * 3].view(h, w, 3)

    def put(self, slot, index, data, **known):
        """A JPEG ring: file ``data`` (bytes) becomes frame ``index`` of the slot.  True: the device decodes it; False: the host
        did (``fallbacks(slot)`` says why); None: it does not decode - a black frame."""
        if self._jpeg is None:
            raise ValueError("put is for pixel_format=\"jpeg\" rings: write BGR / YUV frames into host_frame(slot, index)")
        return self._jpeg.put(slot % self.depth, index, data, **known)

    def fallbacks(self, slot):
        """JPEG ring: frame index -> why the host decoded it, for the frames last ``put`` into the slot"""
        return self._jpeg.fallbacks[slot % self.depth]

    def upload(self, slot):
        """Start the H2D copy of the slot's arena; returns (device arena, frame table on the device, event that fires when
        the frames have landed).  The copy waits for the slot's previous consumer (see ``release``).  A YUV ring copies the
        YUV arena and converts every frame of the table in one launch behind the copy; the event fires after it.  A JPEG ring
        copies the encoded bytes used and decodes them behind the copy."""
        k = slot % self.depth
        with torch.cuda.stream(self._stream):
            if self._busy[k] is not None:
                self._stream.wait_event(self._busy[k])
            if self._jpeg is not None:
                self._jpeg.queue(k, self._dev[k], self.tables[k])
            elif self._layout is None:
                self._dev[k].copy_(self._host[k], non_blocking=True)
            else:
                from .colour import convert_table
                self._yuv.copy_(self._host[k], non_blocking=True)
                convert_table(self._lib, self.tables[k], self._src_ptrs, len(self.shapes), self._layout, self._consts)
        ev = torch.cuda.Event()
        ev.record(self._stream)
        return self._dev[k], self.tables[k], ev

    def release(self, slot, stream=None):
        """Mark the slot's device arena free once the work queued so far on ``stream`` (default: current) is done."""
        ev = torch.cuda.Event()
        ev.record(stream if stream is not None else torch.cuda.current_stream(self.device))
        self._busy[slot % self.depth] = ev
