"""Camera batcher: the reference's ``CameraManager`` (/root/reference/infrenceServer.py:565-679) re-shaped so that
N cameras feed ONE engine in batches.

Reference topology: per source one capture process -> ``Queue(maxsize=2)`` (frames dropped when full, :595-598) ->
one processing process that owns its own model and calls ``recognize_faces(frame, company_id)`` ONE FRAME AT A TIME
(:603-622) -> shared ``Queue(maxsize=10)`` -> display loop (:648-667).  N cameras = N model copies on device 0
and batch size 1 everywhere.

Here the capture side and the queues (sizes, drop-when-full) are kept, but ALL sources are drained by ONE batching
loop: each turn takes at most one frame per source, stacks them and runs ``FaceRecognitionProcessor.recognize_batch``
(one pass of the slot pipeline over the batch), then hands ``(source, processed_frame)`` pairs to the result queue in
source order - the same items the reference's per-camera processes produce.  Threads replace the reference's forked
processes: there is one engine to share, the GPU does the work, and the 30 s gallery sync thread keeps running
(in the reference the forked children never see a sync: threads do not survive fork).

Capture is injected (``capture_factory(source)`` -> object with ``read() -> (ok, frame)`` and ``release()``): the
reference uses ``cv2.VideoCapture`` (:575-584), which is not a dependency of this package.
"""
import logging
import queue
import threading
import time

logger = logging.getLogger(__name__)


class CameraManager:
    def __init__(self, embedding_manager, processor=None, capture_factory=None, max_wait_s=0.005, reopen_after=20,
                 dead_after=200, gate=None, tracks=None, quality=None, hud=None, pixel_format="bgr", matrix="bt601", encode=None,
                 redact=None, chips=None):
        """``processor``: a ``FaceRecognitionProcessor`` (built lazily from ``embedding_manager`` when None).
        ``gate``: an ``activity.ActivityGate``; the engine then runs only for the frames that differ from the last processed
        frame of their source (the sources are its camera ids), and a frame of an unchanged scene is annotated with the
        results held from that last processed frame.  None: every frame goes through the engine, as ever.
        ``tracks``: a ``tracks.FaceTracks``; the processor then embeds only the faces a source's previous frame did not show
        (the sources are its camera ids too).  None: every face is embedded, as ever.
        ``quality``: a ``quality.FaceQuality``; the processor then embeds only the faces judged fit and reports the others as
        Unknown with ``quality_ok`` False.  None: no face is judged, as ever.  Not beside ``tracks`` (ValueError): the two
        combine as ``tracks=FaceTracks(..., quality=q)``, tracks that judge - only fit embeddings enter their bank, and a face
        that turns unfit for a few frames is carried on its track's held row; no further argument is needed here.
        ``hud``: a ``hud.Hud``; the processed frames are then drawn on the DEVICE (``recognize_faces_batch``: the full HUD, on the
        frames or on ``hud.out_size`` previews) and what is queued are the frames that call returns.  None: the plain box drawn
        on the host frame by ``annotate``, as ever.
        ``encode``: a ``jpeg.JpegEncoder``, with a ``hud`` (ValueError without one: the encoder works on the device frames the
        HUD draws on); the drawn frames are then encoded on the DEVICE and what is queued and kept per source is the JPEG
        ``bytes`` (``latest_jpeg(source)``; None for a frame the encoder turned away).  None: arrays, as ever.
        ``redact``: a ``redact.Redactor``, with a ``hud`` (ValueError without one, by the same rule: it masks the device frames
        the HUD draws on); faces are then masked on the DEVICE before the HUD is drawn and before anything is encoded, the
        sources being the keys of its ``linger`` history, and ``latest_frame``, ``latest_jpeg`` and the snapshot and stream
        routes serve masked pictures.  None: nothing is masked, as ever.
        ``chips``: a ``chips.FaceChips``, with or without a ``hud``; the processor call then gets ``chips=`` and every face dict it
        returns carries ``"chip"`` - the face's thumbnail, cut on the DEVICE from the full-size, unmasked, undrawn frame (a face
        the ``redact`` masks has none unless the object says ``masked=True``).  Each source's latest face dicts are kept:
        ``latest_faces(source)``, and the ``GET /api/camera/faces`` route.  None: no chips, as ever.
        ``pixel_format`` / ``matrix``: what the captures deliver - ``"nv12"`` / ``"i420"`` frames (``uint8 [H*3/2, W]``) need a
        ``hud``, since the host never holds a BGR picture of them to draw on (ValueError without one).
        ``"jpeg"``: the captures deliver JPEG files as ``bytes`` (an MJPEG camera); they are decoded on the device behind the ring's
        copy and need a ``hud`` for the same reason.
        ``max_wait_s``: how long a turn waits for a first frame before it looks at ``running`` again; a turn never
        waits for slow cameras once it holds a frame (latency stays that of the slowest *present* frame).
        ``reopen_after`` / ``dead_after``: consecutive failed reads before a capture is re-opened / given up."""
        self.embedding_manager = embedding_manager
        self.processor = processor
        self.capture_factory = capture_factory
        self.max_wait_s = max_wait_s
        self.reopen_after, self.dead_after = max(int(reopen_after), 1), max(int(dead_after), 1)
        self.latest = {}                       # source -> last processed frame (the default consumer's store)
        self._latest_lock = threading.Lock()
        self.running = False
        self.threads = []
        self.frame_queues, self.result_queue = {}, None
        self.company_of = {}                   # source -> company id of the start call that added it
        self._control = threading.Lock()       # start / stop calls, one at a time
        self.stats = {"batches": 0, "frames": 0, "dropped_results": 0, "largest_batch": 0, "dead_sources": []}
        self.gate = gate
        self._held = {}                        # source -> results of its last processed frame (gate only)
        if gate is not None:
            self.stats["gated_frames"] = 0
        self.tracks = tracks
        if quality is not None and tracks is not None:
            raise ValueError("quality together with tracks is not supported yet")
        self.quality = quality
        if pixel_format != "bgr" and hud is None:
            raise ValueError(f"pixel_format={pixel_format!r} needs a hud: the host holds no BGR frame to annotate")
        self.hud, self.pixel_format, self.matrix = hud, pixel_format, matrix
        if encode is not None and hud is None:
            raise ValueError("encode needs a hud: the encoder works on the device frames the HUD draws on")
        self.encode = encode
        if redact is not None and hud is None:
            raise ValueError("redact needs a hud: the redactor masks the device frames the HUD draws on")
        self.redact = redact
        self.chips = chips
        self._faces = {}                       # source -> the face dicts of its last processed frame, with their chips (chips only)
        self._jpeg = {}                        # source -> (count of its frames so far, the latest JPEG bytes) (encode only)
        self._jpeg_new = threading.Condition(self._latest_lock)

    def _forget(self, source):
        """A source that is gone: its gate slot and its track slot are freed, its held results and its redaction history
        dropped."""
        if self.redact is not None:
            try:
                self.redact.forget(source)
            except Exception as e:
                logger.error("Camera %s: the redactor did not forget it: %s", source, e)
        if self.tracks is not None:
            try:
                self.tracks.forget(source)
            except Exception as e:
                logger.error("Camera %s: the tracks did not forget it: %s", source, e)
        if self.chips is not None:
            with self._latest_lock:
                self._faces.pop(source, None)
        if self.gate is not None:
            self._held.pop(source, None)
            try:
                self.gate.forget(source)
            except Exception as e:
                logger.error("Camera %s: the gate did not forget it: %s", source, e)

    # ---- capture side (infrenceServer.py:573-601)
    def capture_frames(self, source, frame_queue):
        """The reference retries a failed read at once (:589-592) - in its own OS process.  Here capture is a thread
        that shares the interpreter with the ONE batching loop feeding the GPU, so a camera that drops (an RTSP
        disconnect makes read() fail immediately) must not spin: failed reads back off (10 ms doubling to 100 ms, one
        warning per 5 s), after ``reopen_after`` consecutive failures the capture is re-opened, and after
        ``dead_after`` the source is marked dead (``stats['dead_sources']``) and its thread ends."""
        cap = self.capture_factory(source)
        logger.info("Camera %s initialized", source)
        fails, delay, last_warn = 0, 0.01, 0.0
        try:
            while self.running:
                ok, frame = cap.read()
                if not ok:
                    if frame is None and getattr(cap, "exhausted", False):
                        break
                    fails += 1
                    now = time.monotonic()
                    if now - last_warn > 5.0:
                        logger.warning("Camera %s: read failed (%d in a row)", source, fails)
                        last_warn = now
                    if fails >= self.dead_after:
                        logger.error("Camera %s: %d failed reads in a row: giving up on this source", source, fails)
                        self.stats["dead_sources"].append(source)
                        self._forget(source)
                        break
                    if fails % self.reopen_after == 0:
                        try:
                            cap.release()
                            cap = self.capture_factory(source)
                            logger.info("Camera %s re-opened", source)
                        except Exception as e:                 # stays failed: the next reads back off again
                            logger.error("Camera %s: re-open failed: %s", source, e)
                    time.sleep(delay)
                    delay = min(delay * 2, 0.1)
                    continue
                fails, delay = 0, 0.01
                try:
                    frame_queue.put_nowait(frame)          # non-blocking: skip the frame when the queue is full (:595-598)
                except queue.Full:
                    pass
        finally:
            cap.release()
            logger.info("Camera %s released", source)

    # ---- batching loop: replaces the N process_camera processes (infrenceServer.py:603-622)
    def take_batch(self, sources):
        """At most one frame per source, in ``sources`` order; blocks up to ``max_wait_s`` for the first one."""
        got = []
        for s in sources:
            try:
                got.append((s, self.frame_queues[s].get_nowait()))
            except queue.Empty:
                pass
        if not got:
            deadline = time.monotonic() + self.max_wait_s
            while not got and time.monotonic() < deadline and self.running:
                for s in sources:
                    try:
                        got.append((s, self.frame_queues[s].get_nowait()))
                    except queue.Empty:
                        pass
                if not got:
                    time.sleep(0.0005)
        return got

    def process_cameras(self, sources=None, company_id=None):
        """The batching loop.  Every turn drains ALL sources running at that moment (``start_cameras`` may add some
        while the loop runs), each under the company it was started with; ``sources`` / ``company_id``, when given,
        are registered first."""
        if self.processor is None:
            from .processor import FaceRecognitionProcessor
            self.processor = FaceRecognitionProcessor(self.embedding_manager)
        for s in sources or ():
            self.company_of.setdefault(s, company_id)
        while self.running:
            batch = self.take_batch([s for s in list(self.frame_queues) if s in self.company_of])
            if not batch:
                continue
            try:
                self.process_batch(batch, [self.company_of.get(s, company_id) for s, _ in batch])
            except Exception as e:                         # logged and survived, as the reference's loop (:620-621)
                logger.error("Error processing cameras %s: %s", [s for s, _ in batch], e)

    def _shape_of(self, frame):
        """what frames must share to go through the engine together: the array's shape, or a JPEG file's picture size"""
        if self.pixel_format != "jpeg":
            return tuple(frame.shape)
        from .jpeg_decode import parse
        hd = parse(frame)
        return ("jpeg", id(frame)) if isinstance(hd, str) else (hd.H, hd.W, 3)     # a file the host must decode goes alone

    def process_batch(self, batch, company_id):
        """batch: [(source, frame)].  Frames of one size go through the engine together - all of them in ONE call when the
        processor takes mixed sizes (``accepts_mixed_sizes``: an engine with a ``det_size``); results leave in batch order.
        ``company_id``: one id for the whole batch, or a list / tuple aligned with ``batch``.  Frames of several
        companies still go through the engine together: the processor call gets the per-frame list then, and the plain
        id whenever all its frames share one.  With a gate the processor also gets ``gate=`` and the frames' sources as
        ``camera_ids=``; where it answers ``UNCHANGED`` the source's held results stand in (here and in the returned list) and
        ``stats["gated_frames"]`` counts the frame.  With a ``hud`` the processor call is ``recognize_faces_batch(..., hud,
        return_results=True, held=self._held)`` with the same arguments (and the manager's pixel format when it is YUV): the frames
        it returns - drawn on the device, an unchanged frame with its held results - are what is queued, and ``annotate`` is not
        called.  With ``encode`` too the call also gets ``encode=``, and what it returns and what is queued is one JPEG ``bytes``
        per frame, kept per source for ``latest_jpeg``.  With ``redact`` the call also gets ``redact=`` and the frames' sources as
        ``redact_keys=``.  With ``chips`` the call - either of the two - also gets ``chips=``, and the face dicts of every frame
        the engine ran for are kept per source for ``latest_faces``; a frame answered ``UNCHANGED`` leaves its source's as they
        are."""
        mixed_ids = isinstance(company_id, (list, tuple))
        if mixed_ids and len(company_id) != len(batch):
            raise ValueError(f"one company id per frame: {len(batch)} frames, {len(company_id)} ids")
        by_shape = {}
        mixed = getattr(self.processor, "accepts_mixed_sizes", False)
        for k, (_, f) in enumerate(batch):
            by_shape.setdefault(None if mixed else self._shape_of(f), []).append(k)
        results, pictures = [None] * len(batch), [None] * len(batch)
        for ks in by_shape.values():
            ids = [company_id[k] for k in ks] if mixed_ids else [company_id]
            one = all(c == ids[0] for c in ids[1:])
            gated = {} if self.gate is None else {"gate": self.gate, "camera_ids": [batch[k][0] for k in ks]}
            if self.tracks is not None:
                gated = dict(gated, tracks=self.tracks, camera_ids=[batch[k][0] for k in ks])
            if self.quality is not None:
                gated = dict(gated, quality=self.quality)
            if self.chips is not None:
                gated = dict(gated, chips=self.chips)
            if self.hud is None:
                res = self.processor.recognize_batch([batch[k][1] for k in ks], ids[0] if one else ids, **gated)
            else:                                     # the same call, then the HUD drawn on the device frames
                if self.pixel_format != "bgr":
                    gated = dict(gated, pixel_format=self.pixel_format, matrix=self.matrix)
                if self.encode is not None:
                    gated = dict(gated, encode=self.encode)
                if self.redact is not None:
                    gated = dict(gated, redact=self.redact, redact_keys=[batch[k][0] for k in ks])
                drawn, res = self.processor.recognize_faces_batch([batch[k][1] for k in ks], ids[0] if one else ids, self.hud,
                                                                  return_results=True, held=self._held, **gated)
            for j, k in enumerate(ks):
                results[k] = None if res is None else res[j]
                if self.hud is not None:
                    pictures[k] = drawn[j]
        if self.chips is not None:                    # before held results stand in: those faces' chips are already kept
            with self._latest_lock:
                for k, (source, _) in enumerate(batch):
                    if isinstance(results[k], list):
                        self._faces[source] = results[k]
        if self.gate is not None:
            from .processor import UNCHANGED
            for k, (source, _) in enumerate(batch):
                if results[k] is UNCHANGED:           # the scene is the same, so the boxes are
                    results[k] = self._held.get(source)
                    self.stats["gated_frames"] += 1
                else:
                    self._held[source] = results[k]
        self.stats["batches"] += 1
        self.stats["frames"] += len(batch)
        self.stats["largest_batch"] = max(self.stats["largest_batch"], len(batch))
        for (source, frame), res, picture in zip(batch, results, pictures):
            if self.hud is not None:
                out = picture
                if self.encode is not None and out is not None:
                    with self._jpeg_new:
                        self._jpeg[source] = (self._jpeg.get(source, (0, None))[0] + 1, out)
                        self._jpeg_new.notify_all()
            else:
                out = frame if res is None else self.processor.annotate(frame, res)
            try:
                self.result_queue.put_nowait((source, out))   # skip when the consumer is behind (:614-617)
            except queue.Full:
                self.stats["dropped_results"] += 1
        return results

    # ---- control (infrenceServer.py:624-679); called by the /api/camera/start|stop routes
    def start_cameras(self, sources, company_id, display=None):
        """Starts the capture threads and the batching loop and returns; processed frames arrive on
        ``self.result_queue`` as ``(source, frame)``.  A consumer thread always drains that queue (the reference's
        cv2.imshow loop, :648-667): it calls ``display(source, frame)`` when given, otherwise it keeps the latest
        processed frame per source (``latest_frame(source)``) - so the unchanged ``POST /api/camera/start`` route,
        which passes no display, neither fills the 10-deep queue nor makes the GPU work for dropped results.

        Called while running, it ADDS the sources that are not running yet, under the given company (the reference's
        ``start_cameras`` appends processes, each with the ``company_id`` of its request: infrenceServer.py:624-646):
        a queue and a capture thread each, and the one batching loop serves them from its next turn on, together with
        the cameras of the other companies.  Sources that already run are left as they are - a repeated identical
        start is a no-op - and ``display`` is that of the first start."""
        with self._control:
            if self.capture_factory is None:
                raise RuntimeError("CameraManager needs capture_factory=<callable(source) -> capture object>")
            if self.running:
                self._add_sources([s for s in sources if s not in self.company_of], company_id)
                return
            self.running = True
            self.frame_queues, self.company_of = {}, {}
            self.result_queue = queue.Queue(maxsize=10)                        # :630
            self._add_sources(list(sources), company_id)
            t = threading.Thread(target=self.process_cameras, daemon=True)
            t.start(); self.threads.append(t)
            self._start_consumer(display)

    def _add_sources(self, sources, company_id):
        for s in sources:
            if s in self.company_of:
                continue
            q = queue.Queue(maxsize=2)                                         # :629
            self.company_of[s] = company_id
            self.frame_queues[s] = q
            t = threading.Thread(target=self.capture_frames, args=(s, q), daemon=True)
            t.start(); self.threads.append(t)

    def _start_consumer(self, display):
        def keep_latest(source, frame):
            with self._latest_lock:
                self.latest[source] = frame

        sink = display if display is not None else keep_latest

        def consume():
            while self.running:
                try:
                    sink(*self.result_queue.get(timeout=1))
                except queue.Empty:
                    continue
                except Exception as e:
                    logger.error("Result consumer failed: %s", e)
        t = threading.Thread(target=consume, daemon=True)
        t.start(); self.threads.append(t)

    def latest_frame(self, source):
        """Last processed frame of ``source`` kept by the default consumer (None before the first result)."""
        with self._latest_lock:
            return self.latest.get(source)

    def latest_jpeg(self, source, after=0, timeout=None):
        """The JPEG ``bytes`` of the last processed frame of ``source`` (None before the first one, and always without an
        encoder).  ``after`` / ``timeout``: as ``(count, bytes)``, waiting up to ``timeout`` seconds for a frame whose count -
        the number of frames the source has produced - is above ``after``; ``(after, None)`` when none came."""
        with self._jpeg_new:
            if timeout is None:
                return self._jpeg.get(source, (0, None))[1]
            self._jpeg_new.wait_for(lambda: self._jpeg.get(source, (0, None))[0] > after, timeout)
            count, data = self._jpeg.get(source, (0, None))
            return (count, data) if count > after else (after, None)

    def latest_faces(self, source):
        """The face dicts of the last frame of ``source`` the engine ran for, each with its ``"chip"`` (None before the first
        one, and always without ``chips``)."""
        with self._latest_lock:
            return self._faces.get(source)

    def source_named(self, text):
        """the source whose ``str()`` is ``text`` - how a route names one (sources are ints or strings) -, or None"""
        with self._latest_lock:
            known = list(self.company_of) + list(self._jpeg) + list(self.latest) + list(self._faces)
        return next((s for s in known if str(s) == str(text)), None)

    def stop_cameras(self):
        """Stops every camera of every company."""
        with self._control:
            self.running = False
            for t in self.threads:
                t.join(timeout=5)
            self.threads.clear()
            for s in list(dict.fromkeys(list(self.company_of) + list(self._held))):
                self._forget(s)
            self._held = {}
            self.company_of = {}
            self.frame_queues = {}
        logger.info("All camera threads stopped")
