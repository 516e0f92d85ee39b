"""Face tracks: carry a face's embedding from one frame of a camera to the next and embed only the faces that are new.

In an active frame nearly every face is one the previous frame of the same camera already showed, a few pixels away, and
``recognize_batch`` pushes it through align and the embed net again to get the same row of the gallery.  ``FaceTracks`` keeps,
per camera and on the device, the boxes of the faces last seen and the embedding each was last given; between detect and
align one launch decides per detection whether it is such a face (csrc/face_tracks.hip; the rule: include/frhip.h
fr_track_associate_f32), the embed net runs for the others only, and a second launch moves rows between the
batch's embeddings and the bank.  What is held is the embedding, never the identity: a carried face goes through the gallery
scan of the current call like any other row, so syncs, evictions and per-company views act on it as on a fresh one.

With ``quality=FaceQuality(...)`` the tracks judge: a third launch between the quality launch and the one host copy decides per
face embed, carry or reject (include/frhip.h fr_track_resolve_quality_i32), the bank holds a track's last FIT
embedding only, and a face that turns unfit for a few frames keeps that row for up to ``max_age`` turns.

With ``template=K`` the tracks fuse: behind the commit launch one more launch keeps a ring of the track's last K unit embeddings
and answers each tracked face with their unit mean, the scan ``query`` (include/frhip.h fr_track_fuse_f32).
"""
import threading

import numpy as np
import torch

from . import _lib

DIM = 512
NO_FACE, EMBED, CARRY, REJECT = 0, 1, 2, 3   # the action column of judging tracks (fr_track_resolve_quality_i32)
T_NONE, T_STARTED, T_JOINED, T_RESTARTED, T_READ = 0, 1, 2, 3, 4   # the event column of fusing tracks (fr_track_fuse_f32)


class FaceTracks:
    """The tracks of ``slots`` cameras, ``entries`` (1 .. 64) faces each, and the two launches of a batch of their frames.

    ``iou_thr=0.5, max_reuse=4, max_misses=1`` are a judgment, not a measurement.  A face 60 pixels wide that moves 10 pixels
    between two frames keeps an IoU of about 0.7, so 0.5 follows a walking person at 30 fps and loses a running one - who is
    then embedded, the safe side.  ``max_reuse=4`` embeds a standing face every fifth active frame: pose and light drift
    slowly, and the embed load of a persistent scene falls to a fifth.  ``max_misses=1`` keeps a track over one frame in which
    the detector lost the face.  A matched face is never carried while another track of its camera overlaps it at all: faces
    that touch or cross are embedded again, which is the guard against handing one person's embedding to another.  None of
    these figures' error rates on real video is measured.

    Camera ids are any hashable values; a new id takes a free slot, ``forget`` gives it back.  One lock orders the launches and
    the state they move, in call order, on the calling thread's current stream.  The bank takes slots x entries x 4 KB of
    device memory: 32 MB with the defaults.

    ``quality`` (a ``quality.FaceQuality``) makes the tracks judge; the object is then passed as ``tracks=`` alone (``quality=``
    beside ``tracks=`` stays a ValueError everywhere): the bank belongs to the tracks, and the quality object is the rule for
    what may enter it.  An unfit face is never embedded; where its track holds a fit row not older than ``max_age`` turns and the
    associate launch does not ask for an embed, the face is carried on that row, otherwise it is rejected.  ``max_age=8`` bounds
    how long one fit row may stand in for a face that never becomes fit again; it is a judgment, not a measurement, like the
    other defaults.  The per-entry state ``tqual`` i32 [slots,entries,4] = (has, age, id, 0) exists only with ``quality``; an
    entry holds a fit row iff ``has == 1`` and its id is the track's, so ``forget``, ``reset`` and the reuse of a retired entry -
    which all end in a track with a fresh id - need no work on it.  Without ``quality`` nothing changes: no launch more, no
    state more.

    ``template`` (0 .. 16; 0: off, nothing is allocated and no launch is added) makes the tracks fuse: each entry keeps the unit
    embeddings of its track's last ``template`` shots and their unit mean, the template, and ``fuse_device`` hands that mean out
    as the row the gallery scan is asked with.  A new shot joins the template only when its dot with it reaches ``join_thr``
    (-1 .. 1); otherwise the template starts over from that shot alone, which is then returned unblended - the guard against
    mixing two people into one row.  With ``template=1`` the template is always the last embedded row and the query equals the
    normed embedding bit for bit.  The state ``tring`` f32 [slots,entries,template,512], ``ttmpl`` i32 [slots,entries,4] =
    (len, head, id, 0) and ``tmean`` f32 [slots,entries,512] takes slots x entries x (template + 1) x 2 KB of device memory
    (and 16 bytes per entry): 176 MB with the default slots and entries at ``template=10``.  An entry holds a template iff
    ``len >= 1`` and its id is the track's, so ``forget``, ``reset`` and a reused entry need no work on it either.
    ``join_thr=0.4`` is the reference's pose-consistency figure for "two shots of one person", and a depth of 10 is the ring
    depth of its ``UnknownPerson`` (peopleCount.py:63); both are a judgment here, not a measurement: the weights of this tree are
    synthetic, and neither the error rate of the join test nor the gain of any depth on real video is known."""

    _CACHE = 64                              # slot arrays kept: one per tuple of camera ids, oldest dropped first

    def __init__(self, device="cuda:0", slots=256, entries=32, iou_thr=0.5, max_reuse=4, max_misses=1, quality=None,
                 max_age=8, template=0, join_thr=0.4):
        if int(slots) < 1:
            raise ValueError("slots must be positive")
        if not 1 <= int(entries) <= 64:
            raise ValueError("entries 1 .. 64 (one lane of a wave each)")
        if not 0.0 < float(iou_thr) <= 1.0 or int(max_reuse) < 0 or int(max_misses) < 0:
            raise ValueError("iou_thr in (0, 1], max_reuse >= 0, max_misses >= 0")
        if int(max_age) < 0:
            raise ValueError("max_age >= 0 (0: a held row never stands in for an unfit face)")
        if not 0 <= int(template) <= 16:
            raise ValueError("template 0 .. 16 shots (0: off)")
        if not -1.0 <= float(join_thr) <= 1.0:                   # false for a NaN
            raise ValueError("join_thr in [-1, 1]")
        if quality is not None:
            from .quality import FaceQuality
            if not isinstance(quality, FaceQuality):
                raise ValueError("quality must be a quality.FaceQuality or None")
        _lib.require_gpu()
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.index is None:                            # "cuda": the current device, by its number
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.slots, self.entries = int(slots), int(entries)
        self.iou_thr, self.max_reuse, self.max_misses = float(iou_thr), int(max_reuse), int(max_misses)
        self.tbox = torch.zeros((self.slots, self.entries, 4), dtype=torch.float32, device=self.device)
        self.tstate = torch.zeros((self.slots, self.entries, 4), dtype=torch.int32, device=self.device)
        self.next_id = torch.zeros(self.slots, dtype=torch.int32, device=self.device)
        self.bank = torch.zeros((self.slots, self.entries, 2, DIM), dtype=torch.float32, device=self.device)
        self.stats = {"faces": 0, "embedded": 0, "carried": 0, "untracked": 0}
        self.quality, self.max_age = quality, int(max_age)
        if quality is not None:                                  # the judging tracks' state and their count of rejected faces
            self.tqual = torch.zeros((self.slots, self.entries, 4), dtype=torch.int32, device=self.device)
            self.stats["rejected"] = 0
        self.template, self.join_thr = int(template), float(join_thr)
        if self.template:                                        # the fusing tracks' state and their counts of joins and restarts
            self.tring = torch.zeros((self.slots, self.entries, self.template, DIM), dtype=torch.float32, device=self.device)
            self.ttmpl = torch.zeros((self.slots, self.entries, 4), dtype=torch.int32, device=self.device)
            self.tmean = torch.zeros((self.slots, self.entries, DIM), dtype=torch.float32, device=self.device)
            self.stats["joined"] = self.stats["restarted"] = 0
        self._slot_of, self._free = {}, list(range(self.slots - 1, -1, -1))
        self._slot_arrays = {}                                   # tuple of camera ids -> int32 [N] on the device
        self._lock = threading.Lock()

    def __len__(self):
        return len(self._slot_of)

    def slot_of(self, camera_id):
        """The slot of a camera id, None when it has none (yet)."""
        return self._slot_of.get(camera_id)

    def forget(self, camera_id):
        """Free the camera's slot; its ``live`` flags are zeroed, so whoever takes the slot next starts without tracks (the
        slot's id counter runs on).  Unknown ids are ignored."""
        with self._lock:
            s = self._slot_of.pop(camera_id, None)
            if s is None:
                return
            self._slot_arrays.clear()                            # the id -> slot map moved
            with torch.cuda.device(self.device):
                self.tstate[s, :, 0].zero_()
            self._free.append(s)

    def reset(self, camera_ids):
        """Drop the tracks of these cameras (their slots stay theirs): for a caller whose embed pass failed between
        ``associate_device`` and ``commit_device``, when the bank does not hold what the state says it holds."""
        with self._lock, torch.cuda.device(self.device):
            for c in camera_ids:
                s = self._slot_of.get(c)
                if s is not None:
                    self.tstate[s, :, 0].zero_()

    def _slots_for(self, camera_ids):
        """int32 [N] on the device for this tuple of ids (under the lock); uploaded once per tuple"""
        key = tuple(camera_ids)
        if len(set(key)) != len(key):
            raise ValueError("a camera id is repeated in one call: a slot's tracks move once per batch")
        hit = self._slot_arrays.pop(key, None)
        if hit is None:
            new = [c for c in key if c not in self._slot_of]
            if len(new) > len(self._free):
                raise ValueError(f"the tracks have {self.slots} slots and {len(self._free)} free: "
                                 f"{len(new)} new camera ids do not fit (forget() frees one)")
            for c in new:
                self._slot_of[c] = self._free.pop()
            hit = torch.tensor([self._slot_of[c] for c in key], dtype=torch.int32).to(self.device)
            while len(self._slot_arrays) >= self._CACHE:
                self._slot_arrays.pop(next(iter(self._slot_arrays)))
        self._slot_arrays[key] = hit                             # most recently used last
        return hit

    def _check(self, t, dtype, shape, what):
        if not (torch.is_tensor(t) and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous()
                and t.device == self.device):
            raise ValueError(f"{what} must be a contiguous {dtype} {list(shape)} tensor on {self.device}")

    def associate_device(self, boxes, counts, camera_ids):
        """``boxes`` f32 [N,cap,4] and ``counts`` i32 [N] as the detector leaves them, frame i from camera ``camera_ids[i]``.
        Returns ``(entry, need, tid)``, int32 [N,cap] device tensors: the track entry of a detection (-1: untracked), 1 where
        it has to be embedded (0: its embedding is in the bank, and in slots past a frame's count), its track id (-1: none).
        Runs on the current stream, no synchronisation; the state moves with the call."""
        ids = list(camera_ids)
        if not (torch.is_tensor(boxes) and boxes.dim() == 3):
            raise ValueError("boxes must be f32 [N,cap,4]")
        n, cap = boxes.shape[0], boxes.shape[1]
        self._check(boxes, torch.float32, (n, cap, 4), "boxes")
        self._check(counts, torch.int32, (n,), "counts")
        if len(ids) != n:
            raise ValueError(f"one camera id per frame: {n} frames, {len(ids)} ids")
        with self._lock, torch.cuda.device(self.device):
            slot = self._slots_for(ids)
            entry = torch.empty((n, cap), dtype=torch.int32, device=self.device)
            need = torch.empty_like(entry)
            tid = torch.empty_like(entry)
            self.lib.fr_track_associate_f32(_lib.ptr(boxes), _lib.ptr(counts), _lib.ptr(slot), n, cap, self.slots, self.entries,
                                            _lib.ptr(self.tbox), _lib.ptr(self.tstate), _lib.ptr(self.next_id), self.iou_thr,
                                            self.max_reuse, self.max_misses, _lib.ptr(entry), _lib.ptr(need), _lib.ptr(tid),
                                            _lib.stream_ptr())
        return entry, need, tid

    def commit_device(self, entry, need, counts, camera_ids, emb, normed):
        """The second launch, over the slot-layout ``emb`` / ``normed`` f32 [N*cap,512]: the rows embedded this turn go to the
        bank, the carried rows come from it (in place); every other row stays as it is.  ``camera_ids``: those of the
        ``associate_device`` call that made ``entry`` and ``need``."""
        ids = list(camera_ids)
        if not (torch.is_tensor(entry) and entry.dim() == 2):
            raise ValueError("entry must be i32 [N,cap]")
        n, cap = entry.shape
        self._check(entry, torch.int32, (n, cap), "entry")
        self._check(need, torch.int32, (n, cap), "need")
        self._check(counts, torch.int32, (n,), "counts")
        self._check(emb, torch.float32, (n * cap, DIM), "emb")
        self._check(normed, torch.float32, (n * cap, DIM), "normed")
        if len(ids) != n:
            raise ValueError(f"one camera id per frame: {n} frames, {len(ids)} ids")
        with self._lock, torch.cuda.device(self.device):
            slot = self._slots_for(ids)
            self.lib.fr_track_commit_f32(_lib.ptr(entry), _lib.ptr(need), _lib.ptr(slot), _lib.ptr(counts), n, cap, self.slots,
                                         self.entries, _lib.ptr(self.bank), _lib.ptr(emb), _lib.ptr(normed), _lib.stream_ptr())

    def resolve_device(self, entry, need, tid, verdict, counts, camera_ids):
        """The judging tracks' launch, between ``FaceQuality.measure_device`` and the host copy: ``entry``, ``need``, ``tid`` of
        this turn's ``associate_device`` and ``verdict`` i32 [N,cap] (0: fit) -> ``(action, need2, entry2)`` i32 [N,cap]:
        0 no face, 1 embed, 2 carry, 3 reject, and the (need, entry) pair ``commit_device`` takes this turn.  ``since`` of
        ``tstate`` and ``tqual`` move with the call.  Runs on the current stream, no synchronisation."""
        if self.quality is None:
            raise ValueError("these tracks do not judge: FaceTracks(..., quality=FaceQuality(...))")
        ids = list(camera_ids)
        if not (torch.is_tensor(entry) and entry.dim() == 2):
            raise ValueError("entry must be i32 [N,cap]")
        n, cap = entry.shape
        for t, what in ((entry, "entry"), (need, "need"), (tid, "tid"), (verdict, "verdict")):
            self._check(t, torch.int32, (n, cap), what)
        self._check(counts, torch.int32, (n,), "counts")
        if len(ids) != n:
            raise ValueError(f"one camera id per frame: {n} frames, {len(ids)} ids")
        with self._lock, torch.cuda.device(self.device):
            slot = self._slots_for(ids)
            action = torch.empty((n, cap), dtype=torch.int32, device=self.device)
            need2 = torch.empty_like(action)
            entry2 = torch.empty_like(action)
            self.lib.fr_track_resolve_quality_i32(_lib.ptr(entry), _lib.ptr(need), _lib.ptr(tid), _lib.ptr(verdict), _lib.ptr(slot),
                                                  _lib.ptr(counts), n, cap, self.slots, self.entries, _lib.ptr(self.tstate),
                                                  _lib.ptr(self.tqual), self.max_age, _lib.ptr(action), _lib.ptr(need2),
                                                  _lib.ptr(entry2), _lib.stream_ptr())
        return action, need2, entry2

    def fuse_device(self, entry, need, tid, counts, camera_ids, normed):
        """The fusing tracks' launch, right behind ``commit_device`` and over the same ``entry`` / ``need`` (``entry2`` /
        ``need2`` under judging tracks), ``tid`` of this turn's ``associate_device`` and the slot-layout ``normed`` f32
        [N*cap,512] the commit left -> ``(query, shots, event)``: f32 [N*cap,512], the row to scan with (the track's template
        where it has one, else the ``normed`` row), and i32 [N,cap]: the shots the template holds (0: none) and 0 none,
        1 started, 2 joined, 3 restarted, 4 read.  ``tring``, ``ttmpl`` and ``tmean`` move with the call.  Runs on the current
        stream, no synchronisation."""
        if not self.template:
            raise ValueError("these tracks do not fuse: FaceTracks(..., template=K)")
        ids = list(camera_ids)
        if not (torch.is_tensor(entry) and entry.dim() == 2):
            raise ValueError("entry must be i32 [N,cap]")
        n, cap = entry.shape
        for t, what in ((entry, "entry"), (need, "need"), (tid, "tid")):
            self._check(t, torch.int32, (n, cap), what)
        self._check(counts, torch.int32, (n,), "counts")
        self._check(normed, torch.float32, (n * cap, DIM), "normed")
        if len(ids) != n:
            raise ValueError(f"one camera id per frame: {n} frames, {len(ids)} ids")
        with self._lock, torch.cuda.device(self.device):
            slot = self._slots_for(ids)
            query = torch.empty((n * cap, DIM), dtype=torch.float32, device=self.device)
            shots = torch.empty((n, cap), dtype=torch.int32, device=self.device)
            event = torch.empty_like(shots)
            self.lib.fr_track_fuse_f32(_lib.ptr(entry), _lib.ptr(need), _lib.ptr(tid), _lib.ptr(slot), _lib.ptr(counts),
                                       _lib.ptr(normed), n, cap, self.slots, self.entries, self.template, self.join_thr,
                                       _lib.ptr(self.tring), _lib.ptr(self.ttmpl), _lib.ptr(self.tmean), _lib.ptr(query),
                                       _lib.ptr(shots), _lib.ptr(event), _lib.stream_ptr())
        return query, shots, event

    def count_events(self, event):
        """Add one batch's joins and restarts to ``stats`` from a host copy of its event column [N,cap]."""
        event = np.asarray(event)
        with self._lock:
            self.stats["joined"] += int((event == T_JOINED).sum())
            self.stats["restarted"] += int((event == T_RESTARTED).sum())

    def count(self, counts, need, entry, action=None):
        """Add one batch to ``stats`` from host copies of its counts [N], need and entry [N,cap] (the batch path reads them
        back anyway): faces = embedded + carried, untracked are the embedded ones no entry was free for.  With the ``action``
        column of judging tracks (``need`` is then not read): faces = embedded + carried + rejected, untracked are the faces
        without an entry, embedded or not."""
        counts, entry = np.asarray(counts), np.asarray(entry)
        valid = np.arange(entry.shape[1])[None, :] < counts[:, None]
        faces = int(valid.sum())
        if action is None:
            embedded = int((valid & (np.asarray(need) != 0)).sum())
            carried, rejected = faces - embedded, None
        else:
            action = np.asarray(action)
            embedded, carried, rejected = (int((valid & (action == a)).sum()) for a in (1, 2, 3))
        with self._lock:
            self.stats["faces"] += faces
            self.stats["embedded"] += embedded
            self.stats["carried"] += carried
            self.stats["untracked"] += int((valid & (entry < 0)).sum())
            if rejected is not None:
                self.stats["rejected"] += rejected
