"""Activity gate: skip the camera frames that show what the last processed frame of the same camera showed.

The engine is deterministic, so a frame of an unchanged scene costs a full detect -> align -> embed -> match pass to reproduce
the previous answer.  The reference sheds load blindly (/root/reference/peopleCount.py:938,962 takes every 2nd frame,
/root/reference/infrenceServer.py:595-598,614-617 drop frames when a queue is full).  ``ActivityGate`` looks instead: per
camera it keeps, on the device, the 16 x 16-cell luma means of the last frame that went through the engine, and a new frame is
*active* when at least ``min_cells`` of its cells moved by more than ``thr`` (csrc/frame_activity.hip; the arithmetic and the
rule: include/frhip.h fr_frame_activity_u8).  The grid moves only when a frame is judged active, so the
comparison is always against the last frame the engine saw: a slow drift accumulates until it crosses ``thr``.
"""
import threading

import numpy as np
import torch

from . import _lib

CELL = 16


class ActivityGate:
    """The state of ``slots`` cameras and the judgment of a batch of their frames.

    ``thr=4, min_cells=2`` are a judgment, not a measurement: the 16 x 16 mean of sensor noise with sigma about 3 has sigma
    about 0.2, so a static scene stays far below 4, and a face 20 pixels wide that moves changes several cells by far more.
    Their false-positive and false-negative rates on real video are not measured.  ``max_idle`` > 0 lets a frame through
    after that many consecutive inactive ones whatever it shows (0: never).

    Camera ids are any hashable values; a new id takes a free slot, ``forget`` gives it back.  One gate may be shared by the
    camera loop and request threads: the launches and the state they move are queued under one lock, in call order, on the
    calling thread's current stream."""

    _CACHE = 64                              # slot arrays kept: one per tuple of camera ids, oldest dropped first

    def __init__(self, device="cuda:0", slots=256, max_hw=(2160, 3840), thr=4, min_cells=2, max_idle=0):
        if int(slots) < 1:
            raise ValueError("slots must be positive")
        if int(max_hw[0]) < CELL or int(max_hw[1]) < CELL:
            raise ValueError(f"max_hw must hold one {CELL} x {CELL} cell at least")
        if not 0 <= int(thr) <= 255 or int(min_cells) < 1 or int(max_idle) < 0:
            raise ValueError("thr 0..255, min_cells >= 1, max_idle >= 0")
        _lib.require_gpu()
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.index is None:                            # "cuda": the current device, by its number
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.slots, self.max_hw = int(slots), (int(max_hw[0]), int(max_hw[1]))
        self.thr, self.min_cells, self.max_idle = int(thr), int(min_cells), int(max_idle)
        cells = (self.max_hw[0] // CELL) * (self.max_hw[1] // CELL)
        self.cells = (cells + 15) // 16 * 16                     # C, the row stride of grid and of the scratch
        self.grid = torch.zeros((self.slots, self.cells), dtype=torch.uint8, device=self.device)
        self.geom = torch.zeros((self.slots, 2), dtype=torch.int32, device=self.device)
        self.idle = torch.zeros(self.slots, dtype=torch.int32, device=self.device)
        self._slot_of, self._free = {}, list(range(self.slots - 1, -1, -1))
        self._slot_arrays = {}                                   # tuple of camera ids -> int32 [N] on the device
        self._lock = threading.Lock()

    def __len__(self):
        return len(self._slot_of)

    def slot_of(self, camera_id):
        """The slot of a camera id, None when it has none (yet)."""
        return self._slot_of.get(camera_id)

    def forget(self, camera_id):
        """Free the camera's slot; its ``geom`` is zeroed, so whoever takes the slot next starts with an active frame.
        Unknown ids are ignored."""
        with self._lock:
            s = self._slot_of.pop(camera_id, None)
            if s is None:
                return
            self._slot_arrays.clear()                            # the id -> slot map moved
            with torch.cuda.device(self.device):
                self.geom[s].zero_()
                self.idle[s].zero_()
            self._free.append(s)

    def _slots_for(self, camera_ids):
        """int32 [N] on the device for this tuple of ids (under the lock); uploaded once per tuple"""
        key = tuple(camera_ids)
        if len(set(key)) != len(key):
            raise ValueError("a camera id is repeated in one call: a slot is judged once per batch")
        hit = self._slot_arrays.pop(key, None)
        if hit is None:
            new = [c for c in key if c not in self._slot_of]
            if len(new) > len(self._free):
                raise ValueError(f"the gate has {self.slots} slots and {len(self._free)} free: "
                                 f"{len(new)} new camera ids do not fit (forget() frees one)")
            for c in new:
                self._slot_of[c] = self._free.pop()
            hit = torch.tensor([self._slot_of[c] for c in key], dtype=torch.int32).to(self.device)
            while len(self._slot_arrays) >= self._CACHE:
                self._slot_arrays.pop(next(iter(self._slot_arrays)))
        self._slot_arrays[key] = hit                             # most recently used last
        return hit

    def judge_device(self, frames, camera_ids, table=None):
        """``frames``: BGR ``uint8 [N,H,W,3]`` on the device, frame i from camera ``camera_ids[i]`` - or, with ``table``, the
        arena and the frame table of a ``RaggedIngest`` (frames of any sizes).  Returns ``(active, changed)``, ``int32 [N]``
        device tensors: ``changed`` is the number of changed cells, -1 for a camera's first frame, a new frame size, or a
        frame the gate does not judge (smaller than a cell, larger than ``max_hw``); such a frame is always active.  Runs on
        the current stream, no synchronisation; the state moves with the call."""
        ids = list(camera_ids)
        if table is None:
            if not (torch.is_tensor(frames) and frames.dim() == 4 and frames.shape[3] == 3 and frames.dtype == torch.uint8
                    and frames.is_contiguous() and frames.device == self.device):
                raise ValueError(f"frames must be a contiguous uint8 [N,H,W,3] tensor on {self.device}")
            n = frames.shape[0]
        else:
            if not (table.dtype == torch.uint8 and table.is_contiguous() and table.numel() % 32 == 0):
                raise ValueError("table must be the uint8 frame table of a RaggedIngest")
            n = table.numel() // 32
        if len(ids) != n:
            raise ValueError(f"one camera id per frame: {n} frames, {len(ids)} ids")
        with self._lock, torch.cuda.device(self.device):
            slot = self._slots_for(ids)
            cur = torch.empty((max(n, 1), self.cells), dtype=torch.uint8, device=self.device)
            changed = torch.empty(n, dtype=torch.int32, device=self.device)
            active = torch.empty(n, dtype=torch.int32, device=self.device)
            state = (_lib.ptr(self.grid), _lib.ptr(self.geom), _lib.ptr(self.idle), self.cells, _lib.ptr(cur),
                     _lib.ptr(changed), _lib.ptr(active), self.thr, self.min_cells, self.max_idle, _lib.stream_ptr())
            if table is None:
                self.lib.fr_frame_activity_u8(_lib.ptr(frames), n, frames.shape[1], frames.shape[2], _lib.ptr(slot),
                                              self.slots, *state)
            else:
                self.lib.fr_frame_activity_refs_u8(_lib.ptr(table), n, _lib.ptr(slot), self.slots, *state)
        return active, changed

    def judge(self, frames, camera_ids, table=None):
        """``judge_device`` with the verdicts on the host: ``(active bool [N], changed int32 [N])`` NumPy arrays, one
        synchronisation."""
        active, changed = self.judge_device(frames, camera_ids, table)
        both = torch.stack([active, changed]).cpu().numpy()
        return both[0] != 0, both[1].astype(np.int32)
