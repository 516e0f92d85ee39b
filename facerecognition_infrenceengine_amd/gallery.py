"""Device-resident gallery + matcher (rows a-6/a-7/a-8/a-10 of SURVEY.md section 8).

Replaces the per-face Python loop over ``dict[id -> float32[512]]`` at
/root/reference/infrenceServer.py:535-552 (and peopleCount.py:866-887) with one HIP scan
of a row-indexed ``[N,512]`` matrix.  Row order = insertion order of the reference's
dict (employees in cursor order, then visitors: infrenceServer.py:264,288); the winner is
the maximum score, lowest row on exact ties (strict ``>`` in the reference loop).

Every scan of plain rows or of a view goes through ``_scan``: one prelude, one table (``_ENTRIES``) that names the
entry point and its arguments.  What is scanned is a ``RowSource``.
"""
import collections
import threading

import numpy as np
import torch

from . import _lib

DIM = 512
TOPK_MAX = 16                  # include/frhip.h FR_TOPK_MAX
SCANS = ("f32", "f16", "f8")
_SHADOW_KIND = {"f16": 1, "f8": 2}      # include/frhip.h FR_SHADOW_F16 / FR_SHADOW_F8
_PIN = threading.local()       # pinned host buffers of read_back, per thread, shapes and dtypes
_TLS = threading.local()       # .topk: what this thread's last top-K call ran (last_topk())
# Rows from which an f16-coarse gallery answers top-K by the certified coarse pass instead of the exact scan.  Not yet
# measured on hardware for the top-K path: the size where the top-1 coarse view scan won (profiles/view_scan.txt).
COARSE_TOPK_MIN_ROWS = 100_000

# What a scan reads: the f32 rows ``G``; ``view``, the int64 slot list the positions go through (None: row = position);
# ``N`` positions; the ``capacity`` of the slab ``G``; the ``coarse`` copy of ``G`` and its ``kind`` "f16" / "f8" (both
# None without one); ``gmax``, the bound on the row norms that goes with an f16 copy (else None).
RowSource = collections.namedtuple("RowSource", "G view N capacity coarse kind gmax")


def last_topk():
    """What the calling thread's last ``match_topk_device`` ran, without a synchronisation: {"path": "coarse" | "exact",
    "flags": device int32 [F] or None}.  On the coarse path flags[f] is 0 where the coarse pass was certified to give the
    exact top-K and 1 where query f was answered by the exact scan instead; both give the same bits."""
    return getattr(_TLS, "topk", None)


class StaleViewError(_lib.FrError):
    """A GalleryView was used after its gallery's membership changed: fetch a fresh view and retry."""


class DuplicateOverflowError(_lib.FrError):
    """``find_duplicates`` met more candidate pairs than ``max_pairs``: ``needed`` is the ``max_pairs`` that suffices."""

    def __init__(self, msg, needed):
        super().__init__(msg)
        self.needed = needed


PAIRS_OVERFLOW, PAIRS_NONFINITE = 1, 2      # include/frhip.h FR_PAIRS_OVERFLOW / FR_PAIRS_NONFINITE


class DuplicatePairs:
    """What ``find_duplicates`` found: ``pairs`` int64 [P,2] positions a < b sorted by (a, b), ``scores`` float32 [P] (the
    dot of the duplicate check, bit for bit), ``ids`` [(id_a, id_b)], ``candidates``: pairs the coarse filter let through."""

    def __init__(self, pairs, scores, ids, candidates):
        self.pairs, self.scores, self.ids, self.candidates = pairs, scores, ids, candidates

    def __len__(self):
        return len(self.pairs)


def _workspace(device, need):
    """Scratch for ONE scan, taken from torch's caching allocator under the current stream: the block is
    owned by that stream, so concurrent matches on different streams never share (or free) each other's
    partial results.  (A per-object buffer did: two pipes driving one matcher overwrote ws_score/ws_idx.)"""
    return torch.empty(max(int(need), 16), dtype=torch.uint8, device=device)


def read_back(device, *tensors):
    """Several device results, ONE synchronisation: asynchronous copies into pinned host memory, then a sync of the
    current stream of ``device``.  Returns the NumPy copies.  The pinned buffers are kept per thread (several may read
    back at once), keyed by the results' shapes and dtypes, 16 sets at the most."""
    pin = _PIN.__dict__.setdefault("bufs", {})
    key = tuple((t.shape, t.dtype) for t in tensors)
    host = pin.get(key)
    if host is None:
        if len(pin) >= 16:
            pin.clear()
        host = pin[key] = [torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in tensors]
    with torch.cuda.device(device):
        for dst, src in zip(host, tensors):
            dst.copy_(src, non_blocking=True)
        torch.cuda.current_stream().synchronize()
    return [h.numpy().copy() for h in host]


def _check_k(k):
    if not 1 <= int(k) <= TOPK_MAX:
        raise ValueError(f"k must be 1..{TOPK_MAX} (got {k})")
    return int(k)


def _queries(lib, device, Q, renormalise, counts, seg_len):
    """The query half of every scan's prelude: (Q as float32 [F,512] on ``device`` - L2-normalised by one launch with
    ``renormalise``, infrenceServer.py:532 -, F); ``counts`` / ``seg_len`` are checked against F.  Called under
    ``torch.cuda.device(device)``."""
    Q = Q.to(device, torch.float32).contiguous().reshape(-1, DIM)
    F = Q.shape[0]
    if counts is not None:
        assert counts.dtype == torch.int32 and counts.is_contiguous() and seg_len > 0 and F == counts.numel() * seg_len
    if renormalise and F:
        Qn = torch.empty_like(Q)
        lib.fr_l2norm_rows_f32(_lib.ptr(Q), _lib.ptr(Qn), F, DIM, _lib.stream_ptr())
        Q = Qn
    return Q, F


def _outputs(device, F, k, path="exact"):
    """(idx int64, score float32) of a top-1 ([F]) or top-``k`` ([F,k]) scan; the latter is what ``last_topk`` reports."""
    if k is not None:
        _TLS.topk = {"path": path, "flags": None}
    shape = (F,) if k is None else (F, k)
    return torch.empty(shape, dtype=torch.int64, device=device), torch.empty(shape, dtype=torch.float32, device=device)


# (top-K, through a slot list, coarse kind used): the workspace entry, the scan entry, and its arguments between Q and
# the outputs; ``p`` is the RowSource with pointers for tensors.  Every entry then takes idx, score, (flags: coarse
# top-K,) workspace, bytes, (counts, seg_len: plain rows only,) stream.
_WS, _WS_TOPK = "fr_gallery_match_workspace", "fr_gallery_topk_workspace"       # the exact scans share theirs
_ENTRIES = {
    (False, False, None): (_WS, "fr_gallery_match_f32", lambda p, F, k, off: (p.G, F, p.N, DIM, off)),
    (False, False, "f16"): ("fr_gallery_match_f16_workspace", "fr_gallery_match_f16",
                            lambda p, F, k, off: (p.coarse, p.G, F, p.N, DIM, off)),
    (False, False, "f8"): ("fr_gallery_match_f8_workspace", "fr_gallery_match_f8",
                           lambda p, F, k, off: (p.coarse, p.G, F, p.N, DIM, off)),
    (False, True, None): (_WS, "fr_gallery_match_view_f32", lambda p, F, k, off: (p.G, p.view, F, p.N, DIM)),
    (False, True, "f16"): ("fr_gallery_match_view_f16_workspace", "fr_gallery_match_view_f16",
                           lambda p, F, k, off: (p.coarse, p.G, p.view, F, p.N, p.capacity, DIM)),
    (False, True, "f8"): ("fr_gallery_match_view_f8_workspace", "fr_gallery_match_view_f8",
                          lambda p, F, k, off: (p.coarse, p.G, p.view, F, p.N, p.capacity, DIM)),
    (True, False, None): (_WS_TOPK, "fr_gallery_topk_f32", lambda p, F, k, off: (p.G, F, p.N, DIM, k, off)),
    (True, False, "f16"): ("fr_gallery_topk_f16_workspace", "fr_gallery_topk_f16",
                           lambda p, F, k, off: (p.coarse, p.G, F, p.N, DIM, k, off, p.gmax)),
    (True, True, None): (_WS_TOPK, "fr_gallery_topk_view_f32", lambda p, F, k, off: (p.G, p.view, F, p.N, DIM, k)),
    (True, True, "f16"): ("fr_gallery_topk_view_f16_workspace", "fr_gallery_topk_view_f16",
                          lambda p, F, k, off: (p.coarse, p.G, p.view, F, p.N, p.capacity, DIM, k, p.gmax)),
}


def _scan(lib, device, src, Q, k, renormalise, kind, row_offset=0, counts=None, seg_len=0):
    """The scan of ``src`` (a RowSource) for the rows of ``Q`` on the current stream of ``device``: the best row per query
    (``k`` None: idx int64 [F], score float32 [F]) or the ``k`` best ([F,k]; records ``last_topk()``).  ``kind``: the
    coarse copy to scan in one pass before the exact f32 re-scoring ("f16" / "f8"; top-K: "f16", the certified pass), or
    None for the exact f32 scan.  ``row_offset`` / ``counts`` / ``seg_len`` go to the scans of plain rows only."""
    with torch.cuda.device(device):
        Q, F = _queries(lib, device, Q, renormalise, counts, seg_len)
        idx, score = _outputs(device, F, k, "coarse" if kind else "exact")
        if F == 0:
            return idx, score
        wsz, entry, head = _ENTRIES[k is not None, src.view is not None, kind]
        kk = () if k is None else (k,)
        flags = None
        if kk and kind:
            flags = _TLS.topk["flags"] = torch.empty(F, dtype=torch.int32, device=device)
        # pointers of tensors that src, flags and counts keep alive until the call returns (_lib.ptr)
        p = RowSource(_lib.ptr(src.G), _lib.ptr(src.view), src.N, src.capacity, _lib.ptr(src.coarse), src.kind,
                      _lib.ptr(src.gmax))
        certified = () if flags is None else (_lib.ptr(flags),)
        padding = (_lib.ptr(counts), seg_len) if src.view is None else ()
        ws = _workspace(device, getattr(lib, wsz)(F, src.N, *kk))
        getattr(lib, entry)(_lib.ptr(Q), *head(p, F, k, row_offset), _lib.ptr(idx), _lib.ptr(score), *certified,
                            _lib.ptr(ws), ws.numel(), *padding, _lib.stream_ptr())
    return idx, score


def _topk_kind(src, min_rows):
    """The coarse kind a top-K scan of ``src`` uses: the certified pass over an f16 copy of at least ``min_rows`` rows."""
    return "f16" if src.kind == "f16" and src.N >= min_rows else None


def _pairs_device(lib, device, src, thr, inclusive, max_pairs, max_ranges=0):
    """fr_gallery_pairs_above_f16 over ``src`` on the current stream of ``device``: (keys int64 [max_pairs], scores
    float32 [max_pairs], counts int32 [4]), device tensors, no synchronisation."""
    max_pairs = int(max_pairs)
    if max_pairs < 1:
        raise ValueError("max_pairs must be at least 1")
    keys = torch.empty(max_pairs, dtype=torch.int64, device=device)
    scores = torch.empty(max_pairs, dtype=torch.float32, device=device)
    counts = torch.empty(4, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        ws = _workspace(device, lib.fr_gallery_pairs_workspace(src.N, max_pairs))
        lib.fr_gallery_pairs_above_f16(_lib.ptr(src.G), _lib.ptr(src.view), src.N, DIM, float(thr), 1 if inclusive else 0,
                                       max_pairs, int(max_ranges), _lib.ptr(keys), _lib.ptr(scores), _lib.ptr(counts),
                                       _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    return keys, scores, counts


def _pairs_host(device, ids, keys, scores, counts):
    """One synchronisation to read the counts, then the P pairs found travel and are sorted on the host."""
    seen, found, flags = (int(v) for v in read_back(device, counts)[0][:3])
    if flags & PAIRS_NONFINITE:
        raise ValueError("find_duplicates: a row holds NaN, an infinity or an element beyond the f16 range (+-65504)")
    if flags & PAIRS_OVERFLOW:
        raise DuplicateOverflowError(f"find_duplicates: {seen} candidate pairs, max_pairs is {keys.numel()}: retry with "
                                     f"max_pairs={seen}", seen)
    k = keys[:found].cpu().numpy()
    s = scores[:found].cpu().numpy()
    order = np.argsort(k, kind="stable")                 # a << 32 | b: the order of (a, b)
    k, s = k[order], s[order]
    pairs = np.stack([k >> 32, k & 0xFFFFFFFF], axis=1).astype(np.int64).reshape(-1, 2)
    return DuplicatePairs(pairs, s, [(ids[a], ids[b]) for a, b in pairs], seen)


class _Decides:
    """What everything that scans shares: the decision launch and ``last_topk``.  Needs ``lib`` and ``device``."""

    last_topk = property(lambda self: last_topk())

    def decide_device(self, idx, score, thr, unknown_thr=None):
        """1 recognised / 0 unknown / 2 dropped (peopleCount.py:876-887 band)."""
        d = torch.empty(idx.shape[0], dtype=torch.int32, device=self.device)
        if idx.shape[0]:
            with torch.cuda.device(self.device):
                self.lib.fr_match_decide(_lib.ptr(idx), _lib.ptr(score), idx.shape[0], float(thr),
                                         float(thr if unknown_thr is None else unknown_thr), _lib.ptr(d),
                                         _lib.stream_ptr())
        return d


class _Rows(_Decides):
    """The host-facing forms and the audit of an object with ``ids``, ``row_source()``, ``match_device`` and
    ``match_topk_device``: GalleryMatcher (rows are positions) and GalleryView (positions in ``ids`` go through slots)."""

    def match(self, Q, thr=0.4, unknown_thr=None):
        """Host-facing: returns (ids list (None = unknown), scores float32[F], idx int64[F])."""
        Q = torch.as_tensor(np.asarray(Q, np.float32)) if not torch.is_tensor(Q) else Q
        idx, score = self.match_device(Q)
        dec = self.decide_device(idx, score, thr, unknown_thr)
        idx_h, score_h, dec_h = read_back(self.device, idx, score, dec)
        ids = [self.ids[i] if (d == 1 and i >= 0) else None for i, d in zip(idx_h, dec_h)]
        return ids, score_h, idx_h

    def match_topk(self, Q, k, min_score=None):
        """Host-facing: (ids, scores float32[F,k], idx int64[F,k]); ``ids[f]`` is a list of k entries in rank order,
        None for empty slots and for slots whose score is below ``min_score``."""
        k = _check_k(k)
        Q = torch.as_tensor(np.asarray(Q, np.float32)) if not torch.is_tensor(Q) else Q
        idx_h, score_h = read_back(self.device, *self.match_topk_device(Q, k))
        ids = [[self.ids[i] if i >= 0 and (min_score is None or s >= min_score) else None for i, s in zip(ri, rs)]
               for ri, rs in zip(idx_h, score_h)]
        return ids, score_h, idx_h

    def find_duplicates_device(self, thr=0.4, inclusive=False, max_pairs=1 << 20, max_ranges=0):
        """The audit of ``find_duplicates`` without a synchronisation: device tensors (keys int64 [max_pairs]: a << 32 | b,
        scores float32 [max_pairs], counts int32 [4]: candidates seen, pairs written, flags (1: more candidates than
        ``max_pairs``, 2: a non-finite row), row ranges used).  The first counts[1] entries hold the pairs, in no order.
        a and b are positions in ``self.ids``.  The f32 rows are read (a view's through its slot list) whatever ``scan``
        the object was built with; the coarse copy is not."""
        return _pairs_device(self.lib, self.device, self.row_source(), thr, inclusive, max_pairs, max_ranges)

    def find_duplicates(self, thr=0.4, inclusive=False, max_pairs=1 << 20):
        """Every pair of rows a < b the enrolment duplicate check would refuse: dot(row a, row b) > ``thr`` (``inclusive``:
        >=) with the dot of ``first_above`` on the rows as stored, bit for bit - one pass over the pairs on the f16 matrix
        cores as a filter, the exact dot for every candidate.  Exact, not approximate, for finite rows
        inside the f16 range; a row outside it raises ValueError.  More than ``max_pairs`` candidates raise
        ``DuplicateOverflowError`` whose ``needed`` is the ``max_pairs`` to retry with.  Returns ``DuplicatePairs``."""
        return _pairs_host(self.device, self.ids, *self.find_duplicates_device(thr, inclusive, max_pairs))


class GalleryMatcher(_Rows):
    """``G[N,512]`` float32 unit rows on the device + the id table."""

    def __init__(self, device="cuda:0", f16_scan=False, scan=None):
        """``scan``: "f32" (default: exact f32 scan on the f32 matrix cores), "f16" or "f8": keep a 16-bit / 8-bit
        copy of the rows, scan THAT in one pass on the f16 / fp8 matrix cores for the whole query batch, then
        re-score the top-4 / top-8 rows per query exactly in f32 (large galleries / many queries: BASELINE
        configs C4 / C5); the f32 rows are kept.  ``f16_scan=True`` is the older spelling of scan="f16"."""
        _lib.require_gpu()
        self.scan = scan or ("f16" if f16_scan else "f32")
        if self.scan not in SCANS:
            raise ValueError("scan must be 'f32', 'f16' or 'f8'")
        self.f16_scan = self.scan == "f16"
        self.G16 = None                       # the coarse copy (f16 or fp8 e4m3 x 256)
        self.coarse_topk_min_rows = COARSE_TOPK_MIN_ROWS
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.ids = []
        self.G = torch.empty((0, DIM), dtype=torch.float32, device=self.device)
        # scan="f16": the largest row norm in G (+inf: a row the f16 copy cannot hold), for the top-K certificate
        self.gmax = torch.zeros(1, dtype=torch.float32, device=self.device) if self.scan == "f16" else None

    def __len__(self):
        return self.G.shape[0]

    def set_rows(self, ids, rows, normalise=True):
        """rows: float32 [N,512] (host or device).  ``normalise`` applies v/||v|| on the
        device exactly as the gallery ingest does (infrenceServer.py:271,324)."""
        rows = torch.as_tensor(np.asarray(rows, np.float32) if not torch.is_tensor(rows) else rows)
        rows = rows.to(self.device, torch.float32).contiguous().reshape(-1, DIM)
        if len(ids) != rows.shape[0]:
            raise ValueError("ids and rows disagree")
        if normalise and rows.shape[0]:
            out = torch.empty_like(rows)
            with torch.cuda.device(self.device):
                self.lib.fr_l2norm_rows_f32(_lib.ptr(rows), _lib.ptr(out), rows.shape[0], DIM, _lib.stream_ptr())
            rows = out
        self.ids = list(ids)
        self.G = rows
        self.G16 = None
        if self.scan != "f32" and rows.shape[0]:
            with torch.cuda.device(self.device):
                if self.scan == "f16":
                    self.G16 = torch.empty(rows.shape, dtype=torch.float16, device=self.device)
                    self.lib.fr_f32_to_f16(_lib.ptr(rows), _lib.ptr(self.G16), rows.numel(), _lib.stream_ptr())
                    self.gmax = torch.zeros(1, dtype=torch.float32, device=self.device)      # a new gallery: a new bound
                    self.lib.fr_gallery_gmax_update(_lib.ptr(rows), None, rows.shape[0], DIM, _lib.ptr(self.gmax),
                                                    _lib.stream_ptr())
                else:
                    self.G16 = torch.empty(rows.shape, dtype=torch.uint8, device=self.device)
                    self.lib.fr_f32_to_f8(_lib.ptr(rows), _lib.ptr(self.G16), rows.numel(), _lib.stream_ptr())

    def row_source(self):
        """The rows a scan of this matcher reads (``RowSource``)."""
        N = self.G.shape[0]
        return RowSource(self.G, None, N, N, self.G16, self.scan if self.G16 is not None else None, self.gmax)

    def match_device(self, Q, renormalise=True, row_offset=0, counts=None, seg_len=0):
        """Q: float32 [F,512] device tensor of ``normed_embedding`` rows.
        Returns device tensors (idx int64[F] (-1: empty gallery), score float32[F]).
        ``counts`` (device int32 [F / seg_len]) marks padding slots of a gathered batch (sharded match): slot f
        is real iff f % seg_len < counts[f // seg_len]; padding costs no scan work and reports (-1, -1)."""
        src = self.row_source()
        return _scan(self.lib, self.device, src, Q, None, renormalise, src.kind, row_offset, counts, seg_len)

    def match_topk_device(self, Q, k, renormalise=True, row_offset=0, counts=None, seg_len=0):
        """The ``k`` best rows per query (1 <= k <= 16): device tensors (idx int64[F,k], score float32[F,k]), ranked by
        score descending, row ascending, among rows scoring > -1; slots past the number of such rows hold (-1, -1.0).
        Column 0 is bit-identical to ``match_device``.  The result is that of the exact f32 scan over the f32 rows,
        bit for bit, whatever ``scan`` the matcher was built with.  scan="f16" with at least ``coarse_topk_min_rows``
        rows gets it from the certified coarse pass (one pass over the f16 rows, exact f32 re-scoring of the best
        groups, the exact scan only for queries the certificate refuses: DESIGN.md 4.6b); "f32", "f8" and smaller
        galleries run the exact scan.  ``last_topk`` tells which.  ``row_offset`` / ``counts`` / ``seg_len``: as
        ``match_device``."""
        k = _check_k(k)
        src = self.row_source()
        kind = _topk_kind(src, self.coarse_topk_min_rows)
        return _scan(self.lib, self.device, src, Q, k, renormalise, kind, row_offset, counts, seg_len)


class DeviceGallery:
    """One device-resident slab of gallery row slots with in-place updates + per-company views
    (SURVEY.md section 8f row 2).

    The reference keeps ``dict[id -> float32[512]]`` (infrenceServer.py:46), inserts/overwrites entries on
    every incremental sync (:271-273, :324-326), deletes inactive people (:250-252) and, PER FRAME, filters
    the dict by the company's member ids (:343-380).  Here the rows live once in HBM: ``upsert`` writes
    changed rows into their slots in place (new ids take a free slot, capacity doubles when full),
    ``remove`` frees slots, and a company view is only an int64 slot list in the reference's dict order -
    ``GalleryView.match_device`` scans the slab through it (no per-company copy of the rows).

    ``scan``: "f32" (default), "f16" or "f8", spelt and meant as ``GalleryMatcher``'s.  With "f16" / "f8" the gallery
    keeps a coarse shadow slab ``S`` beside ``G`` (f16, or fp8 e4m3 x 256: 1 KB / 0.5 KB more per slot) that every
    ``upsert`` writes in the same launch as the f32 rows, and views match by the one-pass coarse scan through the slot
    list with the exact f32 re-rank: the ids are those of the f32 scan.  For large galleries / many queries.  With "f16" a view of
    at least ``coarse_topk_min_rows`` rows also answers top-K from the coarse slab, certified per query to be the exact
    f32 top-K (``GalleryMatcher.match_topk_device``); ``gmax`` is the largest row norm ever written to the slab (it
    never shrinks on ``remove``).
    """

    def __init__(self, device="cuda:0", capacity=1024, scan="f32"):
        if scan not in SCANS:
            raise ValueError("scan must be 'f32', 'f16' or 'f8'")
        _lib.require_gpu()
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.scan = scan
        self.G = torch.zeros((max(int(capacity), 1), DIM), dtype=torch.float32, device=self.device)
        self.S = self._new_shadow(self.G.shape[0])       # the coarse slab; None for scan="f32"
        self.slot_of = {}                # id -> slot
        self._free = []                  # freed slots, reused LIFO
        self._next = 0                   # first never-used slot
        self.generation = 0              # bumps on every membership change (views check it)
        self.coarse_topk_min_rows = COARSE_TOPK_MIN_ROWS
        self.gmax = torch.zeros(1, dtype=torch.float32, device=self.device) if scan == "f16" else None

    def __len__(self):
        return len(self.slot_of)

    @property
    def capacity(self):
        return self.G.shape[0]

    def _new_shadow(self, capacity):
        if self.scan == "f32":
            return None
        return torch.zeros((capacity, DIM), dtype=torch.float16 if self.scan == "f16" else torch.uint8, device=self.device)

    def _grow(self, need):
        cap = self.capacity
        while cap < need:
            cap *= 2
        if cap != self.capacity:
            G = torch.zeros((cap, DIM), dtype=torch.float32, device=self.device)
            G[: self.capacity].copy_(self.G)
            if self.S is not None:                       # the coarse rows move with their slots: bytes, not a reconversion
                S = self._new_shadow(cap)
                S[: self.capacity].copy_(self.S)
                self.S = S
            self.G = G

    def upsert(self, ids, rows, normalise=False):
        """rows: float32 [n,512] (host or device).  Existing ids are overwritten in place (same slot), new
        ids take a slot.  ``normalise`` applies v/||v|| on the device (the manager normalises on the host with
        NumPy, bit-exactly as infrenceServer.py:271, and passes False)."""
        ids = list(ids)
        rows = torch.as_tensor(np.asarray(rows, np.float32) if not torch.is_tensor(rows) else rows)
        rows = rows.to(self.device, torch.float32).contiguous().reshape(-1, DIM)
        if len(ids) != rows.shape[0]:
            raise ValueError("ids and rows disagree")
        if not ids:
            return
        last = {i: k for k, i in enumerate(ids)}          # an id given twice: the last row wins, as dict assignment
        if len(last) != len(ids):
            keep = sorted(last.values())
            ids = [ids[k] for k in keep]
            rows = rows[torch.tensor(keep, device=self.device)]
        new = [i for i in ids if i not in self.slot_of]
        self._grow(self._next + max(len(new) - len(self._free), 0))
        for i in new:
            if self._free:
                self.slot_of[i] = self._free.pop()
            else:
                self.slot_of[i] = self._next
                self._next += 1
        if new:
            self.generation += 1
        slots = torch.tensor([self.slot_of[i] for i in ids], dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            if self.S is None:
                self.lib.fr_gallery_update_rows_f32(_lib.ptr(self.G), _lib.ptr(slots), _lib.ptr(rows), len(ids), DIM,
                                                    1 if normalise else 0, _lib.stream_ptr())
            else:                                        # f32 row + its coarse copy: one launch, one stream
                self.lib.fr_gallery_update_rows_shadow(_lib.ptr(self.G), _lib.ptr(self.S), _SHADOW_KIND[self.scan],
                                                       _lib.ptr(slots), _lib.ptr(rows), len(ids), DIM,
                                                       1 if normalise else 0, _lib.stream_ptr())
                if self.gmax is not None:                # the norms of the rows as stored, on the stream that wrote them
                    self.lib.fr_gallery_gmax_update(_lib.ptr(self.G), _lib.ptr(slots), len(ids), DIM, _lib.ptr(self.gmax),
                                                    _lib.stream_ptr())

    def remove(self, ids):
        n = 0
        for i in ids:
            s = self.slot_of.pop(i, None)
            if s is not None:
                self._free.append(s)
                n += 1
        if n:
            self.generation += 1
        return n

    def view(self, ids):
        """View over the given ids, in the given order (ids not in the gallery are skipped)."""
        return GalleryView(self, [i for i in ids if i in self.slot_of])

    def view_set(self, views):
        """The given views of THIS gallery, all of its current generation, as one ``GalleryViewSet``: a batch whose
        queries belong to different views is then matched in one grouped scan."""
        return GalleryViewSet(views, gallery=self)


def _check_current(obj, what="view"):
    """``obj``: a GalleryView or a GalleryViewSet (``what``: "set"), which is good for one generation of its gallery."""
    if obj.generation != obj.gallery.generation:
        raise StaleViewError(f"{type(obj).__name__} is stale: the gallery's membership changed after the {what} was made")


class GalleryView(_Rows):
    """Ordered subset of a ``DeviceGallery``: the rows one company's frames are matched against."""

    def __init__(self, gallery, ids):
        self.gallery, self.ids = gallery, list(ids)
        self.generation = gallery.generation
        self.lib, self.device = gallery.lib, gallery.device
        self.slots = torch.tensor([gallery.slot_of[i] for i in self.ids], dtype=torch.int64, device=self.device)

    def __len__(self):
        return len(self.ids)

    def rows(self):
        """The view's rows as a [N,512] device tensor (a copy; for tests / export)."""
        return self.gallery.G[self.slots]

    def row_source(self):
        """The rows a scan of this view reads (``RowSource``); a view whose gallery has moved on raises StaleViewError."""
        _check_current(self)
        g = self.gallery
        return RowSource(g.G, self.slots, len(self.ids), g.capacity, g.S, g.scan if g.S is not None else None, g.gmax)

    def match_device(self, Q, renormalise=True):
        """As ``GalleryMatcher.match_device``; idx is the position in ``self.ids`` (-1: empty view).  On a gallery built
        with scan="f16" / "f8": the coarse scan of the shadow slab through the slot list, re-ranked exactly in f32."""
        src = self.row_source()
        return _scan(self.lib, self.device, src, Q, None, renormalise, src.kind)

    def match_topk_device(self, Q, k, renormalise=True):
        """As ``GalleryMatcher.match_topk_device``; idx are positions in ``self.ids``.  The bits of the exact f32 scan
        over the f32 rows, whatever ``scan`` the gallery was built with: a view of at least
        ``gallery.coarse_topk_min_rows`` rows of a scan="f16" gallery gets them from the certified coarse pass through
        the slot list, every other view from the exact scan (``last_topk`` tells which)."""
        k = _check_k(k)
        src = self.row_source()
        return _scan(self.lib, self.device, src, Q, k, renormalise, _topk_kind(src, self.gallery.coarse_topk_min_rows))


GROUP = 32                     # queries per scan group (csrc/match_scan.h QG)


def build_group_tables(view_of, F, seg_len, offsets, lengths):
    """The host side of the grouped scan's tables (include/frhip.h, the grouped entries), a pure function.

    ``view_of``: the view index of every query slot (``seg_len`` == 0: F entries) or of every segment of ``seg_len``
    slots (F / seg_len entries); None or -1: no view - such slots are grouped under an empty view and report
    (-1, -1.0).  ``offsets`` / ``lengths``: where each view's slot list starts in the concatenated list, and its length.
    The slots of one view are packed, in slot order, into groups of at most 32; every slot lands in exactly one group
    and a group never mixes views.  Returns (gtab int64 [ngroups,2], qmap int32 [ngroups*32], max_view_len)."""
    F, seg_len = int(F), int(seg_len)
    vo = np.asarray([-1 if v is None else int(v) for v in view_of], np.int64).reshape(-1)
    if seg_len > 0:
        if F % seg_len or len(vo) * seg_len != F:
            raise ValueError(f"view_of needs one entry per segment: F {F} seg_len {seg_len} entries {len(vo)}")
        vo = np.repeat(vo, seg_len)
    elif len(vo) != F:
        raise ValueError(f"view_of needs one entry per query: F {F} entries {len(vo)}")
    if len(vo) and (vo.min() < -1 or vo.max() >= len(lengths)):
        raise ValueError(f"view_of names a view outside 0..{len(lengths) - 1}")
    gtab, qmap, longest = [], [], 0
    for v in np.unique(vo):
        slots = np.nonzero(vo == v)[0]
        off, n = (0, 0) if v < 0 else (int(offsets[v]), int(lengths[v]))
        for a in range(0, len(slots), GROUP):
            part = slots[a:a + GROUP]
            gtab.append((off, n))
            qmap.append(np.concatenate([part, np.full(GROUP - len(part), -1, np.int64)]))
        longest = max(longest, n)
    gtab = np.asarray(gtab, np.int64).reshape(-1, 2)
    qmap = (np.concatenate(qmap) if qmap else np.zeros(0, np.int64)).astype(np.int32)
    return gtab, qmap, longest


class GalleryViewSet(_Decides):
    """Several views of ONE ``DeviceGallery`` generation, matched together: each query of a batch through its own view,
    in one grouped scan - the frames of a camera batch that belong to different companies.  The concatenated slot
    lists are uploaded once, here.

    The grouped scan is the EXACT f32 scan over the f32 slab, also on a gallery built with scan="f16" / "f8" (there is
    no grouped coarse scan): the ids are those the coarse view scan promises - the f32 scan's - and the scores are
    the exact scan's bits; ``last_topk()`` reports "exact"."""

    _CACHE = 64                # (view_of, F, seg_len) table sets kept: a few hundred bytes each

    def __init__(self, views, gallery=None):
        views = list(views)
        if gallery is None:
            if not views:
                raise ValueError("GalleryViewSet needs a gallery or at least one view")
            gallery = views[0].gallery
        if any(v.gallery is not gallery for v in views):
            raise ValueError("the views of a GalleryViewSet must belong to one gallery")
        for v in views:
            _check_current(v)
        self.gallery, self.views, self.generation = gallery, views, gallery.generation
        self.lib, self.device = gallery.lib, gallery.device
        self.lengths = [len(v) for v in views]
        self.offsets = [int(x) for x in np.concatenate([[0], np.cumsum(self.lengths)])[:-1]]
        slots = [gallery.slot_of[i] for v in views for i in v.ids]
        self.slots = torch.tensor(slots + [0], dtype=torch.int64).to(self.device)     # never empty: a pointer to pass
        self._tables, self._tables_lock = {}, threading.Lock()     # one set serves the camera loop and request threads

    def __len__(self):
        return len(self.views)

    def tables(self, view_of, F, seg_len=0):
        """(gtab, qmap: device tensors, ngroups, max_view_len) for this assignment of views; built once per
        (view_of, F, seg_len) and kept - the last ``_CACHE`` assignments, oldest dropped first.  A miss builds the tables
        on the host and uploads the two small arrays (blocking copies); a hit costs a dict lookup.  A camera set whose
        cameras all deliver sends one assignment turn after turn; a turn in which some are late sends another, a subset
        of the same cameras - those settle in the cache too."""
        key = (tuple(-1 if v is None else int(v) for v in view_of), int(F), int(seg_len))
        with self._tables_lock:
            hit = self._tables.get(key)
            if hit is None:
                gtab, qmap, longest = build_group_tables(key[0], F, seg_len, self.offsets, self.lengths)
                while len(self._tables) >= self._CACHE:
                    self._tables.pop(next(iter(self._tables)))
                hit = self._tables[key] = (torch.from_numpy(gtab).to(self.device), torch.from_numpy(qmap).to(self.device),
                                           gtab.shape[0], longest)
        return hit

    def _scan(self, Q, view_of, k, renormalise, counts, seg_len):
        """The grouped pair called directly, not through ``_ENTRIES``: the tables are arguments no other scan has."""
        _check_current(self, "set")
        gtab, qmap, ngroups, longest = self.tables(view_of, Q.numel() // DIM, seg_len)
        lib, G, kk = self.lib, self.gallery.G, () if k is None else (k,)
        with torch.cuda.device(self.device):
            Q, F = _queries(lib, self.device, Q, renormalise, counts, seg_len)
            idx, score = _outputs(self.device, F, k)
            if F == 0:
                return idx, score
            wsz, entry = ((lib.fr_gallery_match_grouped_workspace, lib.fr_gallery_match_grouped_f32) if k is None else
                          (lib.fr_gallery_topk_grouped_workspace, lib.fr_gallery_topk_grouped_f32))
            ws = _workspace(self.device, wsz(ngroups, longest, *kk))
            entry(_lib.ptr(Q), _lib.ptr(G), _lib.ptr(self.slots), _lib.ptr(gtab), _lib.ptr(qmap), F, ngroups, longest,
                  G.shape[0], DIM, *kk, _lib.ptr(idx), _lib.ptr(score), _lib.ptr(ws), ws.numel(), _lib.ptr(counts), seg_len,
                  _lib.stream_ptr())
        return idx, score

    def match_device(self, Q, view_of, renormalise=True, counts=None, seg_len=0):
        """Q: float32 [F,512] device tensor; ``view_of``: a host sequence naming the view (index into ``self.views``;
        None: no view) of every query, or of every segment of ``seg_len`` slots when ``seg_len`` > 0 (frame -> company).
        Returns device tensors (idx int64[F], score float32[F]): for every query what ``views[v].match_device`` of an
        f32 gallery returns for it - idx is the position in ITS view's ``ids`` - bit for bit; (-1, -1.0) for an
        empty or missing view.  ``counts`` (device int32 [F / seg_len]) marks padding slots as in
        ``GalleryMatcher.match_device``.  One fr_l2norm_rows_f32 launch (``renormalise``) plus the grouped entry, and
        nothing is read back from ``counts``; no host synchronisation once the tables of this ``view_of`` are cached
        (``tables``: the first call with a new assignment uploads them).  Always the exact f32 scan (see the class)."""
        return self._scan(Q, view_of, None, renormalise, counts, seg_len)

    def match_topk_device(self, Q, view_of, k, renormalise=True, counts=None, seg_len=0):
        """The ``k`` best rows of every query in ITS view: (idx int64[F,k], score float32[F,k]), per query what
        ``views[v].match_topk_device`` returns, bit for bit; column 0 is ``match_device``.  Arguments as
        ``match_device``.  Always the exact f32 scan: ``last_topk()`` reports "exact"."""
        return self._scan(Q, view_of, _check_k(k), renormalise, counts, seg_len)
