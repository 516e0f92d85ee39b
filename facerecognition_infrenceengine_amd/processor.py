"""Application classes of the reference's inference script, kept name-for-name so it drops in:
``EmbeddingManager`` (/root/reference/infrenceServer.py:36-398), ``FaceRecognitionProcessor``
(:400-563) and the counting-path ``CameraProcessor`` (/root/reference/peopleCount.py:822-896).

Differences that are the point of this build:
* the gallery is a device-resident ``[N,512]`` matrix per company, rebuilt on sync, not a Python
  dict scanned per face (rows a-7/a-9 of SURVEY.md section 8);
* the store is INJECTED (the reference connects to a remote MongoDB at import,
  infrenceServer.py:682 / db/__init__.py:7-9 - SURVEY.md F5);
* row order is explicit and deterministic: employees in store order, then visitors
  (infrenceServer.py:264,288); ties go to the lowest row (the reference iterates a ``set``, so its
  own tie order is random: infrenceServer.py:357-373).
"""
import collections
import logging
import pickle
import threading
from datetime import datetime

import numpy as np

logger = logging.getLogger(__name__)


class _Unchanged:
    """The type of ``UNCHANGED``: one instance, compared by identity."""
    __slots__ = ()

    def __repr__(self):
        return "UNCHANGED"

    def __reduce__(self):
        return "UNCHANGED"


# What ``recognize_batch`` / ``identify_batch`` return for a frame their ``gate`` judged inactive: the scene is what the last
# processed frame of that camera showed, and the engine did not run for it.  Never None (no gallery) and never [] (no face).
UNCHANGED = _Unchanged()


def _check_gate(gate, camera_ids, n, tracks=None, quality=None):
    """The argument rule of ``recognize_batch`` / ``identify_batch``: the camera ids of a gated or tracked call as a list (None
    without gate and tracks: one list serves both), and no ``quality`` beside ``tracks``; ValueError before anything runs."""
    if gate is None and tracks is None:
        if camera_ids is not None:
            raise ValueError("camera_ids come with a gate (gate=ActivityGate(...)) or with tracks (tracks=FaceTracks(...))")
        return None
    if camera_ids is None:
        raise ValueError(("a gate needs" if gate is not None else "tracks need") + " camera_ids: one camera id per frame")
    ids = list(camera_ids)
    if len(ids) != n:
        raise ValueError(f"one camera id per frame: {n} frames, {len(ids)} ids")
    if len(set(ids)) != len(ids):
        raise ValueError("a camera id is repeated in one call")
    if quality is not None and tracks is not None:
        raise ValueError("quality together with tracks is not supported yet")
    return ids


def _scan_rows(r):
    """The rows of the slot results that the gallery is asked with: the tracks' ``query`` (templates) when the
    call's tracks fuse, else ``normed_embedding``."""
    return r["query"] if "query" in r else r["normed_embedding"]


class _SlotFaces:
    """The host side of one batch: every device-to-host copy the tails of ``recognize_batch`` / ``identify_batch`` make of the
    slot results ``r`` (``n`` frames) and of their scan ``idx`` / ``score`` with its decision ``dec`` (None: a top-K scan, the
    ``identify`` dicts), the counts first - the one synchronisation -, and the dict of each face.  ``track_id`` / ``carried``,
    ``template_shots`` and the quality columns (``track_action`` beside them when the tracks judge) are None for a call without;
    the joins and restarts of the tracks' event column are added to ``tracks.stats`` from the same read-back."""

    def __init__(self, r, n, idx, score, tracks, dec=None):
        shape = (n, r["bbox"].shape[1]) + (() if dec is not None else (-1,))
        self.counts = r["counts"].cpu().numpy()                              # the one synchronisation
        self.idx, self.score = idx.cpu().numpy().reshape(shape), score.cpu().numpy().reshape(shape)
        self.dec = dec.cpu().numpy().reshape(shape) if dec is not None else None
        self.bbox = r["bbox"].cpu().numpy().astype(int)                      # :531 truncation
        self.det_score = r["det_score"].cpu().numpy()
        self.tid = self.carried = self.shots = self.action = self.quality = None
        if "track_id" in r:
            self.tid, self.carried = r["track_id"].cpu().numpy(), r["carried"].cpu().numpy()
        if "template_shots" in r:
            tracks.count_events(r["template_event"].cpu().numpy())
            self.shots = r["template_shots"].cpu().numpy()
        if "quality" in r:
            if "track_action" in r:
                self.action = r["track_action"].cpu().numpy()
            self.quality = tuple(r[key].cpu().numpy() for key in ("quality", "quality_f", "quality_verdict"))

    def fit(self, f, j):
        """True for a call without quality and for a face judged fit; under judging tracks for every face but a rejected one - a
        carried face answers with its track's held fit row whatever this frame's verdict"""
        if self.quality is None:
            return True
        return self.quality[2][f, j] == 0 if self.action is None else self.action[f, j] != 3

    def face(self, f, j, ids, metadata, min_score=None):
        """The dict of face ``j`` of frame ``f`` through the gallery (``ids``, ``metadata``) of its frame: a face that is not fit
        is the Unknown dict / has no candidates.  With tracks it gains ``track_id`` (-1: untracked), ``tracked`` (True: its
        embedding was carried) and, when they fuse, ``template_shots`` (the shots behind the row it was scanned with, 0: its own
        row); with quality, ``quality`` (``FaceQuality.describe``) and ``quality_ok``: this frame's verdict."""
        at = (self.bbox[f, j], self.det_score[f, j])
        if self.dec is not None:
            face = _face_result(*at, self.dec[f, j] if self.fit(f, j) else 0, self.idx[f, j], self.score[f, j], ids, metadata)
        else:
            face = _face_candidates(*at, self.idx[f, j] if self.fit(f, j) else (), self.score[f, j], ids, metadata, min_score)
        if self.tid is not None:
            face["track_id"], face["tracked"] = int(self.tid[f, j]), bool(self.carried[f, j])
        if self.shots is not None:
            face["template_shots"] = int(self.shots[f, j])
        if self.quality is not None:
            from .quality import FaceQuality
            face["quality"] = FaceQuality.describe(*(c[f, j] for c in self.quality))
            face["quality_ok"] = face["quality"]["ok"]
        return face

    def frames(self, galleries, keep, total, min_score=None):
        """What a batch call returns: per frame the list of its faces' dicts through ``galleries[f]`` = (ids, metadata), None for
        a frame without a gallery; with ``keep`` (the active frames of a gated call) spread over ``total`` frames."""
        out = [None if g is None else [self.face(f, j, *g, min_score) for j in range(int(self.counts[f]))]
               for f, g in enumerate(galleries)]
        return _spread(out, keep, total)


# What ``_scan_mixed`` returns (there: what each field holds)
_Scan = collections.namedtuple("_Scan", "n r keep view_set galleries idx score")


def _spread(out, keep, n):
    """Results of the active frames ``keep`` back at their places among ``n`` frames; UNCHANGED for the others."""
    if keep is None:
        return out
    full = [UNCHANGED] * n
    for j, f in enumerate(keep):
        full[f] = out[j]
    return full


class InMemoryStore:
    """Store protocol used by EmbeddingManager (what the Mongo collections + GridFS buckets of
    /root/reference/db/__init__.py:11-26 provide).  Documents use the reference's field names."""

    def __init__(self):
        self.employees, self.visitors = [], []          # documents, insertion order = cursor order
        self.employee_blobs, self.visitor_blobs = {}, {}

    def add_employee(self, _id, company_id, embedding, name="Unknown", status="active", blacklisted=False, **extra):
        self.employee_blobs[_id] = pickle.dumps(np.asarray(embedding, np.float32))
        doc = {"_id": _id, "companyId": company_id, "status": status, "blacklisted": blacklisted,
               "employeeName": name, "lastUpdated": datetime.utcnow(),
               "employeeEmbeddings": {"buffalo_l": {"embeddingId": _id, "status": "done"}}}
        doc.update(extra)
        self.employees.append(doc)
        return doc

    def add_visitor(self, _id, company_id, embedding, name="Unknown", status="done", **extra):
        self.visitor_blobs[_id] = pickle.dumps(np.asarray(embedding, np.float32))
        doc = {"_id": _id, "companyId": company_id, "visitorName": name, "lastUpdated": datetime.utcnow(),
               "visitorEmbeddings": {"buffalo_l": {"embeddingId": _id, "status": status}}}
        doc.update(extra)
        self.visitors.append(doc)
        return doc

    # ---- protocol
    def find_employees(self, since=None):
        """status == done embeddings of active, non-blacklisted employees (infrenceServer.py:66-73,215-219)."""
        return [d for d in self.employees
                if d.get("employeeEmbeddings", {}).get("buffalo_l", {}).get("status") == "done"
                and d.get("status") == "active" and not d.get("blacklisted")
                and (since is None or d["lastUpdated"] > since)]

    def find_visitors(self, since=None):
        return [d for d in self.visitors
                if d.get("visitorEmbeddings", {}).get("buffalo_l", {}).get("status") == "done"
                and (since is None or d["lastUpdated"] > since)]

    def find_inactive_employee_ids(self):
        """infrenceServer.py:236-242."""
        return [str(d["_id"]) for d in self.employees if d.get("status") != "active" or d.get("blacklisted")]

    def read_employee_embedding(self, embedding_id):
        return self.employee_blobs[embedding_id]

    def read_visitor_embedding(self, embedding_id):
        return self.visitor_blobs[embedding_id]

    def company_member_ids(self, company_id):
        """(active non-blacklisted employee ids, visitor ids) of a company, store order
        (infrenceServer.py:351-367)."""
        emp = [str(d["_id"]) for d in self.employees
               if d["companyId"] == company_id and d.get("status") == "active" and not d.get("blacklisted")]
        vis = [str(d["_id"]) for d in self.visitors if d["companyId"] == company_id]
        return emp, vis


class EmbeddingManager:
    """Same public surface as infrenceServer.py:36-398; ``store`` replaces the Mongo connection."""

    def __init__(self, mongodb_uri=None, database_name=None, store=None, device="cuda:0", sync_interval=30, scan="f32"):
        """``scan``: how the views of the device gallery match - "f32" (default, the exact f32 scan), or "f16" / "f8" for
        a large gallery: the one-pass coarse scan with the exact f32 re-rank (``DeviceGallery``), same ids."""
        if store is None:
            raise ValueError("EmbeddingManager needs store=<store object> (the reference's module-level MongoDB "
                             "connection is not reproduced; see INTEGRATION.md for a pymongo adapter)")
        if scan not in ("f32", "f16", "f8"):
            raise ValueError("scan must be 'f32', 'f16' or 'f8'")
        self.store, self.device, self.scan = store, device, scan
        self.embeddings = {}                 # id -> unit float32[512]; dict order = row order
        self.employee_metadata = {}
        self.embeddings_lock = threading.Lock()
        self.last_sync_time = None
        self.is_initial_load = True
        self.sync_interval = sync_interval
        self.sync_thread, self.running = None, False
        self._gallery = None                 # DeviceGallery: one slab of rows in HBM, updated in place
        self._dirty, self._gone = {}, set()  # ids changed / removed since the slab was last brought up to date
        self._matchers = {}                  # company id -> (GalleryView, metadata), rebuilt after a sync
        self._initial_load()

    # ---- ingest (infrenceServer.py:260-341): unpickle, divide by the norm
    def _ingest(self, docs, kind):
        for d in docs:
            try:
                _id = str(d["_id"])
                entry = d[f"{kind}Embeddings"]["buffalo_l"]
                read = self.store.read_employee_embedding if kind == "employee" else self.store.read_visitor_embedding
                embedding = pickle.loads(read(entry["embeddingId"]))
                self.embeddings[_id] = embedding / np.linalg.norm(embedding)
                self._dirty[_id] = None
                self._gone.discard(_id)
                if kind == "employee":
                    self.employee_metadata[_id] = {
                        "name": d.get("employeeName", "Unknown"), "employeeId": d.get("employeeId", "Unknown"),
                        "email": d.get("employeeEmail", ""), "mobile": d.get("employeeMobile", ""),
                        "type": "employee", "lastUpdated": d.get("lastUpdated", datetime.utcnow())}
                else:
                    self.employee_metadata[_id] = {"name": d.get("visitorName", "Unknown"), "type": "visitor",
                                                   "lastUpdated": d.get("lastUpdated", datetime.utcnow())}
            except Exception as e:          # the reference logs and continues (infrenceServer.py:285-286)
                logger.error("error loading %s embedding for %s: %s", kind, d.get("_id"), e)

    def _load_updated_embeddings(self, employees, visitors):
        with self.embeddings_lock:
            self._ingest(employees, "employee")
            self._ingest(visitors, "visitor")
            self._matchers.clear()

    def _initial_load(self):
        self._load_updated_embeddings(self.store.find_employees(), self.store.find_visitors())
        self.last_sync_time = datetime.utcnow()
        self.is_initial_load = False

    def _remove_inactive_embeddings(self):
        with self.embeddings_lock:
            for _id in self.store.find_inactive_employee_ids():
                if _id in self.embeddings:
                    del self.embeddings[_id]
                    self.employee_metadata.pop(_id, None)
                    self._dirty.pop(_id, None)
                    self._gone.add(_id)
            self._matchers.clear()

    def _sync_embeddings(self):
        """infrenceServer.py:185-232: incremental, keyed on lastUpdated."""
        since = self.last_sync_time
        now = datetime.utcnow()
        self._load_updated_embeddings(self.store.find_employees(since), self.store.find_visitors(since))
        self._remove_inactive_embeddings()
        self.last_sync_time = now

    def force_sync(self):
        self._sync_embeddings()

    def start_sync(self):
        if self.sync_thread is None or not self.sync_thread.is_alive():
            self.running = True
            self._stop = threading.Event()
            self.sync_thread = threading.Thread(target=self._sync_loop, daemon=True)
            self.sync_thread.start()

    def stop_sync(self):
        self.running = False
        if self.sync_thread:
            self._stop.set()
            self.sync_thread.join(timeout=5)

    def _sync_loop(self):
        while self.running and not self._stop.wait(self.sync_interval):
            try:
                self._sync_embeddings()
            except Exception as e:
                logger.error("error in sync loop: %s", e)

    # ---- views
    def _company_rows(self, company_id):
        emp, vis = self.store.company_member_ids(company_id)
        seen = set(emp)
        ids = [i for i in emp if i in self.embeddings] + [i for i in vis if i in self.embeddings and i not in seen]
        return ids

    def get_embeddings_for_company(self, company_id):
        """(dict id -> float32[512], dict id -> metadata), as infrenceServer.py:343-380."""
        with self.embeddings_lock:
            ids = self._company_rows(company_id)
            return ({i: self.embeddings[i] for i in ids}, {i: self.employee_metadata[i] for i in ids})

    def get_all(self):
        """peopleCount.py:816-819."""
        with self.embeddings_lock:
            return dict(self.embeddings), dict(self.employee_metadata)

    def _flush_to_device(self):
        """Bring the device slab up to date: only rows that changed since the last flush travel (in-place row
        writes); removed people free their slots.  Called under the lock."""
        from .gallery import DeviceGallery
        if self._gallery is None:
            coarse = {} if self.scan == "f32" else {"scan": self.scan}        # "f32": the call as it always was
            self._gallery = DeviceGallery(self.device, capacity=max(1024, 2 * len(self.embeddings)), **coarse)
        if self._gone:
            self._gallery.remove(self._gone)
            self._gone = set()
        if self._dirty:
            ids = list(self._dirty)
            self._gallery.upsert(ids, np.stack([self.embeddings[i] for i in ids]), normalise=False)  # unit at ingest
            self._dirty = {}

    def get_matcher_for_company(self, company_id):
        """(view, metadata): the company's rows as an ordered view of the device-resident slab.  The membership
        queries the reference issues per frame (infrenceServer.py:351-367) run once per sync; rows are never
        copied per company, and a sync rewrites only the rows whose documents changed."""
        with self.embeddings_lock:
            self._flush_to_device()
            return self._matcher_locked(company_id)

    def _matcher_locked(self, company_id):
        """The cached (view, metadata) of one company, rebuilt when the slab's membership moved on.  Under the lock,
        after ``_flush_to_device``."""
        hit = self._matchers.get(company_id)
        if hit is None or hit[0].generation != self._gallery.generation:
            ids = self._company_rows(company_id) if company_id is not None else list(self.embeddings)
            hit = (self._gallery.view(ids), {i: self.employee_metadata[i] for i in ids})
            self._matchers[company_id] = hit
        return hit

    def get_matchers_for_companies(self, company_ids):
        """(view_set, metadatas, index_of) for a batch whose entries belong to the given companies (one id per entry):
        the views of the DISTINCT companies that have rows, each once, as one ``GalleryViewSet`` over one generation of
        the slab (one lock, one flush); ``metadatas[v]`` goes with ``view_set.views[v]``, and ``index_of[i]`` names the
        view of ``company_ids[i]`` - None where that company has no rows.  Views and sets come from the cache
        ``get_matcher_for_company`` fills (a set per mix of companies, the last 16; a new mix uploads its slot lists)."""
        with self.embeddings_lock:
            self._flush_to_device()
            where, names, views, metadatas = {}, [], [], []
            for c in company_ids:
                if c not in where:
                    view, metadata = self._matcher_locked(c)
                    where[c] = len(views) if len(view) else None
                    if len(view):
                        names.append(c); views.append(view); metadatas.append(metadata)
            key = ("view_set",) + tuple(names)
            hit = self._matchers.get(key)
            if hit is None or hit[0].generation != self._gallery.generation or \
                    any(a is not b for a, b in zip(hit[0].views, views)):
                sets = [k for k in self._matchers if isinstance(k, tuple)]
                for k in sets[:max(len(sets) - 15, 0)]:          # the company mix of a turn varies with the cameras
                    del self._matchers[k]                        # that deliver: keep the last 16 mixes
                hit = self._matchers[key] = (self._gallery.view_set(views), metadatas)
            return hit[0], hit[1], [where[c] for c in company_ids]

    def find_duplicates(self, company_id=None, thr=0.4):
        """The gallery audit: every pair of rows of the company's view (``None``: the whole gallery, as ``get_all``) the
        enrolment duplicate check would refuse - dot > ``thr`` on the rows as stored (``GalleryView.find_duplicates``).  The
        reference checks a new employee against employees and a new visitor against visitors only
        (trainingServer.py:170-200); a company's view is employees then visitors, so the pair it never checks is found
        here.  One lock and one flush; the company's cached view.  Returns [{"a", "b", "score", "a_type", "b_type", "a_name",
        "b_name"}], ordered by the rows' positions in the view."""
        (view, metadata), found = _with_current(lambda: self.get_matcher_for_company(company_id),
                                                lambda view, metadata: view.find_duplicates(thr=thr))
        return [{"a": a, "b": b, "score": float(s), "a_type": metadata[a]["type"], "b_type": metadata[b]["type"],
                 "a_name": metadata[a]["name"], "b_name": metadata[b]["name"]}
                for (a, b), s in zip(found.ids, found.scores)]

    def get_stats(self):
        """infrenceServer.py:386-398."""
        with self.embeddings_lock:
            employees = sum(1 for m in self.employee_metadata.values() if m["type"] == "employee")
            visitors = sum(1 for m in self.employee_metadata.values() if m["type"] == "visitor")
            return {"total_embeddings": len(self.embeddings), "employees": employees, "visitors": visitors,
                    "last_sync": self.last_sync_time.isoformat() if self.last_sync_time else None,
                    "initial_load_complete": not self.is_initial_load}


class FaceRecognitionProcessor:
    """infrenceServer.py:400-563."""

    def __init__(self, embedding_manager, face_detector=None):
        self.embedding_manager = embedding_manager
        self.face_detector = face_detector
        self.detection_threshold = 0.3        # set but never read in the reference (:406)
        self.recognition_threshold = 0.4

    def initialize_detector(self):
        if self.face_detector is None:
            from .face_analysis import FaceAnalysis
            self.face_detector = FaceAnalysis(name="buffalo_l",
                                              providers=["CUDAExecutionProvider", "CPUExecutionProvider"])
            self.face_detector.prepare(ctx_id=0)

    def _scan_frame(self, frame, company_id, k=None):
        """The prelude ``recognize`` and ``identify`` share: None when the company has no gallery, else the frame's faces
        (``detect_embed_device``), then the matcher and metadata its rows went through and the scan's idx / score (top-``k``)."""
        if self.face_detector is None:
            self.initialize_detector()
        matcher, metadata = self.embedding_manager.get_matcher_for_company(company_id)
        if len(matcher) == 0:
            logger.warning("No embeddings found for company %s", company_id)
            return None
        r = _detect_embed(self.face_detector, frame)
        return (r,) + _match_fresh(self.embedding_manager, company_id, matcher, metadata, r["normed_embedding"],
                                   k)                                        # renormalise + scan (:532-542)

    def recognize(self, frame, company_id):
        """Structured form: list of dicts {bbox int[4], person_info, det_score, recognition_score, person_id}."""
        got = self._scan_frame(frame, company_id)
        if got is None:
            return None
        r, matcher, metadata, idx, score = got
        dec = matcher.decide_device(idx, score, self.recognition_threshold)  # :545
        idx, score, dec = idx.cpu().numpy(), score.cpu().numpy(), dec.cpu().numpy()
        bbox = r["bbox"].cpu().numpy().astype(int)                           # :531 truncation
        det = r["det_score"].cpu().numpy()
        return [_face_result(bbox[f], det[f], dec[f], idx[f], score[f], matcher.ids, metadata) for f in range(len(idx))]

    def identify(self, frame, company_id, k=5, min_score=None):
        """Ranked candidate list per face (1 <= k <= 16): a list of dicts {bbox int[4], det_score, candidates}, where
        ``candidates`` is a list of {person_id, person_info, score} in rank order (score descending, gallery row order
        on exact ties), at most k long: empty slots and slots scoring below ``min_score`` are left out.
        ``candidates[0]`` is the row ``recognize`` matches, with the same score bits.  None when the company has no
        gallery, as ``recognize``."""
        if not 1 <= int(k) <= 16:
            raise ValueError(f"k must be 1..16 (got {k})")
        got = self._scan_frame(frame, company_id, int(k))
        if got is None:
            return None
        r, matcher, metadata, idx, score = got
        idx, score = idx.cpu().numpy(), score.cpu().numpy()
        bbox = r["bbox"].cpu().numpy().astype(int)
        det = r["det_score"].cpu().numpy()
        return [_face_candidates(bbox[f], det[f], idx[f], score[f], matcher.ids, metadata, min_score) for f in range(len(idx))]

    @property
    def accepts_mixed_sizes(self):
        """True when ``recognize_batch`` takes frames of differing sizes in one call: the engine has a detection canvas
        (``FaceAnalysis.prepare(det_size=...)``).  The camera batcher then stops grouping frames by shape."""
        if self.face_detector is None:
            self.initialize_detector()
        return getattr(self.face_detector, "det_size", None) is not None

    def _scan_mixed(self, frames, company_ids, k=None, pixel_format="bgr", matrix="bt601", gate=None, camera_ids=None,
                    tracks=None, quality=None, hold=None):
        """One engine pass over ``frames`` and ONE grouped scan in which frame i is matched through the view of
        ``company_ids[i]`` (top-1, or top-``k``), padding slots marked by the device face counts.  Returns None when
        no company has a gallery (nothing is run, a gate is not consulted), else a ``_Scan``: n, the slot results r, keep, the
        view_set, per frame its gallery (ids, metadata) - None without one -, idx, score; device tensors, no synchronisation
        beyond the engine's own.  With a ``gate``, ``keep`` lists the active frames and everything else describes exactly those
        n = len(keep) frames, in order (``keep`` None: all frames, the ungated call's tensors); with none active the slot
        results are None, and galleries / idx / score are None when no active frame's company has a gallery."""
        company_ids = list(company_ids)
        if len(company_ids) != len(frames):
            raise ValueError(f"one company id per frame: {len(frames)} frames, {len(company_ids)} ids")
        if self.face_detector is None:
            self.initialize_detector()
        mgr = self.embedding_manager
        view_set, metadatas, index_of = mgr.get_matchers_for_companies(company_ids)
        for c in sorted({str(c) for c, v in zip(company_ids, index_of) if v is None}):
            logger.warning("No embeddings found for company %s", c)
        if all(v is None for v in index_of):
            return None
        n, r, keep = _detect_embed_batch_gated(self, self.face_detector, frames, pixel_format, matrix, gate, camera_ids, tracks,
                                               quality, hold)
        if keep is not None:                      # the views of the active frames' companies, as a call on those frames has them
            company_ids = [company_ids[f] for f in keep]
            if r is not None:
                view_set, metadatas, index_of = mgr.get_matchers_for_companies(company_ids)
            if r is None or all(v is None for v in index_of):
                return _Scan(n, r, keep, view_set, None, None, None)
        cap = r["bbox"].shape[1]

        def scan(vs, _, of):
            if k is None:
                return vs.match_device(_scan_rows(r), of, counts=r["counts"], seg_len=cap)
            return vs.match_topk_device(_scan_rows(r), of, k, counts=r["counts"], seg_len=cap)
        (view_set, metadatas, index_of), (idx, score) = _with_current(
            lambda: mgr.get_matchers_for_companies(company_ids), scan, (view_set, metadatas, index_of))
        galleries = [None if v is None else (view_set.views[v].ids, metadatas[v]) for v in index_of]
        return _Scan(n, r, keep, view_set, galleries, idx, score)

    def _serve_mixed(self, frames, company_ids, k, min_score, pixel_format, matrix, gate, camera_ids, tracks, quality, hold=None):
        """``recognize_batch`` with one company id per frame (``k`` None) and ``identify_batch`` (top-``k``): the grouped scan,
        the decision launch of the former, the shared read-back.  ``hold``: as ``_detect_embed_batch_gated``."""
        got = self._scan_mixed(frames, company_ids, k, pixel_format, matrix, gate, camera_ids, tracks, quality, hold)
        if got is None:
            return [None] * len(frames)
        if got.idx is None:                       # no frame active, or none of the active ones has a gallery
            return _spread([None] * got.n, got.keep, len(frames))
        dec = got.view_set.decide_device(got.idx, got.score, self.recognition_threshold) if k is None else None
        return _SlotFaces(got.r, got.n, got.idx, got.score, tracks, dec).frames(got.galleries, got.keep, len(frames), min_score)

    def identify_batch(self, frames, company_id, k=5, min_score=None, pixel_format="bgr", matrix="bt601", gate=None,
                       camera_ids=None, tracks=None, quality=None, chips=None):
        """``identify`` for a batch of frames (sizes as ``recognize_batch``): ``company_id`` is one id for all frames or a
        list / tuple with one id per frame.  ONE engine pass, one grouped top-K scan in which every frame is ranked
        through its own company's view, one host synchronisation.  Returns a list with, per frame, what ``identify``
        returns for it - None for a frame whose company has no gallery.  The grouped scan is the exact f32 scan
        whatever ``scan`` the manager was built with: the bits of ``identify``'s exact path.  ``pixel_format`` / ``matrix``,
        ``gate`` / ``tracks`` / ``camera_ids`` / ``quality``: as ``recognize_batch``; a face judged unfit has no candidates - under tracks that
        judge, a REJECTED face has none and a carried one is ranked on its held row.  ``chips``: as ``recognize_batch`` (a face
        dict here has no ``person_info``: to a ``who`` given as types every face counts as unknown)."""
        if not 1 <= int(k) <= 16:
            raise ValueError(f"k must be 1..16 (got {k})")
        camera_ids = _check_gate(gate, camera_ids, len(frames), tracks, quality)
        ids = list(company_id) if isinstance(company_id, (list, tuple)) else [company_id] * len(frames)
        if chips is None:
            return self._serve_mixed(frames, ids, int(k), min_score, pixel_format, matrix, gate, camera_ids, tracks, quality)
        return self._with_chips(chips, lambda hold: self._serve_mixed(frames, ids, int(k), min_score, pixel_format, matrix, gate,
                                                                      camera_ids, tracks, quality, hold))

    def recognize_batch(self, frames, company_id, pixel_format="bgr", matrix="bt601", gate=None, camera_ids=None, tracks=None,
                        quality=None, chips=None):
        """Batch form for the camera batcher (``camera.CameraManager``): ``frames`` = list of BGR uint8 frames (one per
        camera), of one size - or of any sizes when the engine has a ``det_size`` (``accepts_mixed_sizes``; ``bbox`` is
        in each frame's own pixels either way).  ONE pass of the sync-free slot pipeline over the whole batch (pinned staging ->
        copy stream -> detect -> align -> embed -> company view scan -> decision), one host synchronisation at the
        end.  Returns a list (per frame) of lists of the dicts ``recognize`` returns, or None when the company has
        no gallery (the reference returns the frame untouched then, infrenceServer.py:523-525).

        ``company_id`` may also be a list or tuple with one id per frame - cameras of several companies in one batch
        (the reference runs one process per camera, each with its own company: infrenceServer.py:603-646).  Still ONE
        engine pass, then one grouped scan in which every frame is matched through its own company's view, one
        decision launch and the one synchronisation.  The result is then always a list: None stands in for the frames
        whose company has no gallery, the other frames are served.  The grouped scan is the exact f32 scan, also when
        the manager was built with scan="f16" / "f8": the same ids, the exact scan's score bits.

        ``pixel_format="nv12"`` / ``"i420"``: the frames are YUV 4:2:0 as a video decoder produces them (``uint8 [H*3/2, W]``, H
        and W even) with colour ``matrix`` ``"bt601"`` / ``"bt709"`` / ``"jpeg"`` (colour.py).  They cross the link at half of
        BGR's bytes and are converted on the device behind the copy; the results are those of the converted BGR frames.
        ``annotate`` draws on BGR host frames and does not take YUV.

        ``pixel_format="jpeg"``: one ``bytes`` per frame, a JPEG file each.  The files go into the pinned ring as they are and are
        decoded on the device behind the copy; a file the device decoder does not take is decoded by
        ``ingest.decode_image`` on the host, a blob that does not decode at all is a black frame - no faces.  The results are those
        of the decoded BGR frames, bit for bit.

        ``gate`` (an ``activity.ActivityGate``) with ``camera_ids`` (one hashable id per frame, none repeated): the frames go
        through the same ring, the gate judges the ring's device frames (one small device-to-host copy and one
        synchronisation more), and the engine pass, the scan and the decision run on the ACTIVE frames only - a device
        gather of those frames (the selected rows of the frame table under ``det_size``: no frame bytes move), or the ring's
        tensors as they are when every frame is active.  An inactive frame's entry is ``UNCHANGED``; the entries of the
        active frames are what this call returns, without a gate, for exactly those frames with their company ids, in
        order.  They are not the full batch's bits: the embed net's small-batch modes sum in another order, and a gated
        turn embeds fewer faces.  With no frame active nothing but the upload and the gate runs.  When the company has no
        gallery the None of the ungated call comes first: the gate is not consulted and its state does not move.

        ``tracks`` (a ``tracks.FaceTracks``) with the same ``camera_ids``: a face that the camera's previous frame showed at
        nearly the same place, alone, keeps the embedding it was given then for up to ``max_reuse`` turns and skips align and
        the embed net; the held embedding goes through THIS call's scan and decision, so the identity is never cached.  Each
        face dict gains ``"track_id"`` (int, -1: untracked) and ``"tracked"`` (True: carried).  With a gate too, a frame
        answered ``UNCHANGED`` never reaches the tracks and its camera's track state does not move; nor does it when the
        company has no gallery.

        ``quality`` (a ``quality.FaceQuality``): behind align one launch judges every aligned face (sharpness, exposure,
        contrast, size, pose: DESIGN.md 4.5e) and the embed net runs for the fit ones only.  Every face dict gains ``"quality"``
        (the dict of ``FaceQuality.describe``) and ``"quality_ok"``; a rejected face is reported as the Unknown dict whatever the
        scan made of its placeholder row.  Not together with ``tracks`` (ValueError): the two combine through the tracks object.

        ``tracks=FaceTracks(..., quality=q, max_age=8)`` with ``quality=None``: tracks that judge.  The bank
        holds a track's last FIT embedding; an unfit face is never embedded, and where its track holds such a row (not older
        than ``max_age`` turns, no other track touching the face, no re-embed due) it is carried on it through this call's scan.
        Each face dict has ``"track_id"``, ``"tracked"``, ``"quality"`` (this frame's measurement) and ``"quality_ok"`` (this
        frame's verdict); a face is the Unknown dict only when it was rejected: unfit and without a row to carry.

        ``tracks=FaceTracks(..., template=K)``, plain or judging: tracks that fuse.  A tracked face is scanned
        with its track's template - the unit mean of the track's last K embedded shots that agreed with one another - instead
        of this frame's row alone; a shot that does not agree with the template restarts it and is scanned as it is.  Each face
        dict gains ``"template_shots"`` (the shots behind the scanned row, 0: the face's own row), and ``tracks.stats`` counts
        ``"joined"`` and ``"restarted"`` shots.  The same holds for ``identify_batch`` and for mixed-company batches.

        ``chips`` (a ``chips.FaceChips``): the call keeps its ring turn, and once the results are on the host one launch cuts a
        square around every face the object selects out of the ring's FULL-SIZE device frames - BGR as uploaded, converted from
        YUV or decoded from JPEG - and resamples it to a thumbnail; every face dict gains ``"chip"``: JPEG
        ``bytes`` encoded on the device, a ``uint8 [S,S,3]`` array with ``encode=None``, None for a face that is not selected.
        Every other key is what the call returns without chips.  A frame answered ``UNCHANGED`` or None yields no chips.  Calls
        with chips are serialised per processor, with the calls that draw a HUD; while one holds its turn, no more than one
        further batch of the same shape should be started on this processor from other threads (the ring is two slots deep).
        None: the call runs the code it ran before."""
        if chips is None:
            return self._recognize_batch(frames, company_id, pixel_format, matrix, gate, camera_ids, tracks, quality)
        return self._with_chips(chips, lambda hold: self._recognize_batch(frames, company_id, pixel_format, matrix, gate,
                                                                          camera_ids, tracks, quality, hold))

    def _with_chips(self, chips, call):
        """``call(hold)`` - an engine pass that leaves its ring turn in ``hold`` - and, behind it, the chips of its results cut
        from the ring's device frames; the turn is released when the chips have been read back."""
        import torch
        lock = self.__dict__.setdefault("_hud_lock", threading.Lock())
        hold = []
        with lock:
            try:
                results = call(hold)
                if hold and isinstance(results, list):
                    turn, det = hold[0], self.face_detector
                    with torch.cuda.device(det.device):
                        torch.cuda.current_stream(det.device).wait_event(turn.ready)
                        chips.cut(turn.dev if turn.table is None else (turn.dev, turn.table), results, n=len(turn.arr))
            finally:
                for t in hold:
                    t.ring.release(t.turn)
        return results

    def _recognize_batch(self, frames, company_id, pixel_format="bgr", matrix="bt601", gate=None, camera_ids=None, tracks=None,
                         quality=None, hold=None):
        """``recognize_batch``; with ``hold`` (a list) the ring turn the call took is left to the caller to release
        (``_detect_embed_batch_gated``): ``recognize_faces_batch`` draws on the ring's device frames first."""
        camera_ids = _check_gate(gate, camera_ids, len(frames), tracks, quality)
        if isinstance(company_id, (list, tuple)):
            return self._serve_mixed(frames, company_id, None, None, pixel_format, matrix, gate, camera_ids, tracks, quality, hold)
        if self.face_detector is None:
            self.initialize_detector()
        matcher, metadata = self.embedding_manager.get_matcher_for_company(company_id)
        if len(matcher) == 0:
            logger.warning("No embeddings found for company %s", company_id)
            return None
        n, r, keep = _detect_embed_batch_gated(self, self.face_detector, frames, pixel_format, matrix, gate, camera_ids, tracks,
                                               quality, hold)
        if r is None:                                                        # no frame active
            return [UNCHANGED] * len(frames)
        matcher, metadata, idx, score = _match_fresh(self.embedding_manager, company_id, matcher, metadata, _scan_rows(r))
        dec = matcher.decide_device(idx, score, self.recognition_threshold)
        return _SlotFaces(r, n, idx, score, tracks, dec).frames([(matcher.ids, metadata)] * n, keep, len(frames))

    def recognize_faces_batch(self, frames, company_id, hud, return_results=False, held=None, encode=None, redact=None,
                              redact_keys=None, chips=None, **kw):
        """The reference's ``recognize_faces`` for a batch, with the HUD drawn on the DEVICE (``hud``: a ``hud.Hud``): runs
        exactly what ``recognize_batch(frames, company_id, **kw)`` runs (``kw``: ``pixel_format``, ``matrix``, ``gate``,
        ``camera_ids``, ``tracks``, ``quality``), then draws every frame's results into the ring's device frames - the BGR frames
        the ring uploaded or converted from YUV, so a YUV call has a picture too - while it still holds the ring turn, queues the
        device-to-host copy of the drawn frames and only then releases the turn.  Returns one annotated BGR ``uint8`` array per
        frame, the caller's to keep: the frame's own size, or ``hud.out_size`` previews (``[h, w, 3]``: the frame resized to
        fit, top-left, zero padded) - then only the previews cross the link.  ``return_results=True``: ``(frames, results)``
        with ``results`` what ``recognize_batch`` returns.

        A frame without results (no gallery, no face) comes back undrawn.  A frame answered ``UNCHANGED`` is drawn with
        ``held[camera_id]`` when ``held`` (a dict: camera id -> the results of its last processed frame) is given, else undrawn.
        Calls with a HUD are serialised per processor; while one holds its turn, no more than one further batch of the same
        shape should be started on this processor from other threads (the ring is two slots deep).

        ``encode`` (a ``jpeg.JpegEncoder``): the drawn frames - full size, previews, or a det_size engine's arena - are encoded on
        the device while the turn is still held, and what crosses the link is the offsets and then the JPEG stream.  The call
        then returns one ``bytes`` per frame in place of the array (None, with a logged warning, for a frame whose coded rows
        overflowed the encoder's budget).  None: the arrays, as ever.

        ``redact`` (a ``redact.Redactor``): faces are masked on the device before anything is drawn or encoded.
        The engine pass sees the unmasked pixels; behind it the order is: resize to previews (``hud.out_size``), REDACT, draw the
        HUD, encode or copy out - so the HUD lies on top of the mosaic and no unmasked picture of a masked face crosses the
        link.  The regions come from this call's results, ``held`` standing in for ``UNCHANGED`` frames as for the HUD; a frame
        nothing ran for (no gallery, ``UNCHANGED`` with nothing held) is masked as a whole unless the redactor says ``"pass"``.
        ``redact_keys``: one id per frame for the redactor's ``linger`` history; defaults to ``camera_ids``.  None: nothing is
        masked, and the call runs what it ran before.

        ``chips`` (a ``chips.FaceChips``): as ``recognize_batch``; the chips are cut from the full-size frames strictly BEFORE the
        preview resize, the redactor and the HUD draw - the order on the stream is engine pass, chips, previews, redact, HUD,
        frame encoder - so they show the undrawn, unmasked pixels, and they are read back behind the pictures.  A face this
        call's ``redact`` masks gets ``"chip": None`` unless the object says ``masked=True``.  Only this call's own results are
        chipped: ``held`` results are drawn, not chipped again."""
        import torch
        if hud is None:
            raise ValueError("recognize_faces_batch draws with a hud.Hud; without one call recognize_batch")
        lock = self.__dict__.setdefault("_hud_lock", threading.Lock())
        hold = []
        with lock:
            try:
                results = self._recognize_batch(frames, company_id, hold=hold, **kw)
                if self.face_detector is None:
                    self.initialize_detector()
                det = self.face_detector
                if not hold:                                  # no gallery: nothing ran, the frames still owe a picture
                    hold.append(_upload_turn(self, det, frames, kw.get("pixel_format", "bgr"), kw.get("matrix", "bt601")))
                turn = hold[0]
                per_frame = list(results) if isinstance(results, list) else [None] * len(turn.arr)
                if held is not None and kw.get("camera_ids") is not None:
                    per_frame = [held.get(c) if r is UNCHANGED else r for r, c in zip(per_frame, kw["camera_ids"])]
                yuv = kw.get("pixel_format", "bgr") in ("nv12", "i420")
                shapes = [(a.shape[0] * 2 // 3, a.shape[1]) if yuv else a.shape[:2] for a in turn.arr]
                with torch.cuda.device(det.device):
                    stream = torch.cuda.current_stream(det.device)
                    stream.wait_event(turn.ready)
                    src = turn.dev if turn.table is None else (turn.dev, turn.table)
                    pending = None
                    if chips is not None and isinstance(results, list):   # in front of everything that writes the frames
                        pending = chips.begin(src, results, n=len(turn.arr), redact=redact)
                    if redact is None:
                        drawn = hud.draw(src, per_frame, shapes=shapes)
                    else:
                        keys = redact_keys if redact_keys is not None else kw.get("camera_ids")
                        canvas = hud.canvas(src, shapes)                  # the previews, when the HUD draws on previews
                        if canvas is None:
                            redact.apply(src, per_frame, shapes=shapes, keys=keys)
                        else:
                            redact.apply(canvas, per_frame, shapes=shapes, out_hws=[hud.out_hw(hw) for hw in shapes], keys=keys)
                        drawn = hud.draw(src, per_frame, shapes=shapes, canvas=canvas)
                    if encode is not None:
                        coded = encode.encode_device(drawn if drawn.dim() == 4 else (drawn, turn.table), shapes=shapes)
                        turn.ring.release(turn.turn)          # behind the queued encoder: it is the last reader of the slot
                        hold.clear()
                        out = encode.read_back(*coded)
                        if pending is not None:
                            chips.finish(pending)
                        return (out, results) if return_results else out
                    stage = self._hud_stage(tuple(drawn.shape))
                    stage.copy_(drawn, non_blocking=True)
                    turn.ring.release(turn.turn)              # behind the queued copy: the next upload into the slot waits
                    hold.clear()
                    stream.synchronize()
                    if pending is not None:
                        chips.finish(pending)
                host = stage.numpy()
                if drawn.dim() == 4:
                    out = [host[i].copy() for i in range(len(shapes))]
                else:                                         # the arena of a det_size engine: the frames at the ring's offsets
                    out = [host[o:o + h * w * 3].reshape(h, w, 3).copy() for o, (h, w) in zip(turn.ring.offsets, shapes)]
            finally:
                for t in hold:                                # an error on the way: the slot is not left waiting
                    t.ring.release(t.turn)
        return (out, results) if return_results else out

    def _hud_stage(self, shape):
        """Pinned host buffer the drawn frames land in (one per shape, the oldest of 4 dropped)."""
        import torch
        stages = self.__dict__.setdefault("_hud_stages", collections.OrderedDict())
        if shape not in stages:
            while len(stages) >= 4:
                stages.popitem(last=False)
            stages[shape] = torch.empty(shape, dtype=torch.uint8).pin_memory()
        return stages[shape]

    def annotate(self, frame, results):
        """Draw ``recognize`` / ``recognize_batch`` results onto a frame (colours of infrenceServer.py:546-553)."""
        for r in results or ():
            t = r["person_info"]["type"]
            color = (0, 255, 0) if t == "employee" else (0, 255, 255) if t == "visitor" else (0, 0, 255)
            frame = self.draw_enhanced_bounding_box(frame, r["bbox"], color, r["person_info"], r["det_score"],
                                                    r["recognition_score"])
        return frame

    def draw_enhanced_bounding_box(self, frame, bbox, color, person_info, detection_score, recognition_score):
        """The reference's HUD (infrenceServer.py:418-513) is presentation and out of scope; this
        draws a plain 2-px box so ``recognize_faces`` still returns a marked frame."""
        h, w = frame.shape[:2]
        x1, y1, x2, y2 = [int(v) for v in bbox]
        x1, x2 = max(0, min(x1, w - 1)), max(0, min(x2, w - 1))
        y1, y2 = max(0, min(y1, h - 1)), max(0, min(y2, h - 1))
        frame[y1:y1 + 2, x1:x2 + 1] = color; frame[max(y2 - 1, 0):y2 + 1, x1:x2 + 1] = color
        frame[y1:y2 + 1, x1:x1 + 2] = color; frame[y1:y2 + 1, max(x2 - 1, 0):x2 + 1] = color
        return frame

    def recognize_faces(self, frame, company_id):
        try:
            results = self.recognize(frame, company_id)
            if results is None:
                return frame
            frame = self.annotate(frame, results)
        except Exception as e:                # errors are logged and swallowed (:560-563)
            logger.error("Error during face recognition: %s", e)
        return frame


class CameraProcessor:
    """Counting path, peopleCount.py:822-896: whole gallery, 0.45 recognised / < 0.35 unknown,
    the [0.35, 0.45) band is dropped."""

    def __init__(self, embedding_manager, manager, face_detector=None, unknown_clusters=None):
        """``unknown_clusters`` (``process_batch`` only): an ``enrol.UnknownClusters`` bank that clusters the unknown faces
        of every camera on the device, or a dict camera_id -> bank for cameras of different campuses (cameras that map
        to the same bank object share it; a camera without an entry is not clustered)."""
        self.embedding_manager, self.manager, self.face_detector = embedding_manager, manager, face_detector
        self.recognition_threshold = 0.45
        self.unknown_threshold = 0.35
        self.unknown_clusters = unknown_clusters
        self._cluster_lock = threading.Lock()     # a bank's launches are queued in the order its batches arrive
        self._bank_masks = {}                     # bank layout of a batch -> device frame masks (uploaded once)

    def initialize_detector(self):
        if self.face_detector is None:
            from .face_analysis import FaceAnalysis
            self.face_detector = FaceAnalysis(name="buffalo_l").prepare(ctx_id=0)

    def process_frame(self, frame, camera_id):
        if self.face_detector is None:
            self.initialize_detector()
        matcher, metadata = self.embedding_manager.get_matcher_for_company(None)
        if len(matcher) == 0:
            return {"faces": 0, "recognized": 0, "unknown": 0}
        timestamp = datetime.utcnow()
        stats = {"faces": 0, "recognized": 0, "unknown": 0}
        try:
            r = _detect_embed(self.face_detector, frame)
            matcher, metadata, idx, score = _match_fresh(self.embedding_manager, None, matcher, metadata,
                                                         r["normed_embedding"])
            dec = matcher.decide_device(idx, score, self.recognition_threshold, self.unknown_threshold).cpu().numpy()
            idx, score = idx.cpu().numpy(), score.cpu().numpy()
            stats["faces"] = len(idx)
            q = None
            for f in range(len(idx)):
                if dec[f] == 1:
                    pid = matcher.ids[idx[f]]
                    self.manager.process_detection(pid, metadata[pid], camera_id, timestamp, float(score[f]))
                    stats["recognized"] += 1
                elif dec[f] == 0:
                    if q is None:             # re-normalised query rows, as handed on by peopleCount.py:863,884
                        e = r["normed_embedding"].cpu().numpy()
                        q = e / np.linalg.norm(e, axis=1, keepdims=True)
                        bb = r["bbox"].cpu().numpy().astype(int)
                    self.manager.process_unknown_detection(camera_id, timestamp, q[f], bb[f].tolist())
                    stats["unknown"] += 1
        except Exception as e:
            logger.error("Error in face detection: %s", e)
        return stats

    def _banks(self, camera_ids, device):
        """[(bank, device bool [n] mask of its frames, or None when every frame is its)] in batch order."""
        import torch
        uc = self.unknown_clusters
        if uc is None:
            return []
        if not isinstance(uc, dict):
            return [(uc, None)]
        banks, layout = [], []
        for cam in camera_ids:
            b = uc.get(cam)
            k = next((i for i, x in enumerate(banks) if x is b), None) if b is not None else -1
            if k is None:
                banks.append(b)
                k = len(banks) - 1
            layout.append(k)
        if len(banks) == 1 and all(k == 0 for k in layout):
            return [(banks[0], None)]
        key = tuple(layout)
        masks = self._bank_masks.get(key)
        if masks is None:                         # a new camera layout: the one upload (and wait) this path ever makes
            while len(self._bank_masks) >= 8:
                self._bank_masks.pop(next(iter(self._bank_masks)))
            masks = self._bank_masks[key] = [torch.tensor([k == i for k in layout], dtype=torch.bool).to(device)
                                             for i in range(len(banks))]
        return list(zip(banks, masks))

    def process_batch(self, frames, camera_ids, quality=None, chips=None):
        """Batch form of ``process_frame``: ``frames`` = list of BGR uint8 frames (of one size, or of any sizes when the
        engine has a ``det_size``), ``camera_ids`` = their cameras.  ONE pass of the slot pipeline over the batch,
        whole-gallery scan, the 0.45 / 0.35 decision and - with ``unknown_clusters`` - the clustering of the unknown
        faces (re-normalised rows, one ``assign_batch`` per bank, batch order) all stay on the device; then ONE group
        of device-to-host copies.  The manager then gets, frame by frame and face by face, the calls ``process_frame``
        would make (one ``timestamp`` for the whole batch).  With clusters, a manager that defines
        ``process_unknown_cluster(camera_id, timestamp, cluster, is_new, detection_count, bbox)`` gets that call for
        a clustered face instead of ``process_unknown_detection`` (no embedding travels to the host); a face its bank
        refused (capacity) goes to ``process_unknown_detection``.  Returns one stats dict per frame, with clusters plus
        ``"unknown_clusters": [(cluster, is_new, detection_count), ...]``.  Errors are logged and swallowed as
        ``process_frame``'s are; only ``len(camera_ids) != len(frames)`` raises (ValueError), before anything runs.

        ``quality`` (a ``quality.FaceQuality``): the engine pass judges every aligned face and embeds the fit ones only.  A
        rejected face is taken out of the unknown mask before ``assign_batch`` - it opens and joins no cluster - and reaches
        neither ``process_detection`` nor the unknown fan-out; it still counts under ``"faces"``, and every stats dict gains
        ``"low_quality"``, the number of such faces of the frame.

        ``chips`` (a ``chips.FaceChips``): the call keeps its ring turn and, with the decisions on the host, cuts a thumbnail of
        every face the object selects out of the ring's full-size device frames.  ``who`` is given the dict
        ``{"bbox", "person_info": metadata | {"type": "unknown"}, "recognition_score", "cluster", "is_new"}`` of a face that
        reaches the manager (``cluster`` None without one), so ``who=lambda r: r.get("is_new")`` gives one thumbnail per new
        unknown cluster.  Each stats dict gains ``"chips": [(face index, chip), ...]``, and a manager that defines
        ``process_face_chip(camera_id, timestamp, person_id, cluster, bbox, chip)`` gets that call right behind the face's
        detection call (``person_id`` None for an unknown, ``cluster`` None without one); every other call is unchanged.  A face
        rejected by ``quality`` gets no chip.  Calls with chips are serialised per processor; while one holds its turn, no more
        than one further batch of the same shape should be started on this processor from other threads (the ring is two slots
        deep).  None: the call runs the code it ran before."""
        if chips is None:
            return self._process_batch(frames, camera_ids, quality)
        hold = []
        with self.__dict__.setdefault("_hud_lock", threading.Lock()):
            try:
                return self._process_batch(frames, camera_ids, quality, chips, hold)
            finally:
                for t in hold:
                    t.ring.release(t.turn)

    def _process_batch(self, frames, camera_ids, quality=None, chips=None, hold=None):
        """``process_batch``; with ``chips``, ``hold`` (a list) receives the ring turn, which the caller releases."""
        import torch
        from . import _lib
        if self.face_detector is None:
            self.initialize_detector()
        n = len(frames)
        if len(camera_ids) != n:                  # the caller's mistake, and the one error that raises (gallery or not)
            raise ValueError(f"{n} frames but {len(camera_ids)} camera ids")
        clustered = self.unknown_clusters is not None
        stats = [dict({"faces": 0, "recognized": 0, "unknown": 0}, **({"unknown_clusters": []} if clustered else {}),
                      **({"low_quality": 0} if quality is not None else {}), **({"chips": []} if chips is not None else {}))
                 for _ in range(n)]
        matcher, metadata = self.embedding_manager.get_matcher_for_company(None)
        if len(matcher) == 0 or n == 0:
            return stats
        timestamp = datetime.utcnow()
        try:
            det = self.face_detector
            if chips is None:
                n, r = _detect_embed_batch(self, det, frames, quality=quality)
            else:
                n, r, _ = _detect_embed_batch_gated(self, det, frames, quality=quality, hold=hold)
            E = r["normed_embedding"]
            matcher, metadata, idx, score = _match_fresh(self.embedding_manager, None, matcher, metadata, E)
            dec = matcher.decide_device(idx, score, self.recognition_threshold, self.unknown_threshold)
            cap = r["bbox"].shape[1]
            S = n * cap
            banks = self._banks(camera_ids, det.device)
            use_cb = bool(banks) and hasattr(self.manager, "process_unknown_cluster")
            ints = [idx, dec.to(torch.int64)]
            qn = None
            if banks:
                with self._cluster_lock, torch.cuda.device(det.device):
                    qn = torch.empty_like(E)                                          # peopleCount.py:863
                    _lib.load().fr_l2norm_rows_f32(_lib.ptr(E), _lib.ptr(qn), S, 512, _lib.stream_ptr())
                    unknown = (torch.arange(cap, device=det.device)[None, :] < r["counts"][:, None]) & (dec.view(n, cap) == 0)
                    if quality is not None:                                           # a rejected face joins no cluster
                        unknown = unknown & (r["quality_verdict"] == 0)
                    trip = None
                    for bank, mask in banks:
                        take = (unknown if mask is None else unknown & mask[:, None]).reshape(-1)
                        t = torch.stack(bank.assign_batch(qn, take))                  # [3,S]: cluster, is_new, count
                        trip = t if trip is None else torch.where(take[None, :], t, trip)   # a slot belongs to one bank
                ints.append(trip.reshape(-1).to(torch.int64))
            if quality is not None:
                ints.append(r["quality_verdict"].reshape(-1).to(torch.int64))         # last, behind the banks' columns
            # ---- the one group of device -> host copies
            counts = r["counts"].cpu().numpy()
            ints = torch.cat(ints).cpu().numpy()
            verdict_h = None
            if quality is not None:
                ints, verdict_h = ints[:-S], ints[-S:]
            flt = torch.cat([score.reshape(S, 1), r["bbox"].reshape(S, 4)], dim=1).cpu().numpy()
            idx_h, dec_h = ints[:S], ints[S:2 * S]
            trip_h = ints[2 * S:].reshape(3, S) if banks else None
            score_h, bb = flt[:, 0], flt[:, 1:].astype(int)                           # :531 truncation
            q = None
            unbanked = isinstance(self.unknown_clusters, dict) and any(self.unknown_clusters.get(c) is None for c in camera_ids)
            if not use_cb or unbanked:                                                # the embeddings travel as well
                e = (E if qn is None else qn).cpu().numpy()
                q = e / np.linalg.norm(e, axis=1, keepdims=True) if qn is None else e
            chip_of = {}                                                              # slot -> chip (chips only)
            if chips is not None:
                chosen, slots = [[] for _ in range(n)], [[] for _ in range(n)]
                for f in range(n):
                    for s in range(f * cap, f * cap + int(counts[f])):
                        if (verdict_h is not None and verdict_h[s] != 0) or dec_h[s] not in (0, 1):
                            continue                                                  # no call reaches the manager for it
                        cl = int(trip_h[0, s]) if trip_h is not None and dec_h[s] == 0 else -1
                        chosen[f].append({"bbox": bb[s].tolist(),
                                          "person_info": metadata[matcher.ids[idx_h[s]]] if dec_h[s] == 1 else {"type": "unknown"},
                                          "recognition_score": float(score_h[s]), "cluster": cl if cl >= 0 else None,
                                          "is_new": bool(trip_h[1, s]) if cl >= 0 else False})
                        slots[f].append(s)
                turn = hold[0]
                with torch.cuda.device(det.device):
                    torch.cuda.current_stream(det.device).wait_event(turn.ready)
                    chips.cut(turn.dev if turn.table is None else (turn.dev, turn.table), chosen, n=len(turn.arr))
                for f in range(n):
                    for d, s in zip(chosen[f], slots[f]):
                        if d["chip"] is not None:
                            chip_of[s] = d["chip"]
                            stats[f]["chips"].append((s - f * cap, d["chip"]))
            chip_cb = chips is not None and hasattr(self.manager, "process_face_chip")
            refused = 0
            for f in range(n):
                st, cam = stats[f], camera_ids[f]
                st["faces"] = int(counts[f])
                for s in range(f * cap, f * cap + int(counts[f])):
                    if verdict_h is not None and verdict_h[s] != 0:
                        st["low_quality"] += 1
                    elif dec_h[s] == 1:
                        pid = matcher.ids[idx_h[s]]
                        self.manager.process_detection(pid, metadata[pid], cam, timestamp, float(score_h[s]))
                        if chip_cb and s in chip_of:
                            self.manager.process_face_chip(cam, timestamp, pid, None, bb[s].tolist(), chip_of[s])
                        st["recognized"] += 1
                    elif dec_h[s] == 0:
                        cl = int(trip_h[0, s]) if trip_h is not None else -1
                        if cl != -1:
                            st["unknown_clusters"].append((cl, int(trip_h[1, s]), int(trip_h[2, s])))
                        if cl >= 0 and use_cb:
                            self.manager.process_unknown_cluster(cam, timestamp, cl, int(trip_h[1, s]), int(trip_h[2, s]),
                                                                 bb[s].tolist())
                        else:
                            if cl == -2:
                                refused += 1
                            if q is None:                 # only a refused row needs its embedding here: a second, rare copy
                                q = qn.cpu().numpy()
                            self.manager.process_unknown_detection(cam, timestamp, q[s], bb[s].tolist())
                        if chip_cb and s in chip_of:
                            self.manager.process_face_chip(cam, timestamp, None, cl if cl >= 0 else None, bb[s].tolist(), chip_of[s])
                        st["unknown"] += 1
            if refused:
                logger.warning("Unknown-person clusters full: %d faces of this batch were not clustered", refused)
        except Exception as e:
            logger.error("Error in face detection: %s", e)
        return stats


def _face_result(bbox, det_score, decision, row, score, ids, metadata):
    """One face of ``recognize`` / ``recognize_batch``: ``row`` is the position in ``ids`` the scan chose, ``decision`` what
    fr_match_decide made of its score (1: recognised; infrenceServer.py:545-552)."""
    if decision == 1:
        pid = ids[row]
        return {"bbox": bbox, "person_id": pid, "person_info": metadata[pid], "det_score": float(det_score),
                "recognition_score": score}
    return {"bbox": bbox, "person_id": None, "person_info": {"name": "Unknown", "type": "unknown"},
            "det_score": float(det_score), "recognition_score": 0}


def _face_candidates(bbox, det_score, rows, scores, ids, metadata, min_score):
    """One face of ``identify`` / ``identify_batch``: its ranked rows (positions in ``ids``) and scores as candidates."""
    cands = []
    for i, s in zip(rows, scores):
        if i < 0 or (min_score is not None and s < min_score):
            break                                             # ranked: everything behind is empty or lower
        cands.append({"person_id": ids[i], "person_info": metadata[ids[i]], "score": s})
    return {"bbox": bbox, "det_score": float(det_score), "candidates": cands}


def _detect_embed(detector, frame):
    """detect -> align -> embed of one frame under the engine's lock: one engine may be shared by threads
    (/root/reference/trainingServer.py:115,227) and ``get_batch`` takes the same lock."""
    lock = getattr(detector, "_lock", None)
    dev = _to_device(frame, detector.device)
    if lock is None:
        return detector.detect_embed_device(dev)
    with lock:
        return detector.detect_embed_device(dev)


def _detect_embed_batch(owner, det, frames, pixel_format="bgr", matrix="bt601", quality=None):
    """``_detect_embed_batch_gated`` without a gate: (number of frames, the slot results)."""
    n, r, _ = _detect_embed_batch_gated(owner, det, frames, pixel_format, matrix, quality=quality)
    return n, r


def _detect_embed_batch_gated(owner, det, frames, pixel_format="bgr", matrix="bt601", gate=None, camera_ids=None, tracks=None,
                              quality=None, hold=None):
    """One pass of the sync-free slot pipeline over a batch of host frames (``recognize_batch`` and
    ``CameraProcessor.process_batch``): pinned staging ring (kept on ``owner``, one per batch shape and pixel format) -> copy
    stream -> ``detect_embed_slots(compact_embed=True)`` under the engine's lock.  Frames of one size, or of any sizes when the
    engine has a ``det_size``.  ``pixel_format`` ``"nv12"`` / ``"i420"``: the frames are YUV 4:2:0, ``uint8 [H*3/2, W]``, and the
    ring converts them on the device behind its copy (ingest.py).  Returns (number of frames, the slot results: device tensors,
    keep).

    ``gate`` (``activity.ActivityGate``) with ``camera_ids``: the gate judges the ring's device frames behind the copy - one
    small device-to-host copy and one synchronisation - and the engine runs on the active frames only: ``keep`` is the list of
    their indices, the frame count and the slot results are theirs (a device gather of the frames; under ``det_size`` the
    selected rows of the ring's frame table and of ``det_scale``, no frame bytes move).  With none active the slot results are
    None and nothing but the upload and the gate has run.  ``keep`` None: every frame, the ring's tensors as they are - the code
    path of a call without a gate.

    ``tracks`` (``tracks.FaceTracks``) with ``camera_ids``: handed to the engine pass with the camera ids of the frames that
    reach it - all of them, or with a gate the kept ones, so a frame judged inactive never moves its camera's tracks.

    ``quality`` (``quality.FaceQuality``): handed to the engine pass, which then embeds the faces judged fit only; a call
    without it passes no such argument on, and runs the code it always ran.

    ``hold`` (a list): the ring turn is NOT released here.  A ``_HeldTurn`` is appended instead - the ring, the turn, the host
    frames, the ring's device frames of the WHOLE batch (and their frame table under ``det_size``) and the upload's event - and
    the caller releases it (``ring.release(turn)``) once its own work on those device frames is queued: until then the next
    upload into that slot waits.  None: released here, as ever."""
    import torch
    arr, ring, turn = _ring_turn(owner, det, frames, pixel_format, matrix)
    n, det_size = len(arr), getattr(det, "det_size", None)
    with det._lock, torch.cuda.device(det.device):
        _fill_turn(ring, turn, arr, det_size)
        if det_size is None:
            dev, ready = ring.upload(turn)
            ragged = {}
        else:                                         # one arena, one copy, one engine pass whatever the frames' sizes
            dev, table, ready = ring.upload(turn)
            ragged = {"table": table, "det_scale": ring.det_scale}
        if hold is not None:
            hold.append(_HeldTurn(ring, turn, arr, dev, ragged.get("table"), ready))
        keep = None
        if gate is not None:
            torch.cuda.current_stream(det.device).wait_event(ready)
            active, _ = gate.judge(dev, camera_ids, table=ragged.get("table"))          # the extra copy and synchronisation
            if not active.all():
                keep = [int(f) for f in np.flatnonzero(active)]
                n = len(keep)
                if n == 0:
                    if hold is None:
                        ring.release(turn)
                    return 0, None, keep
                sel = torch.tensor(keep, dtype=torch.int64).to(det.device)
                if det_size is None:
                    dev = dev.index_select(0, sel)                                      # the one device copy
                else:                                 # the arena stays where it is: the table's rows name the active frames
                    ragged = {"table": ragged["table"].view(-1, 32).index_select(0, sel).reshape(-1),
                              "det_scale": ragged["det_scale"].index_select(0, sel)}
        if tracks is not None:
            ragged = dict(ragged, tracks=tracks, camera_ids=camera_ids if keep is None else [camera_ids[f] for f in keep])
        if quality is not None:
            ragged = dict(ragged, quality=quality)
        r = det.detect_embed_slots(dev, ready_event=ready, compact_embed=True, **ragged)    # results go to the host anyway
        if hold is None:
            ring.release(turn)
    return n, r, keep


# A ring turn whose release is the caller's (``_detect_embed_batch_gated(hold=...)``): ``dev`` is the ring's device batch
# uint8 [n,H,W,3] - or its arena, with ``table`` the frame table - of ALL the call's frames, ``ready`` the upload's event
_HeldTurn = collections.namedtuple("_HeldTurn", "ring turn arr dev table ready")


def _upload_turn(owner, det, frames, pixel_format, matrix):
    """The front of ``_detect_embed_batch_gated`` alone: the frames into their ring and up to the device (a YUV ring converts
    them there); the turn is the caller's to release.  For a call that has nothing to run the engine on, but a picture to return."""
    import torch
    arr, ring, turn = _ring_turn(owner, det, frames, pixel_format, matrix)
    with det._lock, torch.cuda.device(det.device):
        _fill_turn(ring, turn, arr, getattr(det, "det_size", None))
        if getattr(det, "det_size", None) is None:
            dev, ready = ring.upload(turn)
            return _HeldTurn(ring, turn, arr, dev, None, ready)
        dev, table, ready = ring.upload(turn)
        return _HeldTurn(ring, turn, arr, dev, table, ready)


# One JPEG file of a batch (``pixel_format="jpeg"``): its bytes, the (H, W, 3) of its picture, what ``jpeg_decode.parse`` made of
# its header and - where the device does not take it - the host's decode (None: it does not decode, a black frame)
_Encoded = collections.namedtuple("_Encoded", "data shape header image")


def _encoded_frames(frames):
    """The files of a JPEG batch as ``_Encoded``.  A file the device decoder does not take is decoded here, by
    ``ingest.decode_image``, since its size is needed before a ring can be chosen; a blob that does not decode at all takes the
    size of the batch's first picture (16 x 16 when there is none) and goes through the engine as a black frame - no faces."""
    from .ingest import decode_image
    from .jpeg_decode import parse
    out = []
    for f in frames:
        if not isinstance(f, (bytes, bytearray, memoryview)):
            raise ValueError("jpeg frames of a batch must be bytes, one file per frame")
        hd = parse(f)
        if isinstance(hd, str):
            img = decode_image(f)
            out.append(_Encoded(f, None if img is None else img.shape, hd, img))
        else:
            out.append(_Encoded(f, (hd.H, hd.W, 3), hd, None))
    first = next((e.shape for e in out if e.shape is not None), (16, 16, 3))
    return [e if e.shape is not None else e._replace(shape=first) for e in out]


def _fill_turn(ring, turn, arr, det_size):
    """the frames of a batch into the ring's pinned slot"""
    if arr and isinstance(arr[0], _Encoded):
        for i, e in enumerate(arr):
            ring.put(turn, i, e.data, header=e.header, decoded=e.image)
    elif det_size is None:
        host = ring.host_buffer(turn)
        for i, a in enumerate(arr):
            host[i] = a
    else:
        for i, a in enumerate(arr):
            ring.host_frame(turn, i)[...] = a


def _ring_turn(owner, det, frames, pixel_format, matrix):
    """The frames of a batch as validated contiguous arrays, the pinned staging ring of their batch shape and pixel format (kept
    on ``owner``, made on first use, the oldest of 8 dropped) and the turn of that ring the batch takes.  Host work only, outside
    the engine's lock."""
    from .colour import check_pixel_format, check_yuv_shape
    from .ingest import FrameIngest, RaggedIngest
    det_size = getattr(det, "det_size", None)
    jpeg = pixel_format == "jpeg"
    arr = _encoded_frames(frames) if jpeg else [np.ascontiguousarray(np.asarray(f)) for f in frames]
    yuv = not jpeg and check_pixel_format(pixel_format, matrix)[0] is not None
    if jpeg:
        shapes = tuple(e.shape[:2] for e in arr)
    elif yuv:
        if any(a.ndim != 2 or a.dtype != np.uint8 for a in arr):
            raise ValueError(f"{pixel_format} frames of a batch must be uint8 [H*3/2, W]")
        shapes = tuple(check_yuv_shape(a.shape) for a in arr)
    else:
        if any(a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8 for a in arr):
            raise ValueError("frames of a batch must be uint8 [H,W,3] of one size (any sizes with prepare(det_size=...))")
        shapes = tuple(a.shape[:2] for a in arr)
    n, (h, w) = len(arr), shapes[0]
    if det_size is None and any(s != (h, w) for s in shapes):
        raise ValueError("frames of a batch must be uint8 [H,W,3] of one size (any sizes with prepare(det_size=...))")
    stages = owner.__dict__.setdefault("_stages", {})
    key = (n, h, w) if det_size is None else (shapes, det_size)
    fmt = {"pixel_format": pixel_format, "matrix": matrix} if yuv else {"pixel_format": "jpeg"} if jpeg else {}
    if yuv:                                           # the BGR rings keep the keys they always had
        key += (pixel_format, matrix)
    elif jpeg:
        key += ("jpeg",)
    if key not in stages:
        while len(stages) >= 8:                       # a few (cameras present, frame size) shapes at most: drop the oldest ring
            stages.pop(next(iter(stages)))
        stages[key] = [FrameIngest(n, h, w, det.device, depth=2, **fmt) if det_size is None else
                       RaggedIngest(key[0], det_size, det.device, depth=2, **fmt), 0]
    ring, turn = stages[key]
    stages[key][1] = turn + 1
    return arr, ring, turn


def _with_current(fetch, run, got=None):
    """``run(*got)`` with ``got`` = what ``fetch()`` returns, a view or view set first (``got`` given: fetched already).  A
    sync on another thread may have changed the slab's membership since (the generation moved on): on StaleViewError
    fetch once more and run again instead of dropping the frame.  Returns (what was fetched, what ``run`` returned)."""
    from .gallery import StaleViewError
    got = fetch() if got is None else got
    try:
        return got, run(*got)
    except StaleViewError:
        got = fetch()
        return got, run(*got)


def _match_fresh(manager, company_id, matcher, metadata, Q, k=None):
    """Scan through the company's view, the current one if this one is stale (``_with_current``).  ``k``: the top-k form
    (idx / score [F,k]) instead of the single best row."""
    (matcher, metadata), (idx, score) = _with_current(
        lambda: manager.get_matcher_for_company(company_id),
        lambda m, _: m.match_device(Q) if k is None else m.match_topk_device(Q, k), (matcher, metadata))
    return matcher, metadata, idx, score


def _to_device(frame, device):
    import torch
    a = np.ascontiguousarray(np.asarray(frame))
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
        raise ValueError("frame must be uint8 [H,W,3] BGR")
    return torch.from_numpy(a).to(device)[None]
