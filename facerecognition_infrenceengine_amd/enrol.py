"""Enrolment arithmetic and unknown-person clustering on the engine.

Mirrors /root/reference/trainingServer.py:170-247,328,355-358,393 (largest face -> pose consistency ->
mean -> duplicate check -> pickled float32[512] row) and /root/reference/peopleCount.py:52-91,432-449
(10-deep running mean, first cluster with dot >= 0.65).  The O(N) per-row GridFS read + cosine loop of
the reference's duplicate check becomes one first-above scan of the device gallery (``first_above``).

``Enroller.enrol`` is the one-job form; ``Enroller.enrol_batch`` / ``enrol_slots`` run a whole batch of jobs with one
engine pass and one `fr_enrol_batch_f32` call, giving job for job what enrolling them one after the other gives
(DESIGN.md 4.6d).
"""
import pickle

import numpy as np
import torch

from . import _lib
from .gallery import GalleryView, StaleViewError, read_back  # noqa: F401  (StaleViewError: what a stale view raises here)

DIM = 512
# include/frhip.h FR_ENROL_* (tests/test_enrol_batch_abi.py compares)
ENROL_DONE, ENROL_NO_FACE, ENROL_DIFFERENT, ENROL_DUPLICATE = 0, 1, 2, 3
ENROL_MAX_POSES, ENROL_MAX_JOBS = 8, 256
STATUS_NAMES = {ENROL_DONE: "done", ENROL_NO_FACE: "no_face", ENROL_DIFFERENT: "different_people",
                ENROL_DUPLICATE: "duplicate"}


def largest_face_index(faces):
    """trainingServer.py:234-239: first index of the max bbox area."""
    areas = [(f.bbox[2] - f.bbox[0]) * (f.bbox[3] - f.bbox[1]) for f in faces]
    return areas.index(max(areas))


class Enroller:
    def __init__(self, face_analysis, similarity_threshold=0.4, duplicate_threshold=0.4, quality=None, decoder=None, orient=False):
        """``quality`` (a ``quality.FaceQuality``): ``process_image`` has the engine judge the aligned faces, and ``enrol`` refuses a
        job whose pose image shows an unfit largest face (``{"status": "low_quality", "image": i, "reasons": [...]}``) - a gallery
        row lives for years.  ``enrol_batch`` and ``enrol_slots`` of such an Enroller raise ValueError: the batch kernel
        (fr_enrol_batch_f32) picks the largest face on the device and takes no mask yet.  None: no face is judged, as ever.

        ``decoder`` (a ``jpeg_decode.JpegDecoder`` on the engine's device): ``enrol_batch`` decodes encoded images on the device
        in one call, image by image falling back to the host decoder for what the device does not take; the pixels are the
        same pixels, so every job's result is that of the host-decoded run.  None: decoded on the host, as ever.

        ``orient=True``: encoded images are turned as their EXIF orientation says before the detector sees them - the picture
        ``cv2.imdecode`` hands the reference's worker (trainingServer.py:219-221), where the default passes an upright phone photo
        on as coded, lying on its side.  Host decode (``process_image``, ``enrol``) and device decode (``enrol_batch`` through ``decoder``,
        and its host fallback) honour it alike; a ``decoder`` built with another ``orient`` raises ValueError here."""
        self.orient = bool(orient)
        if decoder is not None and bool(getattr(decoder, "orient", False)) != self.orient:
            raise ValueError(f"Enroller(orient={self.orient}) with a decoder built with orient={bool(getattr(decoder, 'orient', False))}")
        self.decoder = decoder
        self.app, self.similarity_threshold, self.duplicate_threshold = face_analysis, similarity_threshold, duplicate_threshold
        self.quality = quality
        self.lib = _lib.load()
        self.device = face_analysis.device

    def process_image(self, image):
        """trainingServer.py:216-247: normed embedding of the largest face, or None.  ``image``: a BGR uint8 array, or
        the encoded bytes the reference reads from GridFS (``:219-221``: decoded here, None when they do not decode)."""
        face = self._largest_face(image)
        return None if face is None else face.normed_embedding

    def _largest_face(self, image):
        """The Face ``process_image`` takes its embedding from, or None; with ``quality`` it carries the verdict."""
        if isinstance(image, (bytes, bytearray, memoryview)):
            from .ingest import decode_image
            image = decode_image(image, orient=getattr(self, "orient", False))
            if image is None:
                return None
        faces = self.app.get(image) if self.quality is None else self.app.get(image, quality=self.quality)
        if not faces:
            return None
        return faces[largest_face_index(faces) if len(faces) > 1 else 0]

    def check_image_similarity(self, embeddings):
        """trainingServer.py:202-214: first (i, j), i < j, with cosine < threshold."""
        k = len(embeddings)
        if k < 2:
            return True, None
        x = torch.from_numpy(np.asarray(embeddings, np.float32)).to(self.device).contiguous()
        out = torch.empty((k, k), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self.lib.fr_cosine_matrix_f32(_lib.ptr(x), _lib.ptr(x), k, k, DIM, _lib.ptr(out), _lib.stream_ptr())
        s = out.cpu().numpy()
        for i in range(k):
            for j in range(i + 1, k):
                if s[i, j] < self.similarity_threshold:
                    return False, (i, j)
        return True, None

    def mean_embedding(self, embeddings):
        """trainingServer.py:355: np.mean(face_embeddings, axis=0) (float32, NOT renormalised)."""
        x = torch.from_numpy(np.asarray(embeddings, np.float32)).to(self.device).contiguous()
        out = torch.empty(DIM, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self.lib.fr_mean_rows_f32(_lib.ptr(x), x.shape[0], DIM, _lib.ptr(out), _lib.stream_ptr())
        return out.cpu().numpy()

    def check_duplicate(self, new_embedding, matcher):
        """trainingServer.py:170-200 against a GalleryMatcher of unit rows, or a company's GalleryView: (is_dup, id of the
        first row, in the matcher's / the view's order, with cosine > threshold)."""
        idx, score = first_above(self.lib, matcher, new_embedding, self.duplicate_threshold, inclusive=False)
        return (idx >= 0), (matcher.ids[idx] if idx >= 0 else None)

    def enrol(self, pose_images, matcher):
        """Whole job arithmetic (trainingServer.py:312-398).  Returns dict(status=..., ...).  With ``quality``: the first pose
        image whose largest face is not fit ends the job, before the similarity check, with ``{"status": "low_quality",
        "image": its index, "reasons": [...]}``."""
        if self.quality is None:
            embs = [e for e in (self.process_image(im) for im in pose_images) if e is not None]
        else:
            embs = []
            for i, im in enumerate(pose_images):
                face = self._largest_face(im)
                if face is None:
                    continue
                if not face.quality_ok:
                    return {"status": "low_quality", "image": i, "reasons": list(face.quality["reasons"])}
                embs.append(face.normed_embedding)
        if not embs:
            return {"status": "no_face"}
        ok, pair = self.check_image_similarity(embs)
        if not ok:
            return {"status": "different_people", "pair": pair}
        avg = self.mean_embedding(embs)
        dup, dup_id = self.check_duplicate(avg, matcher)
        if dup:
            return {"status": "duplicate", "duplicate_id": dup_id, "embedding": avg}
        return {"status": "done", "embedding": avg, "blob": pickle.dumps(avg)}       # :393 gallery row format

    # ------------------------------------------------------------------ batches
    def enrol_slots(self, slots, job_images, gallery):
        """The whole arithmetic of a batch of jobs on the device, no host synchronisation (include/frhip.h
        fr_enrol_batch_f32: largest face, pose consistency, mean, duplicate check against ``gallery`` and against the
        batch's own earlier ``done`` jobs, in job order).

        slots: the dict of one ``FaceAnalysis.detect_embed_slots`` call, or a list of such dicts (their images are numbered
        on, in list order).  job_images: per job, the list of its image indices, in the reference's position order.
        gallery: a GalleryMatcher of unit rows or a GalleryView (a stale one raises StaleViewError).
        Returns device tensors on the current stream: status i32 [J] (ENROL_*), pair i32 [J,2], face i32 [I] (the chosen
        slot of each image in ``job_images`` order, flattened; -1: no face), avg f32 [J,512], row f32 [J,512], dup_pos
        i64 [J] (gallery position, len(gallery) + i for the batch's job i, -1), dup_score f32 [J].
        An Enroller with ``quality`` raises ValueError: the kernel takes no mask of unfit faces yet."""
        if getattr(self, "quality", None) is not None:
            raise ValueError("an Enroller with quality enrols job by job (enrol): the batch kernel takes no quality mask yet")
        parts = list(slots) if isinstance(slots, (list, tuple)) else [slots]
        job_images = [list(im) for im in job_images]
        J = len(job_images)
        if J > ENROL_MAX_JOBS:
            raise ValueError(f"at most {ENROL_MAX_JOBS} jobs a batch (got {J})")
        max_poses = max((len(im) for im in job_images), default=0)
        if max_poses > ENROL_MAX_POSES:
            raise ValueError(f"at most {ENROL_MAX_POSES} images a job (got {max_poses})")
        firsts, row0 = [], 0                       # first row of every image: known from the shapes alone
        for p in parts:
            n, cap = p["bbox"].shape[0], p["bbox"].shape[1]
            firsts += [row0 + k * cap for k in range(n)]
            row0 += n * cap
        order = [int(i) for im in job_images for i in im]
        if any(not 0 <= i < len(firsts) for i in order):
            raise ValueError("job_images names an image the slots do not hold")
        src = gallery.row_source()
        dev, I = self.device, len(order)
        job_first = np.cumsum([0] + [len(im) for im in job_images])
        # one pinned staging block, one asynchronous copy: image order, first rows, job_first
        host = torch.from_numpy(np.concatenate([order, [firsts[i] for i in order], job_first]).astype(np.int32))
        status = torch.empty(J, dtype=torch.int32, device=dev)
        pair = torch.empty((J, 2), dtype=torch.int32, device=dev)
        face = torch.empty(I, dtype=torch.int32, device=dev)
        avg = torch.empty((J, DIM), dtype=torch.float32, device=dev)
        row = torch.empty((J, DIM), dtype=torch.float32, device=dev)
        dup_pos = torch.empty(J, dtype=torch.int64, device=dev)
        dup_score = torch.empty(J, dtype=torch.float32, device=dev)
        out = {"status": status, "pair": pair, "face": face, "avg": avg, "row": row, "dup_pos": dup_pos,
               "dup_score": dup_score}
        if J == 0:
            return out
        with torch.cuda.device(dev):
            meta = host.pin_memory().to(dev, non_blocking=True)
            E = torch.cat([p["normed_embedding"].reshape(-1, DIM) for p in parts]).to(dev, torch.float32).contiguous()
            bbox = torch.cat([p["bbox"].reshape(-1, 4) for p in parts]).to(dev, torch.float32).contiguous()
            counts = torch.cat([p["counts"].reshape(-1) for p in parts]).to(dev, torch.int32)
            img_first, jf = meta[I:2 * I], meta[2 * I:]
            img_count = counts.index_select(0, meta[:I].to(torch.int64)).contiguous()     # the detector's counts, never read here
            ws = torch.empty(int(self.lib.fr_enrol_batch_workspace(J, src.N)), dtype=torch.uint8, device=dev)
            self.lib.fr_enrol_batch_f32(_lib.ptr(E), _lib.ptr(bbox), E.shape[0], _lib.ptr(img_first), _lib.ptr(img_count),
                                        I, _lib.ptr(jf), J, max_poses, DIM, _lib.ptr(src.G), _lib.ptr(src.view), src.N,
                                        float(self.similarity_threshold), float(self.duplicate_threshold),
                                        _lib.ptr(status), _lib.ptr(pair), _lib.ptr(face), _lib.ptr(avg), _lib.ptr(row),
                                        _lib.ptr(dup_pos), _lib.ptr(dup_score), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
        return out

    def _engine_pass(self, images):
        """One ``detect_embed_slots`` call per image shape (one call in all with a ``det_size`` engine), grouped as
        camera.CameraManager.process_batch groups frames.  images: BGR arrays (or device tensors), None for what did not decode.
        Returns (slot dicts, image index of every input image)."""
        mixed = getattr(self.app, "det_size", None) is not None
        by_shape = {}
        for k, im in enumerate(images):
            if im is not None:
                by_shape.setdefault(None if mixed else tuple(im.shape), []).append(k)
        parts, index, base = [], [None] * len(images), 0
        for ks in by_shape.values():
            if any(torch.is_tensor(images[k]) for k in ks):     # decoded on the device (``decoder``): they are there already
                frames = self.app._to_device([images[k] for k in ks])
                frames = frames if mixed else torch.stack(frames)
            else:
                frames = [np.ascontiguousarray(images[k]) for k in ks]
                frames = self.app._to_device(frames if mixed else np.stack(frames))
            parts.append(self.app.detect_embed_slots(frames))
            for n, k in enumerate(ks):
                index[k] = base + n
            base += len(ks)
        if any(i is None for i in index) or not parts:          # an image without a face: one slot whose count is 0
            parts.append({"counts": torch.zeros(1, dtype=torch.int32, device=self.device),
                          "bbox": torch.zeros((1, 1, 4), dtype=torch.float32, device=self.device),
                          "normed_embedding": torch.zeros((1, DIM), dtype=torch.float32, device=self.device)})
            index = [base if i is None else i for i in index]
        return parts, index

    def enrol_batch(self, jobs, gallery, ids=None, commit=False):
        """``enrol`` for a list of jobs: job for job what ``enrol(jobs[j], gallery)`` returns when every ``done`` job's row
        is upserted (normalise=True) behind the gallery before the next job runs - a batch sees its own earlier jobs.
        jobs: a list of lists of images (BGR arrays, or encoded bytes as ``process_image`` accepts; what does not decode
        is an image without a face).  gallery: a GalleryMatcher of unit rows or a GalleryView.  ids: optional, one id per
        job.  One engine pass, one ``enrol_slots``, one group of device-to-host copies.

        Returns an ``EnrolBatchResult``: a list with one dict per job, keyed as ``enrol``'s (status, pair, duplicate_id,
        embedding, blob); a duplicate of the batch's own job i carries ``duplicate_of_job: i`` and ``duplicate_id =
        ids[i]`` (None without ``ids``).  commit=True (needs a GalleryView and ``ids``): the ``done`` rows are upserted into
        ``gallery.gallery`` under their ids in one call, and ``result.view`` is the view of the old ids followed by the
        done ids in job order - the gallery the next batch is checked against.
        An Enroller with ``quality`` raises ValueError: the batch kernel picks the largest face on the device and takes no mask."""
        if getattr(self, "quality", None) is not None:
            raise ValueError("an Enroller with quality enrols job by job (enrol): the batch kernel takes no quality mask yet")
        jobs = [list(job) for job in jobs]
        if len(jobs) > ENROL_MAX_JOBS:
            raise ValueError(f"at most {ENROL_MAX_JOBS} jobs a batch (got {len(jobs)})")
        if any(len(job) > ENROL_MAX_POSES for job in jobs):
            raise ValueError(f"at most {ENROL_MAX_POSES} images a job (got {max(len(job) for job in jobs)})")
        if ids is not None and len(ids) != len(jobs):
            raise ValueError("ids and jobs disagree")
        if commit and not (isinstance(gallery, GalleryView) and ids is not None):
            raise ValueError("commit=True needs a GalleryView and ids")
        N = gallery.row_source().N                                   # a stale view raises: before the engine runs
        result = EnrolBatchResult()
        if not jobs:
            result.view = gallery if commit else None
            return result
        images = [im for job in jobs for im in job]
        encoded = [k for k, im in enumerate(images) if isinstance(im, (bytes, bytearray, memoryview))]
        if encoded and self.decoder is not None:                     # one device decode for all of them, falling back per image
            with torch.cuda.device(self.device):
                decoded = self.decoder.decode_frames([images[k] for k in encoded])
        else:
            from .ingest import decode_image
            decoded = [decode_image(images[k], orient=getattr(self, "orient", False)) for k in encoded]
        for k, im in zip(encoded, decoded):
            images[k] = im
        job_images, k = [], 0
        with torch.cuda.device(self.device):
            parts, index = self._engine_pass(images)
            for job in jobs:
                job_images.append(index[k:k + len(job)])
                k += len(job)
            out = self.enrol_slots(parts, job_images, gallery)
            # the one synchronisation of the batch
            status, pair, avg, dup_pos = read_back(self.device, out["status"], out["pair"], out["avg"], out["dup_pos"])
        for j in range(len(jobs)):
            st = int(status[j])
            r = {"status": STATUS_NAMES[st]}
            if st == ENROL_DIFFERENT:
                r["pair"] = (int(pair[j, 0]), int(pair[j, 1]))
            elif st in (ENROL_DONE, ENROL_DUPLICATE):
                r["embedding"] = avg[j].copy()
                if st == ENROL_DONE:
                    r["blob"] = pickle.dumps(r["embedding"])        # :393 gallery row format
                elif dup_pos[j] < N:
                    r["duplicate_id"] = gallery.ids[int(dup_pos[j])]
                else:
                    r["duplicate_of_job"] = int(dup_pos[j]) - N
                    r["duplicate_id"] = ids[r["duplicate_of_job"]] if ids is not None else None
            result.append(r)
        if commit:
            done = [j for j in range(len(jobs)) if int(status[j]) == ENROL_DONE]
            if done:
                rows = out["avg"][torch.tensor(done, device=self.device)]
                gallery.gallery.upsert([ids[j] for j in done], rows, normalise=True)
            have = set(gallery.ids)
            result.view = gallery.gallery.view(list(gallery.ids) + [ids[j] for j in done if ids[j] not in have])
        return result


def first_above(lib, matcher, embedding, thr, inclusive):
    """Lowest gallery row whose dot with the L2-normalised query passes the threshold.  ``matcher``: a GalleryMatcher, or
    a GalleryView (position in the view's order; scanned through its slot list by the blocked entry)."""
    src = matcher.row_source()
    q = torch.from_numpy(np.asarray(embedding, np.float32).reshape(1, DIM)).to(matcher.device)
    qn = torch.empty_like(q)
    idx = torch.empty(1, dtype=torch.int64, device=matcher.device)
    score = torch.empty(1, dtype=torch.float32, device=matcher.device)
    ws = torch.empty(8, dtype=torch.uint8, device=matcher.device)
    with torch.cuda.device(matcher.device):
        s = _lib.stream_ptr()
        lib.fr_l2norm_rows_f32(_lib.ptr(q), _lib.ptr(qn), 1, DIM, s)
        tail = (1, src.N, DIM, float(thr), 1 if inclusive else 0, 0, _lib.ptr(idx), _lib.ptr(score), _lib.ptr(ws), 8, s)
        if src.view is None:
            lib.fr_gallery_first_above_f32(_lib.ptr(qn), _lib.ptr(src.G), *tail)
        else:
            lib.fr_gallery_first_above_blocked_f32(_lib.ptr(qn), _lib.ptr(src.G), _lib.ptr(src.view), None, *tail)
    return int(idx.item()), float(score.item())


class EnrolBatchResult(list):
    """What ``Enroller.enrol_batch`` returns: the list of per-job dicts; ``view`` is the GalleryView that holds the rows
    a ``commit=True`` call enrolled (None without a commit)."""
    view = None


class UnknownClusters:
    """peopleCount.py:52-91 + :432-449 on the device: cluster means live in one [C,512] matrix (NOT unit rows,
    exactly as the reference keeps them); assignment = first cluster with dot(avg, e) >= threshold.

    All of the state is on the device - the means, the ``depth``-deep rings they are the mean of, and the counters
    (include/frhip.h fr_unknown_assign_batch_f32) - and a whole batch of faces is assigned, in the reference's
    sequential order, by ONE launch with no host synchronisation (``assign_batch``)."""

    STATE_N, STATE_OVERFLOW, STATE_HEADER = 0, 1, 4         # include/frhip.h FR_UNKNOWN_*

    def __init__(self, device="cuda:0", threshold=0.65, depth=10, capacity=1024):
        _lib.require_gpu()
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.threshold, self.depth, self.capacity = threshold, int(depth), int(capacity)
        if self.depth < 1 or self.capacity < 1:
            raise ValueError("UnknownClusters needs depth >= 1 and capacity >= 1")
        self.avg = torch.zeros((self.capacity, DIM), dtype=torch.float32, device=self.device)
        self._hist = torch.zeros((self.capacity, self.depth, DIM), dtype=torch.float32, device=self.device)
        self._state = torch.zeros(self.STATE_HEADER + 3 * self.capacity, dtype=torch.int32, device=self.device)

    def assign_batch(self, E, take=None):
        """Rows of ``E`` (device or host float32 [F,512]) in order; ``take``: optional device int32 / bool [F], rows whose
        entry is 0 are skipped.  Returns three device int32 [F] tensors: the cluster index of each row (-1: not taken,
        -2: refused because all ``capacity`` clusters exist - see ``overflowed``), 1 where the row created its cluster,
        and the cluster's detection count after the row.  One launch on the current stream, no host synchronisation."""
        if not torch.is_tensor(E):
            E = torch.from_numpy(np.ascontiguousarray(np.asarray(E, np.float32)))
        E = E.to(self.device, torch.float32).reshape(-1, DIM).contiguous()
        F = E.shape[0]
        if take is not None:
            take = torch.as_tensor(take).to(self.device, torch.int32).reshape(-1).contiguous()
            if take.shape[0] != F:
                raise ValueError(f"take has {take.shape[0]} entries for {F} rows")
        cluster, is_new, count = (torch.empty(F, dtype=torch.int32, device=self.device) for _ in range(3))
        with torch.cuda.device(self.device):
            self.lib.fr_unknown_assign_batch_f32(_lib.ptr(E), _lib.ptr(take), F, DIM, float(self.threshold),
                                                 _lib.ptr(self.avg), _lib.ptr(self._hist), _lib.ptr(self._state),
                                                 self.capacity, self.depth, _lib.ptr(cluster), _lib.ptr(is_new),
                                                 _lib.ptr(count), _lib.stream_ptr())
        return cluster, is_new, count

    def assign(self, embedding):
        """One embedding -> its cluster index (``assign_batch`` of one row and one read-back)."""
        hit = int(self.assign_batch(np.asarray(embedding, np.float32).reshape(1, DIM))[0].item())
        if hit == -2:
            raise RuntimeError("UnknownClusters capacity exceeded")
        return hit

    @property
    def overflowed(self):
        """Rows refused so far because the bank was full (sticky)."""
        return int(self._state[self.STATE_OVERFLOW].item())

    def _counters(self):
        s = self._state.cpu().numpy()
        n = int(s[self.STATE_N])
        return n, s[self.STATE_HEADER:self.STATE_HEADER + 3 * n].reshape(n, 3)

    @property
    def counts(self):
        """detection_count per cluster (a copy from the device)."""
        return [int(c) for c in self._counters()[1][:, 2]]

    @property
    def hist(self):
        """Per cluster, the rows of its ring oldest first (a copy from the device): a list of float32 [K,512] arrays."""
        n, c = self._counters()
        rows = self._hist[:n].cpu().numpy()
        out = []
        for k in range(n):
            length, head = int(c[k, 0]), int(c[k, 1])
            start = head if length == self.depth else 0
            out.append(rows[k, [(start + j) % self.depth for j in range(length)]])
        return out
