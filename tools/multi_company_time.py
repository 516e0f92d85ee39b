"""Times one camera turn of a multi-company server: 8 companies x 8 cameras, 64 seeded 640x480 frames, a 10 k-row
gallery split evenly between the companies (synthetic weights, the engine as FaceAnalysis.prepare() makes it).
  (a) one mixed call: recognize_batch(frames, [one company id per frame]) - one engine pass, one grouped scan;
  (b) what there was before: eight recognize_batch calls of 8 frames, one per company.
Both end in their own host synchronisation; (a) and (b) alternate inside one loop, median of 20 turns after 3 warm-ups,
a device synchronise around each timed region, ms per turn of 64 frames.  The answers of (a) and (b) are compared first.
The scan alone, on the turn's own query slots: the grouped scan (with the face counts as padding marks, as
recognize_batch runs it, and without) against eight view.match_device calls over the same slots.
The condition is (a) <= (b); the size of the gain is a figure.
Usage: python tools/multi_company_time.py [OUT.txt]"""
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from facerecognition_infrenceengine_amd import FaceAnalysis                                               # noqa: E402
from facerecognition_infrenceengine_amd.processor import (EmbeddingManager, FaceRecognitionProcessor,     # noqa: E402
                                                          InMemoryStore, _detect_embed_batch)
from make_golden import synth_frame                                                                       # noqa: E402

COMPANIES, CAMERAS, ROWS, RUNS, WARM = 8, 8, 10_000, 20, 3


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(fns, runs=RUNS, warm=WARM):
    """median / min / max ms of each function, the functions taking turns inside one loop"""
    for _ in range(warm):
        for fn in fns:
            fn()
    ts = [[] for _ in fns]
    for _ in range(runs):
        for k, fn in enumerate(fns):
            ts[k].append(timed(fn))
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        app = FaceAnalysis(name="buffalo_l").prepare(ctx_id=0)
    names = [f"company{c}" for c in range(COMPANIES)]
    frames = [synth_frame(480, 640, 100 + s) for s in range(COMPANIES * CAMERAS)]
    ids = [names[s // CAMERAS] for s in range(len(frames))]
    rng = np.random.default_rng(7)
    store = InMemoryStore()
    for i in range(ROWS):
        store.add_employee(f"e{i}", names[i % COMPANIES], rng.standard_normal(512).astype(np.float32), name=f"E{i}")
    for c in range(COMPANIES):                               # somebody to recognise: the faces of each company's first camera
        for j, f in enumerate(app.get(frames[c * CAMERAS])):
            store.add_employee(f"face{c}_{j}", names[c], f.embedding, name=f"F{c}{j}")
    mgr = EmbeddingManager(store=store, device="cuda:0")
    proc = FaceRecognitionProcessor(mgr, face_detector=app)

    def mixed():
        return proc.recognize_batch(frames, ids)

    def one_by_one():
        out = []
        for c in range(COMPANIES):
            out += proc.recognize_batch(frames[c * CAMERAS:(c + 1) * CAMERAS], names[c])
        return out

    a, b = mixed(), one_by_one()
    faces = sum(len(f) for f in a)
    known = sum(r["person_id"] is not None for f in a for r in f)
    # (a) embeds 64 frames' faces in one forward, (b) eight frames' at a time: the embed net picks its kernels by the number
    # of faces, so scores agree to f16-conv rounding (5e-4) and a face whose score lies that close to the threshold may
    # be decided either way.  Boxes and detector scores must be equal; ids wherever the score is clear of the threshold.
    thr = proc.recognition_threshold
    for x, y in zip(a, b):
        assert len(x) == len(y), "the mixed call and the per-company calls find different faces"
        for p, q in zip(x, y):
            assert np.array_equal(p["bbox"], q["bbox"]) and p["det_score"] == q["det_score"]
            sp, sq = float(p["recognition_score"]), float(q["recognition_score"])
            if p["person_id"] is not None and q["person_id"] is not None:
                assert p["person_id"] == q["person_id"] and abs(sp - sq) < 5e-4, "the two ways name different people"
            elif p["person_id"] is not None or q["person_id"] is not None:
                assert abs(max(sp, sq) - thr) < 5e-4, "a face clear of the threshold is decided differently"
    lines = [f"multi-company turn: {COMPANIES} companies x {CAMERAS} cameras, 640x480, {ROWS} gallery rows split evenly, "
             f"{faces} faces ({known} recognised, same boxes and ids both ways); median of {RUNS} after {WARM} warm-ups "
             f"(min .. max), ms per turn of {len(frames)} frames, (a) and (b) alternating"]
    fmt = lambda t: f"{t[0]:10.3f} ({t[1]:.3f} .. {t[2]:.3f})"                                            # noqa: E731
    ta, tb = alternate([mixed, one_by_one])
    lines += [f"(a) one mixed recognize_batch of 64 frames      {fmt(ta)}   {len(frames) / ta[0] * 1e3:8.0f} frames/s",
              f"(b) eight recognize_batch calls of 8 frames     {fmt(tb)}   {len(frames) / tb[0] * 1e3:8.0f} frames/s",
              f"(b) / (a) = {tb[0] / ta[0]:.2f}   {'(a) <= (b): ok' if ta[0] <= tb[0] else '(a) NOT below (b)'}"]
    # the scan alone, on this turn's query slots
    n, r = _detect_embed_batch(proc, app, frames)
    Q, counts, cap = r["normed_embedding"], r["counts"], r["bbox"].shape[1]
    view_set, _, index_of = mgr.get_matchers_for_companies(ids)
    parts = [Q[c * CAMERAS * cap:(c + 1) * CAMERAS * cap].contiguous() for c in range(COMPANIES)]
    torch.cuda.synchronize()
    tg, tn, tv = alternate([lambda: view_set.match_device(Q, index_of, counts=counts, seg_len=cap),
                            lambda: view_set.match_device(Q, index_of, seg_len=cap),
                            lambda: [view_set.views[c].match_device(parts[c]) for c in range(COMPANIES)]])
    lines += [f"scan alone, {Q.shape[0]} query slots ({cap} per frame), views of {len(view_set.views[0])} rows:",
              f"    grouped scan, face counts as padding marks  {fmt(tg)}",
              f"    grouped scan, every slot scanned            {fmt(tn)}",
              f"    eight view.match_device calls               {fmt(tv)}   / grouped (all slots) = {tv[0] / tn[0]:.2f}"]
    for line in lines:
        print(line, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ta[0] <= tb[0] else 1


if __name__ == "__main__":
    sys.exit(main())
