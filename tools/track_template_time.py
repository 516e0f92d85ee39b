"""Times track templates on one MI355X; writes profiles/track_template.txt.  Medians of 30 turns after 3 warm-ups,
the variants alternating in one process (the helpers of tools/quality_time.py).

  1. the launches alone on the C2 shape, 64 frames x 4 detection slots, 32 entries per camera, depth 10, HIP events round each:
     fr_track_fuse_f32 through FaceTracks.fuse_device with every ring full - once with every face embedded (every wave joins: the
     dot, nine ring rows read, one written, the mean and the unit row) and once with every face carried (every wave reads its
     template) - and beside it, in the same session, fr_track_commit_f32 through FaceTracks.commit_device on the same columns.
  2. FaceRecognitionProcessor.recognize_batch of 64 x 1080p host frames, the same frames every turn (synthetic weights, cap_o = 4,
     a 10 000-row gallery), wall time of the whole call per turn:
       template=0     FaceTracks() of this tree
       template=10    FaceTracks(template=10)
     with the faces embedded and carried and the shots joined and restarted per turn as FaceTracks.stats counted them.

``--plain-only --root TREE`` times the template=0 call alone with the package of another checkout (the parent commit, built), in a
process of its own: the two trees must agree on that call within its own spread.

The condition, printed, not asserted: template=10 may cost the fuse launch of part 1 and the wider read-back over template=0, and
no more than that beyond the template=0 call's own min-to-max spread in this run.
Not measured: recognition accuracy on real video, the error rates of join_thr = 0.4 and of any depth.
Usage: python tools/track_template_time.py [--frames 64] [--reps 30] [--out profiles/track_template.txt] [--plain-only --root TREE]"""
import argparse
import os
import statistics
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
from quality_time import H, W, WARM, alternate                                                   # noqa: E402

DEPTH = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "track_template.txt"))
    ap.add_argument("--root", default=HERE, help="the checkout whose package is timed")
    ap.add_argument("--plain-only", action="store_true", help="the template=0 call alone (a tree without the feature)")
    a = ap.parse_args()
    assert a.reps >= 30, "medians of at least 30"
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests", "golden"))
    from facerecognition_infrenceengine_amd import FaceAnalysis, FaceTracks
    from facerecognition_infrenceengine_amd.processor import EmbeddingManager, FaceRecognitionProcessor, InMemoryStore
    from make_golden import synth_frame
    N, dev = a.frames, torch.device("cuda:0")
    lines = [f"track templates: {N} x {H} x {W} frames, medians of {a.reps} turns after {WARM} warm-ups, variants alternating in one "
             f"process", f"device: {torch.cuda.get_device_name(0)}",
             f"tree: {'this one' if root == HERE else 'another checkout (--root)'}", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def row(k, v, unit="ms", scale=1.0, tail=""):
        say(f"   {k}: median {statistics.median(v) * scale:9.3f} {unit}, mean {statistics.fmean(v) * scale:9.3f} "
            f"(min {min(v) * scale:.3f}, max {max(v) * scale:.3f}){tail}")

    base = [synth_frame(H, W, 900 + i) for i in range(8)]
    frames = [base[i % 8] for i in range(N)]
    cams = list(range(N))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        app = FaceAnalysis(name="synthetic", arch="r100", cap_o=4).prepare(ctx_id=0)
    r = np.random.default_rng(1)
    store = InMemoryStore()
    for i in range(10000):
        store.add_employee(f"n{i}", "acme", r.standard_normal(512).astype(np.float32), name=f"N{i}")
    proc = FaceRecognitionProcessor(EmbeddingManager(store=store, device="cuda:0"), face_detector=app)
    plain = FaceTracks(dev, slots=N)
    tr = {"template=0 ": plain}
    variants = {"template=0 ": lambda: proc.recognize_batch(frames, "acme", tracks=plain, camera_ids=cams)}
    fuse_us = None

    if not a.plain_only:
        # ---- 1. the launches alone
        cap = 4
        S = N * cap
        xy = torch.rand((N, cap, 2), generator=torch.Generator().manual_seed(2)) * torch.tensor([W - 200.0, H - 200.0])
        boxes = torch.cat([xy, xy + 120.0], dim=2).contiguous().to(dev)
        counts = torch.full((N,), cap, dtype=torch.int32, device=dev)
        emb = torch.randn((S, 512), device=dev)
        normed = torch.nn.functional.normalize(emb, dim=1)
        alone = FaceTracks(dev, slots=N, template=DEPTH, join_thr=0.4)
        entry, need, tid = alone.associate_device(boxes, counts, cams)          # every face takes an entry and is embedded
        carried = torch.zeros_like(need)
        keep = []
        for _ in range(DEPTH + 1):                                              # the same rows again and again: every shot joins
            keep[:] = alone.fuse_device(entry, need, tid, counts, cams, normed)
        torch.cuda.synchronize()
        assert int(alone.ttmpl[:, :cap, 0].min()) == DEPTH and int((keep[2] == 2).sum()) == S, "the rings are not full"

        def fuse_join():
            keep[:] = alone.fuse_device(entry, need, tid, counts, cams, normed)

        def fuse_read():
            keep[:] = alone.fuse_device(entry, carried, tid, counts, cams, normed)

        def commit():
            alone.commit_device(entry, need, counts, cams, emb, normed)
        t = alternate({"fr_track_fuse_f32, every face joins ": fuse_join, "fr_track_fuse_f32, every face carried": fuse_read,
                       "fr_track_commit_f32                  ": commit}, a.reps)
        assert int((keep[2] == 4).sum()) == S
        say(f"1. the launches alone, {N} frames x {cap} detection slots ({S} slots, every one holding a tracked face), {alone.entries} "
            f"entries per camera, depth {DEPTH}, rings full, HIP events round each (output allocation included)")
        for k, v in t.items():
            row(k, v, "us", 1e3)
        fuse_us = statistics.median(t["fr_track_fuse_f32, every face joins "])
        say(f"   a joining face moves {(DEPTH + 4) * 2} KB (in: the row, the template, {DEPTH - 1} ring rows; out: a ring row, the "
            f"template, the query): {S * (DEPTH + 4) * 2 / 1024:.1f} MB per launch here - what is timed is a launch's latency")
        say()
        # ---- 2. the call
        fused = FaceTracks(dev, slots=N, template=DEPTH)
        tr[f"template={DEPTH}"] = fused
        variants[f"template={DEPTH}"] = lambda: proc.recognize_batch(frames, "acme", tracks=fused, camera_ids=cams)

    t = alternate(variants, a.reps, wall=True)
    turns = a.reps + WARM
    say(f"2. recognize_batch, {N} x 1080p host frames per turn, the same frames every turn (synthetic weights, cap_o 4, 10 000 gallery "
        f"rows), wall time of the call;")
    say(f"   defaults iou_thr {plain.iou_thr}, max_reuse {plain.max_reuse}, max_misses {plain.max_misses}" +
        ("" if a.plain_only else f", join_thr {fused.join_thr}"))
    for k, v in t.items():
        s = tr[k].stats
        row(k, v, tail=f"; per turn {s['faces'] / turns / N:.2f} faces/frame, {s['embedded'] / turns:.1f} embedded, "
            f"{s['carried'] / turns:.1f} carried" +
            (f", {s['joined'] / turns:.1f} joined, {s['restarted'] / turns:.1f} restarted" if "joined" in s else ""))
    un = t["template=0 "]
    spread = max(un) - min(un)
    say(f"   the template=0 call, its own spread: {spread:.3f} ms")
    if not a.plain_only:
        extra = statistics.median(t[f"template={DEPTH}"]) - statistics.median(un)
        say(f"   template={DEPTH} - template=0: {extra:+.3f} ms; allowed: the fuse launch of part 1, {fuse_us:.3f} ms, and the wider "
            f"read-back, beyond them the spread above: {'within' if extra <= fuse_us + spread else 'NOT within'}"
            f"{'' if abs(extra) > spread else '; the difference is inside the spread: this run does not resolve it'}")
    say()
    say("the call is bound by the host's copy of the frames into the pinned ring and the link, not by the engine pass")
    say("not measured: recognition accuracy on real video, the error rates of join_thr = 0.4 and of any depth")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
