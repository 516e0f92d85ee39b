"""Times the judging face tracks on one MI355X; writes profiles/track_quality.txt.  Medians of 30 turns after 3
warm-ups, the variants alternating in one process (the helpers of tools/quality_time.py).

  1. the launches alone on the C2 shape, 64 frames x 4 detection slots, 32 entries per camera, HIP events round each:
     fr_track_resolve_quality_i32 through FaceTracks.resolve_device; beside it, in the same session, the associate + commit pair,
     fr_warp_affine_5pt_slots over all 256 slots of 64 x 1080p frames and fr_face_quality_f16 over the same slots - the three
     things a judging call may cost over a tracks-only call when every face is accepted.
  2. FaceRecognitionProcessor.recognize_batch of 64 x 1080p host frames, the same frames every turn (synthetic weights, cap_o = 4,
     a 10 000-row gallery), wall time of the whole call per turn:
       tracks only                      FaceTracks() of this tree
       judging tracks, accepting all    FaceTracks(quality=accept-all): the tracks-only result, bit for bit
       judging tracks, half unfit       every other turn sharp_min is the median sharpness of these frames' faces
     with the faces embedded, carried and rejected per turn as FaceTracks.stats counted them.

``--plain-only --root TREE`` times the tracks-only call alone with the package of another checkout (the parent commit, built), in a
process of its own: the two trees must agree on that call within its own spread.

The condition, printed, not asserted: accepting all may cost the slot warp, the quality launch and the resolve launch of part 1
over tracks-only, and no more than that beyond the tracks-only call's own min-to-max spread in this run.
Not measured: real video, the defaults' error rates.
Usage: python tools/track_quality_time.py [--frames 64] [--reps 30] [--out profiles/track_quality.txt] [--plain-only --root TREE]"""
import argparse
import os
import statistics
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
from quality_time import H, TEMPLATE, W, WARM, alternate                                        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "track_quality.txt"))
    ap.add_argument("--root", default=HERE, help="the checkout whose package is timed")
    ap.add_argument("--plain-only", action="store_true", help="the tracks-only call alone (a tree without the feature)")
    a = ap.parse_args()
    assert a.reps >= 30, "medians of at least 30"
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests", "golden"))
    from facerecognition_infrenceengine_amd import FaceAnalysis, FaceTracks, _lib
    from facerecognition_infrenceengine_amd.processor import EmbeddingManager, FaceRecognitionProcessor, InMemoryStore
    from make_golden import synth_frame
    N, dev = a.frames, torch.device("cuda:0")
    lines = [f"judging face tracks: {N} x {H} x {W} frames, medians of {a.reps} turns after {WARM} warm-ups, variants alternating in "
             f"one process", f"device: {torch.cuda.get_device_name(0)}",
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
    tr = {"tracks only                  ": plain}
    variants = {"tracks only                  ": lambda: proc.recognize_batch(frames, "acme", tracks=plain, camera_ids=cams)}
    alone_sum = None

    if not a.plain_only:
        from facerecognition_infrenceengine_amd import FaceQuality
        inf = float("inf")
        accept = dict(min_eye=0, mean_lo=0, mean_hi=255, contrast_min=0, sharp_min=0, clip_max=6400, yaw_max=inf, pitch_lo=-inf,
                      pitch_hi=inf)
        q_all = FaceQuality(**accept)
        # ---- 1. the launches alone
        cap, lib = 4, _lib.load()
        S = N * cap
        d_frames = torch.from_numpy(np.stack(frames)).to(dev)
        g = np.random.default_rng(2)
        kps = (TEMPLATE[None, None] * g.uniform(1.0, 4.0, (N, cap, 1, 1)) + g.uniform(0, 1, (N, cap, 1, 2)) * [W - 500, H - 500])
        kps = torch.from_numpy(kps.astype(np.float32)).to(dev).contiguous()
        xy = torch.rand((N, cap, 2), generator=torch.Generator().manual_seed(2)) * torch.tensor([W - 200.0, H - 200.0])
        boxes = torch.cat([xy, xy + 120.0], dim=2).contiguous().to(dev)
        counts = torch.full((N,), cap, dtype=torch.int32, device=dev)
        crops = torch.empty((S, 112, 112, 8), dtype=torch.float16, device=dev)
        emb = torch.randn((S, 512), device=dev)
        normed = torch.nn.functional.normalize(emb, dim=1)
        alone = FaceTracks(dev, slots=N, quality=q_all)
        entry, need, tid = alone.associate_device(boxes, counts, cams)
        verdict = torch.zeros((N, cap), dtype=torch.int32, device=dev)
        keep = []

        def pair():
            e, n, _ = alone.associate_device(boxes, counts, cams)
            alone.commit_device(e, n, counts, cams, emb, normed)

        def resolve():
            keep[:] = alone.resolve_device(entry, need, tid, verdict, counts, cams)

        def warp():
            lib.fr_warp_affine_5pt_slots(_lib.ptr(d_frames), N, H, W, _lib.ptr(kps), _lib.ptr(counts), cap, 112, _lib.ptr(crops),
                                         _lib.stream_ptr())

        def quality():
            keep[:] = q_all.measure_device(crops, kps, counts, cap)
        warp()
        t = alternate({"fr_track_resolve_quality_i32     ": resolve, "fr_track_associate + _commit_f32 ": pair,
                       "fr_warp_affine_5pt_slots         ": warp, "fr_face_quality_f16              ": quality}, a.reps)
        say(f"1. the launches alone, {N} frames x {cap} detection slots ({S} slots, every one holding a face), {alone.entries} entries "
            f"per camera, HIP events round each")
        for k, v in t.items():
            row(k, v, "us", 1e3)
        alone_sum = sum(statistics.median(t[k]) for k in t if not k.startswith("fr_track_associate"))
        say(f"   slot warp + quality launch + resolve launch, medians: {alone_sum * 1e3:.1f} us")
        say()
        # ---- 2. the call
        d = app.detect_embed_slots(torch.from_numpy(np.stack(base)).to(dev), compact_embed=True, quality=q_all)
        cnt = d["counts"].cpu().numpy()
        sharp = np.concatenate([d["quality"][f, :cnt[f], 2].cpu().numpy() for f in range(len(base))])
        q_half = FaceQuality(**dict(accept, sharp_min=int(np.median(sharp))))
        all_t, half_t = FaceTracks(dev, slots=N, quality=q_all), FaceTracks(dev, slots=N, quality=q_all)
        tr["judging tracks, accepting all"], tr["judging tracks, half unfit   "] = all_t, half_t
        turn = [0]

        def half():
            turn[0] += 1
            half_t.quality = q_half if turn[0] % 2 == 0 else q_all
            proc.recognize_batch(frames, "acme", tracks=half_t, camera_ids=cams)
        variants["judging tracks, accepting all"] = lambda: proc.recognize_batch(frames, "acme", tracks=all_t, camera_ids=cams)
        variants["judging tracks, half unfit   "] = half

    t = alternate(variants, a.reps, wall=True)
    turns = a.reps + WARM
    say(f"2. recognize_batch, {N} x 1080p host frames per turn, the same frames every turn (synthetic weights, cap_o 4, 10 000 gallery "
        f"rows), wall time of the call;")
    say(f"   defaults iou_thr {plain.iou_thr}, max_reuse {plain.max_reuse}, max_misses {plain.max_misses}" +
        ("" if a.plain_only else f", max_age {all_t.max_age}; half unfit: sharp_min = {q_half.sharp_min} on every other turn"))
    for k, v in t.items():
        s = tr[k].stats
        row(k, v, tail=f"; per turn {s['faces'] / turns / N:.2f} faces/frame, {s['embedded'] / turns:.1f} embedded, "
            f"{s['carried'] / turns:.1f} carried" + (f", {s['rejected'] / turns:.1f} rejected" if "rejected" in s else ""))
    un = t["tracks only                  "]
    spread = max(un) - min(un)
    say(f"   the tracks-only call, its own spread: {spread:.3f} ms")
    if not a.plain_only:
        extra = statistics.median(t["judging tracks, accepting all"]) - statistics.median(un)
        say(f"   accepting all - tracks only: {extra:+.3f} ms; allowed: the launches of part 1, {alone_sum:.3f} ms, beyond them the "
            f"spread above: {'within' if extra <= alone_sum + spread else 'NOT within'}")
    say()
    say("the call is bound by the host's copy of the frames into the pinned ring and the link, not by the engine pass")
    say("not measured: real video, the error rates of the defaults")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
