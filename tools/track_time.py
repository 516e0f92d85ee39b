"""Times the face tracks on one MI355X; writes profiles/face_tracks.txt.  Medians of 30 turns after 3 warm-ups,
the variants alternating in one process (as tools/activity_gate_time.py, whose wall-time helper this uses).

  1. the two launches alone (fr_track_associate_f32, fr_track_commit_f32 through FaceTracks) on the C2 shape, 64 frames x 4
     detection slots, HIP events round both; beside them one small device-to-host copy with its synchronisation.
  2. FaceRecognitionProcessor.recognize_batch of 64 x 1080p host frames (synthetic weights, cap_o = 4, a 10 000-row gallery), wall
     time of the whole call per turn:
       untracked                   the code path of a call without tracks
       tracked, max_reuse = 0      every face embedded: the two launches and the host work round them, nothing saved
       tracked, 100 % persistent   the same frames every turn (default max_reuse = 4: one turn in five embeds everything)
       tracked,  75 % persistent   one frame in four shows its other picture each turn, the rest repeat
     with the faces embedded and carried per turn as FaceTracks.stats counted them.  The mean is given beside the median: the
     persistent variants alternate between cheap turns and an embedding turn.

No pass mark, nothing here is asserted in a test.  Not measured: real video (how much of a scene persists, how often faces touch),
the defaults' error rates, the camera loop with capture threads.
Usage: python tools/track_time.py [--frames 64] [--reps 30] [--out profiles/face_tracks.txt]"""
import argparse
import os
import statistics
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from activity_gate_time import WARM, wall_alternate                                            # noqa: E402
from det_size_ab import alternate                                                              # noqa: E402

H, W = 1080, 1920


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "face_tracks.txt"))
    a = ap.parse_args()
    assert a.reps >= 30, "medians of at least 30"
    from facerecognition_infrenceengine_amd import FaceAnalysis, FaceTracks
    from facerecognition_infrenceengine_amd.processor import EmbeddingManager, FaceRecognitionProcessor, InMemoryStore
    from make_golden import synth_frame
    N, dev = a.frames, torch.device("cuda:0")
    lines = [f"face tracks: {N} x {H} x {W} frames, medians of {a.reps} turns after {WARM} warm-ups, variants alternating in one process",
             f"device: {torch.cuda.get_device_name(0)}", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    base = [synth_frame(H, W, 900 + i) for i in range(16)]
    set_a, set_b = [base[i % 8] for i in range(N)], [base[8 + i % 8] for i in range(N)]
    cams = list(range(N))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        app = FaceAnalysis(name="synthetic", arch="r100", cap_o=4).prepare(ctx_id=0)
    r = np.random.default_rng(1)
    store = InMemoryStore()
    for i in range(10000):
        store.add_employee(f"n{i}", "acme", r.standard_normal(512).astype(np.float32), name=f"N{i}")
    proc = FaceRecognitionProcessor(EmbeddingManager(store=store, device="cuda:0"), face_detector=app)

    # ---- 1. the two launches alone, on detections of the shape the batch path hands them
    cap = 4
    g = torch.Generator().manual_seed(2)
    xy = torch.rand((N, cap, 2), generator=g) * torch.tensor([W - 200.0, H - 200.0])
    boxes = torch.cat([xy, xy + 120.0], dim=2).contiguous().to(dev)
    counts = torch.full((N,), cap, dtype=torch.int32, device=dev)
    emb = torch.randn((N * cap, 512), device=dev)
    normed = torch.nn.functional.normalize(emb, dim=1)
    alone = FaceTracks(dev, slots=N)

    def launches():
        entry, need, _ = alone.associate_device(boxes, counts, cams)
        alone.commit_device(entry, need, counts, cams, emb, normed)
    probe = torch.zeros(N * (2 * cap + 1), dtype=torch.int32, device=dev)
    med, rng = alternate({"launches": launches}, a.reps, warmup=WARM)
    sync_s = statistics.median(wall_alternate({"sync": lambda: probe.cpu()}, a.reps)["sync"])
    say(f"1. the two launches alone, {N} frames x {cap} detection slots, {alone.entries} entries per camera (HIP events round both)")
    say(f"   fr_track_associate_f32 + fr_track_commit_f32 via FaceTracks: {med['launches'] * 1e3:7.1f} us "
        f"(min {rng['launches'][0] * 1e3:.1f}, max {rng['launches'][1] * 1e3:.1f})")
    say(f"   one small device-to-host copy with its synchronisation (wall): {sync_s * 1e6:.1f} us")
    say()

    # ---- 2. recognize_batch, untracked against tracked
    def tracked(tracks, swap):
        state = {"turn": 0, "frames": list(set_a), "shown": [0] * N}

        def turn():
            state["turn"] += 1
            if swap:                                             # cameras with i % swap == turn % swap show their other picture
                for i in range(state["turn"] % swap, N, swap):
                    state["shown"][i] ^= 1
                    state["frames"][i] = (set_a, set_b)[state["shown"][i]][i]
            proc.recognize_batch(state["frames"], "acme", tracks=tracks, camera_ids=cams)
        return turn
    tr = {"tracked, max_reuse = 0   ": (FaceTracks(dev, slots=N, max_reuse=0), 0),
          "tracked, 100 % persistent": (FaceTracks(dev, slots=N), 0),
          "tracked,  75 % persistent": (FaceTracks(dev, slots=N), 4)}
    variants = {"untracked                ": lambda: proc.recognize_batch(set_a, "acme")}
    variants.update({k: tracked(t, swap) for k, (t, swap) in tr.items()})
    t = wall_alternate(variants, a.reps)
    turns = a.reps + WARM
    say(f"2. recognize_batch, {N} x 1080p host frames per turn (synthetic weights, cap_o 4, 10 000 gallery rows), wall time of the call;")
    say(f"   defaults iou_thr {alone.iou_thr}, max_reuse {alone.max_reuse}, max_misses {alone.max_misses}")
    for k, v in t.items():
        m = statistics.median(v)
        line = (f"   {k}: median {m * 1e3:8.3f} ms, mean {statistics.fmean(v) * 1e3:8.3f} ms per turn (min {min(v) * 1e3:.3f}, "
                f"max {max(v) * 1e3:.3f})")
        if k in tr:
            s = tr[k][0].stats
            line += (f"; per turn {s['faces'] / turns / N:.2f} faces/frame, {s['embedded'] / turns:.1f} embedded, "
                     f"{s['carried'] / turns:.1f} carried, {s['untracked'] / turns:.1f} untracked")
        say(line)
    un, zero = t["untracked                "], t["tracked, max_reuse = 0   "]
    extra = statistics.median(zero) - statistics.median(un)
    say(f"   tracked with max_reuse = 0 - untracked: {extra * 1e3:+.3f} ms (the untracked call's own spread: "
        f"{(max(un) - min(un)) * 1e3:.3f} ms; the launches alone: {med['launches']:.3f} ms)")
    say()
    say("not measured: real video (how much of a scene persists, how often faces touch), the error rates of the defaults, the camera")
    say("loop with capture threads")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
