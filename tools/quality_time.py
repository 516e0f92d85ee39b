"""Times face quality on one MI355X; writes profiles/face_quality.txt.  Medians of 30 turns after 3 warm-ups,
the variants alternating in one process (as tools/track_time.py, whose helpers this uses).

  1. fr_face_quality_f16 alone at 1024 slots (64 frames x 16 slots, every slot holding a face), HIP events round the launch;
     beside it, in the same session, fr_warp_affine_5pt_slots over the same slots of 64 x 1080p frames - the launch that writes
     the crops the quality launch reads, so the yardstick for a kernel that moves 108 KB per face.
  2. FaceRecognitionProcessor.recognize_batch of 64 x 1080p host frames (synthetic weights, cap_o = 4, a 10 000-row gallery), wall
     time of the whole call per turn:
       without quality             the code path of a call without the argument
       quality, accepting all      every face aligned in its slot, judged and embedded
       quality, rejecting half     sharp_min = the median sharpness of these frames' faces: about half are not embedded

``--plain-only --root TREE`` times the call without quality alone with the package of another checkout (the parent commit, built),
in a process of its own: the two trees must agree on that call within its own spread.

No pass mark, nothing here is asserted in a test.  Not measured: real video, and real faces against the default thresholds.
Usage: python tools/quality_time.py [--frames 64] [--reps 30] [--out profiles/face_quality.txt] [--plain-only --root TREE]"""
import argparse
import os
import statistics
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 1080, 1920
WARM = 3
TEMPLATE = np.array([[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366], [41.5493, 92.3655], [70.7299, 92.2041]], np.float32)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(variants, reps, wall=False):
    """{name: fn} -> {name: [ms]}: the variants take turns inside every repetition; HIP events, or the wall time of whole calls"""
    import time
    for _ in range(WARM):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            if wall:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                t[k].append((time.perf_counter() - t0) * 1e3)
            else:
                t[k].append(timed(fn))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "face_quality.txt"))
    ap.add_argument("--root", default=HERE, help="the checkout whose package is timed")
    ap.add_argument("--plain-only", action="store_true", help="the call without quality alone (a tree without the feature)")
    a = ap.parse_args()
    assert a.reps >= 30, "medians of at least 30"
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests", "golden"))
    from facerecognition_infrenceengine_amd import FaceAnalysis, _lib
    from facerecognition_infrenceengine_amd.processor import EmbeddingManager, FaceRecognitionProcessor, InMemoryStore
    from make_golden import synth_frame
    N, dev = a.frames, torch.device("cuda:0")
    lines = [f"face quality: {N} x {H} x {W} frames, medians of {a.reps} turns after {WARM} warm-ups, variants alternating in one process",
             f"device: {torch.cuda.get_device_name(0)}", f"tree: {'this one' if root == HERE else 'another checkout (--root)'}", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def row(k, v, unit="ms", scale=1.0):
        say(f"   {k}: median {statistics.median(v) * scale:9.3f} {unit} (min {min(v) * scale:.3f}, max {max(v) * scale:.3f})")

    base = [synth_frame(H, W, 900 + i) for i in range(8)]
    frames = [base[i % 8] for i in range(N)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        app = FaceAnalysis(name="synthetic", arch="r100", cap_o=4).prepare(ctx_id=0)
    r = np.random.default_rng(1)
    store = InMemoryStore()
    for i in range(10000):
        store.add_employee(f"n{i}", "acme", r.standard_normal(512).astype(np.float32), name=f"N{i}")
    proc = FaceRecognitionProcessor(EmbeddingManager(store=store, device="cuda:0"), face_detector=app)
    variants = {"without quality        ": lambda: proc.recognize_batch(frames, "acme")}

    if not a.plain_only:
        from facerecognition_infrenceengine_amd import FaceQuality
        inf = float("inf")
        accept = dict(min_eye=0, mean_lo=0, mean_hi=255, contrast_min=0, sharp_min=0, clip_max=6400, yaw_max=inf, pitch_lo=-inf,
                      pitch_hi=inf)
        q_all = FaceQuality(**accept)
        # ---- 1. the launch alone, beside the launch that writes its input
        cap, lib = 16, _lib.load()
        S = N * cap
        d_frames = torch.from_numpy(np.stack(frames)).to(dev)
        g = np.random.default_rng(2)
        kps = (TEMPLATE[None, None] * g.uniform(1.0, 4.0, (N, cap, 1, 1)) + g.uniform(0, 1, (N, cap, 1, 2)) * [W - 500, H - 500])
        kps = torch.from_numpy(kps.astype(np.float32)).to(dev).contiguous()
        counts = torch.full((N,), cap, dtype=torch.int32, device=dev)
        crops = torch.empty((S, 112, 112, 8), dtype=torch.float16, device=dev)

        def warp():
            lib.fr_warp_affine_5pt_slots(_lib.ptr(d_frames), N, H, W, _lib.ptr(kps), _lib.ptr(counts), cap, 112, _lib.ptr(crops),
                                         _lib.stream_ptr())
        warp()
        keep = []

        def quality():
            keep[:] = q_all.measure_device(crops, kps, counts, cap)
        t = alternate({"fr_face_quality_f16     ": quality, "fr_warp_affine_5pt_slots": warp}, a.reps)
        say(f"1. the launches alone, {S} slots ({N} frames x {cap}, every slot holding a face), HIP events round each launch")
        for k, v in t.items():
            row(k, v, "us", 1e3)
        mq = statistics.median(t["fr_face_quality_f16     "])
        say(f"   the quality launch reads {S * 82 * 82 * 16 / 1e6:.1f} MB (window plus ring, 16 bytes a pixel): "
            f"{S * 82 * 82 * 16 / 1e9 / (mq * 1e-3):.0f} GB/s")
        say()
        # ---- 2. the call: a sharp_min that rejects about half of these frames' faces
        d = app.detect_embed_slots(torch.from_numpy(np.stack(base)).to(dev), compact_embed=True, quality=q_all)
        cnt = d["counts"].cpu().numpy()
        sharp = np.concatenate([d["quality"][f, :cnt[f], 2].cpu().numpy() for f in range(len(base))])
        q_half = FaceQuality(**dict(accept, sharp_min=int(np.median(sharp))))
        rejected = int((sharp < q_half.sharp_min).sum()) * (N // len(base))
        variants["quality, accepting all "] = lambda: proc.recognize_batch(frames, "acme", quality=q_all)
        variants["quality, rejecting half"] = lambda: proc.recognize_batch(frames, "acme", quality=q_half)

    t = alternate(variants, a.reps, wall=True)
    say(f"2. recognize_batch, {N} x 1080p host frames per turn (synthetic weights, cap_o 4, 10 000 gallery rows), wall time of the call")
    for k, v in t.items():
        row(k, v)
    un = t["without quality        "]
    say(f"   the call without quality, its own spread: {max(un) - min(un):.3f} ms")
    if not a.plain_only:
        say(f"   faces per turn: {int(cnt.sum()) * (N // len(base))}; rejected by sharp_min = {q_half.sharp_min}: {rejected}")
    say()
    say("not measured: real video, and real faces against the default thresholds")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
