"""A/B of ``det_size``: what the detection canvas costs and what it saves.

One process, after warm-up, the variants alternating; every figure is a median of ``--reps`` HIP-event timings.
Writes ``profiles/det_size.txt`` (``--out``):

  1. fr_letterbox_u8 for 64 x 1080p -> (640, 640): kernel time against the bytes it must move (computed from the shapes);
  2. the detect stage alone on the same 64 seeded 1080p frames: det_size=None (full pyramid of the full frame, the unchanged
     path) against det_size=(640, 640) (letterbox + cascade on the canvas + unscale), with the per-level pixel counts;
  3. the step time of detect_embed_slots for the same two variants, and a 64-frame mixed batch (4K / 1080p / VGA) in ONE call
     under det_size against the sum of the three per-shape calls an engine without it needs.

    python tools/det_size_ab.py [--frames 64] [--reps 30]
"""
import argparse
import math
import os
import statistics
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

HBM_ACHIEVABLE = 6.3e12          # bytes/s a float4 copy reaches on MI355X (8 TB/s spec)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(variants, reps, warmup=3):
    """{name: fn} -> {name: median ms}; the variants take turns inside every repetition"""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            t[k].append(timed(fn))
    return {k: statistics.median(v) for k, v in t.items()}, {k: (min(v), max(v)) for k, v in t.items()}


def letterbox_bytes(shapes, det_size):
    """bytes fr_letterbox_u8 must move: per image row of the canvas the two source rows it blends (a row counted once when
    consecutive canvas rows share it), over the source columns in use; plus every byte of the canvas"""
    from facerecognition_infrenceengine_amd.letterbox import letterbox_geometry
    dw, dh = det_size
    rd = 0
    for h, w in shapes:
        nh, nw, _ = letterbox_geometry(h, w, det_size)
        ry = np.float32(h) / np.float32(nh)
        fy = (np.arange(nh, dtype=np.float32) + np.float32(0.5)) * ry - np.float32(0.5)
        y0 = np.floor(fy).astype(np.int64)
        rows = np.unique(np.clip(np.concatenate([y0, y0 + 1]), 0, h - 1)).size
        rd += rows * w * 3
    return rd, len(shapes) * dh * dw * 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det_size.txt"))
    a = ap.parse_args()
    assert a.reps >= 30, "medians of at least 30"
    from facerecognition_infrenceengine_amd import FaceAnalysis, _lib
    from facerecognition_infrenceengine_amd.mtcnn import pyramid_scales
    from make_golden import synth_frame
    N, DS = a.frames, (640, 640)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = FaceAnalysis(name="buffalo_l").prepare(ctx_id=0)
    canv = plain.clone_with(det_size=DS)
    lines = [f"det_size A/B: {N} frames, medians of {a.reps} HIP-event timings, variants alternating in one process",
             f"device: {torch.cuda.get_device_name(0)}", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    base = [synth_frame(1080, 1920, 900 + i) for i in range(8)]
    hd = torch.from_numpy(np.ascontiguousarray(np.stack([base[i % 8] for i in range(N)]))).cuda()

    # ---- 1. the letterbox kernel alone
    _, src = canv._source(hd)
    canvas = torch.empty((N, DS[1], DS[0], 3), dtype=torch.uint8, device="cuda")
    lib = canv.lib

    def lb():
        lib.fr_letterbox_u8(_lib.ptr(src.table), N, _lib.ptr(canvas), DS[1], DS[0], _lib.stream_ptr())
    med, rng = alternate({"letterbox": lb}, a.reps)
    rd, wr = letterbox_bytes([(1080, 1920)] * N, DS)
    us = med["letterbox"] * 1e3
    rate = (rd + wr) / (med["letterbox"] * 1e-3)
    say(f"1. fr_letterbox_u8, {N} x 1080p -> 640 x 640: {us:.1f} us (min {rng['letterbox'][0] * 1e3:.1f}, max {rng['letterbox'][1] * 1e3:.1f})")
    say(f"   bytes it must move: {rd / 1e6:.1f} MB read (source rows in use) + {wr / 1e6:.1f} MB written = {(rd + wr) / 1e6:.1f} MB")
    say(f"   -> {rate / 1e12:.2f} TB/s = {100 * rate / HBM_ACHIEVABLE:.0f} % of an achievable {HBM_ACHIEVABLE / 1e12:.1f} TB/s HBM rate; "
        f"time at that rate {(rd + wr) / HBM_ACHIEVABLE * 1e6:.0f} us.  Designed memory-bound: no matrix work, two 8-byte loads and three byte lerps per pixel.")
    say()

    # ---- 2. the detect stage alone
    def det_none():
        plain.det.detect_batch(hd)

    def det_canvas():
        _, s = canv._source(hd)
        canv._detect(hd, s)
    med, rng = alternate({"none": det_none, "canvas": det_canvas}, a.reps)

    def level_px(h, w, det):
        return [int(math.ceil(h * s)) * int(math.ceil(w * s)) for s in pyramid_scales(h, w, det.minsize, det.factor)]
    pf, pc = level_px(1080, 1920, plain.det), level_px(640, 640, canv.det)
    pimg = level_px(360, 640, canv.det)
    say(f"2. detect stage, {N} x 1080p: det_size=None {med['none']:.3f} ms (min {rng['none'][0]:.3f}, max {rng['none'][1]:.3f}); "
        f"det_size=(640, 640) {med['canvas']:.3f} ms (min {rng['canvas'][0]:.3f}, max {rng['canvas'][1]:.3f}): "
        f"{med['none'] / med['canvas']:.2f}x")
    say(f"   pyramid pixels per frame: full frame {sum(pf)} over {len(pf)} levels {pf}")
    say(f"   canvas {sum(pc)} over {len(pc)} levels {pc} (of which the 640 x 360 image {sum(pimg)}): "
        f"{sum(pf) / sum(pc):.2f}x fewer pixels on the canvas, {sum(pf) / sum(pimg):.2f}x on the image alone")
    say()

    # ---- 3. the step
    def step_none():
        plain.detect_embed_slots(hd)

    def step_canvas():
        canv.detect_embed_slots(hd)
    kinds = [(2160, 3840)] * (N // 8) + [(1080, 1920)] * (N // 2) + [(480, 640)] * (N - N // 8 - N // 2)
    mixed = [torch.from_numpy(synth_frame(h, w, 950 + i % 4)).cuda() for i, (h, w) in enumerate(kinds)]
    groups = {}
    for t in mixed:
        groups.setdefault(tuple(t.shape), []).append(t)
    stacks = [torch.stack(g) for g in groups.values()]

    def step_mixed():
        canv.detect_embed_slots(mixed)

    def step_groups():
        for s in stacks:
            plain.detect_embed_slots(s)
    med, rng = alternate({"none": step_none, "canvas": step_canvas, "mixed": step_mixed, "groups": step_groups}, a.reps)
    say(f"3. detect_embed_slots step, {N} x 1080p: det_size=None {med['none']:.3f} ms; det_size=(640, 640) {med['canvas']:.3f} ms: "
        f"{med['none'] / med['canvas']:.2f}x")
    say(f"   mixed batch ({', '.join(f'{len(g)} x {k[0]}x{k[1]}' for k, g in groups.items())}): ONE call under det_size "
        f"{med['mixed']:.3f} ms; {len(stacks)} per-shape calls without it {med['groups']:.3f} ms: {med['groups'] / med['mixed']:.2f}x")
    say("   (the two variants do not find the same faces: under det_size the minimum face is 20 canvas pixels, 60 frame pixels at 1080p)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
