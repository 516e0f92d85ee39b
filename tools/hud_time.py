"""Times the device HUD on one MI355X; writes profiles/hud.txt.  Medians of 30 after 3 warm-ups, the variants
alternating in one process (as tools/activity_gate_time.py, whose wall clock helper this uses).

  1. the draw launch alone on 64 x 1080p frames with 4 faces each (scale 2), HIP events: fr_hud_draw_u8 and fr_hud_draw_refs_u8,
     beside fr_letterbox_u8 of the same frames to 640 x 360 and beside a device copy of the same frames, in the same session.
     The draw touches only the tiles inside HUD extents, so it is expected below the copy; reported either way, with the bytes
     of the pixels inside the extents (read and written once) over the time.
  2. FaceRecognitionProcessor.recognize_faces_batch of 64 x 1080p host frames (synthetic weights, cap_o = 4, a 1 000-row gallery),
     full size and with out_size = (640, 360), against recognize_batch alone and against recognize_batch followed by the host
     annotate loop (the plain box), wall time of the whole call; the device-to-host bytes of each path.
  3. --section parent: recognize_batch + the host annotate loop alone, with nothing this tool needs beyond what the tree before
     the HUD had - so the same file can be run on that tree, in a process of its own, for the comparison with the parent.

No pass mark, nothing here is asserted in a test.  Not measured: real video, a viewer behind the previews, YUV cameras.
Usage: python tools/hud_time.py [--frames 64] [--reps 30] [--section all|parent] [--out profiles/hud.txt]"""
import argparse
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

H, W, WARM = 1080, 1920, 3


def wall_alternate(variants, reps):
    """{name: fn} -> {name: [seconds]}: wall time of whole calls (they synchronise themselves), the variants taking turns"""
    for _ in range(WARM):
        for fn in variants.values():
            fn()
    t = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t[k].append(time.perf_counter() - t0)
    return t


def event_alternate(variants, reps):
    """{name: fn} -> {name: [milliseconds]}: HIP events round each launch, the variants taking turns"""
    for _ in range(WARM):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t[k].append(a.elapsed_time(b))
    return t


def processor(n_gallery=1000):
    from facerecognition_infrenceengine_amd import FaceAnalysis
    from facerecognition_infrenceengine_amd.processor import EmbeddingManager, FaceRecognitionProcessor, InMemoryStore
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        app = FaceAnalysis(name="synthetic", arch="r100", cap_o=4).prepare(ctx_id=0)
    r = np.random.default_rng(1)
    store = InMemoryStore()
    for i in range(n_gallery):
        store.add_employee(f"n{i}", "acme", r.standard_normal(512).astype(np.float32), name=f"N{i}")
    return FaceRecognitionProcessor(EmbeddingManager(store=store, device="cuda:0"), face_detector=app)


def host_frames(n):
    from make_golden import synth_frame
    base = [synth_frame(H, W, 900 + i) for i in range(8)]
    return [base[i % 8] for i in range(n)]


def annotate_loop(proc, frames):
    """the call the camera loop makes without a HUD: recognize_batch, then the plain box on every host frame"""
    res = proc.recognize_batch(frames, "acme")
    return [f if r is None else proc.annotate(f, r) for f, r in zip(frames, res)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--section", default="all", choices=("all", "parent"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hud.txt"))
    a = ap.parse_args()
    assert a.reps >= 30, "medians of at least 30"
    N, dev = a.frames, torch.device("cuda:0")
    lines = [f"device HUD: {N} x {H} x {W} frames, medians of {a.reps} after {WARM} warm-ups, variants alternating in one process",
             f"device: {torch.cuda.get_device_name(0)}", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def report(t, unit=1e3, what="ms per turn"):
        for k, v in t.items():
            m = statistics.median(v)
            say(f"   {k:44s}: {m * unit:9.3f} {what} (min {min(v) * unit:.3f}, max {max(v) * unit:.3f})")

    def finish():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    frames = host_frames(N)
    if a.section == "parent":
        proc = processor()
        t = wall_alternate({"recognize_batch + host annotate loop": lambda: annotate_loop(proc, [f.copy() for f in frames]),
                            "the frame copies alone": lambda: [f.copy() for f in frames]}, a.reps)
        say(f"recognize_batch + the host annotate loop, {N} x 1080p host frames per turn (synthetic weights, cap_o 4, 1 000 gallery rows),")
        say("wall time of the call, in a process of its own (the loop draws on copies of the frames; the copies are timed beside it)")
        report(t)
        finish()
        return

    from facerecognition_infrenceengine_amd import Hud, _lib
    from facerecognition_infrenceengine_amd.letterbox import frame_table
    lib = _lib.load()

    # ---- 1. the draw launch alone, beside the letterbox and a device copy
    hd = torch.from_numpy(np.ascontiguousarray(np.stack(frames))).to(dev)
    spare = torch.empty_like(hd)
    tab, _ = frame_table([hd.data_ptr() + i * H * W * 3 for i in range(N)], [(H, W)] * N, (640, 360))
    table = torch.from_numpy(tab).to(dev)
    canvas = torch.empty((N, 360, 640, 3), dtype=torch.uint8, device=dev)
    hud = Hud(scale=2)
    boxes = [(200, 150, 420, 430), (700, 300, 900, 560), (1200, 120, 1330, 290), (1500, 600, 1800, 980)]
    results = [[{"bbox": np.array(b), "person_id": None, "det_score": 0.9, "recognition_score": 0.6,
                 "person_info": {"name": f"Person {i}", "employeeId": f"E-{i:04d}", "type": ("employee", "visitor", "unknown")[(i + j) % 3]}}
                for j, b in enumerate(boxes)] for i in range(N)]
    buf, cap, at_faces, at_text = hud.pack(results, [(H, W)] * N)
    rec = torch.from_numpy(buf).to(dev)
    font = torch.from_numpy(hud.font.copy()).to(dev)
    tail = (_lib.ptr(rec[:at_faces]), cap, _lib.ptr(rec[at_faces:at_text]), _lib.ptr(rec[at_text:]), hud.max_chars, _lib.ptr(font),
            hud.scale)
    variants = {"fr_hud_draw_u8": lambda: lib.fr_hud_draw_u8(_lib.ptr(hd), N, H, W, *tail, _lib.stream_ptr()),
                "fr_hud_draw_refs_u8": lambda: lib.fr_hud_draw_refs_u8(_lib.ptr(table), N, *tail, _lib.stream_ptr()),
                "fr_letterbox_u8 -> 640 x 360": lambda: lib.fr_letterbox_u8(_lib.ptr(table), N, _lib.ptr(canvas), 360, 640, _lib.stream_ptr()),
                "device copy of the frames": lambda: spare.copy_(hd)}
    t = event_alternate(variants, a.reps)
    # the pixels inside the extents, by the definition's own geometry (tests/helpers/hud_ref.py panel_rect restated in Hud.records'
    # terms): the bounding rectangle of box, ticks, bars, letters and panel, clipped to the frame
    faces = buf[at_faces:at_text].view(np.int32).reshape(N, cap, 16)
    s, area = hud.scale, 0
    for f in range(N):
        for x1, y1, x2, y2, *rest in faces[f, :len(boxes)].tolist():
            lens = rest[6:6 + rest[5]]
            pw, ph = max(lens) * 12 * s + 20 * s, len(lens) * 18 * s + 10 * s
            px, py = max(0, min(x1, W - pw)), max(0, y2 + 10 * s)
            if py + ph > H:
                py = max(0, y1 - ph - 10 * s)
            ex0, ey0 = max(0, min(x1 - s, px)), max(0, min(y1 - 12 * s, py))
            ex1, ey1 = min(W - 1, max(x2 + 28 * s, px + pw)), min(H - 1, max(y2 + 15 * s, py + ph))
            area += (ex1 - ex0 + 1) * (ey1 - ey0 + 1)
    say(f"1. the draw launch alone (HIP events round the launch): {len(boxes)} faces per frame, scale {s}, {area / N / 1e3:.0f} k pixels of a frame "
        f"inside HUD extents ({100 * area / (N * H * W):.1f} % of it)")
    report(t, unit=1e3, what="us")
    draw = statistics.median(t["fr_hud_draw_u8"]) * 1e-3
    say(f"   the extents' pixels read and written once: {area * 6 / 1e6:.1f} MB -> {area * 6 / draw / 1e12:.2f} TB/s; the copy moves "
        f"{2 * N * H * W * 3 / 1e6:.1f} MB -> {2 * N * H * W * 3 / (statistics.median(t['device copy of the frames']) * 1e-3) / 1e12:.2f} TB/s")
    say(f"   draw / copy = {statistics.median(t['fr_hud_draw_u8']) / statistics.median(t['device copy of the frames']):.3f}, "
        f"draw / letterbox = {statistics.median(t['fr_hud_draw_u8']) / statistics.median(t['fr_letterbox_u8 -> 640 x 360']):.3f}")
    say()
    del hd, spare, canvas, table, rec
    torch.cuda.empty_cache()

    # ---- 2. the whole call
    proc = processor()
    full, small = Hud(scale=2), Hud(scale=1, out_size=(640, 360))
    variants = {"recognize_batch": lambda: proc.recognize_batch(frames, "acme"),
                "recognize_batch + host annotate loop": lambda: annotate_loop(proc, [f.copy() for f in frames]),
                "recognize_faces_batch, full size": lambda: proc.recognize_faces_batch(frames, "acme", full),
                "recognize_faces_batch, out_size (640, 360)": lambda: proc.recognize_faces_batch(frames, "acme", small),
                "the frame copies alone": lambda: [f.copy() for f in frames]}
    t = wall_alternate(variants, a.reps)
    nfaces = sum(len(r) for r in proc.recognize_batch(frames, "acme"))
    say(f"2. the whole call, {N} x 1080p host frames per turn (synthetic weights, cap_o 4, 1 000 gallery rows, {nfaces} faces in the batch), wall time")
    report(t)
    base = t["recognize_batch"]
    for k in ("recognize_batch + host annotate loop", "recognize_faces_batch, full size", "recognize_faces_batch, out_size (640, 360)"):
        say(f"   {k} - recognize_batch: {(statistics.median(t[k]) - statistics.median(base)) * 1e3:+.3f} ms "
            f"(recognize_batch's own spread: {(max(base) - min(base)) * 1e3:.3f} ms)")
    say(f"   device-to-host bytes per turn: full size {N * H * W * 3 / 1e6:.1f} MB, previews {N * 360 * 640 * 3 / 1e6:.1f} MB "
        f"(the host-to-device upload, {N * H * W * 3 / 1e6:.1f} MB, is the same in every variant; the annotate loop reads nothing back)")
    say()
    say("not measured: real video, a viewer behind the previews, YUV cameras")
    finish()


if __name__ == "__main__":
    main()
