"""Times the device JPEG encoder on one MI355X; writes profiles/jpeg.txt.  Medians of 30 after 3 warm-ups, the
variants alternating in one process (the helpers of tools/hud_time.py).

  1. the encoder's two launches alone (HIP events round the call): 64 x 1080p frames with a HUD drawn on them (4 faces each,
     scale 2) and 64 previews of 640 x 360 of the same frames, fr_jpeg_encode_u8 and - full size - fr_jpeg_encode_refs_u8, beside
     a device copy of the same frames; the bytes produced.
  2. FaceRecognitionProcessor.recognize_faces_batch of 64 x 1080p host frames (synthetic weights, cap_o = 4, a 1 000-row gallery),
     full size and with out_size = (640, 360), with and without ``encode``, beside recognize_batch alone: wall time of the
     whole call, and the device-to-host bytes of each path.
  3. --section parent: the array-returning recognize_faces_batch alone, full size and previews, with nothing this tool needs
     beyond what the tree before the encoder had - so the same file can be run on that tree, in a process of its own.

No pass mark, nothing here is asserted in a test.  Not measured: real video (the synthetic frames are smooth and compress far
better than a camera's), a viewer behind the routes, YUV cameras.
Usage: python tools/jpeg_time.py [--frames 64] [--reps 30] [--quality 80] [--section all|parent] [--out profiles/jpeg.txt]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from hud_time import H, W, WARM, event_alternate, host_frames, processor, wall_alternate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--quality", type=int, default=80)
    ap.add_argument("--section", default="all", choices=("all", "parent"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg.txt"))
    a = ap.parse_args()
    assert a.reps >= 30, "medians of at least 30"
    N, dev = a.frames, torch.device("cuda:0")
    lines = [f"device JPEG encoder: {N} x {H} x {W} frames, quality {a.quality}, medians of {a.reps} after {WARM} warm-ups, "
             f"variants alternating in one process", f"device: {torch.cuda.get_device_name(0)}", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def report(t, unit=1e3, what="ms per turn"):
        for k, v in t.items():
            m = statistics.median(v)
            say(f"   {k:52s}: {m * unit:9.3f} {what} (min {min(v) * unit:.3f}, max {max(v) * unit:.3f})")

    def finish():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    from facerecognition_infrenceengine_amd import Hud
    frames = host_frames(N)
    full, small = Hud(scale=2), Hud(scale=1, out_size=(640, 360))
    if a.section == "parent":
        proc = processor()
        t = wall_alternate({"recognize_faces_batch, full size (arrays)": lambda: proc.recognize_faces_batch(frames, "acme", full),
                            "recognize_faces_batch, out_size (640, 360) (arrays)": lambda: proc.recognize_faces_batch(frames, "acme", small)},
                           a.reps)
        say(f"the array-returning recognize_faces_batch, {N} x 1080p host frames per turn (synthetic weights, cap_o 4, 1 000 gallery "
            f"rows), wall time of the call, in a process of its own")
        report(t)
        finish()
        return

    from facerecognition_infrenceengine_amd import JpegEncoder
    from facerecognition_infrenceengine_amd.letterbox import frame_table
    enc = JpegEncoder(a.quality)

    # ---- 1. the two launches alone, beside a device copy
    boxes = [(200, 150, 420, 430), (700, 300, 900, 560), (1200, 120, 1330, 290), (1500, 600, 1800, 980)]
    results = [[{"bbox": np.array(b), "person_id": None, "det_score": 0.9, "recognition_score": 0.6,
                 "person_info": {"name": f"Person {i}", "employeeId": f"E-{i:04d}", "type": ("employee", "visitor", "unknown")[(i + j) % 3]}}
                for j, b in enumerate(boxes)] for i in range(N)]
    hd = torch.from_numpy(np.ascontiguousarray(np.stack(frames))).to(dev)
    previews = small.draw(hd, results)
    full.draw(hd, results)
    spare, spare_small = torch.empty_like(hd), torch.empty_like(previews)
    tab, _ = frame_table([hd.data_ptr() + i * H * W * 3 for i in range(N)], [(H, W)] * N)
    table = torch.from_numpy(tab).to(dev)
    variants = {"fr_jpeg_encode_u8, 1080p": lambda: enc.encode_device(hd),
                "fr_jpeg_encode_refs_u8, 1080p": lambda: enc.encode_device((hd, table), shapes=[(H, W)] * N),
                "device copy of the 1080p frames": lambda: spare.copy_(hd),
                "fr_jpeg_encode_u8, 640 x 360": lambda: enc.encode_device(previews),
                "device copy of the 640 x 360 previews": lambda: spare_small.copy_(previews)}
    t = event_alternate(variants, a.reps)
    big = sum(len(b) for b in enc.encode(hd))
    little = sum(len(b) for b in enc.encode(previews))
    say(f"1. the encoder's two launches alone (HIP events round the call): frames with a HUD drawn on them, {len(boxes)} faces per frame")
    report(t, unit=1e3, what="us")
    say(f"   bytes produced: 1080p {big / 1e6:.2f} MB of {N * H * W * 3 / 1e6:.1f} MB ({big / N / 1e3:.1f} KB per frame, 1 : "
        f"{N * H * W * 3 / big:.1f}); 640 x 360 {little / 1e6:.2f} MB of {N * 360 * 640 * 3 / 1e6:.1f} MB ({little / N / 1e3:.1f} KB per frame)")
    say(f"   encode / copy: 1080p {statistics.median(t['fr_jpeg_encode_u8, 1080p']) / statistics.median(t['device copy of the 1080p frames']):.1f}, "
        f"640 x 360 {statistics.median(t['fr_jpeg_encode_u8, 640 x 360']) / statistics.median(t['device copy of the 640 x 360 previews']):.1f}")
    say()
    del hd, spare, previews, spare_small, table
    enc = JpegEncoder(a.quality)
    torch.cuda.empty_cache()

    # ---- 2. the whole call
    proc = processor()
    variants = {"recognize_batch": lambda: proc.recognize_batch(frames, "acme"),
                "recognize_faces_batch, full size, arrays": lambda: proc.recognize_faces_batch(frames, "acme", full),
                "recognize_faces_batch, full size, encode": lambda: proc.recognize_faces_batch(frames, "acme", full, encode=enc),
                "recognize_faces_batch, out_size (640, 360), arrays": lambda: proc.recognize_faces_batch(frames, "acme", small),
                "recognize_faces_batch, out_size (640, 360), encode": lambda: proc.recognize_faces_batch(frames, "acme", small, encode=enc)}
    t = wall_alternate(variants, a.reps)
    sizes = {k: sum(len(b) for b in proc.recognize_faces_batch(frames, "acme", h, encode=enc)) for k, h in (("full", full), ("small", small))}
    say(f"2. the whole call, {N} x 1080p host frames per turn (synthetic weights, cap_o 4, 1 000 gallery rows), wall time")
    report(t)
    base = t["recognize_batch"]
    for k in list(variants)[1:]:
        say(f"   {k} - recognize_batch: {(statistics.median(t[k]) - statistics.median(base)) * 1e3:+.3f} ms "
            f"(recognize_batch's own spread: {(max(base) - min(base)) * 1e3:.3f} ms)")
    say(f"   device-to-host bytes per turn: full size {N * H * W * 3 / 1e6:.1f} MB as arrays, {sizes['full'] / 1e6:.2f} MB as JPEG; previews "
        f"{N * 360 * 640 * 3 / 1e6:.1f} MB as arrays, {sizes['small'] / 1e6:.2f} MB as JPEG (the host-to-device upload, "
        f"{N * H * W * 3 / 1e6:.1f} MB, is the same in every variant)")
    say()
    say("not measured: real video (the synthetic frames compress far better than a camera's), a viewer behind the routes, YUV cameras")
    finish()


if __name__ == "__main__":
    main()
