"""Times face chips on one MI355X; writes profiles/chips.txt.  The conditions of tools/hud_time.py: 64 x 1080p host
frames with 4 faces each, medians of 30 after 3 warm-ups, the variants alternating in one process.

  1. the launches alone (HIP events): fr_face_chips_u8 for the 256 chips at S = 112 (the 4 boxes of tools/redact_time.py, margin
     30 %), beside fr_warp_affine_5pt_slots over the same 256 slots and a device copy of the frames; and the encoder's two launches
     (JpegEncoder.encode_device) on the [256,112,112,3] batch of chips.
  2. --section parent: FaceRecognitionProcessor.recognize_batch WITHOUT chips - nothing this tool needs beyond what the tree before
     the chips had, so the same file runs on that tree in a process of its own; --own FILE and --parent FILE (such runs of this
     tree and of the parent commit's) are then set side by side, and the tool says whether their difference lies inside the call's
     own spread.
  3. recognize_batch with chips for every face, and under tracks with who=lambda r: not r.get("tracked").

No pass mark, nothing here is asserted in a test.  Not measured: real video, YUV and MJPEG cameras, det_size engines.
Usage: python tools/chips_time.py [--frames 64] [--reps 30] [--section all|parent] [--own FILE] [--parent FILE] [--out profiles/chips.txt]"""
import argparse
import os
import re
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from hud_time import H, W, WARM, event_alternate, host_frames, processor, wall_alternate  # noqa: E402

BOXES = [(200, 150, 420, 430), (700, 300, 900, 560), (1200, 120, 1330, 290), (1500, 600, 1800, 980)]
TEMPLATE = np.array([[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366], [41.5493, 92.3655], [70.7299, 92.2041]], np.float32)
LINE = re.compile(r"^\s+(.+?)\s*:\s+([\d.]+) ms per turn \(min ([\d.]+), max ([\d.]+)\)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--section", default="all", choices=("all", "parent"))
    ap.add_argument("--parent", default=None, help="the file a --section parent run on the parent commit's tree wrote")
    ap.add_argument("--own", default=None, help="the file a --section parent run on this tree wrote")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chips.txt"))
    a = ap.parse_args()
    assert a.reps >= 30, "medians of at least 30"
    N, dev = a.frames, torch.device("cuda:0")
    lines = [f"face chips: {N} x {H} x {W} frames, medians of {a.reps} after {WARM} warm-ups, variants alternating in one process",
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
        lines[:] = []
        say(f"recognize_batch without chips, {N} x 1080p host frames per turn (synthetic weights, cap_o 4, 1 000 gallery rows),")
        say("wall time of the call, in a process of its own")
        report(wall_alternate({"recognize_batch": lambda: proc.recognize_batch(frames, "acme")}, a.reps))
        finish()
        return

    from facerecognition_infrenceengine_amd import FaceChips, FaceTracks, _lib
    lib = _lib.load()

    # ---- 1. the launches alone
    hd = torch.from_numpy(np.ascontiguousarray(np.stack(frames))).to(dev)
    spare = torch.empty_like(hd)
    results = [[{"bbox": np.array(b), "person_info": {"type": "unknown"}} for b in BOXES] for _ in range(N)]
    chips = FaceChips(size=112, margin=30)
    recs, owners = chips.records(results)
    F, S = len(recs), chips.size
    assert len(owners) == F == 4 * N
    d_recs = torch.from_numpy(recs).to(dev)
    out = torch.empty((F, S, S, 3), dtype=torch.uint8, device=dev)
    cap = len(BOXES)
    centres = np.array([[(x1 + x2) / 2, (y1 + y2) / 2] for x1, y1, x2, y2 in BOXES], np.float32)
    scale = np.array([(x2 - x1 + 1) / 112.0 for x1, y1, x2, y2 in BOXES], np.float32)
    kps = (TEMPLATE[None] - 56.0) * scale[:, None, None] + centres[:, None, :]              # the template laid over each box
    kps = torch.from_numpy(np.broadcast_to(kps[None], (N, cap, 5, 2)).astype(np.float32).copy()).to(dev)
    counts = torch.full((N,), cap, dtype=torch.int32, device=dev)
    crops = torch.empty((N * cap, 112, 112, 8), dtype=torch.float16, device=dev)
    keep = []

    def cut():
        lib.fr_face_chips_u8(_lib.ptr(hd), N, H, W, _lib.ptr(d_recs), F, S, 0, _lib.ptr(out), _lib.stream_ptr())

    def warp():
        lib.fr_warp_affine_5pt_slots(_lib.ptr(hd), N, H, W, _lib.ptr(kps), _lib.ptr(counts), cap, 112, _lib.ptr(crops), _lib.stream_ptr())

    def encode():
        keep[:] = chips.encode.encode_device(out)
    cut()
    t = event_alternate({"fr_face_chips_u8, 256 chips, S = 112": cut, "fr_warp_affine_5pt_slots, 256 slots": warp,
                         "device copy of the frames": lambda: spare.copy_(hd),
                         "JpegEncoder.encode_device, [256,112,112,3]": encode}, a.reps)
    sides = [int(r[3]) for r in recs[:cap]]
    inside = 0
    for _, x0, y0, L in recs[:cap].tolist():                  # the pixels of a frame the squares cover, clipped to the frame
        inside += max(0, min(x0 + L, W) - max(x0, 0)) * max(0, min(y0 + L, H) - max(y0, 0))
    say(f"1. the launches alone (HIP events round each): {F} chips of {S} x {S} from {N} frames, squares of side {sides} "
        f"(margin {chips.margin} %), {inside / 1e3:.0f} k source pixels per frame")
    report(t, unit=1e3, what="us")
    med = {k: statistics.median(v) * 1e-3 for k, v in t.items()}
    read = N * inside * 3
    say(f"   the cut reads every source byte of a square once, plus a row per band boundary: {read / 1e6:.1f} MB read, "
        f"{F * S * S * 3 / 1e6:.1f} MB written -> {read / med['fr_face_chips_u8, 256 chips, S = 112'] / 1e12:.3f} TB/s read; "
        f"the copy moves {2 * N * H * W * 3 / 1e6:.0f} MB at {2 * N * H * W * 3 / med['device copy of the frames'] / 1e12:.2f} TB/s")
    say(f"   cut / slot warp = {med['fr_face_chips_u8, 256 chips, S = 112'] / med['fr_warp_affine_5pt_slots, 256 slots']:.2f}: the warp "
        f"reads 4 taps per output pixel ({F * 112 * 112 * 4 * 3 / 1e6:.1f} MB at most, whatever the face's size), the cut every pixel "
        f"of the square ({read / 1e6:.1f} MB)")
    say()
    del hd, spare, out, crops
    torch.cuda.empty_cache()

    # ---- 2. and 3. the whole call
    proc = processor()
    every = FaceChips(size=112, margin=30)
    fresh = FaceChips(size=112, margin=30, who=lambda r: not r.get("tracked"))
    tracks = FaceTracks(device="cuda:0", slots=max(256, N))
    cams = list(range(N))
    variants = {"recognize_batch": lambda: proc.recognize_batch(frames, "acme"),
                "recognize_batch, chips for every face": lambda: proc.recognize_batch(frames, "acme", chips=every),
                "recognize_batch, tracks": lambda: proc.recognize_batch(frames, "acme", tracks=tracks, camera_ids=cams),
                "recognize_batch, tracks, chips of fresh faces": lambda: proc.recognize_batch(frames, "acme", tracks=tracks, camera_ids=cams,
                                                                                              chips=fresh)}
    t = wall_alternate(variants, a.reps)
    res = proc.recognize_batch(frames, "acme", chips=every)
    nfaces = sum(len(r) for r in res)
    nbytes = sum(len(x["chip"]) for r in res for x in r if x["chip"] is not None)
    say(f"2. recognize_batch with chips=None, {N} x 1080p host frames per turn (synthetic weights, cap_o 4, 1 000 gallery rows, "
        f"{nfaces} faces in the batch), wall time")
    report({"recognize_batch": t["recognize_batch"]})

    def figures(path):
        got = {}
        for raw in open(path).read().splitlines():
            m = LINE.match(raw)
            if m:
                got[m.group(1)] = (raw, float(m.group(2)), float(m.group(4)) - float(m.group(3)))
        return got
    if a.parent and a.own and os.path.exists(a.parent) and os.path.exists(a.own):
        own, parent = figures(a.own), figures(a.parent)
        say("   the same call alone, each tree in a process of its own in the same session (--section parent): this tree, then the "
            "parent commit's tree")
        k = "recognize_batch"
        if k in own and k in parent:
            say(own[k][0] + "   <- this tree")
            say(parent[k][0] + "   <- parent")
            d, spread = own[k][1] - parent[k][1], max(own[k][2], parent[k][2])
            say(f"      this tree - parent: {d:+.3f} ms; the call's own spread (the wider of the two): {spread:.3f} ms -> "
                f"{'inside' if abs(d) <= spread else 'OUTSIDE'} it")
    else:
        say("   (no runs of the two trees in processes of their own were given: --own FILE --parent FILE)")
    say()
    say(f"3. the same call with chips (S = 112, margin 30 %, JPEG quality 85: {nbytes / max(nfaces, 1):.0f} bytes per chip on these frames)")
    report({k: v for k, v in t.items() if k != "recognize_batch"})
    base, spread = statistics.median(t["recognize_batch"]), max(t["recognize_batch"]) - min(t["recognize_batch"])
    say(f"   chips for every face - plain = {(statistics.median(t['recognize_batch, chips for every face']) - base) * 1e3:+.3f} ms "
        f"(the plain call's own spread: {spread * 1e3:.3f} ms)")
    d = statistics.median(t["recognize_batch, tracks, chips of fresh faces"]) - statistics.median(t["recognize_batch, tracks"])
    say(f"   under tracks, chips of the faces embedded afresh - tracks alone = {d * 1e3:+.3f} ms (the same frames every turn: "
        f"a face is fresh once in max_reuse + 1 turns)")
    say()
    say("not measured: real video, YUV and MJPEG cameras, det_size engines, chips beside a HUD")
    finish()


if __name__ == "__main__":
    main()
