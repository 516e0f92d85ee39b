"""Times face redaction on one MI355X; writes profiles/redact.txt.  The conditions of tools/hud_time.py: 64 x 1080p
host frames with 4 faces each, medians of 30 after 3 warm-ups, the variants alternating in one process.

  1. the launch alone (HIP events): fr_redact_u8 at block 16, pixelate and fill, on the 4 faces' regions and with every frame one
     whole-picture region, beside a device copy of the same frames and the HUD draw launch (scale 2) of the same session.
  2. --section parent: FaceRecognitionProcessor.recognize_faces_batch WITHOUT a redactor, full size and 640 x 360 previews, plain
     and encoded - nothing this tool needs beyond what the tree before the redaction had, so the same file runs on that tree in a
     process of its own; --own FILE and --parent FILE (such runs of this tree and of the parent commit's, each a process of its
     own with the same four variants) are then set side by side, and the tool says whether their difference lies inside the
     call's own spread.
  3. the same calls with redact=, pixelate at block 16.

No pass mark, nothing here is asserted in a test.  Not measured: real video, the flicker of a frame-anchored mosaic on moving
faces, how well a mosaic of a given block withstands de-pixelation, YUV and MJPEG cameras, linger.
Usage: python tools/redact_time.py [--frames 64] [--reps 30] [--section all|parent] [--own FILE] [--parent FILE] [--out profiles/redact.txt]"""
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
LINE = re.compile(r"^\s+(.+?)\s*:\s+([\d.]+) ms per turn \(min ([\d.]+), max ([\d.]+)\)")


def plain_calls(proc, frames, redact=None):
    """the four calls of sections 2 and 3; ``redact`` None: the arguments the tree before the redaction takes"""
    from facerecognition_infrenceengine_amd import Hud, JpegEncoder
    full, small, enc = Hud(scale=2), Hud(scale=1, out_size=(640, 360)), JpegEncoder(80)
    kw = {} if redact is None else {"redact": redact}
    tag = "" if redact is None else ", redact"
    return {f"full size{tag}": lambda: proc.recognize_faces_batch(frames, "acme", full, **kw),
            f"out_size (640, 360){tag}": lambda: proc.recognize_faces_batch(frames, "acme", small, **kw),
            f"full size, encode{tag}": lambda: proc.recognize_faces_batch(frames, "acme", full, encode=enc, **kw),
            f"out_size (640, 360), encode{tag}": lambda: proc.recognize_faces_batch(frames, "acme", small, encode=enc, **kw)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--section", default="all", choices=("all", "parent"))
    ap.add_argument("--parent", default=None, help="the file a --section parent run on the parent commit's tree wrote")
    ap.add_argument("--own", default=None, help="the file a --section parent run on this tree wrote")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "redact.txt"))
    a = ap.parse_args()
    assert a.reps >= 30, "medians of at least 30"
    N, dev = a.frames, torch.device("cuda:0")
    lines = [f"face redaction: {N} x {H} x {W} frames, medians of {a.reps} after {WARM} warm-ups, variants alternating in one process",
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
        say(f"recognize_faces_batch without a redactor, {N} x 1080p host frames per turn (synthetic weights, cap_o 4, 1 000 gallery rows),")
        say("wall time of the call, in a process of its own")
        report(wall_alternate(plain_calls(proc, frames), a.reps))
        finish()
        return

    from facerecognition_infrenceengine_amd import Hud, Redactor, _lib
    lib = _lib.load()

    # ---- 1. the launch alone, beside a device copy and the HUD draw
    hd = torch.from_numpy(np.ascontiguousarray(np.stack(frames))).to(dev)
    spare = torch.empty_like(hd)
    results = [[{"bbox": np.array(b), "person_id": None, "det_score": 0.9, "recognition_score": 0.6,
                 "person_info": {"name": f"Person {i}", "employeeId": f"E-{i:04d}", "type": ("employee", "visitor", "unknown")[(i + j) % 3]}}
                for j, b in enumerate(BOXES)] for i in range(N)]
    red = Redactor(block=16)
    shapes = [(H, W)] * N
    cnt, regs, cap = red.regions(results, shapes)
    wcnt, wregs, wcap = red.regions([None] * N, shapes)
    faces_dev = torch.from_numpy(np.concatenate([cnt, regs.reshape(-1)])).to(dev)
    whole_dev = torch.from_numpy(np.concatenate([wcnt, wregs.reshape(-1)])).to(dev)
    hud = Hud(scale=2)
    buf, hcap, at_faces, at_text = hud.pack(results, shapes)
    rec = torch.from_numpy(buf).to(dev)
    font = torch.from_numpy(hud.font.copy()).to(dev)

    def launch(table, c, mode):
        return lambda: lib.fr_redact_u8(_lib.ptr(hd), N, H, W, _lib.ptr(table), c, _lib.ptr(table[N:]), 16, mode, 0, _lib.stream_ptr())
    variants = {"fr_redact_u8, pixelate, 4 faces": launch(faces_dev, cap, 0),
                "fr_redact_u8, fill, 4 faces": launch(faces_dev, cap, 1),
                "fr_redact_u8, pixelate, whole picture": launch(whole_dev, wcap, 0),
                "fr_redact_u8, fill, whole picture": launch(whole_dev, wcap, 1),
                "fr_hud_draw_u8": lambda: lib.fr_hud_draw_u8(_lib.ptr(hd), N, H, W, _lib.ptr(rec[:at_faces]), hcap, _lib.ptr(rec[at_faces:at_text]),
                                                             _lib.ptr(rec[at_text:]), hud.max_chars, _lib.ptr(font), hud.scale, _lib.stream_ptr()),
                "device copy of the frames": lambda: spare.copy_(hd)}
    t = event_alternate(variants, a.reps)
    area = 0
    for x1, y1, x2, y2 in regs[0, :cnt[0]].tolist():         # the tiles (16 rows x 64 pixels) the regions meet, clipped to the frame
        tx0, tx1, ty0, ty1 = max(x1, 0) // 64, min(x2, W - 1) // 64, max(y1, 0) // 16, min(y2, H - 1) // 16
        area += sum(min(64, W - 64 * tx) for tx in range(tx0, tx1 + 1)) * sum(min(16, H - 16 * ty) for ty in range(ty0, ty1 + 1))
    held = int(sum((x2 - x1 + 1) * (y2 - y1 + 1) for x1, y1, x2, y2 in np.clip(regs[0, :cnt[0]], 0, [W - 1, H - 1, W - 1, H - 1]).tolist()))
    say(f"1. the launch alone (HIP events round the launch): block 16, {len(BOXES)} faces per frame with a margin of {red.margin} %, "
        f"{held / 1e3:.0f} k pixels of a frame held ({100 * held / (H * W):.1f} % of it), {area / 1e3:.0f} k pixels in tiles a region meets")
    report(t, unit=1e3, what="us")
    med = {k: statistics.median(v) * 1e-3 for k, v in t.items()}
    say(f"   pixelate, 4 faces: the met tiles read once, the held pixels written once: {N * (area + held) * 3 / 1e6:.1f} MB -> "
        f"{N * (area + held) * 3 / med['fr_redact_u8, pixelate, 4 faces'] / 1e12:.2f} TB/s")
    say(f"   pixelate, whole picture: every byte read and written once: {2 * N * H * W * 3 / 1e6:.1f} MB -> "
        f"{2 * N * H * W * 3 / med['fr_redact_u8, pixelate, whole picture'] / 1e12:.2f} TB/s; the copy moves the same bytes at "
        f"{2 * N * H * W * 3 / med['device copy of the frames'] / 1e12:.2f} TB/s")
    say(f"   pixelate 4 faces / copy = {med['fr_redact_u8, pixelate, 4 faces'] / med['device copy of the frames']:.3f}, "
        f"pixelate 4 faces / HUD draw = {med['fr_redact_u8, pixelate, 4 faces'] / med['fr_hud_draw_u8']:.3f}, "
        f"pixelate whole picture / copy = {med['fr_redact_u8, pixelate, whole picture'] / med['device copy of the frames']:.3f}")
    say()
    del hd, spare, rec, faces_dev, whole_dev
    torch.cuda.empty_cache()

    # ---- 2. and 3. the whole call, without and with a redactor
    proc = processor()
    variants = dict(plain_calls(proc, frames))
    variants.update(plain_calls(proc, frames, Redactor(block=16)))
    t = wall_alternate(variants, a.reps)
    nfaces = sum(len(r) for r in proc.recognize_batch(frames, "acme"))
    say(f"2. recognize_faces_batch with redact=None, {N} x 1080p host frames per turn (synthetic weights, cap_o 4, 1 000 gallery rows, "
        f"{nfaces} faces in the batch), wall time")
    plain = {k: v for k, v in t.items() if not k.endswith(", redact")}
    report(plain)
    def figures(path):
        out = {}
        for raw in open(path).read().splitlines():
            m = LINE.match(raw)
            if m:
                out[m.group(1)] = (raw, float(m.group(2)), float(m.group(4)) - float(m.group(3)))
        return out
    if a.parent and a.own and os.path.exists(a.parent) and os.path.exists(a.own):
        own, parent = figures(a.own), figures(a.parent)
        say("   the same four calls alone, each tree in a process of its own in the same session (--section parent): this tree, then the "
            "parent commit's tree")
        for k in plain:
            if k not in own or k not in parent:
                continue
            say(own[k][0] + "   <- this tree")
            say(parent[k][0] + "   <- parent")
            d, spread = own[k][1] - parent[k][1], max(own[k][2], parent[k][2])
            say(f"      this tree - parent: {d:+.3f} ms; the call's own spread (the wider of the two): {spread:.3f} ms -> "
                f"{'inside' if abs(d) <= spread else 'OUTSIDE'} it")
    else:
        say("   (no runs of the two trees in processes of their own were given: --own FILE --parent FILE)")
    say()
    say("3. the same calls with redact=Redactor(block=16) (pixelate, margin 25 %, everybody)")
    report({k: v for k, v in t.items() if k.endswith(", redact")})
    for k in plain:
        d = statistics.median(t[k + ", redact"]) - statistics.median(plain[k])
        say(f"   {k}: redact - plain = {d * 1e3:+.3f} ms (the plain call's own spread: {(max(plain[k]) - min(plain[k])) * 1e3:.3f} ms)")
    say()
    say("not measured: real video, the flicker of a frame-anchored mosaic on moving faces, how well a mosaic of a given block "
        "withstands de-pixelation, YUV and MJPEG cameras, linger")
    finish()


if __name__ == "__main__":
    main()
