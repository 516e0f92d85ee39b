"""Times the device JPEG decoder on one MI355X; writes profiles/jpeg_decode.txt.  Medians of 30 after 3
warm-ups, the variants alternating in one process (the helpers of tools/hud_time.py).

The workload: 64 x 1080p frames (the synthetic frames of the other tools with sensor-like noise added, so that the files have a
camera's size and not a cartoon's) as (a) Pillow's quality-80 4:2:0 files without DRI - what an MJPEG camera sends -, (b) the
project's own encoder's files (one restart interval per MCU row), (c) Pillow's 4:2:2 files.

  1. the decoder's four launches alone (HIP events round fr_jpeg_decode_refs_u8, the files on the device already), beside a
     device copy of the decoded frames and beside fr_yuv420_to_bgr_u8 on the same frames as NV12; the bytes that cross the link.
     Also read back: the rounds behind round 0 the entropy launch counted, per restart interval.
     ``--section launches [--kind K]`` runs these launches only (ten times each) for a kernel trace, and ``--section stages
     --trace DIR`` appends the traces' medians per kernel to the profile: the split by stage.
  2. host bytes to device frames, wall time with a synchronisation: ``JpegDecoder.decode_device`` (parse, one pinned staging
     copy, the launches) beside the BGR ring's way (the frames copied into pinned memory and up) and beside the 64 files through
     ``ingest.decode_image`` on the host, which is what the decoder replaces.
  3. the rounds the self-synchronising walk needs: the definition's simulation at the kernel's subsequence size on one file of
     each kind (not read from the device).

  2b. ``recognize_batch`` of the 64 frames from a BGR ring, an NV12 ring and a JPEG ring (each kind of file), wall time of the
     call, and the bytes that cross the link for each.

No pass mark, nothing here is asserted in a test.  Not measured: real camera streams.
Usage: python tools/jpeg_decode_time.py [--frames 64] [--reps 30] [--section all|launches] [--out profiles/jpeg_decode.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from hud_time import H, W, WARM, event_alternate, host_frames, wall_alternate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--section", default="all", choices=("all", "launches", "stages"))
    ap.add_argument("--kind", default=None, help="--section launches: this kind of file only (a key of the workload)")
    ap.add_argument("--trace", default=None, help="--section stages: directory holding trace_*/ with rocprofv3 kernel traces (csv)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode.txt"))
    a = ap.parse_args()
    assert a.reps >= 30, "medians of at least 30"
    if a.section == "stages":
        return stages(a)
    N, dev = a.frames, torch.device("cuda:0")
    lines = [f"device JPEG decoder: {N} x {H} x {W} frames, medians of {a.reps} after {WARM} warm-ups, variants alternating in one "
             f"process", f"device: {torch.cuda.get_device_name(0)}", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def report(t, unit=1e3, what="ms"):
        for k, v in t.items():
            m = statistics.median(v)
            say(f"   {k:58s}: {m * unit:10.3f} {what} (min {min(v) * unit:.3f}, max {max(v) * unit:.3f})")

    from facerecognition_infrenceengine_amd import JpegEncoder
    from facerecognition_infrenceengine_amd.colour import yuv420_to_bgr
    from facerecognition_infrenceengine_amd.ingest import FrameIngest, decode_image
    from facerecognition_infrenceengine_amd.jpeg_decode import JpegDecoder, parse
    from tests.helpers import jpeg_decode_cases as cases

    rng = np.random.default_rng(0)
    frames = [np.clip(f.astype(np.int16) + rng.normal(0, 4, f.shape).round().astype(np.int16), 0, 255).astype(np.uint8)
              for f in host_frames(8)]
    frames = [frames[i % 8] for i in range(N)]
    base = {"pillow q80 4:2:0": [cases.pil_file(f, 80, "420") for f in frames[:8]],
            "pillow q80 4:2:2": [cases.pil_file(f, 80, "422") for f in frames[:8]],
            "own encoder q80": JpegEncoder(80).encode(torch.from_numpy(np.stack(frames[:8])).to(dev))}
    files = {k: [v[i % 8] for i in range(N)] for k, v in base.items()}
    dec = JpegDecoder(dev)

    # ---- 1. the launches alone: the files on the device, descriptors and tables built once
    from facerecognition_infrenceengine_amd import _lib
    from facerecognition_infrenceengine_amd.letterbox import frame_table
    lib = _lib.load()
    out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
    tab, _ = frame_table([out.data_ptr() + i * H * W * 3 for i in range(N)], [(H, W)] * N)
    refs = torch.from_numpy(tab).to(dev)
    status = torch.empty(N, dtype=torch.int32, device=dev)
    launches, keep = {}, []
    for kind, blobs in files.items():
        recs, headers = dec.describe(blobs)
        data, at = bytearray(), 0
        for f, hd in enumerate(headers):
            recs["scan_off"][f] = len(data)
            data += bytes(blobs[f][hd.scan:]) + bytes(-len(blobs[f][hd.scan:]) % 16)
        segments = max(hd.segments for hd in headers)
        stream = torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).to(dev)
        table = torch.from_numpy(recs.view(np.uint8).copy()).to(dev)
        ws_bytes = int(lib.fr_jpeg_decode_workspace(N, H, W, segments))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        keep.append((stream, table, ws, ws_bytes, segments, [hd.segments for hd in headers]))

        def launch(stream=stream, table=table, ws=ws, ws_bytes=ws_bytes, segments=segments, nbytes=len(data)):
            qt, ht = dec._tables_on_device()
            lib.fr_jpeg_decode_refs_u8(_lib.ptr(stream), nbytes, _lib.ptr(table), N, H, W, segments, _lib.ptr(qt), int(qt.shape[0]),
                                       _lib.ptr(ht), int(ht.shape[0]), _lib.ptr(dec._natural), _lib.ptr(refs), _lib.ptr(status),
                                       _lib.ptr(ws), ws_bytes, _lib.stream_ptr())
        launches[f"fr_jpeg_decode_refs_u8, {kind}"] = launch
    if a.section == "launches":
        for _ in range(10):
            for name, fn in launches.items():
                if a.kind is None or name.endswith(", " + a.kind):
                    fn()
        torch.cuda.synchronize()
        assert (status.cpu().numpy() == 0).all()
        return
    spare = torch.empty_like(out)
    nv12 = torch.randint(0, 256, (N, H * 3 // 2, W), dtype=torch.uint8, device=dev)
    variants = dict(launches)
    variants["device copy of the decoded frames"] = lambda: spare.copy_(out)
    variants["fr_yuv420_to_bgr_u8 (NV12 of the same size)"] = lambda: yuv420_to_bgr(nv12, "nv12", "bt601")
    t = event_alternate(variants, a.reps)
    assert (status.cpu().numpy() == 0).all()
    want = np.stack([cases.pil_decode(b) for b in files["own encoder q80"][:2]])
    assert np.array_equal(out[:2].cpu().numpy(), want), "the device's pixels are not Pillow's"
    say("1. the decoder's four launches alone (HIP events round the call), the files on the device")
    report(t, unit=1.0, what="ms")
    for kind, blobs in files.items():
        total = sum(len(b) for b in blobs)
        say(f"   {kind}: {total / 1e6:.2f} MB cross the link in place of {N * H * W * 3 / 1e6:.1f} MB of BGR ({total / N / 1e3:.1f} KB per "
            f"frame, 1 : {N * H * W * 3 / total:.1f}); NV12 would be {N * H * W * 3 / 2e6:.1f} MB")
    # what the entropy launch itself counted: per restart interval the most rounds behind round 0 any of its chunks needed
    for kind, (_, _, ws, ws_bytes, segments, per_frame) in zip(files, keep):
        words = ws.cpu().numpy().view(np.int32).reshape(N, ws_bytes // N // 4)
        seen = np.concatenate([words[f, 2 * segments:2 * segments + per_frame[f]] for f in range(N)])
        say(f"   {kind}: rounds behind round 0 read from the device, per restart interval ({len(seen)} intervals): "
            f"median {int(np.median(seen))}, most {int(seen.max())}, least {int(seen.min())}")
    say()
    del spare, nv12

    # ---- 2. host bytes -> device frames
    ring = FrameIngest(N, H, W, dev, depth=2)
    turn = [0]

    def bgr_ring():
        host = ring.host_buffer(turn[0])
        for i, f in enumerate(frames):
            host[i] = f
        _, ready = ring.upload(turn[0])
        ready.synchronize()
        ring.release(turn[0])
        turn[0] += 1

    def device_decode(blobs):
        dec.decode_device(blobs, out=out)
        torch.cuda.synchronize()
    variants = {f"JpegDecoder.decode_device, {kind}": (lambda blobs=blobs: device_decode(blobs)) for kind, blobs in files.items()}
    variants["BGR ring: copy into pinned memory, upload"] = bgr_ring
    variants["ingest.decode_image on the host, pillow q80 4:2:0"] = lambda: [decode_image(b) for b in files["pillow q80 4:2:0"]]
    t = wall_alternate(variants, a.reps)
    say(f"2. host bytes to device frames, {N} frames, wall time with a synchronisation")
    report(t)
    say()

    # ---- 2b. the whole call: recognize_batch from a BGR, an NV12 and a JPEG ring
    from hud_time import processor
    from tests.helpers import yuv_ref
    proc = processor()
    bgr = [cases.pil_decode(b) for b in base["own encoder q80"]]            # the pictures the files hold
    bgr = [bgr[i % 8] for i in range(N)]
    nv12 = [yuv_ref.bgr_to_yuv420(f, "nv12") for f in bgr[:8]]
    nv12 = [nv12[i % 8] for i in range(N)]
    variants = {"recognize_batch, BGR ring": lambda: proc.recognize_batch(bgr, "acme"),
                "recognize_batch, NV12 ring": lambda: proc.recognize_batch(nv12, "acme", pixel_format="nv12")}
    for kind, blobs in files.items():
        variants[f"recognize_batch, JPEG ring, {kind}"] = lambda blobs=blobs: proc.recognize_batch(blobs, "acme", pixel_format="jpeg")
    t = wall_alternate(variants, a.reps)
    say(f"2b. recognize_batch of {N} x 1080p host frames (synthetic weights, cap_o 4, 1 000 gallery rows), wall time of the call")
    report(t)
    say(f"   host-to-device bytes per call: BGR {N * H * W * 3 / 1e6:.1f} MB, NV12 {N * H * W * 3 / 2e6:.1f} MB, JPEG "
        + ", ".join(f"{kind} {(64 * N + sum(len(b) for b in blobs)) / 1e6:.2f} MB" for kind, blobs in files.items()))
    say()

    # ---- 3. the rounds of the self-synchronising walk (the definition's simulation)
    from tests.helpers import jpeg_decode_ref as ref
    say(f"3. the self-synchronising walk, simulated by the definition at S = {ref.S} bytes, {ref.LANES} lanes (one file of each kind)")
    for kind, blobs in files.items():
        stats = ref.new_stats()
        t0 = time.perf_counter()
        ref.coefficients(blobs[0], stats, simulate=True)
        say(f"   {kind}: {parse(blobs[0]).segments} intervals, {stats['chunks']} chunks, at most {stats['sync_rounds_max']} rounds behind "
            f"round 0 in a chunk ({time.perf_counter() - t0:.0f} s on the host)")
    say()
    say("not measured: real camera streams")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def stages(a):
    """--section stages: the medians per kernel of the kernel traces under ``--trace``/trace_*, appended to ``--out``"""
    import csv
    import glob
    lines = ["", "4. the four launches by stage (rocprofv3 --kernel-trace of `--section launches --kind K`, ten calls of 64 frames; "
                 "median (min - max) per launch)"]
    for d in sorted(glob.glob(os.path.join(a.trace, "trace_*"))):
        if not os.path.isdir(d):
            continue
        per = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    name = row.get("Kernel_Name", "")
                    if "jpegd_" in name:
                        short = name[name.index("jpegd_"):].split("E")[0].split("(")[0]
                        per.setdefault(short, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6)
        lines.append(f"   {os.path.basename(d)[6:].replace('_', ' ')}:" + ("" if per else " no kernel trace found"))
        for name in ("jpegd_segments", "jpegd_entropy", "jpegd_idct", "jpegd_colour"):
            v = per.get(name)
            if v:
                lines.append(f"      {name:16s}: {statistics.median(v):9.3f} ms ({min(v):.3f} - {max(v):.3f}; {len(v)} launches)")
    print("\n".join(lines))
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
