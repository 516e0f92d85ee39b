"""Times the device JPEG decoder's oriented last launch (DESIGN.md 4.5j "Orientation") on one MI355X; writes
profiles/jpeg_orient.txt.  Medians of 30 after 3 warm-ups, the variants alternating in one process (the helpers of
tools/hud_time.py).

The workloads: 64 x 1080p files at quality 80, 4:2:0, no DRI (the kind tools/jpeg_decode_time.py uses), and 8 files of
4032 x 3024, what a phone sends.  The variants: fr_jpeg_decode_refs_u8 (the baseline) and fr_jpeg_decode_oriented_refs_u8 with
every frame at orientation 1, 3 and 6.  ``--lib LABEL=PATH`` (repeatable) adds another build of the library: its old entry, and
its new entry at 6 when it has one - the parent commit's build, or a build whose last launch is written another way.

  1. all four launches (HIP events round the call), the files on the device.
  2. the launches one by one: ``--section launches`` runs every variant ten times in a fixed order for a kernel trace, and
     ``--section stages --trace DIR`` appends the traces' medians per kernel and variant to the profile.
  1b. ``--section libs``: the ``--lib`` builds alone in a process of their own (the parent commit's baseline), appended.
  3. ``FaceAnalysis.get_batch_jpeg`` of the phone-sized files (tagged 6) with and without ``orient``, wall time of the call
     (synthetic weights, det_size 640).

No pass mark, nothing here is asserted in a test.
Usage: python tools/jpeg_orient_time.py [--reps 30] [--section all|launches|stages|libs] [--lib LABEL=PATH] [--out profiles/jpeg_orient.txt]"""
import argparse
import ctypes
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

from hud_time import WARM, event_alternate, wall_alternate  # noqa: E402

OLD, NEW = "fr_jpeg_decode_refs_u8", "fr_jpeg_decode_oriented_refs_u8"
SIZES = {"64 x 1080p": (64, 1080, 1920), "8 x 4032 x 3024": (8, 3024, 4032)}


def pictures(h, w, count):
    """synthetic frames with sensor-like noise, so that the files have a camera's size; the phone-sized ones are a quarter-size
    frame enlarged (the synthetic faces are drawn for video sizes)"""
    from make_golden import synth_frame
    rng = np.random.default_rng(0)
    out = []
    for i in range(count):
        k = 4 if h > 2000 else 1
        f = synth_frame(h // k, w // k, 900 + i)
        f = np.repeat(np.repeat(f, k, axis=0), k, axis=1)
        out.append(np.clip(f.astype(np.int16) + rng.normal(0, 4, f.shape).round().astype(np.int16), 0, 255).astype(np.uint8))
    return out


def entries(a):
    """label -> {OLD: fn, NEW: fn or None}: the project's library first, then every ``--lib``"""
    from facerecognition_infrenceengine_amd import _lib
    lib = _lib.load()
    out = {"": {OLD: lib.fr_jpeg_decode_refs_u8, NEW: lib.fr_jpeg_decode_oriented_refs_u8}}
    for spec in a.lib:
        label, path = spec.split("=", 1)
        cdll, fns = ctypes.CDLL(os.path.abspath(path)), {}
        for name in (OLD, NEW):
            fn = getattr(cdll, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = _lib.SIGNATURES[name]
            fns[name] = fn
        out[label] = fns
    return out


def variants_of(a, dev):
    """name -> launch function, for both workloads; the keep-alive list; the status tensors"""
    from facerecognition_infrenceengine_amd import _lib
    from facerecognition_infrenceengine_amd.jpeg_decode import JpegDecoder
    from facerecognition_infrenceengine_amd.letterbox import frame_table
    from tests.helpers import jpeg_decode_cases as cases
    lib = _lib.load()
    dec = JpegDecoder(dev)
    libs = entries(a)
    variants, keep, sizes = {}, [], {}
    for load, (N, H, W) in SIZES.items():
        base = [cases.pil_file(f, 80, "420") for f in pictures(H, W, 8 if N > 8 else 2)]
        blobs = [base[i % len(base)] for i in range(N)]
        sizes[load] = sum(len(b) for b in blobs)
        recs, headers = dec.describe(blobs)
        data = bytearray()
        for f, hd in enumerate(headers):
            recs["scan_off"][f] = len(data)
            data += bytes(blobs[f][hd.scan:]) + bytes(-len(blobs[f][hd.scan:]) % 16)
        stream = torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).to(dev)
        table = torch.from_numpy(recs.view(np.uint8).copy()).to(dev)
        ws_bytes = int(lib.fr_jpeg_decode_workspace(N, H, W, 1))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty(N * H * W * 3, dtype=torch.uint8, device=dev)
        status = torch.empty(N, dtype=torch.int32, device=dev)
        refs = {}
        for turned in (False, True):
            tab, _ = frame_table([out.data_ptr() + i * H * W * 3 for i in range(N)], [(W, H) if turned else (H, W)] * N)
            refs[turned] = torch.from_numpy(tab).to(dev)
        words = {o: torch.full((N,), o, dtype=torch.int32, device=dev) for o in (1, 3, 6)}
        qt, ht = dec._tables_on_device()
        keep.append((stream, table, ws, out, status, refs, words, blobs, (N, H, W)))

        def launch(fn, o, N=N, H=H, W=W, stream=stream, table=table, ws=ws, ws_bytes=ws_bytes, status=status, refs=refs, words=words,
                   nbytes=len(data)):
            qt, ht = dec._tables_on_device()
            head = (_lib.ptr(stream), nbytes, _lib.ptr(table), N, H, W, 1, _lib.ptr(qt), int(qt.shape[0]), _lib.ptr(ht), int(ht.shape[0]),
                    _lib.ptr(dec._natural), _lib.ptr(refs[o is not None and o > 4]))
            tail = (_lib.ptr(status), _lib.ptr(ws), ws_bytes, _lib.stream_ptr())
            rc = fn(*head, *tail) if o is None else fn(*head, _lib.ptr(words[o]), *tail)
            assert rc == 0
        for label, fns in libs.items():
            tag = f" [{label}]" if label else ""
            variants[f"{load}: {OLD}{tag}"] = lambda fn=fns[OLD], launch=launch: launch(fn, None)
            for o in ((1, 3, 6) if not label else (6,)):
                if fns[NEW] is not None:
                    variants[f"{load}: {NEW}, orientation {o}{tag}"] = lambda fn=fns[NEW], o=o, launch=launch: launch(fn, o)
    return variants, keep, sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--section", default="all", choices=("all", "launches", "stages", "libs"))
    ap.add_argument("--lib", action="append", default=[], help="LABEL=PATH: another build of libfrhip.so to time beside the project's")
    ap.add_argument("--trace", default=None, help="directory of the rocprofv3 kernel trace (csv): --section launches notes the "
                                                  "variants' order there, --section stages reads both")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_orient.txt"))
    a = ap.parse_args()
    assert a.reps >= 30, "medians of at least 30"
    if a.section == "stages":
        return stages(a)
    dev = torch.device("cuda:0")
    lines = [f"device JPEG decoder, EXIF orientation: medians of {a.reps} after {WARM} warm-ups, variants alternating in one process",
             f"device: {torch.cuda.get_device_name(0)}", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def report(t, unit=1.0, what="ms"):
        for k, v in t.items():
            m = statistics.median(v)
            say(f"   {k:78s}: {m * unit:10.3f} {what} (min {min(v) * unit:.3f}, max {max(v) * unit:.3f})")

    variants, keep, sizes = variants_of(a, dev)
    if a.section == "launches":
        for _ in range(10):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        if a.trace:                                      # the order, for --section stages
            os.makedirs(a.trace, exist_ok=True)
            with open(os.path.join(a.trace, "variants.txt"), "w") as f:
                f.write("\n".join(variants) + "\n")
        return
    if a.section == "libs":                              # the --lib builds alone, in a process of their own: appended
        t = event_alternate({k: fn for k, fn in variants.items() if k.endswith("]")}, a.reps)
        lines[:] = ["1b. all four launches, the --lib builds alone in a process of their own"]
        report(t)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
        return
    t = event_alternate(variants, a.reps)
    for k in keep:
        assert (k[4].cpu().numpy() == 0).all()
    # once more at 6: the pixels are the host decoder's, turned
    from facerecognition_infrenceengine_amd.jpeg_decode import orient
    from tests.helpers import jpeg_decode_cases as cases
    for load, k in zip(SIZES, keep):
        variants[f"{load}: {NEW}, orientation 6"]()
        N, H, W = k[8]
        got = k[3][:H * W * 3].cpu().numpy().reshape(W, H, 3)
        assert np.array_equal(got, orient(cases.pil_decode(k[7][0]), 6)), "the device's pixels are not Pillow's, turned"
    say("1. all four launches (HIP events round the call), the files on the device")
    report(t)
    for load, nbytes in sizes.items():
        N, H, W = SIZES[load]
        say(f"   {load}: {nbytes / 1e6:.2f} MB of files for {N * H * W * 3 / 1e6:.1f} MB of BGR")
    say()
    del variants, t
    blobs = keep[1][7]
    del keep
    torch.cuda.empty_cache()

    # ---- 3. the call above: get_batch_jpeg of the phone-sized files
    from facerecognition_infrenceengine_amd import FaceAnalysis
    from tests.helpers import exif_cases
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        app = FaceAnalysis(name="synthetic", arch="r100", cap_o=4).prepare(ctx_id=0, det_size=(640, 640))
    tagged = [exif_cases.with_orientation(b, 6) for b in blobs]
    t = wall_alternate({"get_batch_jpeg(orient=False), 8 x 4032 x 3024 tagged 6": lambda: app.get_batch_jpeg(tagged),
                        "get_batch_jpeg(orient=True), 8 x 4032 x 3024 tagged 6": lambda: app.get_batch_jpeg(tagged, orient=True)}, a.reps)
    say("3. FaceAnalysis.get_batch_jpeg of the phone-sized files (synthetic weights, det_size 640), wall time of the call")
    report(t, unit=1e3)
    say()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def stages(a):
    """--section stages: per variant of ``--section launches`` the medians per kernel of the kernel trace under ``--trace``,
    appended to ``--out``.  Every call is four launches and the variants ran in a fixed order, ten times: the trace's jpegd_
    rows in order of their start are that order."""
    import csv
    import glob
    names = [ln.strip() for ln in open(os.path.join(a.trace, "variants.txt")) if ln.strip()]
    rows = []
    for path in glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "")
                if "jpegd_" in name:
                    short = name[name.index("jpegd_"):].split("E")[0].split("(")[0]
                    rows.append((int(row["Start_Timestamp"]), short, (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6))
    rows.sort()
    lines = ["2. the launches one by one (rocprofv3 --kernel-trace of `--section launches`: every variant ten times in turn; median "
             "(min - max) per launch)"]
    if len(rows) != 40 * len(names):
        lines.append(f"   {len(rows)} jpegd_ launches in the trace where {40 * len(names)} were expected: not split")
    else:
        per = {}
        for i in range(0, len(rows), 4):
            for _, short, ms in rows[i:i + 4]:
                per.setdefault((names[i // 4 % len(names)], short), []).append(ms)
        for name in names:
            lines.append(f"   {name}")
            for (n, short), v in per.items():
                if n == name:
                    lines.append(f"      {short:22s}: {statistics.median(v):9.3f} ms ({min(v):.3f} - {max(v):.3f}; {len(v)} launches)")
    lines.append("")
    print("\n".join(lines))
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
