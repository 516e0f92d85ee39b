"""Times SCRFDHIP.detect_batch for 1 and 64 resident 640 x 640 canvases (warm-up, median of >= 20 runs, device events) on the
10GF-shaped seeded graph of tests/helpers/scrfd_onnx.py, reports the plan's own 2*MAC count and the achieved fraction of the f16
matrix-core peak, and - same process, same frames - MTCNN under prepare(det_size=(640, 640)) as the figure a user switching
detectors would see (the two detectors do different work: a figure, not a gate).  Prints its lines and, given a path, writes
them there too.  ``--trace``: a short SCRFD-only run (N = 1 and 64, a few calls each) to put under
``rocprofv3 --kernel-trace --stats``.  Usage: python tools/scrfd_time.py [OUT.txt] [--trace]"""
import os
import statistics
import sys
import tempfile
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from facerecognition_infrenceengine_amd import FaceAnalysis                       # noqa: E402
from facerecognition_infrenceengine_amd.scrfd import SCRFDHIP                     # noqa: E402
from tests.helpers.scrfd_onnx import CFG_10G, lowpass_frames, write_scrfd_onnx    # noqa: E402

F16_PEAK = 2.5e15          # dense f16 MFMA peak of the MI355X, FLOP/s


def median_ms(fn, runs=25, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def main():
    args = [a for a in sys.argv[1:] if a != "--trace"]
    trace = "--trace" in sys.argv[1:]
    lines = []
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "det_10g.onnx")
        write_scrfd_onnx(path, CFG_10G, seed=11, fold_bn=True, dynamic=True, score_bias=-7.5)
        det = SCRFDHIP(path)
    macs2 = det.plan((640, 640)).macs2
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mt = None if trace else FaceAnalysis(name="no-such-pack").prepare(ctx_id=0, det_size=(640, 640))
    for n in (1, 64):
        canvas = torch.from_numpy(lowpass_frames(n, 640, 640, seed=5)).cuda()
        scale = torch.ones(n, dtype=torch.float32, device="cuda")
        if trace:
            median_ms(lambda: det.detect_batch(canvas, scale), runs=5, warm=2)
            continue
        med, lo, hi = median_ms(lambda: det.detect_batch(canvas, scale))
        arena = sum(b.numel() for b in det._arena(n, (640, 640)).blocks) / 2 ** 20
        lines.append(f"SCRFD  N={n:2d}  {med:8.3f} ms/call (min {lo:.3f}, max {hi:.3f}); 2*MAC = {macs2 * n / 1e9:.1f} G; "
                     f"{macs2 * n / (med * 1e-3) / 1e12:.1f} TFLOP/s = {100 * macs2 * n / (med * 1e-3) / F16_PEAK:.2f} % of the f16 peak; activation arena {arena:.0f} MiB")
        med, lo, hi = median_ms(lambda: mt.det.detect_batch(canvas))
        lines.append(f"MTCNN  N={n:2d}  {med:8.3f} ms/call (min {lo:.3f}, max {hi:.3f}) on the same canvases (synthetic weights, det_size 640 x 640)")
    text = "\n".join(lines)
    print(text)
    if args:
        with open(args[0], "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
