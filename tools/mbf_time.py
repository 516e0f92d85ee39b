"""Times PlanRecogniserHIP.forward at B = 1, 64 and 256 resident crops (warm-up, median of >= 20 runs, device events) on the
MobileFaceNet-shaped seeded graph of tests/helpers/mbf_onnx.py, and - same process - the IResNet-50 forward as the figure a user
switching packs would see (the two networks do different work: a figure, not a gate).  For the three depthwise layers that move
the most bytes it times fr_dw_conv_f16 alone at B = 256 and reports bytes in + bytes out over time as a fraction of the HBM
rate.  Prints its lines and, given a path, writes them there too.  Usage: python tools/mbf_time.py [OUT.txt]"""
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from facerecognition_infrenceengine_amd import _lib, weights                      # noqa: E402
from facerecognition_infrenceengine_amd.iresnet import IResNetHIP                 # noqa: E402
from facerecognition_infrenceengine_amd.mbf import PlanRecogniserHIP              # noqa: E402
from tests.helpers.mbf_onnx import CFG_FULL, write_mbf_onnx                       # noqa: E402
from tests.helpers.mbf_ref import seeded_crops                                    # noqa: E402

HBM_RATE = 8.0e12          # HBM3E rate of the MI355X, bytes/s


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
    lines = []
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "w600k_mbf.onnx")
        write_mbf_onnx(path, CFG_FULL, seed=21, fold_bn=True)
        rec = PlanRecogniserHIP(path)
    r50 = IResNetHIP(weights.synth_iresnet_state("r50"), "r50", "cuda:0")
    base = seeded_crops(8, seed=8).cuda()
    for n in (1, 64, 256):
        x = base.repeat((n + 7) // 8, 1, 1, 1)[:n].contiguous()
        med, lo, hi = median_ms(lambda: rec.forward(x))
        arena = sum(b.numel() for b in rec._arena(n).blocks) / 2 ** 20
        lines.append(f"mbf  B={n:3d}  {med:8.3f} ms/forward (min {lo:.3f}, max {hi:.3f}); {n / (med * 1e-3):9.0f} faces/s; 2*MAC = "
                     f"{rec.flops_per_face * n / 1e9:.2f} G; activation arena {arena:.1f} MiB")
        med, lo, hi = median_ms(lambda: r50.forward(x))
        lines.append(f"r50  B={n:3d}  {med:8.3f} ms/forward (min {lo:.3f}, max {hi:.3f}); {n / (med * 1e-3):9.0f} faces/s (synthetic weights, same crops)")
    # the depthwise layers alone, B = 256: bytes in + bytes out over time
    plan, lib, B = rec.plan, _lib.load(), 256
    dws = [(i, s) for i, s in enumerate(plan.steps) if s["op"] == "dwconv"]

    def nbytes(s):
        (ci, hi, wi), (co, ho, wo) = plan.shapes[s["x"]], plan.shapes[s["out"]]
        return 2 * B * (ci * hi * wi + co * ho * wo)
    seen = set()
    for i, s in sorted(dws, key=lambda e: -nbytes(e[1])):
        (c, h, w), (_, ho, wo) = plan.shapes[s["x"]], plan.shapes[s["out"]]
        if (c, h, w, s["stride"]) in seen or len(seen) == 3:
            continue
        seen.add((c, h, w, s["stride"]))
        wt, bias, slope, cp, _ = rec.packed[i]
        x = torch.randn((B, h, w, cp), device="cuda").to(torch.float16)
        y = torch.empty((B, ho, wo, cp), dtype=torch.float16, device="cuda")
        st = _lib.stream_ptr()
        med, lo, hi = median_ms(lambda: lib.fr_dw_conv_f16(_lib.ptr(x), _lib.ptr(wt), _lib.ptr(bias), _lib.ptr(slope), _lib.ptr(y), B, h, w, cp,
                                                          s["k"], s["stride"], s["pad"], ho, wo, s["act"], st))
        lines.append(f"dw {s['k']}x{s['k']} s{s['stride']}  {h}x{w}x{c} -> {ho}x{wo}  B={B}  {med * 1e3:8.1f} us (min {lo * 1e3:.1f}); "
                     f"{nbytes(s) / 1e6:.1f} MB in + out; {nbytes(s) / (med * 1e-3) / 1e12:.2f} TB/s = {100 * nbytes(s) / (med * 1e-3) / HBM_RATE:.1f} % of the HBM rate")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
