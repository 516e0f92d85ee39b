"""Dev tool -> profiles/pnet_coarse_ab.txt: the detector alone on the bench's 64 x 1080p batch with the fused P-Net in two tiers
(MTCNNHIP.coarse_p23 True: a coarse hi-only pass, then the split form over its list) against the one-tier split kernel (False),
same process, one stream, rounds interleaved, median of 10 calls per round, minimum of the medians; the P-Net phase from the
cascade's phase marks; the cells the second tier visits and the cells the exact pass re-evaluates per batch.
usage: python tools/ab_pnet_coarse.py [rounds]
       python tools/ab_pnet_coarse.py trace on|off     four batches of one setting, to be run under rocprofv3 --kernel-trace
                                                       (tools/det_trace_sum.py prints the last batch's kernels)"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import warnings
import torch, bench
from facerecognition_infrenceengine_amd import FaceAnalysis
from facerecognition_infrenceengine_amd.mtcnn import detect_plan
warnings.simplefilter("ignore")
app = FaceAnalysis(name="synthetic", arch="r100", cap_o=4).prepare(ctx_id=0)
det = app.det
det.one_stream = True
frames = bench.synth_frames(64, 1080, 1920, 0, torch.device("cuda:0"))
det.refined_cells = torch.zeros(1, dtype=torch.int32, device="cuda")
det.visited_cells = torch.zeros(1, dtype=torch.int32, device="cuda")


def counted():
    """(cells on the coarse lists, cells the exact pass re-evaluated, faces) of one batch"""
    det.refined_cells.zero_(); det.visited_cells.zero_()
    out = det.detect_batch(frames)
    torch.cuda.synchronize()
    return int(det.visited_cells[0]), int(det.refined_cells[0]), int(out[3].sum())


if len(sys.argv) > 2 and sys.argv[1] == "trace":
    det.coarse_p23 = sys.argv[2] == "on"
    for _ in range(4):
        c = counted()
    print("coarse_p23", det.coarse_p23, "visited / refined / faces per batch", c)
    sys.exit(0)


def median_ms(reps=10):
    """(detect_batch ms, P-Net phase ms): medians over ``reps`` calls, HIP events on the caller's stream"""
    for _ in range(3):
        det.detect_batch(frames)
    torch.cuda.synchronize()
    tot, pn = [], []
    for _ in range(reps):
        det.phase_marks = []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); det.detect_batch(frames); e1.record(); torch.cuda.synchronize()
        m = dict(det.phase_marks)
        det.phase_marks = None
        tot.append(e0.elapsed_time(e1)); pn.append(m["start"].elapsed_time(m["pnet"]))
    return sorted(tot)[reps // 2], sorted(pn)[reps // 2]


rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 6
ncell = sum(64 * (h - 4) * (w - 4) for _, _, h, w in detect_plan(64, 1080, 1920, det).geo)
settings = (("split kernel (coarse_p23 off)", False), ("two tiers (coarse_p23 on)", True))
print(f"# detector alone, 64 x 1080p, one stream, coarse_margin {det.coarse_margin}: median of 10 per round, ms (detect_batch | P-Net phase)")
for name, on in settings:
    det.coarse_p23 = on
    v, r, f = counted()
    print(f"# {name}: {ncell} cells, {v} on the coarse lists ({100.0 * v / ncell:.2f} %), {r} re-evaluated exactly, {f} faces")
acc = {name: [] for name, _ in settings}
for rnd in range(rounds):
    row = []
    for name, on in settings:
        det.coarse_p23 = on
        acc[name].append(median_ms())
        row.append(f"{name}: {acc[name][-1][0]:.3f} | {acc[name][-1][1]:.3f}")
    print(f"round {rnd}:  " + "   ".join(row), flush=True)
for name, _ in settings:
    print(f"min of medians  {name:30s} detect {min(t for t, _ in acc[name]):.3f} ms   P-Net phase {min(p for _, p in acc[name]):.3f} ms")
