"""Dev tool -> profiles/pnet_pyramid_ab.txt: the detector alone on a 64 x 1080p batch under its two P-Net launch plans,
MTCNNHIP.pyramid_launch False (a launch chain per level, levels 1.. on two side streams / on one stream) against True (every
layer one launch over the whole pyramid), same process, rounds interleaved, median of 10 calls per round, minimum of the
medians; the P-Net phase from the cascade's phase marks; then split_pconv1_min_px re-taken under the pyramid plan.
usage: python tools/ab_pnet_pyramid.py [rounds]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import math, warnings
import torch, bench
from facerecognition_infrenceengine_amd import FaceAnalysis
from facerecognition_infrenceengine_amd.mtcnn import pyramid_scales
warnings.simplefilter("ignore")
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 6
app = FaceAnalysis(name="synthetic", arch="r100", cap_o=4).prepare(ctx_id=0)
det = app.det
frames = bench.synth_frames(64, 1080, 1920, 0, torch.device("cuda:0"))


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


plans = (("per-level, 2 side streams", dict(pyramid_launch=False, one_stream=False)),
         ("per-level, one stream", dict(pyramid_launch=False, one_stream=True)),
         ("pyramid-wide", dict(pyramid_launch=True, one_stream=False)))
print(f"# detector alone, 64 x 1080p, split_pconv1_min_px {det.split_pconv1_min_px}: median of 10 per round, ms (detect_batch | P-Net phase)")
acc = {name: [] for name, _ in plans}
for rnd in range(rounds):
    row = []
    for name, attrs in plans:
        for k, v in attrs.items():
            setattr(det, k, v)
        acc[name].append(median_ms())
        row.append(f"{name}: {acc[name][-1][0]:.3f} | {acc[name][-1][1]:.3f}")
    print(f"round {rnd}:  " + "   ".join(row), flush=True)
for name, _ in plans:
    print(f"min of medians  {name:28s} detect {min(t for t, _ in acc[name]):.3f} ms   P-Net phase {min(p for _, p in acc[name]):.3f} ms")

print("\n# split_pconv1_min_px under the pyramid plan: levels whose conv1 takes the f16 form, three interleaved rounds, min of medians")
det.pyramid_launch, det.one_stream = True, False
lv = []
for s in pyramid_scales(1080, 1920):
    h, w = det.p1.out_hw(int(math.ceil(1080 * s)), int(math.ceil(1920 * s)))
    lv.append(h * w)
print("# conv1 map pixels per level:", lv)
gates = [10 ** 9] + [lv[i] for i in (0, 1, 2, 3, 4, 5, 6, 8)] + [25]
res = {g: [] for g in gates}
for rnd in range(3):
    for g in gates:
        det.split_pconv1_min_px = g
        res[g].append(median_ms())
        nl = len(det._tls.path["pconv1_mfma_levels"])
for g in gates:
    det.split_pconv1_min_px = g
    nl = sum(1 for p in lv if p >= g)
    print(f"  min_px {g:>10d}: f16 levels {nl:2d}   detect {min(t for t, _ in res[g]):.3f} ms   P-Net phase {min(p for _, p in res[g]):.3f} ms", flush=True)
