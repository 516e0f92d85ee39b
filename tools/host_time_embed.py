"""Dev tool: host time (Python + ctypes + allocator, no sync inside) against GPU time of the embed net alone, synthetic r100, in every
batch-size mode - is a forward waiting for the interpreter?  Per batch size the medians of: "host issue ms" = time.perf_counter
around forward without a synchronise, "done ms" = the same until torch.cuda.synchronize returns, "GPU ms" = HIP events around the
call.  Prints one JSON line {row: ms}; ``--profile`` adds the cProfile of 100 forwards of 16 faces (split-K, launch by launch:
the most interpreter work per launch)."""
import json, os, sys, time, cProfile, pstats
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from facerecognition_infrenceengine_amd import weights
from facerecognition_infrenceengine_amd.iresnet import IResNetHIP

net = IResNetHIP(weights.synth_iresnet_state("r100", seed=1234), "r100", "cuda:0")
g = torch.Generator().manual_seed(3)
crops = torch.zeros((256, 112, 112, 8), dtype=torch.float16)
crops[..., :3] = (torch.rand((256, 112, 112, 3), generator=g) * 2 - 1).to(torch.float16)
crops = crops.cuda()
rows = {}


def measure(B, tag):
    x = crops[:B].contiguous()
    for _ in range(5):
        net.forward(x)
    torch.cuda.synchronize()
    host, done, gpu = [], [], []
    for _ in range(200 if B <= 8 else 100 if B <= 64 else 30):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); t0 = time.perf_counter(); net.forward(x); t1 = time.perf_counter(); e1.record(); torch.cuda.synchronize(); t2 = time.perf_counter()
        host.append((t1 - t0) * 1e3); done.append((t2 - t0) * 1e3); gpu.append(e0.elapsed_time(e1))
    for name, v in (("host issue ms", host), ("done ms", done), ("GPU ms", gpu)):
        rows["%s %s" % (tag, name)] = round(float(np.median(v)), 4)


for B in (1, 4, 8, 16, 48, 64, 128, 256):
    measure(B, "b%d" % B)
net.enable_fp8(crops[:64].contiguous(), gptq=False)          # the launches do not depend on how the weights were rounded
measure(256, "b256_fp8")
print(json.dumps(rows))
if "--profile" in sys.argv:
    net.fp8 = False
    x = crops[:16].contiguous()
    pr = cProfile.Profile(); pr.enable()
    for _ in range(100):
        net.forward(x)
    pr.disable(); torch.cuda.synchronize()
    pstats.Stats(pr).sort_stats("tottime").print_stats(14)
