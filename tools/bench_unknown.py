"""Developer script: what one UnknownClusters.assign_batch launch costs for a crowd of unknown faces, and what the
per-face assign() loop it replaces costs for the same rows.

F = 256 taken rows against n = 16 and n = 1024 live clusters, once with rows that hit early clusters and once with
rows that miss (each creates a cluster).  Per cell: 3 warm-ups, then 20 repeats, every repeat from the same restored
state; stream time (events around the call) and wall time (host clock, device idle before and after).

  python tools/bench_unknown.py --impl batch [--loop-json loop.json]     this tree: one assign_batch per repeat
  python tools/bench_unknown.py --impl loop --root DIR --out loop.json   the tree at DIR (a checkout of the commit before
                                                                         assign_batch, built): assign() row by row

The two run as separate processes (each loads its own libfrhip.so); the first form prints the ratio per cell when it
is given the second's JSON.
"""
import argparse
import json
import os
import sys
import time
from collections import deque

import numpy as np

F, WARMUP, REPEATS = 256, 3, 20


def unit(v):
    v = np.asarray(v, np.float32)
    return (v / np.linalg.norm(v)).astype(np.float32)


def cell_rows(n, kind):
    """(the n centres that become the live clusters, the F timed rows)"""
    rng = np.random.default_rng(1000 + n)
    C = np.stack([unit(v) for v in rng.standard_normal((n, 512))])
    if kind == "hit":           # near copies of the first 8 centres: the scan ends in its first round
        rows = np.stack([unit(C[i % 8] + 0.02 * rng.standard_normal(512)) for i in range(F)])
    else:                       # fresh directions: every row scans all n (and the clusters made before it) and opens one
        rows = np.stack([unit(v) for v in rng.standard_normal((F, 512))])
    return C, rows


def summary(ts):
    ts = sorted(ts)
    return {"median_ms": 0.5 * (ts[len(ts) // 2 - 1] + ts[len(ts) // 2]) if len(ts) % 2 == 0 else ts[len(ts) // 2],
            "min_ms": ts[0], "max_ms": ts[-1]}


def timed(torch, run, restore):
    stream_ms, wall_ms = [], []
    for k in range(WARMUP + REPEATS):
        restore()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if k >= WARMUP:
            stream_ms.append(a.elapsed_time(b))
            wall_ms.append((t1 - t0) * 1e3)
    return {"stream": summary(stream_ms), "wall": summary(wall_ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--impl", choices=["batch", "loop"], required=True)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out")
    ap.add_argument("--loop-json")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from facerecognition_infrenceengine_amd.enrol import UnknownClusters
    results = {}
    for n in (16, 1024):
        for kind in ("hit", "miss"):
            C, rows = cell_rows(n, kind)
            uc = UnknownClusters("cuda:0", capacity=n + F + 8)
            if args.impl == "batch":
                uc.assign_batch(C)
                dev_rows = torch.from_numpy(rows).cuda()
                saved = [t.clone() for t in (uc.avg, uc._hist, uc._state)]

                def restore():
                    for dst, src in zip((uc.avg, uc._hist, uc._state), saved):
                        dst.copy_(src)

                def run():
                    uc.assign_batch(dev_rows)
                check = lambda: int(uc._state[0].item())
            else:
                for c in C:
                    uc.assign(c)
                saved = (uc.avg.clone(), [list(d) for d in uc.hist], list(uc.counts))

                def restore():
                    uc.avg.copy_(saved[0])
                    uc.hist = [deque(d, maxlen=uc.depth) for d in saved[1]]
                    uc.counts = list(saved[2])

                def run():
                    for e in rows:
                        uc.assign(e)
                check = lambda: len(uc.hist)
            r = timed(torch, run, restore)
            assert check() == (n if kind == "hit" else n + F), (check(), n, kind)       # the rows did what the cell says
            results[f"n{n}_{kind}"] = r
            print(json.dumps({"impl": args.impl, "cell": f"n{n}_{kind}", **r}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f)
    if args.loop_json:
        loop = json.load(open(args.loop_json))
        for cell, r in results.items():
            for clock in ("stream", "wall"):
                b, l = r[clock], loop[cell][clock]
                print(f"{cell:11s} {clock:6s} batch {b['median_ms']:8.3f} ms [{b['min_ms']:.3f}, {b['max_ms']:.3f}]   "
                      f"loop {l['median_ms']:8.3f} ms [{l['min_ms']:.3f}, {l['max_ms']:.3f}]   "
                      f"loop/batch {l['median_ms'] / b['median_ms']:7.1f}x   "
                      f"faster beyond spread: {b['max_ms'] < l['min_ms']}")


if __name__ == "__main__":
    main()
