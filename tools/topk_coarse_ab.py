"""A/B of the two top-K paths of a view of an f16-coarse ``DeviceGallery``: the exact f32 top-K scan
(``coarse_topk_min_rows`` out of reach) and the certified coarse top-K (``coarse_topk_min_rows = 0``), same view, same
queries, every query certified (asserted: the flags are all 0, and both paths return the same bits).

One process per gallery size, each under its own ``timeout``, started one after the other by a parent that never touches
the GPU; a size that fails ends the run.  Inside a process the variants alternate after warm-up; every figure is the median
(and min - max) of ``--reps`` HIP-event timings on one stream.  ``match_topk_device(renormalise=False)`` is timed.  The
slab is filled in a shuffled id order, so the view is a permutation of the slots.  Queries are noisy copies of 16 base
directions, each with 16 planted gallery rows (scores about 0.5 .. 0.93, one per sixteenth of the gallery) above a random
background below 0.3: what a certified identification looks like.  Also timed: the exact fallback launch when no query is
flagged (fr_gallery_topk_view_masked_f32 with an all-zero mask), the fixed cost the coarse path pays for having it.

    python tools/topk_coarse_ab.py [--reps 30] [--out profiles/topk_coarse.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (10_000, 100_000, 1_000_000)
QUERIES = (16, 256, 1024)
KS = (5, 16)
LIMIT = {10_000: 240, 100_000: 300, 1_000_000: 540}        # seconds per size


def one_size(N, reps):
    import torch
    from facerecognition_infrenceengine_amd import _lib
    from facerecognition_infrenceengine_amd.gallery import DeviceGallery, last_topk

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    g = torch.Generator(device="cuda").manual_seed(7)
    G = torch.randn((N, 512), generator=g, device="cuda")
    G /= G.norm(dim=1, keepdim=True)
    base = torch.randn((16, 512), generator=g, device="cuda")
    base /= base.norm(dim=1, keepdim=True)
    scores = torch.linspace(0.93, 0.5, 16, device="cuda")
    for c in range(16):                                      # 16 rows per base direction, one per sixteenth of the gallery
        w = torch.randn((16, 512), generator=g, device="cuda")
        w -= (w @ base[c])[:, None] * base[c]
        w /= w.norm(dim=1, keepdim=True)
        rows = torch.arange(16, device="cuda") * (N // 16) + 4 * c
        G[rows] = scores[:, None] * base[c] + (1 - scores * scores).sqrt()[:, None] * w
    order = torch.randperm(N, generator=g, device="cuda")
    ids = order.tolist()
    gal = DeviceGallery("cuda:0", capacity=N + 1024, scan="f16")
    for c in range(0, N, 250_000):
        gal.upsert(ids[c:c + 250_000], G[order[c:c + 250_000]])
    view = gal.view(range(N))
    lib = gal.lib
    out = []
    for F in QUERIES:
        Q = base[torch.arange(F, device="cuda") % 16] + 0.004 * torch.randn((F, 512), generator=g, device="cuda")
        Q /= Q.norm(dim=1, keepdim=True)
        for K in KS:
            def run(min_rows):
                gal.coarse_topk_min_rows = min_rows
                return view.match_topk_device(Q, K, renormalise=False)
            ci, cs = run(0)
            flags = last_topk()["flags"]
            assert last_topk()["path"] == "coarse" and int(flags.sum()) == 0, ("not all certified", N, F, K, int(flags.sum()))
            xi, xs = run(1 << 40)
            assert last_topk()["path"] == "exact"
            assert torch.equal(ci, xi) and torch.equal(cs.view(torch.int32), xs.view(torch.int32)), (N, F, K)
            mask = torch.zeros(F, dtype=torch.int32, device="cuda")
            ti = torch.empty((F, K), dtype=torch.int64, device="cuda")
            ts = torch.empty((F, K), dtype=torch.float32, device="cuda")
            ws = torch.empty(lib.fr_gallery_topk_workspace(F, N, K), dtype=torch.uint8, device="cuda")
            variants = {"exact": lambda: run(1 << 40), "coarse": lambda: run(0),
                        "idle_fallback": lambda: lib.fr_gallery_topk_view_masked_f32(
                            _lib.ptr(Q), _lib.ptr(gal.G), _lib.ptr(view.slots), F, N, 512, K, _lib.ptr(ti), _lib.ptr(ts),
                            _lib.ptr(ws), ws.numel(), _lib.ptr(mask), _lib.stream_ptr())}
            for _ in range(3):
                for fn in variants.values():
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k in variants}
            for _ in range(reps):
                for k, fn in variants.items():
                    t[k].append(timed(fn))
            out.append({"N": N, "F": F, "K": K, "device": torch.cuda.get_device_name(0),
                        **{k: [statistics.median(v), min(v), max(v)] for k, v in t.items()}})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_coarse.txt"))
    ap.add_argument("--size", type=int, default=0, help="(internal) measure one gallery size and print its rows as JSON")
    a = ap.parse_args()
    assert a.reps >= 30, "medians of at least 30"
    if a.size:
        print("ROWS " + json.dumps(one_size(a.size, a.reps)), flush=True)
        return 0
    rows = []
    for N in SIZES:                                          # one child per size, each under its own time limit
        cmd = ["timeout", "-k", "10", str(LIMIT[N]), sys.executable, os.path.abspath(__file__), "--size", str(N),
               "--reps", str(a.reps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print(f"size {N}: exit status {p.returncode}; nothing more is started", flush=True)
            return 2
        rows += json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("ROWS ")][-1][5:])
        print(f"size {N}: done", flush=True)
    lines = [f"top-K A/B on one view of an f16-coarse DeviceGallery: medians (min - max) of {a.reps} HIP-event timings, ms,",
             "variants alternating in one process per gallery size, one stream; every query certified (flags all 0) and",
             "both paths bit-equal (asserted before timing).  exact = fr_gallery_topk_view_f32, coarse = fr_gallery_topk_view_f16",
             "(coarse pass + certified re-rank + idle exact launch + select), idle = the exact launch with no query flagged.",
             f"device: {rows[0]['device']}", ""]

    def cell(v):
        return f"{v[0]:.4f} ({v[1]:.4f} - {v[2]:.4f})"

    wins = {}
    for r in rows:
        spread = r["exact"][2] - r["exact"][1]
        gain = r["exact"][0] - r["coarse"][0]
        ok = gain > spread
        wins.setdefault(r["N"], []).append(ok)
        lines.append(f"N={r['N']:>9,} F={r['F']:>4} K={r['K']:>2}: exact {cell(r['exact'])} | coarse {cell(r['coarse'])} | "
                     f"idle {cell(r['idle_fallback'])} | {r['exact'][0] / r['coarse'][0]:.2f}x | gain {gain:.4f} vs exact spread "
                     f"{spread:.4f}: {'faster' if ok else 'NOT faster'}")
    lines.append("")
    cond = [r for r in rows if r["N"] == 1_000_000 and r["F"] == 256]
    met = all(r["exact"][0] - r["coarse"][0] > r["exact"][2] - r["exact"][1] for r in cond)
    lines.append("condition (N = 1 M, F = 256, K = 5 and 16: coarse faster than exact by more than the exact scan's own min - max "
                 f"spread): {'met' if met else 'NOT met'}")
    cross = None
    for N in sorted(wins, reverse=True):
        if not all(wins[N]):
            break
        cross = N
    lines.append(f"smallest measured size from which the coarse path wins at every F and K: {cross}")
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if met else 1


if __name__ == "__main__":
    sys.exit(main())
