"""A/B of the gallery scans a view can use: the f32 view scan, the coarse f16 / fp8 view scans through the
slot list, and the contiguous coarse scans of the same rows (``GalleryMatcher(scan=...)``).

One process, after warm-up, the variants alternating; every figure is a median of ``--reps`` HIP-event timings on one
stream.  ``match_device(renormalise=False)`` is timed: the scan and its re-rank / reduce, nothing else.  The slab is
filled in a shuffled id order, so the view in id order is a permutation of the slots (the gather case, not a contiguous
run).  Achieved bytes/s are stated against the algorithmic ``N * 512 * b`` per pass (b = 4 / 2 / 1), one pass per 32-query
group for the f32 scan and per 256-query tile for the coarse ones.  Writes ``profiles/view_scan.txt`` (``--out``).

    python tools/view_scan_ab.py [--reps 30]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (10_000, 100_000, 1_000_000)
QUERIES = (16, 256, 1024)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(variants, reps, warmup=3):
    """{name: fn} -> {name: median ms}; the variants take turns inside every repetition"""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            t[k].append(timed(fn))
    return {k: statistics.median(v) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_scan.txt"))
    a = ap.parse_args()
    assert a.reps >= 30, "medians of at least 30"
    from facerecognition_infrenceengine_amd.gallery import DeviceGallery, GalleryMatcher
    lines = [f"view scan A/B: medians of {a.reps} HIP-event timings, variants alternating in one process, one stream",
             f"device: {torch.cuda.get_device_name(0)}",
             "columns: ms | algorithmic TB/s = passes * N * 512 * b / time (passes: ceil(F/32) f32, ceil(F/256) coarse)", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device="cuda").manual_seed(7)
    verdict = []
    for N in SIZES:
        G = torch.randn((N, 512), generator=g, device="cuda")
        G /= G.norm(dim=1, keepdim=True)
        order = torch.randperm(N, generator=g, device="cuda")
        ids = order.tolist()
        views, flat = {}, {}
        for scan in ("f32", "f16", "f8"):
            gal = DeviceGallery("cuda:0", capacity=N + 1024, scan=scan)
            for c in range(0, N, 250_000):
                gal.upsert(ids[c:c + 250_000], G[order[c:c + 250_000]])
            views[scan] = gal.view(range(N))
            if scan != "f32":
                flat[scan] = GalleryMatcher("cuda:0", scan=scan)
                flat[scan].set_rows(range(N), G, normalise=False)
        for F in QUERIES:
            Q = torch.randn((F, 512), generator=g, device="cuda")
            Q /= Q.norm(dim=1, keepdim=True)
            ref = views["f32"].match_device(Q, renormalise=False)[0]
            for scan in ("f16", "f8"):                       # the timed variants compute the same ids
                assert torch.equal(views[scan].match_device(Q, renormalise=False)[0], ref)
                assert torch.equal(flat[scan].match_device(Q, renormalise=False)[0], ref)
            variants = {"view f32": lambda: views["f32"].match_device(Q, renormalise=False),
                        "view f16": lambda: views["f16"].match_device(Q, renormalise=False),
                        "view f8": lambda: views["f8"].match_device(Q, renormalise=False),
                        "flat f16": lambda: flat["f16"].match_device(Q, renormalise=False),
                        "flat f8": lambda: flat["f8"].match_device(Q, renormalise=False)}
            med = alternate(variants, a.reps)
            width = {"view f32": 4, "view f16": 2, "view f8": 1, "flat f16": 2, "flat f8": 1}
            cells = []
            for k, ms in med.items():
                passes = -(-F // 32) if k == "view f32" else -(-F // 256)
                cells.append(f"{k} {ms:.4f} ms {passes * N * 512 * width[k] / (ms * 1e-3) / 1e12:.2f} TB/s")
            say(f"N={N:>9,} F={F:>4}: " + " | ".join(cells))
            say(f"{'':>21}view f16 = {med['view f32'] / med['view f16']:.2f}x the f32 view scan, {med['view f16'] / med['flat f16']:.2f}x the time of "
                f"the contiguous f16 scan; view f8 = {med['view f32'] / med['view f8']:.2f}x the f32 view scan, "
                f"{med['view f8'] / med['flat f8']:.2f}x the time of the contiguous fp8 scan")
            if (N, F) == (1_000_000, 256):
                verdict = [med["view f32"], med["view f16"], med["view f8"]]
        del views, flat, G
        torch.cuda.empty_cache()
    say()
    ok = verdict[1] < verdict[0] and verdict[2] < verdict[0]
    say(f"condition (N = 1 M, F = 256: each coarse view scan faster than the f32 view scan): f32 {verdict[0]:.4f} ms, "
        f"f16 {verdict[1]:.4f} ms, fp8 {verdict[2]:.4f} ms -> {'met' if ok else 'NOT met'}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
