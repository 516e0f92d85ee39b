"""Time of the gallery audit on one view of a ``DeviceGallery``, beside the nearest thing the library offered
before it: ``view.match_topk_device(view.rows(), k=2)``, the exact f32 scan of every row against the view (at most one partner
per row).

Unit Gaussian rows with 0.1 % planted duplicate pairs (cosine 0.8), slab filled in a shuffled id order, thr = 0.4.  One process
per gallery size, each under its own ``timeout``, started one after the other by a parent that never touches the GPU; a size
that fails ends the run.  Inside a process the two variants alternate after 3 warm-ups; every figure is the median (min .. max)
of ``--reps`` wall-clock timings with a synchronise on either side.  The 1 M step is sized from the 100 k figures x 100 before it
is started: what does not fit the step's limit is reported as NOT MEASURED.  The split over the launches comes from a
``rocprofv3 --kernel-trace --stats`` run of a few audits at 100 k rows, a process of its own.

    python tools/gallery_audit_time.py [--reps 20] [--out profiles/gallery_audit.txt] [--no-trace]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (10_000, 100_000, 1_000_000)
LIMIT = {10_000: 180, 100_000: 360, 1_000_000: 540}        # seconds per size
PEAK_F16 = 2.5e15                                          # FLOP/s, the f16 MFMA peak DESIGN.md uses
THR = 0.4
KERNELS = ("gallery_gmax_update", "pair_gather_f16", "pair_scan_f16", "pair_recheck")
RESOURCES = """kernel resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, the library's flags):
  pair_scan_f16     208 VGPRs  0 AGPRs  36 SGPRs  0 B scratch  128 KB dynamic LDS  2 waves/SIMD (one block of 8 waves per CU)
  pair_recheck       36 VGPRs  0 AGPRs  36 SGPRs  0 B scratch  no LDS              8 waves/SIMD
  pair_gather_f16    13 VGPRs  0 AGPRs  22 SGPRs  0 B scratch  no LDS              8 waves/SIMD"""     # quoted from the compile, not measured here


def one_size(N, reps, base, audits_only=0):
    import torch
    from facerecognition_infrenceengine_amd.gallery import DeviceGallery

    g = torch.Generator(device="cuda").manual_seed(11)
    G = torch.randn((N, 512), generator=g, device="cuda")
    G /= G.norm(dim=1, keepdim=True)
    ndup = max(N // 1000, 1)
    src, dst = torch.arange(ndup, device="cuda"), N - 1 - torch.arange(ndup, device="cuda")
    w = torch.randn((ndup, 512), generator=g, device="cuda")
    w -= (w * G[src]).sum(1, keepdim=True) * G[src]
    w /= w.norm(dim=1, keepdim=True)
    G[dst] = 0.8 * G[src] + 0.6 * w
    order = torch.randperm(N, generator=g, device="cuda")
    ids = order.tolist()
    gal = DeviceGallery("cuda:0", capacity=N + 1024)
    for c in range(0, N, 250_000):
        gal.upsert(ids[c:c + 250_000], G[order[c:c + 250_000]])
    view = gal.view(range(N))
    del G

    def audit():
        return view.find_duplicates_device(thr=THR, max_pairs=1 << 20)

    keys, _, counts = audit()
    cnt = counts.cpu().tolist()
    assert cnt[2] == 0, cnt
    k = keys[:cnt[1]].cpu()
    found = set(zip((k >> 32).tolist(), (k & 0xFFFFFFFF).tolist()))
    assert all((i, N - 1 - i) in found for i in range(ndup)), "a planted pair is missing"
    if audits_only:                                          # the run a kernel trace is taken of
        for _ in range(audits_only):
            audit()
        torch.cuda.synchronize()
        return {"N": N}
    variants = {"audit": audit}
    if base:
        rows = view.rows()
        variants["topk2"] = lambda: view.match_topk_device(rows, k=2)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(3):
        for fn in variants.values():
            fn()
    t = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            t[name].append(timed(fn))
    return {"N": N, "device": torch.cuda.get_device_name(0), "planted": ndup, "pairs": cnt[1], "candidates": cnt[0], "ranges": cnt[3],
            **{name: [statistics.median(v), min(v), max(v)] for name, v in t.items()}}


def child(args, limit, prefix=()):
    cmd = [*prefix, sys.executable, os.path.abspath(__file__), *args]
    p = subprocess.run(["timeout", "-k", "10", str(limit), *cmd], stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        return p.returncode, None
    return 0, json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("ROW ")][-1][4:])


def kernel_split(N, audits):
    """average ms per launch of the audit's kernels from rocprofv3's kernel stats, or a reason why there is none"""
    if not shutil.which("rocprofv3"):
        return None, "rocprofv3 not found"
    d = tempfile.mkdtemp(prefix="audit_trace_")
    try:
        rc, _ = child(["--size", str(N), "--audits-only", str(audits)], 300,
                      ("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"))
        if rc != 0:
            return None, f"the traced run ended with status {rc}"
        split = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name", "")
                for kname in KERNELS:
                    if kname in name and row.get("AverageNs"):
                        split[kname] = (float(row["AverageNs"]) / 1e6, int(row["Calls"]))
        return (split, None) if split else (None, "no kernel stats in the profiler's output")
    finally:
        shutil.rmtree(d, ignore_errors=True)


def cell(v):
    return f"{v[0]:.3f} ({v[1]:.3f} .. {v[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gallery_audit.txt"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--size", type=int, default=0, help="(internal) measure one gallery size and print its row as JSON")
    ap.add_argument("--no-base", action="store_true", help="(internal) the audit alone")
    ap.add_argument("--audits-only", type=int, default=0, help="(internal) run this many audits and nothing else")
    a = ap.parse_args()
    if a.size:
        print("ROW " + json.dumps(one_size(a.size, a.reps, not a.no_base, a.audits_only)), flush=True)
        return 0
    rows, notes = [], []
    for N in SIZES:                                          # one child per size, each under its own time limit
        args = ["--size", str(N), "--reps", str(a.reps)]
        if N == 1_000_000:                                   # sized from the 100 k figures x 100; setup (2 GB of rows) allowed 60 s
            r100 = rows[-1]
            runs = a.reps + 4
            est_a, est_b = r100["audit"][0] * 100 * runs / 1e3, r100["topk2"][0] * 100 * runs / 1e3
            if 60 + est_a > LIMIT[N]:
                notes.append(f"N=1,000,000: NOT MEASURED (the audit alone is estimated at {est_a:.0f} s of a {LIMIT[N]} s step)")
                continue
            if 60 + est_a + est_b > LIMIT[N]:
                notes.append(f"N=1,000,000: topk2 NOT MEASURED (estimated at {est_b:.0f} s of a {LIMIT[N]} s step)")
                args.append("--no-base")
        rc, row = child(args, LIMIT[N])
        if rc != 0:
            print(f"size {N}: exit status {rc}; nothing more is started", flush=True)
            return 2
        rows.append(row)
        print(f"size {N}: done", flush=True)
    split, why = (None, "--no-trace") if a.no_trace else kernel_split(100_000, 5)
    lines = [f"gallery audit (find_duplicates_device, thr {THR}, max_pairs 2^20) on one view of a DeviceGallery: ms, median (min .. max) of",
             f"{a.reps} wall-clock timings with a synchronise on either side, after 3 warm-ups, the variants alternating in one process per",
             "size.  Unit Gaussian rows, 0.1 % planted duplicate pairs (cosine 0.8), slab filled in a shuffled id order.",
             "topk2 = view.match_topk_device(view.rows(), k=2): the exact f32 scan of every row against the view.",
             f"f16 = N^2 / 2 x 1024 FLOP / median, as a fraction of {PEAK_F16 / 1e15:.1f} PFLOP/s.", f"device: {rows[0]['device']}", ""]
    met = None
    for r in rows:
        frac = r["N"] ** 2 / 2 * 1024 / (r["audit"][0] * 1e-3) / PEAK_F16
        line = (f"N={r['N']:>9,}: audit {cell(r['audit'])} | f16 {frac:.3f} | {r['ranges']} row ranges | {r['pairs']} pairs "
                f"({r['planted']} planted), {r['candidates']} candidates = {r['candidates'] / max(r['pairs'], 1):.2f} per pair")
        if "topk2" in r:
            gain = r["topk2"][0] - r["audit"][0]
            spread = (r["topk2"][2] - r["topk2"][1]) + (r["audit"][2] - r["audit"][1])
            line += f" | topk2 {cell(r['topk2'])} | {r['topk2'][0] / r['audit'][0]:.1f}x"
            if r["N"] == 100_000:
                met = gain > -spread
        lines.append(line)
    lines += notes
    lines.append("")
    lines.append("condition (100 k rows: the audit not slower than topk2 by more than both sides' min .. max spread): "
                 + ("NOT MEASURED" if met is None else "met" if met else "NOT met"))
    lines.append("")
    if split:
        lines.append("the launches at 100 k rows (rocprofv3 --kernel-trace --stats, average ms per launch, a separate process):")
        for kname in KERNELS:
            if kname in split:
                lines.append(f"  {kname:<22} {split[kname][0]:.4f} ms  ({split[kname][1]} calls)")
    else:
        lines.append(f"the split over the launches: NOT MEASURED ({why})")
    lines += ["", RESOURCES]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if met else 1


if __name__ == "__main__":
    sys.exit(main())
