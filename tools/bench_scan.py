"""Dev tool: gallery scan timings (HIP events), f32 exact vs one-pass f16 / fp8 GEMM scan + f32 re-rank.
usage: python tools/bench_scan.py [NxF ...]
       python tools/bench_scan.py --topk [--out FILE] [NxF ...]    exact top-K scan (K = 1, 4, 16) against the top-1 scan"""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from facerecognition_infrenceengine_amd import _lib
from facerecognition_infrenceengine_amd.gallery import GalleryMatcher


def topk_mode(argv):
    """fr_gallery_topk_f32 at K = 1, 4, 16 against fr_gallery_match_f32 in ONE process, calls interleaved round by round,
    HIP events around every call, median of the rounds.  The baseline is the base build tools/ab/libfrhip_base.so when
    it is there (see tools/ab_lib.py), else this tree's own fr_gallery_match_f32."""
    out = None
    if "--out" in argv:
        out = argv[argv.index("--out") + 1]
        argv = [a for i, a in enumerate(argv) if a != "--out" and argv[i - 1] != "--out"]
    cases = [tuple(int(v) for v in a.split("x")) for a in argv] or [(10_000, 256), (1_000_000, 256)]
    lib = _lib.load()
    base_path = os.path.join(ROOT, "tools", "ab", "libfrhip_base.so")
    P, I, L, Z = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
    if os.path.exists(base_path):
        base, base_name = C.CDLL(base_path), "base build's fr_gallery_match_f32"
        base.fr_gallery_match_f32.argtypes = [P, P, I, L, I, L, P, P, P, Z, P, I, P]
        base.fr_gallery_match_f32.restype = I
        base.fr_gallery_match_workspace.argtypes, base.fr_gallery_match_workspace.restype = [I, L], Z
    else:
        base, base_name = lib, "this build's fr_gallery_match_f32"
    lines = [f"exact top-K scan, {torch.cuda.get_device_name(0)}; baseline = {base_name}; per call: HIP events, "
             f"rounds interleaved (baseline, K=1, K=4, K=16), median", ""]
    g = torch.Generator(device="cuda").manual_seed(1)
    rounds, warm = 30, 5
    for N, F in cases:
        G = torch.randn((N, 512), generator=g, device="cuda"); G /= G.norm(dim=1, keepdim=True)
        Q = torch.randn((F, 512), generator=g, device="cuda"); Q /= Q.norm(dim=1, keepdim=True)
        s = _lib.stream_ptr()
        idx1 = torch.empty(F, dtype=torch.int64, device="cuda"); sc1 = torch.empty(F, dtype=torch.float32, device="cuda")
        ws1 = torch.empty(base.fr_gallery_match_workspace(F, N), dtype=torch.uint8, device="cuda")
        runs = {"top-1": lambda: base.fr_gallery_match_f32(_lib.ptr(Q), _lib.ptr(G), F, N, 512, 0, _lib.ptr(idx1), _lib.ptr(sc1),
                                                           _lib.ptr(ws1), ws1.numel(), None, 0, s)}
        outs = {}
        for K in (1, 4, 16):
            ik = torch.empty((F, K), dtype=torch.int64, device="cuda"); sk = torch.empty((F, K), dtype=torch.float32, device="cuda")
            wk = torch.empty(lib.fr_gallery_topk_workspace(F, N, K), dtype=torch.uint8, device="cuda")
            outs[K] = (ik, sk, wk)
            runs[f"K={K}"] = (lambda ik=ik, sk=sk, wk=wk, K=K: lib.fr_gallery_topk_f32(
                _lib.ptr(Q), _lib.ptr(G), F, N, 512, K, 0, _lib.ptr(ik), _lib.ptr(sk), _lib.ptr(wk), wk.numel(), None, 0, s))
        times = {k: [] for k in runs}
        for r in range(warm + rounds):
            for name, fn in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); rc = fn(); e1.record(); e1.synchronize()
                assert rc == 0, (name, rc)
                if r >= warm:
                    times[name].append(e0.elapsed_time(e1) * 1e3)
        same = all(torch.equal(outs[K][0][:, 0], idx1) and torch.equal(outs[K][1][:, 0].contiguous().view(torch.int32), sc1.view(torch.int32))
                   for K in outs)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        groups = (F + 31) // 32
        lines.append(f"N = {N}, F = {F} ({rounds} rounds; gallery bytes read = {groups} query groups x N x 2 KB; column 0 == top-1 bit for bit: {same})")
        lines.append(f"  {'call':<8}{'median us':>12}{'min us':>10}{'ratio':>8}{'gallery TB/s':>14}")
        for k, v in med.items():
            lines.append(f"  {k:<8}{v:>12.1f}{min(times[k]):>10.1f}{v / med['top-1']:>8.2f}{groups * N * 2048 / v / 1e6:>14.2f}")
        lines.append("")
        del G, Q
    text = "\n".join(lines)
    print(text, flush=True)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


if "--topk" in sys.argv[1:]:
    topk_mode([a for a in sys.argv[1:] if a != "--topk"])
    raise SystemExit(0)

g = torch.Generator(device="cuda").manual_seed(1)
cases = [(10_000, 256), (125_000, 2048), (1_000_000, 256), (1_000_000, 2048), (1_250_000, 2048)]
if len(sys.argv) > 1:
    cases = [tuple(int(v) for v in a.split("x")) for a in sys.argv[1:]]
for N, F in cases:
    G = torch.randn((N, 512), generator=g, device="cuda"); G /= G.norm(dim=1, keepdim=True)
    Q = torch.randn((F, 512), generator=g, device="cuda"); Q /= Q.norm(dim=1, keepdim=True)
    ref = None
    for scan in ("f32", "f16", "f8"):
        if scan == "f32" and N * F > 3e8:
            continue
        m = GalleryMatcher("cuda:0", scan=scan)
        m.set_rows(range(N), G, normalise=False)
        for _ in range(3):
            idx, score = m.match_device(Q, renormalise=False)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 10
        e0.record()
        for _ in range(n):
            idx, score = m.match_device(Q, renormalise=False)
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / n
        b = {"f32": 4, "f16": 2, "f8": 1}[scan]
        same = "" if ref is None else f" ids==first: {bool(torch.equal(idx, ref))}"
        if ref is None:
            ref = idx
        print(f"N={N} F={F} {scan}: {ms*1e3:8.1f} us  {2*N*F*512/ms/1e9:8.1f} TFLOP/s  gallery bytes/time {N*512*b/ms/1e9:7.2f} TB/s{same}", flush=True)
        del m
    del G, Q
