"""Times the enrolment arithmetic of one batch of 256 jobs x 3 poses (synthetic embeddings, no engine) against views of
10 k / 100 k / 1 M rows: median of 20 runs after 3 warm-ups, a device synchronise around each timed region, ms per batch.
  (a) the one-job arithmetic, job by job: check_image_similarity + mean_embedding + check_duplicate (a GalleryMatcher
      holding the view's rows);
  (b) one fr_gallery_first_above_f32 call with F = 256 on the same dense rows;
  (c) Enroller.enrol_slots through the view, and its scan alone (fr_gallery_first_above_blocked_f32, F = 256).
The condition is (c) < (a) at every size; (c)-scan against (b) is a figure, not a gate.
Usage: python tools/enrol_time.py [OUT.txt] [--sizes 10000,100000,1000000]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from facerecognition_infrenceengine_amd import _lib                                            # noqa: E402
from facerecognition_infrenceengine_amd.enrol import DIM, Enroller                             # noqa: E402
from facerecognition_infrenceengine_amd.gallery import DeviceGallery, GalleryMatcher           # noqa: E402

J, POSES, RUNS, WARM = 256, 3, 20, 3


class _NoEngine:
    device = torch.device("cuda:0")


def median_ms(fn, runs=RUNS, warm=WARM):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def unit_rows(n, gen):
    x = torch.empty((n, DIM), dtype=torch.float32, device="cuda:0")
    for a in range(0, n, 1 << 16):                      # in pieces: no second copy of a 2 GB slab
        r = torch.randn((min(1 << 16, n - a), DIM), generator=gen, device="cuda:0")
        x[a:a + r.shape[0]] = r / r.norm(dim=1, keepdim=True)
    return x


def main():
    args, sizes = [], [10_000, 100_000, 1_000_000]
    it = iter(sys.argv[1:])
    for a in it:
        if a == "--sizes":
            sizes = [int(v) for v in next(it).split(",")]
        else:
            args.append(a)
    lib, dev = _lib.load(), torch.device("cuda:0")
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    en = Enroller(_NoEngine())
    people = unit_rows(J, gen)
    poses = people[:, None, :] + 0.5 * unit_rows(J * POSES, gen).reshape(J, POSES, DIM)
    poses = (poses / poses.norm(dim=2, keepdim=True)).reshape(J * POSES, DIM).contiguous()
    poses_h = poses.cpu().numpy()
    slots = {"counts": torch.ones(J * POSES, dtype=torch.int32, device=dev),
             "bbox": torch.tensor([10.0, 20.0, 110.0, 140.0], device=dev).repeat(J * POSES, 1, 1),
             "normed_embedding": poses}
    job_images = [list(range(j * POSES, (j + 1) * POSES)) for j in range(J)]
    lines = [f"enrolment arithmetic, {J} jobs x {POSES} poses, median of {RUNS} after {WARM} warm-ups (min .. max), ms per batch"]
    print(lines[0], flush=True)
    for n in sizes:
        dg = DeviceGallery("cuda:0", capacity=n)
        dg.G = unit_rows(n, gen)
        perm = np.random.default_rng(n).permutation(n)
        dg.slot_of = {i: int(perm[i]) for i in range(n)}
        dg._next = n
        view = dg.view(range(n))
        m = GalleryMatcher("cuda:0")
        m.G, m.ids = view.rows().contiguous(), list(range(n))

        def one_by_one():
            for j in range(J):
                embs = list(poses_h[j * POSES:(j + 1) * POSES])
                ok, _ = en.check_image_similarity(embs)
                dup, _ = en.check_duplicate(en.mean_embedding(embs), m)
                assert ok and not dup

        out = en.enrol_slots(slots, job_images, view)
        torch.cuda.synchronize()
        assert int((out["status"] != 0).sum()) == 0                  # strangers to the gallery and to each other: all done
        q = out["row"].clone()
        idx = torch.empty(J, dtype=torch.int64, device=dev)
        score = torch.empty(J, dtype=torch.float32, device=dev)
        ws = torch.empty(J * 8, dtype=torch.uint8, device=dev)

        def old_scan():
            lib.fr_gallery_first_above_f32(_lib.ptr(q), _lib.ptr(m.G), J, n, DIM, 0.4, 0, 0, _lib.ptr(idx), _lib.ptr(score),
                                           _lib.ptr(ws), J * 8, _lib.stream_ptr())

        def blocked_scan():
            lib.fr_gallery_first_above_blocked_f32(_lib.ptr(q), _lib.ptr(dg.G), _lib.ptr(view.slots), None, J, n, DIM, 0.4, 0, 0,
                                                   _lib.ptr(idx), _lib.ptr(score), _lib.ptr(ws), J * 8, _lib.stream_ptr())

        fmt = lambda t: f"{t[0]:10.3f} ({t[1]:.3f} .. {t[2]:.3f})"
        a = median_ms(one_by_one)
        b = median_ms(old_scan)
        c = median_ms(lambda: en.enrol_slots(slots, job_images, view))
        cs = median_ms(blocked_scan)
        lines += [f"N = {n:8d}  (a) job by job            {fmt(a)}",
                  f"N = {n:8d}  (b) first_above F=256     {fmt(b)}",
                  f"N = {n:8d}  (c) enrol_slots           {fmt(c)}   {'< (a): ok' if c[0] < a[0] else 'NOT below (a)'}",
                  f"N = {n:8d}  (c) blocked scan alone    {fmt(cs)}   (b) / this = {b[0] / cs[0]:.2f}"]
        for line in lines[-4:]:
            print(line, flush=True)
        del dg, view, m
        torch.cuda.empty_cache()
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
