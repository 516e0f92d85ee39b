"""Times frame ingest with a BGR ring against an NV12 ring: 64 x 1080p seeded frames that cross PCIe EVERY step through
``FrameIngest`` -> ``detect_embed_slots`` (synthetic weights, cap_o = 4: bench.py's C2 geometry), both rings in ONE process,
the legs alternating.  The two legs see the same pixels: the BGR frames are the device conversion of the NV12 frames.

  pipelined  blocks of BLOCK steps, step i + 1's upload queued before step i's cascade, a device synchronise around each
             block; a leg's figure is the median over its blocks of (block time / BLOCK), >= 20 steps per leg
  serial     one step at a time with a synchronise behind it (copy, conversion and engine pass end to end, no overlap):
             median of the steps
  convert    the conversion launch alone (64 x 1080p, NV12 and I420), device events, median of 20; its bytes - 1.5 B/px read,
             3 B/px written - against the time give an achieved rate, set beside the HBM peak (8.0 TB/s) and the measured
             copy rate (6.29 TB/s) of the MI355X

``--convert-only`` runs just the last part, a few launches: the run to put under ``rocprofv3 --kernel-trace --stats`` (a run
of its own; the tracer slows the host, so step times are taken without it).  No pass mark: the figures are recorded as they
come out.
Usage: python tools/ingest_yuv_time.py [OUT.txt] [--convert-only] [--frames 64] [--rounds 6]"""
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from facerecognition_infrenceengine_amd import FaceAnalysis, _lib, colour                      # noqa: E402
from facerecognition_infrenceengine_amd.ingest import FrameIngest                              # noqa: E402

H, W, BLOCK, WARM = 1080, 1920, 5, 2
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


def synth_bgr(n, seed, device):
    """structured synthetic BGR frames (low-pass + mid + fine noise), as bench.py makes them"""
    import torch.nn.functional as F
    g = torch.Generator(device=device).manual_seed(seed)
    low = torch.rand((n, 3, H // 16, W // 16), generator=g, device=device)
    mid = torch.rand((n, 3, H // 4, W // 4), generator=g, device=device)
    img = 0.6 * F.interpolate(low, (H, W), mode="bicubic", align_corners=False) \
        + 0.3 * F.interpolate(mid, (H, W), mode="bilinear", align_corners=False) \
        + 0.1 * torch.rand((n, 3, H, W), generator=g, device=device)
    return (img.permute(0, 2, 3, 1).clamp(0, 1) * 255).round().to(torch.uint8).contiguous()


def to_nv12(bgr):
    """float limited-range BT.601, chroma = mean of the 2x2 block: u8 [N,H,W,3] -> u8 [N,H*3/2,W] (input manufacture only)"""
    b, g, r = (bgr[..., i].float() for i in range(3))
    y = 16 + (65.481 * r + 128.553 * g + 24.966 * b) / 255
    u = 128 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255
    v = 128 + (112.0 * r - 93.786 * g - 18.214 * b) / 255
    n = bgr.shape[0]
    mean = lambda c: c.reshape(n, H // 2, 2, W // 2, 2).mean(dim=(2, 4))
    q = lambda c: (c + 0.5).floor().clamp(0, 255).to(torch.uint8)
    out = torch.empty((n, H * 3 // 2, W), dtype=torch.uint8, device=bgr.device)
    out[:, :H] = q(y)
    out[:, H:] = torch.stack([q(mean(u)), q(mean(v))], dim=3).reshape(n, H // 2, W)
    return out


def convert_times(lib, n, lines):
    px = n * H * W
    dst = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda:0")
    for layout in ("nv12", "i420"):
        src = torch.randint(0, 256, (n, H * 3 // 2, W), dtype=torch.uint8, device="cuda:0")
        ts = []
        for i in range(WARM + 20):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            colour.yuv420_to_bgr(src, layout, "bt601", out=dst)
            b.record()
            b.synchronize()
            if i >= WARM:
                ts.append(a.elapsed_time(b) * 1e-3)
        t = statistics.median(ts)
        nbytes = px * 3 // 2 + px * 3
        lines.append(f"convert {layout} {n} x {H} x {W}: {t * 1e6:8.1f} us (min {min(ts) * 1e6:.1f}, max {max(ts) * 1e6:.1f}; device events, "
                     f"median of 20)  {nbytes / 1e6:.1f} MB moved -> {nbytes / t / 1e12:.2f} TB/s = {100 * nbytes / t / HBM_PEAK:.0f} % of the "
                     f"8.0 TB/s HBM peak, {100 * nbytes / t / HBM_COPY:.0f} % of the 6.29 TB/s copy rate; at the peak the bytes take "
                     f"{nbytes / HBM_PEAK * 1e6:.1f} us")
        print(lines[-1], flush=True)


def main():
    argv, out, n, rounds = sys.argv[1:], None, 64, 6
    only = "--convert-only" in argv
    it = iter(a for a in argv if a != "--convert-only")
    for a in it:
        if a == "--frames":
            n = int(next(it))
        elif a == "--rounds":
            rounds = int(next(it))
        else:
            out = a
    lib, dev = _lib.load(), torch.device("cuda:0")
    lines = []
    if not only:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            app = FaceAnalysis(name="synthetic", arch="r100", cap_o=4).prepare(ctx_id=0)
        nv12 = to_nv12(synth_bgr(n, 5, dev))
        bgr = colour.yuv420_to_bgr(nv12, "nv12")
        rings = {"bgr": FrameIngest(n, H, W, dev, depth=3), "nv12": FrameIngest(n, H, W, dev, depth=3, pixel_format="nv12")}
        for k in range(3):                              # what the capture side would have written
            rings["bgr"].host_buffer(k)[...] = bgr.cpu().numpy()
            rings["nv12"].host_buffer(k)[...] = nv12.cpu().numpy()
        link = {"bgr": bgr.numel(), "nv12": nv12.numel()}
        del bgr, nv12
        s_det = torch.cuda.Stream(device=dev)
        counts = {k: torch.empty(n, dtype=torch.int32).pin_memory() for k in rings}
        turn = {k: 0 for k in rings}

        def block(leg, steps, serial):
            """`steps` steps of one leg; pipelined: the next step's upload is queued before this step's engine pass"""
            ring = rings[leg]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ahead = ring.upload(turn[leg])
            for s in range(steps):
                i = turn[leg]
                frames, ready = ahead
                if not serial and s + 1 < steps:
                    ahead = ring.upload(i + 1)
                r = app.detect_embed_slots(frames, det_stream=s_det, ready_event=ready)
                ring.release(i)
                counts[leg].copy_(r["counts"], non_blocking=True)
                turn[leg] = i + 1
                if serial:
                    torch.cuda.synchronize()
                    if s + 1 < steps:
                        ahead = ring.upload(i + 1)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps, int(counts[leg].sum())

        for leg in rings:                               # warm-up: every shape, both rings
            block(leg, 3, False)
        per = {(leg, mode): [] for leg in rings for mode in ("pipelined", "serial")}
        faces = {}
        for _ in range(rounds):                         # the legs alternate
            for leg in rings:
                t, faces[leg] = block(leg, BLOCK, False)
                per[(leg, "pipelined")].append(t)
            for leg in rings:
                for _ in range(BLOCK):
                    per[(leg, "serial")].append(block(leg, 1, True)[0])
        assert faces["bgr"] == faces["nv12"] > 0, faces       # the same pixels: the same faces
        lines.append(f"ingest {n} x {H} x {W} frames per step, FrameIngest -> detect_embed_slots (synthetic weights, cap_o 4), frames cross "
                     f"PCIe every step; {rounds} alternating rounds; {faces['bgr']} faces per step in both legs")
        for mode, what in (("pipelined", f"median of {rounds} blocks of {BLOCK} steps ({rounds * BLOCK} steps)"),
                           ("serial", f"median of {rounds * BLOCK} steps")):
            for leg in rings:
                ts = per[(leg, mode)]
                lines.append(f"{mode:9s} {leg:4s} ring: {statistics.median(ts) * 1e3:8.3f} ms per step (min {min(ts) * 1e3:.3f}, max "
                             f"{max(ts) * 1e3:.3f}; {what})  link bytes per step {link[leg] / 1e6:.1f} MB")
            a, b = (statistics.median(per[(leg, mode)]) for leg in ("bgr", "nv12"))
            lines.append(f"{mode:9s} nv12 / bgr = {b / a:.3f}" + ("" if b <= a else "   (the NV12 leg is SLOWER)"))
        for line in lines:
            print(line, flush=True)
        del rings, app
        torch.cuda.empty_cache()
    convert_times(lib, n, lines)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
