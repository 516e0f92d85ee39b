"""Times the activity gate on one MI355X; writes profiles/activity_gate.txt.  Medians of 30 after 3 warm-ups, the
variants alternating in one process (as tools/det_size_ab.py, whose timing helpers this uses).

  1. the gate alone on 64 x 1080p, uniform form and table form (two launches each: cell means, judge), HIP events: time, and the
     algorithmic bytes (the frames' cell area read once + the cell arrays) / time.  The yardstick is fr_letterbox_u8 on the same
     frames in the same session (its bytes as tools/det_size_ab.py counts them), not a fixed number; the ratio is recorded.
  2. FaceRecognitionProcessor.recognize_batch of 64 x 1080p host frames (synthetic weights, cap_o = 4, a 1 000-row gallery), wall
     time of the whole call: ungated against gated with 64, 32, 8 and 0 active frames.  A gated variant has its own gate; before
     each of its turns k cameras switch to their other frame (active) and the rest repeat the previous turn's frame (inactive).
     The condition for the feature: gated with all 64 active costs no more than the ungated call's own min - max spread plus the
     gate-alone time plus one synchronisation (a small device-to-host copy, timed here too).  Stated either way.

No pass mark, nothing here is asserted in a test.  Not measured: real video, the defaults' false-positive / false-negative rates,
the camera loop with capture threads.
Usage: python tools/activity_gate_time.py [--frames 64] [--reps 30] [--out profiles/activity_gate.txt]"""
import argparse
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from det_size_ab import alternate, letterbox_bytes                                             # noqa: E402

H, W, WARM = 1080, 1920, 3


def wall_alternate(variants, reps):
    """{name: fn} -> {name: [seconds]}: wall time of whole calls (they synchronise themselves), the variants taking turns"""
    for _ in range(WARM):
        for fn in variants.values():
            fn()
    t = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t[k].append(time.perf_counter() - t0)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "activity_gate.txt"))
    a = ap.parse_args()
    assert a.reps >= 30, "medians of at least 30"
    from facerecognition_infrenceengine_amd import ActivityGate, FaceAnalysis, _lib
    from facerecognition_infrenceengine_amd.letterbox import frame_table
    from facerecognition_infrenceengine_amd.processor import UNCHANGED, EmbeddingManager, FaceRecognitionProcessor, InMemoryStore
    from make_golden import synth_frame
    N, dev = a.frames, torch.device("cuda:0")
    lines = [f"activity gate: {N} x {H} x {W} frames, medians of {a.reps} after {WARM} warm-ups, variants alternating in one process",
             f"device: {torch.cuda.get_device_name(0)}", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    base = [synth_frame(H, W, 900 + i) for i in range(16)]
    set_a, set_b = [base[i % 8] for i in range(N)], [base[8 + i % 8] for i in range(N)]
    lib = _lib.load()

    # ---- 1. the gate alone, beside the letterbox
    hd = torch.from_numpy(np.ascontiguousarray(np.stack(set_a))).to(dev)
    tab, _ = frame_table([hd.data_ptr() + i * H * W * 3 for i in range(N)], [(H, W)] * N, (640, 640))
    table = torch.from_numpy(tab).to(dev)
    canvas = torch.empty((N, 640, 640, 3), dtype=torch.uint8, device=dev)
    g_u, g_t = ActivityGate(dev, slots=N), ActivityGate(dev, slots=N)
    cams = list(range(N))
    variants = {"uniform": lambda: g_u.judge_device(hd, cams), "table": lambda: g_t.judge_device(hd, cams, table=table),
                "letterbox": lambda: lib.fr_letterbox_u8(_lib.ptr(table), N, _lib.ptr(canvas), 640, 640, _lib.stream_ptr())}
    med, rng = alternate(variants, a.reps, warmup=WARM)
    cells = (H // 16) * (W // 16)
    gate_bytes = N * (cells * 256 * 3 + 3 * cells)              # cell area read; cur written, cur and grid read by the judge
    rd, wr = letterbox_bytes([(H, W)] * N, (640, 640))
    lb_rate = (rd + wr) / (med["letterbox"] * 1e-3)
    say(f"1. the gate alone (HIP events round both launches; every frame inactive: the steady state of an idle fleet, no grid copy)")
    say(f"   fr_letterbox_u8 -> 640 x 640, the yardstick: {med['letterbox'] * 1e3:7.1f} us (min {rng['letterbox'][0] * 1e3:.1f}, max "
        f"{rng['letterbox'][1] * 1e3:.1f}); {(rd + wr) / 1e6:.1f} MB -> {lb_rate / 1e12:.2f} TB/s")
    for k, what in (("uniform", "fr_frame_activity_u8     "), ("table", "fr_frame_activity_refs_u8")):
        rate = gate_bytes / (med[k] * 1e-3)
        say(f"   {what} via ActivityGate.judge_device: {med[k] * 1e3:7.1f} us (min {rng[k][0] * 1e3:.1f}, max {rng[k][1] * 1e3:.1f}); "
            f"{gate_bytes / 1e6:.1f} MB -> {rate / 1e12:.2f} TB/s = {rate / lb_rate:.2f} x the letterbox's rate in this session")
    gate_s = med["uniform"] * 1e-3
    probe = torch.zeros(2 * N, dtype=torch.int32, device=dev)
    sync = wall_alternate({"sync": lambda: probe.cpu()}, a.reps)["sync"]
    sync_s = statistics.median(sync)
    say(f"   one small device-to-host copy with its synchronisation (wall): {sync_s * 1e6:.1f} us")
    say()
    del hd, canvas, table, g_u, g_t
    torch.cuda.empty_cache()

    # ---- 2. recognize_batch, ungated against gated at four active fractions
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        app = FaceAnalysis(name="synthetic", arch="r100", cap_o=4).prepare(ctx_id=0)
    r = np.random.default_rng(1)
    store = InMemoryStore()
    for i in range(1000):
        store.add_employee(f"n{i}", "acme", r.standard_normal(512).astype(np.float32), name=f"N{i}")
    proc = FaceRecognitionProcessor(EmbeddingManager(store=store, device="cuda:0"), face_detector=app)
    seen = {}

    def gated(k):
        gate, state = ActivityGate(dev, slots=N), {"flip": False, "frames": list(set_a)}

        def turn():
            state["flip"] = not state["flip"]
            src = set_b if state["flip"] else set_a
            for i in range(k):                                   # cameras 0 .. k-1 show their other frame, the rest repeat
                state["frames"][i] = src[i]
            res = proc.recognize_batch(state["frames"], "acme", gate=gate, camera_ids=cams)
            seen[k] = sum(x is not UNCHANGED for x in res)
        return turn
    variants = {"ungated": lambda: proc.recognize_batch(set_a, "acme")}
    variants.update({f"gated {k:2d} active": gated(k) for k in (N, N // 2, N // 8, 0)})
    t = wall_alternate(variants, a.reps)
    say(f"2. recognize_batch, {N} x 1080p host frames per turn (synthetic weights, cap_o 4, 1 000 gallery rows), wall time of the call")
    for k, v in t.items():
        m = statistics.median(v)
        say(f"   {k:16s}: {m * 1e3:8.3f} ms per turn (min {min(v) * 1e3:.3f}, max {max(v) * 1e3:.3f})  {N / m:9.0f} frames/s")
    assert [seen[k] for k in (N, N // 2, N // 8, 0)] == [N, N // 2, N // 8, 0], seen      # the variants did what they say
    un, g_all = t["ungated"], t[f"gated {N:2d} active"]
    extra = statistics.median(g_all) - statistics.median(un)
    allowed = (max(un) - min(un)) + gate_s + sync_s
    say(f"   gated with all {N} active - ungated: {extra * 1e3:+.3f} ms; allowed: the ungated call's spread {(max(un) - min(un)) * 1e3:.3f} ms + "
        f"the gate {gate_s * 1e3:.3f} ms + one synchronisation {sync_s * 1e3:.3f} ms = {allowed * 1e3:.3f} ms: "
        f"the condition {'HOLDS' if extra <= allowed else 'DOES NOT HOLD'}")
    say()
    say("not measured: real video, the false-positive / false-negative rates of thr = 4, min_cells = 2, the camera loop with capture threads")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
