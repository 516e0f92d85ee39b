"""The C call list an eager few-frame ``MTCNNHIP.detect_batch`` records (the argument ``_make_sequence`` receives), reduced
to what does not change from run to run.  ``python tests/golden/make_detect_calls.py`` writes detect_calls.json; it was
run once, on the commit before the detector host was split into stages, and is not run again: the fixture pins that
commit's launches, their order, their streams' fork / join notes and every small-integer argument."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ((1, 96, 128), (3, 96, 128))


def capture(n, h, w):
    """-> (reduced call list, number of replays, results of calls 2 and 3) of three calls on one n x h x w batch."""
    import numpy as np
    import torch
    sys.path.insert(0, HERE)
    from make_golden import synth_frame
    from facerecognition_infrenceengine_amd import weights
    from facerecognition_infrenceengine_amd.mtcnn import MTCNNHIP
    det = MTCNNHIP(*weights.synth_mtcnn_states(seed=4321), device="cuda:0", cap_o=4)
    seen, replays = [], []
    make, replay = det._make_sequence, det._replay
    det._make_sequence = lambda calls, *a: (seen.append(calls), make(calls, *a))[1]
    det._replay = lambda *a: (replays.append(1), replay(*a))[1]
    frames = torch.from_numpy(np.stack([synth_frame(h, w, 7 + i) for i in range(n)])).cuda()
    outs = [[t.clone() for t in det.detect_batch(frames)] for _ in range(3)]
    torch.cuda.synchronize()
    assert len(seen) == 1, "the second call records, once"
    reduced = [[fid, len(slots), [s if s < 65536 else "P" for s in slots], [list(r) for r in roles]]
               for fid, slots, roles in seen[0]]
    return reduced, len(replays), outs[1], outs[2]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    out = {"%dx%dx%d" % s: capture(*s)[0] for s in SHAPES}
    with open(os.path.join(HERE, "detect_calls.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
