"""Inputs for the HUD kernel's tests: packed records (include/frhip.h fr_hud_draw_u8) built by hand or from a seed, with
garbage in every slot behind a frame's count, and the expected pictures from tests/helpers/hud_ref.py."""
import numpy as np

from tests.helpers import hud_ref

K = hud_ref.K


def face(box, colour=(0, 255, 0), dh=0, rh=0, lines=(b"Unknown Person", b"Detection: 0.93")):
    return {"box": tuple(box), "colour": tuple(colour), "dh": dh, "rh": rh, "lines": [bytes(b) for b in lines]}


def pack(frames_faces, cap, max_chars=40, seed=0, counts=None):
    """``frames_faces``: per frame a list of ``face(...)`` -> (counts int32 [n], faces int32 [n,cap,K], text uint8
    [n,cap,4,max_chars]).  Every slot behind a frame's count, every line behind a face's line count and every byte behind a
    line's length is filled with seeded garbage: nothing there may be read for meaning.  ``counts`` overrides the counts (a
    partial count over full records)."""
    rng = np.random.default_rng(seed)
    n = len(frames_faces)
    faces = rng.integers(-2 ** 31, 2 ** 31 - 1, (n, cap, K), dtype=np.int64).astype(np.int32)
    text = rng.integers(0, 256, (n, cap, 4, max_chars), dtype=np.int64).astype(np.uint8)
    cnt = np.zeros(n, np.int32)
    for f, fs in enumerate(frames_faces):
        assert len(fs) <= cap
        cnt[f] = len(fs)
        for j, a in enumerate(fs):
            faces[f, j, 0:4] = a["box"]
            faces[f, j, 4:7] = a["colour"]
            faces[f, j, 7], faces[f, j, 8], faces[f, j, 9] = a["dh"], a["rh"], len(a["lines"])
            faces[f, j, 14:16] = 0
            for i, b in enumerate(a["lines"]):
                assert len(b) <= max_chars
                faces[f, j, 10 + i] = len(b)
                text[f, j, i, :len(b)] = np.frombuffer(b, np.uint8)
    if counts is not None:
        cnt[:] = counts
    return cnt, faces, text


def random_faces(rng, count, lo=-40, hi=140, max_chars=40):
    """``count`` faces with corners in [lo, hi] (ordered), random colours, heights and printable strings"""
    out = []
    for _ in range(count):
        xs, ys = np.sort(rng.integers(lo, hi + 1, 2)), np.sort(rng.integers(lo, hi + 1, 2))
        span = int(ys[1] - ys[0])
        lines = [bytes(rng.integers(0x20, 0x7F, int(rng.integers(0, max_chars + 1)), dtype=np.int64).astype(np.uint8))
                 for _ in range(int(rng.integers(0, 5)))]
        out.append(face((int(xs[0]), int(ys[0]), int(xs[1]), int(ys[1])), tuple(int(v) for v in rng.integers(0, 256, 3)),
                        int(rng.integers(0, span + 1)), int(rng.integers(0, span + 1)), lines))
    return out


def noise(rng, n, H, W):
    return rng.integers(0, 256, (n, H, W, 3), dtype=np.int64).astype(np.uint8)


def expected(frames, counts, faces, text, scale=1, font=None):
    """hud_ref over a batch: uint8 [n,H,W,3]"""
    return np.stack([hud_ref.draw_records(frames[f], counts[f], faces[f], text[f], scale, font) for f in range(len(frames))])
