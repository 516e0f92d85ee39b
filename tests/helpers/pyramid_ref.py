"""Hand-built level tables for the pyramid-wide P-Net launches (fr_pnet_pyramid_conv1 / _p23 / _band_tiles,
fr_pnet_finish_levels) and their float64 reference (tests/test_gpu_pnet_pyramid_pins.py, tests/test_pyramid_ref_host.py).

Host only.  A table is a batch size, a frame size and up to 16 levels (hs, ws, f16, scale): a level's size does not follow
from the frame (conv1 resizes inside its tile load), so the tables reach what no natural pyramid does - one level, sixteen,
f16 flags interleaved with f32 ones, the smallest level first, two levels of one size, grids at the 512-block cap, conv1
levels above the 4096-tile switch next to small ones.

``reference`` evaluates, per level and frame, in float64 through tests/helpers/detect_ref.py: conv1; the split arithmetic of
conv1's f16 form; the split conv2 / conv3 / heads chained behind the form the level runs; the exact heads; the logit
differences; and beside every value the magnitude A that bounds the f32 rounding error (|y - y64| <= C_F32 * A).
``decide`` turns that into what the kernels must do with every cell: pass, fail, or undecided."""
import math
import os
import sys

import numpy as np
import torch

from oracle import detect as odetect
from tests.helpers import detect_ref as ref

C_F32 = 4e-7                 # tests/test_gpu_detect_precision.py: f32 accumulation bound per sum |w x| + |b|
EXPF = 1e-6                  # docs/KERNEL_NOTES.md 4.13: what passes through the device's expf (the list kernels' one tolerance)
REFINE_MARGIN = 2e-3         # mtcnn.py refine_margin: the band round the threshold logit
WEIGHT_SEED = 5
SLOPES = (-1.5, -0.3, 0.0, 0.2, 0.7, 1.0, 1.6, 3.0)     # tests/test_gpu_detect_precision.py: negative slopes take conv1's activate-then-pool branch
FAIL, PASS, UNDECIDED = 0, 1, 2


class Table:
    """N frames of FH x FW bytes (kinds: "rand" seeded bytes, "synth" make_golden.synth_frame, "zero"), levels
    (hs, ws, f16, scale), the face threshold and the capacity of a level's candidate list"""

    def __init__(self, why, frames, FH, FW, levels, thr, cap=512, seed=0):
        self.why, self.kinds, self.N, self.FH, self.FW = why, tuple(frames), len(frames), FH, FW
        self.levels, self.thr, self.cap, self.seed = [tuple(l) for l in levels], float(np.float32(thr)), cap, seed

    def geo(self, li):
        hs, ws = self.levels[li][:2]
        return (hs - 1) // 2, (ws - 1) // 2

    def band(self, band):
        """(lo, hi) as mtcnn.py _band_logits states them, as the float32 values the entries take"""
        lt = math.log(self.thr / (1.0 - self.thr))
        return float(np.float32(lt - REFINE_MARGIN)), float(np.float32(lt + REFINE_MARGIN)) if band else float("-inf")


_S = (0.9, 0.709, 0.6, 0.5, 0.3546, 0.81, 0.43, 0.25)          # <= 1: a cell's box corner floor((2 c + 1) / scale) names the cell


def _lv(sizes, flags):
    return [(hs, ws, f, _S[i % len(_S)]) for i, ((hs, ws), f) in enumerate(zip(sizes, flags))]


# thresholds: chosen per table from the float64 reference's own scores (tests/test_pyramid_ref_host.py asserts what they must give)
TABLES = {
    "one_f32": Table("a single f32 level: the level-finding loops never advance, first[1] is the grid",
                     ("synth", "rand"), 100, 130, _lv([(37, 53)], [0]), 0.3),
    "one_f16": Table("a single f16 level: one entry in the f16 table, in the band tiles' table and in the tile list",
                     ("synth", "rand"), 100, 130, _lv([(45, 61)], [1]), 0.5),
    "sixteen": Table("16 levels, the maximum, f16 on the first five; the last four are a 5 x 5 map from an odd and an even size "
                     "(one cell), one row and one column of cells",
                     ("synth", "rand"), 100, 130,
                     _lv([(61, 83), (53, 70), (45, 64), (40, 51), (33, 47), (29, 41), (26, 35), (23, 30), (20, 27), (17, 23), (15, 20),
                          (13, 17), (11, 11), (12, 12), (11, 140), (140, 11)], [1] * 5 + [0] * 11), 0.1, cap=1024),
    "interleaved": Table("f16 flags 0,1,0,1,1,0: k != l in conv1 mode 0's two tables and in the band tiles' remap, level numbers "
                         "1, 3, 4 in the tile list", ("synth", "rand"), 100, 130,
                         _lv([(50, 71), (64, 40), (31, 90), (47, 47), (25, 33), (38, 52)], [0, 1, 0, 1, 1, 0]), 0.3),
    "ascending": Table("the smallest level first: first[] grows by more each level", ("synth", "rand"), 100, 130,
                       _lv([(15, 19), (24, 31), (37, 50), (58, 77)], [0, 1, 0, 1]), 0.2),
    "twins": Table("two levels of one size, one f16 and one f32, with buffers of their own", ("synth", "rand"), 100, 130,
                   _lv([(41, 57), (41, 57), (23, 29)], [1, 0, 0]), 0.1),
    "grid512": Table("a level of exactly 512 conv2/conv3 tiles and one of 518 (grid capped at 512, seg_cap two tiles, six blocks "
                     "with two), each followed by a one-block level", ("synth",), 100, 130,
                     _lv([(27, 16331), (19, 41), (27, 16523), (13, 15)], [0, 1, 1, 0]), 0.65, cap=16384),
    "rpb8": Table("an f16 and an f32 level of 4098 conv1 tiles (8 tiles per block, the last block with two) next to "
                  "one-tile-per-block levels in the same launch", ("synth", "rand", "synth"), 100, 130,
                  _lv([(19, 43651), (33, 47), (20, 43653), (26, 35)], [1, 1, 0, 0]), 0.8, cap=16384),
    "odd_even_1": Table("hs and ws odd and even in all four combinations, in both forms, one frame", ("synth",), 100, 130,
                        _lv([(37, 53), (37, 52), (36, 53), (36, 52), (31, 45), (31, 44), (30, 45), (30, 44), (12, 11)], [1, 1, 1, 1, 0, 0, 0, 0, 0]), 0.5),
    "odd_even_3": Table("the same levels, three frames", ("synth", "rand", "synth"), 100, 130,
                        _lv([(37, 53), (37, 52), (36, 53), (36, 52), (31, 45), (31, 44), (30, 45), (30, 44), (12, 11)], [1, 1, 1, 1, 0, 0, 0, 0, 0]), 0.5),
}


# ------------------------------------------------------------------------------------------------------------ inputs
def states(seed=WEIGHT_SEED):
    """weights.synth_mtcnn_states with the mixed PReLU slopes of tests/test_gpu_detect_precision.py _states (the same draw)"""
    from facerecognition_infrenceengine_amd import weights
    p, r, o = weights.synth_mtcnn_states(seed=seed)
    g = torch.Generator().manual_seed(seed)
    base = torch.tensor(SLOPES)
    for st in (p, r, o):
        for k in sorted(st):
            if k.startswith("prelu"):
                n = st[k].numel()
                idx = torch.cat([torch.randperm(len(SLOPES), generator=g),
                                 torch.randint(0, len(SLOPES), (max(0, n - len(SLOPES)),), generator=g)])[:n]
                st[k] = base[idx] * torch.empty(n).uniform_(0.8, 1.2, generator=g)
    return p, r, o


def frames(table):
    """the table's frames, uint8 [N, FH, FW, 3] (BGR)"""
    golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
    if golden not in sys.path:
        sys.path.insert(0, golden)
    from make_golden import synth_frame
    g = torch.Generator().manual_seed(1000 + table.seed)
    out = []
    for i, kind in enumerate(table.kinds):
        if kind == "synth":
            out.append(torch.from_numpy(synth_frame(table.FH, table.FW, 50 + 7 * table.seed + i)))
        elif kind == "rand":
            out.append(torch.randint(0, 256, (table.FH, table.FW, 3), generator=g, dtype=torch.uint8))
        else:
            out.append(torch.zeros((table.FH, table.FW, 3), dtype=torch.uint8))
    return torch.stack(out).contiguous()


def level_images(table, fr):
    """per level: float32 [N, hs, ws, 3] - oracle/detect.py's resize and normalisation, which fr_pyramid_resize_norm equals bit
    for bit (tests/test_gpu_detect_precision.py)"""
    f = fr.numpy()
    out = []
    for hs, ws, _, _ in table.levels:
        out.append(torch.stack([odetect._to_net(odetect.resize_bilinear(f[n][:, :, ::-1].astype(np.float32), hs, ws))[0].permute(1, 2, 0)
                                for n in range(table.N)]).contiguous())
    return out


# ------------------------------------------------------------------------------------------------------------ layout
def layout(N, H1, W1):
    """csrc/pnet_fused.hip p23_layout and fr_pnet_band_tiles_count, restated: the cells of a level, its conv2/conv3 tiles
    (8 x 32 cells), the blocks of its launch, the capacity of a block's list segment, the workspace
    [dl | 512 counts | segments] in bytes, and the conv1 tiles (8 x 32 map pixels) the band list can name."""
    H3, W3 = H1 - 4, W1 - 4
    cells = N * H3 * W3
    tiles = N * (-(-W3 // 32)) * (-(-H3 // 8))
    grid = min(tiles, 512)
    seg_cap = -(-tiles // grid) * 256
    return dict(cells=cells, tiles=tiles, grid=grid, seg_cap=seg_cap, workspace_bytes=cells * 4 + 512 * 4 + grid * seg_cap * 4,
                band_tiles=N * (-(-H1 // 8)) * (-(-W1 // 32)), regions=(-(-H1 // 8), -(-W1 // 32)))


def conv1_tiles(N, hs, ws):
    """tiles of 16 x 64 conv pixels of a level (fr_pnet_pyramid_conv1): from 4096 a block walks 8 of them"""
    return N * ((hs + 13) // 16) * ((ws + 61) // 64)


# ------------------------------------------------------------------------------------------------------------ reference
def _cat(rows):
    return [torch.cat([r[i] for r in rows]) for i in range(len(rows[0]))]


def reference(table, images, layers, c=C_F32):
    """images: per level float32 [N, hs, ws, 3] (level_images, or fr_pyramid_resize_norm's); layers: detect_ref.pnet_layers.
    Per level a dict of float64 NCHW tensors over the N frames:
      conv1, conv1_A       the exact conv1 map [N, 10, H1, W1] and its bound
      split1, split1_A     the split arithmetic of conv1's f16 form
      shead, shead_A       conv2 -> conv3 -> heads in split arithmetic [N, 6, H3, W3], chained behind the map the level's form
                           leaves (f16: split1; else conv1), the bound carried along
      head, head_A         the exact heads, and the bound of the f32 chain conv1 -> conv2 -> conv3 -> heads
      dl, dl_A, sdl        head[1] - head[0] with its bound; shead[1] - shead[0]"""
    out = []
    for li, (hs, ws, f16, _) in enumerate(table.levels):
        rows = []
        for n in range(table.N):
            x = images[li][n:n + 1].permute(0, 3, 1, 2).double().cpu()
            y1, A1 = ref.apply(layers[0], x, c)
            s1, As1 = ref.apply(layers[0], x, c, split=True)
            b, Ab = (s1, As1) if f16 else (y1, A1)
            s2, As2 = ref.apply(layers[1], b, c, split=True, carry=ref.split_carry(b, Ab, c))
            sh, Ash = ref.apply(layers[2], s2, c, split=True, carry=ref.split_carry(s2, As2, c))
            e2, A2 = ref.apply(layers[1], y1, c, carry=A1)
            eh, Aeh = ref.apply(layers[2], e2, c, carry=A2)
            rows.append((y1, A1, s1, As1, sh, Ash, eh, Aeh))
        y1, A1, s1, As1, sh, Ash, eh, Aeh = _cat(rows)
        out.append(dict(conv1=y1, conv1_A=A1, split1=s1, split1_A=As1, shead=sh, shead_A=Ash, head=eh, head_A=Aeh,
                        dl=eh[:, 1] - eh[:, 0], dl_A=Aeh[:, 1] + Aeh[:, 0], sdl=sh[:, 1] - sh[:, 0]))
    return out


def decide(r, thr, lo, hi, c=C_F32):
    """(verdict, reeval) of every cell of a level, int8 / bool [N, H3, W3].
    The fused kernel lists a cell for the exact pass when lo <= dl <= hi (hi > lo: the band), or dl >= lo (no band), dl being
    its split logit difference - here the reference's.  Such a cell is decided by f32 arithmetic: its probability
    p = 1 / (1 + exp(-dl)) lies within 0.25 * C_F32 * dl_A + EXPF of the float64 one (|dp/d dl| <= 1/4), and inside that of
    thr it is UNDECIDED.  Any other cell is decided by where the band lies - below lo it fails, above hi it passes on its split
    heads - which is the f32 decision as long as the split error stays inside the margin: UNDECIDED when the float64 dl lies
    within REFINE_MARGIN of the threshold logit after all (tests assert how few those are, then that the kernels agree)."""
    lt = math.log(thr / (1.0 - thr))
    dl, sdl = r["dl"], r["sdl"]
    band = hi > lo
    reeval = (sdl >= lo) & (sdl <= hi) if band else sdl >= lo
    p = torch.sigmoid(dl)
    bound = 0.25 * c * r["dl_A"] + EXPF
    v_re = torch.where((p - thr).abs() <= bound, UNDECIDED, torch.where(p > thr, PASS, FAIL))
    v_out = torch.where((dl - lt).abs() <= REFINE_MARGIN, UNDECIDED, torch.where(dl > lt, PASS, FAIL))
    return torch.where(reeval, v_re, v_out).to(torch.int8), reeval


def conditions(table, refs):
    """What a table's thresholds must give, on the reference alone, with and without the band.  Raises AssertionError."""
    for band in (True, False):
        lo, hi = table.band(band)
        npass = nund = ncell = nabove = 0
        empty = False
        for li, r in enumerate(refs):
            v, _ = decide(r, table.thr, lo, hi)
            listed = (v == PASS).flatten(1).sum(1)
            maybe = (v != FAIL).flatten(1).sum(1)
            if v[0].numel() >= 20:
                assert int(listed.max()) >= 1, f"level {li}: no frame has a listed cell"
            assert int(maybe.max()) <= table.cap, f"level {li}: {int(maybe.max())} cells for {table.cap} slots"
            empty |= bool((maybe == 0).any())
            npass += int(listed.sum()); nund += int((v == UNDECIDED).sum()); ncell += v.numel()
            nabove += int((r["sdl"] >= lo).sum())
        assert empty, "every (level, frame) may list a cell"
        assert npass >= 30, f"{npass} pass cells"
        assert nund <= 0.02 * ncell and nund <= 0.10 * nabove, (nund, ncell, nabove)


def emit_boxes(cy, cx, scale):
    """detect_ops.hip pnet_emit's box of cell (cy, cx), float32 operation by operation"""
    f, s = np.float32, np.float32(scale)
    cx, cy = np.asarray(cx).astype(np.float32), np.asarray(cy).astype(np.float32)
    return np.stack([np.floor((f(2) * cx + f(1)) / s), np.floor((f(2) * cy + f(1)) / s),
                     np.floor((f(2) * cx + f(12)) / s), np.floor((f(2) * cy + f(12)) / s)], -1).astype(np.float32)
