"""The pyramid-wide P-Net launches (fr_pnet_pyramid_conv1 modes 0 / 1, fr_pnet_pyramid_p23, fr_pnet_pyramid_band_tiles,
fr_pnet_finish_levels) on the small hand-built level tables of tests/helpers/pyramid_ref.py, through the C ABI alone:

1. bit for bit against the per-level entries mtcnn.py _level calls (fr_dconv_mfma_f32 layer 0 / fr_pnet_conv1_band,
   fr_pnet23_split_f16, fr_pnet_band_tiles, fr_pnet_finish_levels with one level);
2. nothing else written: every buffer is pre-filled with a sentinel (NaN, 0x7f bytes, -7) and carries a guard zone of it on
   both sides;
3. against the float64 reference: conv1's f32 map, the f16 form's split map, the split heads, the exact pass's rows, and
   which cells are listed (every *pass* cell, no *fail* cell, raster order, the boxes of pnet_emit's float formula);
4. the tile list's edges: an empty band, a list capacity below the count;
5. the entries' refusals.
Each table runs with the band (hi = lt + refine_margin) and without it (hi = -inf).  Run with -s for the measured lines."""
import ctypes
import time

import numpy as np
import pytest
import torch

from facerecognition_infrenceengine_amd import _lib
from facerecognition_infrenceengine_amd.mtcnn import _MConv
from tests.helpers import detect_ref as ref
from tests.helpers import pyramid_ref as P

pytestmark = pytest.mark.gpu

C_F32 = P.C_F32
GUARD = 64                                   # elements of sentinel in front of and behind every buffer
NAMES = sorted(P.TABLES)
CASES = [(n, b) for n in NAMES for b in (True, False)]
INF = float("inf")
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _measured():
    t0 = time.time()
    yield
    if REPORT:
        print("\n" + "\n".join(REPORT))
    print(f"tests/test_gpu_pnet_pyramid_pins.py: {time.time() - t0:.1f} s wall")


def _report(line):
    REPORT.append(line)
    print(line)


# ---------------------------------------------------------------------------------------------------- sentinel buffers
class Buf:
    """a device buffer pre-filled with a sentinel, GUARD elements of it in front and behind; ``t`` is the payload"""

    def __init__(self, shape, dtype, fill):
        n = int(np.prod(shape))
        self.raw = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
        self.t = self.raw[GUARD:GUARD + n].view(*shape)
        self.fill = fill

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def guards_intact(self):
        return bool(_sentinel(self.raw[:GUARD], self.fill).all() and _sentinel(self.raw[-GUARD:], self.fill).all())


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _sentinel(t, fill=None):
    """elementwise: still the sentinel's bit pattern"""
    if t.dtype == torch.float32:
        return _bits(t) == _bits(torch.tensor(float("nan"), device=t.device))
    return t == (0x7f if t.dtype == torch.uint8 else -7)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------- inputs
@pytest.fixture(scope="module")
def net():
    st = P.states()[0]
    L = ref.pnet_layers(st)
    p1 = _MConv(0, st["conv1.weight"].float(), st["conv1.bias"].float(), st["prelu1.weight"].float(), "cuda:0")
    w2p = torch.zeros((16, 10, 16)); w2p[:, :9, :10] = st["conv2.weight"].float().permute(0, 2, 3, 1).reshape(16, 9, 10)
    w3p = torch.zeros((32, 10, 16)); w3p[:, :9, :16] = st["conv3.weight"].float().permute(0, 2, 3, 1).reshape(32, 9, 16)
    hw = torch.cat([st["conv4_1.weight"].reshape(2, 32), st["conv4_2.weight"].reshape(4, 32)]).float()
    hb = torch.cat([st["conv4_1.bias"], st["conv4_2.bias"]]).float()
    p23 = tuple(t.float().contiguous().cuda() for t in (w2p, st["conv2.bias"], st["prelu2.weight"], w3p, st["conv3.bias"],
                                                         st["prelu3.weight"], hw.t(), hb))
    return dict(lib=_lib.load(), L=L, p1=p1, p1w=[_lib.ptr(p1.w), _lib.ptr(p1.b), _lib.ptr(p1.slope)], p23=p23,
                p23p=[_lib.ptr(t) for t in p23])


_FRAMES, _REFS = {}, {}


def _frames(name):
    if name not in _FRAMES:
        _FRAMES[name] = P.frames(P.TABLES[name]).cuda()
    return _FRAMES[name]


def _reference(net, name):
    """the float64 reference of a table on fr_pyramid_resize_norm's level images, computed once; the table's conditions hold on it"""
    if name not in _REFS:
        t, fr, lib = P.TABLES[name], _frames(name), net["lib"]
        images = []
        for hs, ws, _, _ in t.levels:
            img = torch.full((t.N, hs, ws, 3), float("nan"), device="cuda")
            assert lib.fr_pyramid_resize_norm(_lib.ptr(fr), t.N, t.FH, t.FW, hs, ws, _lib.ptr(img), _lib.stream_ptr()) == 0
            images.append(img)
        torch.cuda.synchronize()
        refs = P.reference(t, [i.cpu() for i in images], net["L"])
        P.conditions(t, refs)
        _REFS[name] = refs
    return _REFS[name]


# ---------------------------------------------------------------------------------------------------- the two runners
def _alloc(t):
    """every level's buffers (its own: no two levels share one), sentinel-filled, and its fr_pnet_level entry"""
    levels, entries = [], []
    for li, (hs, ws, f16, scale) in enumerate(t.levels):
        H1, W1 = t.geo(li)
        lay = P.layout(t.N, H1, W1)
        b = dict(x1=Buf((t.N, H1, W1, 12), torch.float32, float("nan")), xs=Buf((t.N, H1, W1, 64), torch.uint8, 0x7f),
                 head=Buf((t.N, H1 - 4, W1 - 4, 6), torch.float32, float("nan")),
                 wsp=Buf((lay["workspace_bytes"] // 4,), torch.int32, -7),
                 bc=Buf((t.N * (-(-(H1 - 4) * (W1 - 4) // 256)),), torch.int32, -7),
                 boxes=Buf((t.N, t.cap, 4), torch.float32, float("nan")), scores=Buf((t.N, t.cap), torch.float32, float("nan")),
                 regs=Buf((t.N, t.cap, 4), torch.float32, float("nan")), counts=Buf((t.N,), torch.int32, -7))
        b["wsp"].t[:lay["cells"]].view(torch.float32).fill_(float("nan"))          # dl: floats
        b.update(lay=lay, H1=H1, W1=W1, f16=f16)
        levels.append(b)
        entries.append(_lib.PnetLevel(b["x1"].ptr, b["head"].ptr, b["wsp"].ptr, H1, W1, float(scale), b["boxes"].ptr, b["scores"].ptr,
                                      b["regs"].ptr, b["counts"].ptr, b["bc"].ptr, b["xs"].ptr, hs, ws, int(f16)))
    return levels, entries


def run_pyramid(net, name, lo, hi, all_heads=0, short=0, finish=True):
    """the six launches in the order include/frhip.h states.  short: mode 1 is given a list capacity that many below the count
    (and nothing runs behind it)."""
    t, fr, lib, s = P.TABLES[name], _frames(name), net["lib"], _lib.stream_ptr()
    levels, entries = _alloc(t)
    n = len(entries)
    lv = (_lib.PnetLevel * n)(*entries)
    nts = [b["lay"]["band_tiles"] for b in levels if b["f16"]]
    ntile, words = sum(nts), sum((x + 31) // 32 for x in nts)
    out = dict(levels=levels, tbuf=None, tiles=None)
    lib.fr_pnet_pyramid_conv1(0, _lib.ptr(fr), t.N, t.FH, t.FW, lv, n, *net["p1w"], None, None, 0, s)
    lib.fr_pnet_pyramid_p23(lv, n, t.N, *net["p23p"], all_heads, lo, hi, s)
    if ntile:
        tbuf, tiles = Buf((1 + words,), torch.int32, -7), Buf((ntile,), torch.int32, -7)
        out.update(tbuf=tbuf, tiles=tiles)
        lib.fr_pnet_pyramid_band_tiles(lv, n, t.N, tbuf.ptr, tiles.ptr, s)
        cap = ntile
        if short:
            torch.cuda.synchronize()
            cap = int(tbuf.t[0]) - short
            assert cap > 0, "the table lists too few tiles for this case"
        out["list_cap"] = cap
        lib.fr_pnet_pyramid_conv1(1, _lib.ptr(fr), t.N, t.FH, t.FW, lv, n, *net["p1w"], tiles.ptr, tbuf.ptr, cap, s)
    if finish and not short:
        lib.fr_pnet_finish_levels(lv, n, t.N, *net["p23p"], t.thr, t.cap, lo, None, s)
    torch.cuda.synchronize()
    return out


def run_per_level(net, name, lo, hi, all_heads=0):
    """the per-level calls of mtcnn.py _level: conv1 (fr_dconv_mfma_f32 layer 0 with y_split, or fr_pnet_conv1_band mode 0),
    fr_pnet23_split_f16 with the exact pass deferred, fr_pnet_band_tiles + fr_pnet_conv1_band mode 1 on an f16 level,
    fr_pnet_finish_levels with one level"""
    t, fr, lib, s = P.TABLES[name], _frames(name), net["lib"], _lib.stream_ptr()
    levels, entries = _alloc(t)
    p1 = net["p1"]
    for li, (b, e) in enumerate(zip(levels, entries)):
        hs, ws = t.levels[li][:2]
        H1, W1 = b["H1"], b["W1"]
        if b["f16"]:
            lib.fr_pnet_conv1_band(0, _lib.ptr(fr), t.N, t.FH, t.FW, hs, ws, *net["p1w"], None, b["xs"].ptr, None, None, 0, s)
        else:
            lib.fr_dconv_mfma_f32(0, None, *net["p1w"], b["x1"].ptr, t.N, hs, ws, None, None, _lib.ptr(fr), t.FH, t.FW, None, 0,
                                  b["xs"].ptr, s)
        lib.fr_pnet23_split_f16(b["x1"].ptr, b["xs"].ptr, t.N, H1, W1, *net["p23p"], b["head"].ptr, all_heads | 2, lo, hi, None,
                                b["wsp"].ptr, b["lay"]["workspace_bytes"], s)
        if b["f16"]:
            nt = b["lay"]["band_tiles"]
            b["tbuf"], b["tiles"] = Buf((1 + (nt + 31) // 32,), torch.int32, -7), Buf((nt,), torch.int32, -7)
            lib.fr_pnet_band_tiles(b["wsp"].ptr, t.N, H1, W1, b["tbuf"].ptr, b["tiles"].ptr, s)
            lib.fr_pnet_conv1_band(1, _lib.ptr(fr), t.N, t.FH, t.FW, hs, ws, *net["p1w"], b["x1"].ptr, None, b["tiles"].ptr,
                                   b["tbuf"].ptr, nt, s)
        lib.fr_pnet_finish_levels((_lib.PnetLevel * 1)(e), 1, t.N, *net["p23p"], t.thr, t.cap, lo, None, s)
    torch.cuda.synchronize()
    return dict(levels=levels)


_RUNS = {}


def _runs(net, name, band):
    """(pyramid run, per-level run) of a table at its thresholds, made once"""
    if (name, band) not in _RUNS:
        lo, hi = P.TABLES[name].band(band)
        _RUNS[name, band] = (run_pyramid(net, name, lo, hi), run_per_level(net, name, lo, hi))
    return _RUNS[name, band]


# ---------------------------------------------------------------------------------------------------- reading a run
def _workspace(b):
    """(dl [N,H3,W3] f32, counts [grid], segments [grid, seg_cap], in-segment mask, the rest of the 512 counters)"""
    lay, w = b["lay"], b["wsp"].t
    N = b["x1"].t.shape[0]
    dl = w[:lay["cells"]].view(torch.float32).view(N, b["H1"] - 4, b["W1"] - 4)
    counts = w[lay["cells"]:lay["cells"] + lay["grid"]]
    rest = w[lay["cells"] + lay["grid"]:lay["cells"] + 512]
    seg = w[lay["cells"] + 512:].view(lay["grid"], lay["seg_cap"])
    mask = torch.arange(lay["seg_cap"], device="cuda")[None, :] < counts[:, None]
    return dl, counts, seg, mask, rest


def _listed_cells(b):
    """flat indices of the cells on the level's exact-pass lists, sorted"""
    _, _, seg, mask, _ = _workspace(b)
    return torch.sort(seg[mask].long()).values


def _level_tiles(run, li, per_level):
    """sorted tile numbers listed for level li"""
    if per_level:
        b = run["levels"][li]
        return torch.sort(b["tiles"].t[:int(b["tbuf"].t[0])]).values
    e = run["tiles"].t[:int(run["tbuf"].t[0])]
    return torch.sort(e[(e >> 27) == li] & ((1 << 27) - 1)).values


def _tile_mask(b, tiles):
    """bool [N, H1, W1]: the map pixels inside the listed conv1 tiles (8 x 32 map pixels each)"""
    N = b["x1"].t.shape[0]
    ry, rx = b["lay"]["regions"]
    m = torch.zeros(N * ry * rx, dtype=torch.bool, device="cuda")
    m[tiles.long()] = True
    m = m.view(N, ry, rx).repeat_interleave(8, 1).repeat_interleave(32, 2)
    return m[:, :b["H1"], :b["W1"]]


def _rows(t, counts):
    """bool [N, cap]: the slots below each frame's count"""
    return torch.arange(t.shape[1], device="cuda")[None, :] < counts[:, None]


# ---------------------------------------------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("name,band", CASES)
def test_pyramid_launches_equal_the_per_level_entries_bit_for_bit(net, name, band):
    _reference(net, name)                                   # the table's conditions hold before anything is compared
    pyr, per = _runs(net, name, band)
    t = P.TABLES[name]
    total = 0
    for li, (a, b) in enumerate(zip(pyr["levels"], per["levels"])):
        tag = (name, band, li)
        assert _same(a["xs"].t, b["xs"].t), tag                                     # the whole split map
        assert _same(a["x1"].t, b["x1"].t), tag                                     # x1: all of it (f32), inside the listed tiles (f16)
        da, ca, sa, ma, _ = _workspace(a)
        db, cb, sb, mb, _ = _workspace(b)
        assert _same(da, db), tag                                                   # dl
        assert torch.equal(ca, cb) and bool((ca >= 0).all()), tag                   # the per-block counts
        big = torch.iinfo(torch.int32).max
        assert torch.equal(torch.sort(torch.where(ma, sa, big), 1).values, torch.sort(torch.where(mb, sb, big), 1).values), tag
        assert _same(a["head"].t, b["head"].t), tag                                 # the head rows the level writes (the others: sentinel)
        if a["f16"]:
            ta, tb = _level_tiles(pyr, li, False), _level_tiles(per, li, True)
            assert torch.equal(ta, tb) and torch.equal(torch.unique(ta), ta), tag   # the tile list, per level as a set
            total += ta.numel()
        assert torch.equal(a["bc"].t, b["bc"].t) and torch.equal(a["counts"].t, b["counts"].t), tag
        rows = _rows(a["scores"].t, a["counts"].t)
        for k in ("boxes", "scores", "regs"):                                       # the candidate lists, in order
            assert torch.equal(_bits(a[k].t)[rows], _bits(b[k].t)[rows]), (tag, k)
    if pyr["tbuf"] is not None:
        assert int(pyr["tbuf"].t[0]) == total, (name, band)                         # ... and its count
        w0 = 1
        for li, a in enumerate(per["levels"]):                                      # the bitmaps, one level behind the other
            if a["f16"]:
                nw = a["tbuf"].t.numel() - 1
                assert torch.equal(pyr["tbuf"].t[w0:w0 + nw], a["tbuf"].t[1:]), (name, band, li)
                w0 += nw
    assert any(int(a["counts"].t.sum()) for a in pyr["levels"])


# ---------------------------------------------------------------------------------------------------- 2. nothing else
@pytest.mark.parametrize("name,band", CASES)
def test_pyramid_launches_write_nothing_else(net, name, band):
    pyr, per = _runs(net, name, band)
    lo, _ = P.TABLES[name].band(band)
    for run, per_level in ((pyr, False), (per, True)):
        for li, b in enumerate(run["levels"]):
            tag = (name, band, li, per_level)
            for k in ("x1", "xs", "head", "wsp", "bc", "boxes", "scores", "regs", "counts"):
                assert b[k].guards_intact(), (tag, k)
            sx = _sentinel(b["x1"].t)
            if b["f16"]:                    # x1 exists inside the listed tiles only
                inside = _tile_mask(b, _level_tiles(run, li, per_level))
                assert torch.equal(sx.any(-1), ~inside) and torch.equal(sx.all(-1), ~inside), tag
            else:
                assert not bool(sx.any()), tag
            assert not bool((b["xs"].t.view(torch.int32) == 0x7f7f7f7f).all(-1).any()), tag      # every pixel of the split map is written
            dl, counts, seg, mask, rest = _workspace(b)
            assert not bool(_sentinel(dl).any()), tag
            assert bool((seg[~mask] == -7).all()) and bool((rest == -7).all()), tag               # segments past their counts, counters past the grid
            sh = _sentinel(b["head"].t)
            written = (dl >= lo) | ~torch.isfinite(dl)          # all_heads = 0: the rows of the cells that can be kept
            assert torch.equal(sh.any(-1), ~written) and torch.equal(sh.all(-1), ~written), tag
            assert not bool((b["bc"].t == -7).any()) and not bool((b["counts"].t == -7).any()), tag
            rows = _rows(b["scores"].t, b["counts"].t)
            for k in ("boxes", "scores", "regs"):                                                 # candidate slots past the counts
                assert bool(_sentinel(b[k].t)[~rows].all()) and not bool(_sentinel(b[k].t)[rows].any()), (tag, k)
        lists = [(run["tbuf"], run["tiles"])] if not per_level else [(b["tbuf"], b["tiles"]) for b in run["levels"] if b["f16"]]
        for tbuf, tiles in lists:
            if tbuf is not None:
                assert tbuf.guards_intact() and tiles.guards_intact(), (name, band, per_level)
                n = int(tbuf.t[0])
                assert bool((tiles.t[n:] == -7).all()) and not bool((tiles.t[:n] == -7).any()), (name, band, per_level)
                assert n >= 0


# ---------------------------------------------------------------------------------------------------- 3. float64
def _nchw(x):
    return x.permute(0, 3, 1, 2).double().cpu()


def _ratio(tag, got, want, A, c=C_F32):
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), tag
    r = ref.ratio(got, want, A) / c
    return r


@pytest.mark.parametrize("name", NAMES)
def test_conv1_maps_vs_float64(net, name):
    """conv1's f32 map per element; the f16 form's split map, decoded, against the split arithmetic (allowance: that of
    test_split_frame_conv1_kernels_vs_split_arithmetic: the stored map's own representation error 2^-21 |S| + 2^-24); an f32
    level's split map is the split of its f32 map, bit for bit"""
    refs = _reference(net, name)
    pyr, _ = _runs(net, name, True)
    worst = {0: 0.0, 1: 0.0}
    for li, (b, r) in enumerate(zip(pyr["levels"], refs)):
        hl = b["xs"].t.view(torch.float16).view(*b["xs"].t.shape[:3], 2, 16)
        assert float(hl[..., 10:].float().abs().max()) == 0.0, (name, li)
        if b["f16"]:
            dec = hl[..., 0, :10].float() + hl[..., 1, :10].float()
            S = r["split1"]
            worst[1] = max(worst[1], _ratio((name, li), _nchw(dec), S, r["split1_A"] + (2.0 ** -21 * S.abs() + 2.0 ** -24) / C_F32))
        else:
            x1 = b["x1"].t
            assert float(x1[..., 10:].abs().max()) == 0.0, (name, li)
            assert torch.equal(hl[..., 0, :12], x1.half()) and torch.equal(hl[..., 1, :12], (x1 - x1.half().float()).half()), (name, li)
            worst[0] = max(worst[0], _ratio((name, li), _nchw(x1[..., :10]), r["conv1"], r["conv1_A"]))
    _report(f"{name:<12s} conv1 f32 map worst err/bound {worst[0]:.3f}; f16 split map {worst[1]:.3f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0, (name, worst)


@pytest.mark.parametrize("name", NAMES)
def test_split_heads_vs_float64_and_the_empty_band(net, name):
    """all_heads = 1 and both thresholds at +inf: no cell is listed, so every head row is the split arithmetic's - within
    C_F32 * A of the chained split reference - and dl == head1 - head0 bit for bit; the band is empty: tbuf[0] == 0, mode 1
    writes nothing, every count is 0."""
    refs = _reference(net, name)
    run = run_pyramid(net, name, INF, -INF, all_heads=1)
    worst = 0.0
    for li, (b, r) in enumerate(zip(run["levels"], refs)):
        dl, counts, seg, mask, rest = _workspace(b)
        head = b["head"].t
        worst = max(worst, _ratio((name, li), _nchw(head), r["shead"], r["shead_A"]))
        assert torch.equal(_bits(dl), _bits(head[..., 1] - head[..., 0])), (name, li)
        assert not bool(counts.any()) and bool((seg == -7).all()), (name, li)
        if b["f16"]:
            assert bool(_sentinel(b["x1"].t).all()), (name, li)
        assert not bool(b["counts"].t.any()) and not bool(b["bc"].t.any()), (name, li)
        for k in ("boxes", "scores", "regs"):
            assert bool(_sentinel(b[k].t).all()) and b[k].guards_intact(), (name, li, k)
    if run["tbuf"] is not None:
        assert not bool(run["tbuf"].t.any()) and bool((run["tiles"].t == -7).all()), name
    _report(f"{name:<12s} split heads (all_heads, thresholds +inf) worst err/bound {worst:.3f}")
    assert worst <= 1.0, (name, worst)


@pytest.mark.parametrize("name,band", CASES)
def test_exact_rows_and_candidates_vs_float64(net, name, band):
    """The rows the exact pass wrote against the float64 f32 chain; the candidate lists against the reference's verdicts: every
    pass cell listed, no fail cell, raster order, pnet_emit's boxes in numpy float32, scores and regressions within their
    rows' bounds (+ 1e-6 through expf)."""
    t = P.TABLES[name]
    refs = _reference(net, name)
    pyr, _ = _runs(net, name, band)
    lo, hi = t.band(band)
    w_row = w_score = w_reg = 0.0
    nre = nlisted = nund = 0
    for li, (b, r) in enumerate(zip(pyr["levels"], refs)):
        tag = (name, band, li)
        H3, W3 = b["H1"] - 4, b["W1"] - 4
        cells = _listed_cells(b).cpu()
        nre += cells.numel()
        head = b["head"].t.reshape(-1, 6).cpu().double()
        want, A = (x.permute(0, 2, 3, 1).reshape(-1, 6) for x in (r["head"], r["head_A"]))
        if cells.numel():
            assert torch.equal(torch.unique(cells), cells), tag
            w_row = max(w_row, _ratio(tag, head[cells], want[cells], A[cells]))
        verdict, _ = P.decide(r, t.thr, lo, hi)
        nund += int((verdict == P.UNDECIDED).sum())
        swant, sA = (x.permute(0, 2, 3, 1).reshape(-1, 6) for x in (r["shead"], r["shead_A"]))
        exact = torch.zeros(head.shape[0], dtype=torch.bool)
        exact[cells] = True
        xs_of = {float(v): i for i, v in enumerate(P.emit_boxes(np.zeros(W3), np.arange(W3), t.levels[li][3])[:, 0])}
        ys_of = {float(v): i for i, v in enumerate(P.emit_boxes(np.arange(H3), np.zeros(H3), t.levels[li][3])[:, 1])}
        counts = b["counts"].t.cpu()
        boxes, scores, regs = (b[k].t.cpu() for k in ("boxes", "scores", "regs"))
        for f in range(t.N):
            n = int(counts[f])
            bx = boxes[f, :n].numpy()
            cx = np.array([xs_of[float(v)] for v in bx[:, 0]], dtype=np.int64)
            cy = np.array([ys_of[float(v)] for v in bx[:, 1]], dtype=np.int64)
            assert np.array_equal(bx.view(np.int32), P.emit_boxes(cy, cx, t.levels[li][3]).view(np.int32)), (tag, f)
            cell = cy * W3 + cx
            assert (np.diff(cell) > 0).all(), (tag, f)                              # raster order, no cell twice
            listed = torch.zeros(H3 * W3, dtype=torch.bool)
            listed[torch.from_numpy(cell)] = True
            v = verdict[f].reshape(-1)
            assert bool(listed[v == P.PASS].all()), (tag, f, "a pass cell is missing")
            assert not bool(listed[v == P.FAIL].any()), (tag, f, "a fail cell is listed")
            nlisted += n
            if n:
                g = torch.from_numpy(cell) + f * H3 * W3
                ex = exact[g]
                rw = torch.where(ex[:, None], want[g], swant[g])
                rA = torch.where(ex[:, None], A[g], sA[g])
                assert torch.equal(head[g].float(), torch.cat([head[g][:, :2].float(), regs[f, :n]], 1)), (tag, f)     # the row's regs, as written
                w_reg = max(w_reg, _ratio((tag, f), regs[f, :n].double(), rw[:, 2:], rA[:, 2:]))
                p = torch.sigmoid(rw[:, 1] - rw[:, 0])
                e = (scores[f, :n].double() - p).abs() / (0.25 * C_F32 * (rA[:, 1] + rA[:, 0]) + P.EXPF)
                w_score = max(w_score, float(e.max()))
    _report(f"{name:<12s} {'band' if band else 'no band'}: {nre} cells re-evaluated, rows worst err/bound {w_row:.3f}; {nlisted} candidates "
            f"({nund} cells undecided), regs {w_reg:.3f}, scores {w_score:.3f}")
    assert w_row <= 1.0 and w_reg <= 1.0 and w_score <= 1.0, (name, band, w_row, w_reg, w_score)


# ---------------------------------------------------------------------------------------------------- 4. the tile list's edges
@pytest.mark.parametrize("name", ["grid512", "interleaved", "rpb8", "sixteen"])
def test_tile_list_capacity_below_the_count(net, name):
    """mode 1 with list_cap three below the count: exactly the first list_cap tiles of the list are written (without the band:
    every cell at or above lo is listed, so the list is long enough)"""
    lo, hi = P.TABLES[name].band(False)
    run = run_pyramid(net, name, lo, hi, short=3)
    n, cap = int(run["tbuf"].t[0]), run["list_cap"]
    assert cap == n - 3 and cap >= 1
    first = run["tiles"].t[:cap]
    for li, b in enumerate(run["levels"]):
        sx = _sentinel(b["x1"].t)
        if not b["f16"]:
            assert not bool(sx.any()), (name, li)
            continue
        inside = _tile_mask(b, first[(first >> 27) == li] & ((1 << 27) - 1))
        assert torch.equal(sx.any(-1), ~inside) and torch.equal(sx.all(-1), ~inside), (name, li)
        assert b["x1"].guards_intact()
    dropped = run["tiles"].t[cap:n]
    assert dropped.numel() == 3 and not bool((dropped == -7).any())


# ---------------------------------------------------------------------------------------------------- 5. refusals
def test_pyramid_entries_refuse_bad_arguments(net):
    """each refusal raises (FR_E_INVALID) before any launch: every buffer keeps its sentinel"""
    name = "interleaved"
    t, fr, lib, s = P.TABLES[name], _frames(name), net["lib"], _lib.stream_ptr()
    levels, entries = _alloc(t)
    n = len(entries)
    tbuf, tiles = Buf((64,), torch.int32, -7), Buf((64,), torch.int32, -7)
    f = _lib.ptr(fr)

    def table(edit=None, count=n):
        es = [_lib.PnetLevel(*[getattr(e, k) for k, _ in _lib.PnetLevel._fields_]) for e in (entries * 3)[:max(count, 1)]]
        if edit:
            edit(es)
        return (_lib.PnetLevel * len(es))(*es)

    def conv1(lv, count, mode=0, lst=(None, None, 0)):
        lib.fr_pnet_pyramid_conv1(mode, f, t.N, t.FH, t.FW, lv, count, *net["p1w"], *lst, s)

    def p23(lv, count):
        lib.fr_pnet_pyramid_p23(lv, count, t.N, *net["p23p"], 0, 0.0, -INF, s)

    def band(lv, count):
        lib.fr_pnet_pyramid_band_tiles(lv, count, t.N, tbuf.ptr, tiles.ptr, s)

    def setter(i, **kw):
        def edit(es):
            for k, v in kw.items():
                setattr(es[i], k, v)
        return edit

    def no_f16(es):
        for e in es:
            e.f16 = 0

    for count in (0, 17):                                                            # nlevels 0 and 17
        for call in (conv1, p23, band):
            with pytest.raises(_lib.FrError, match="levels|bad argument"):
                call(table(count=count), count)
    with pytest.raises(_lib.FrError, match="mode must be 0 or 1"):
        conv1(table(), n, mode=2)
    with pytest.raises(_lib.FrError, match="needs a tile list"):
        conv1(table(), n, mode=1)
    with pytest.raises(_lib.FrError, match="needs a tile list"):
        conv1(table(), n, mode=1, lst=(tiles.ptr, tbuf.ptr, 0))
    with pytest.raises(_lib.FrError, match="level 2: bad entry"):
        conv1(table(setter(2, hs=2, H1=0)), n)                                       # hs < 3
    with pytest.raises(_lib.FrError, match="level 1: bad entry"):
        conv1(table(setter(1, H1=entries[1].H1 + 1)), n)                             # H1 != (hs - 1) / 2
    with pytest.raises(_lib.FrError, match="level 5: bad entry"):
        conv1(table(setter(5, W1=entries[5].W1 - 1)), n)
    with pytest.raises(_lib.FrError, match="level 3: bad entry"):
        conv1(table(setter(3, x1s=None)), n)                                         # null x1s
    with pytest.raises(_lib.FrError, match="level 3: bad entry"):
        p23(table(setter(3, x1s=None)), n)
    with pytest.raises(_lib.FrError, match="level 4: bad entry"):
        p23(table(setter(4, head=None)), n)                                          # null head
    with pytest.raises(_lib.FrError, match="no level in the f16 form"):
        band(table(no_f16), n)
    rc = lib._c.fr_pnet_pyramid_band_tiles(table(no_f16), n, t.N, tbuf.ptr, tiles.ptr, s)
    assert rc == lib._c.fr_pnet_pyramid_conv1(2, f, t.N, t.FH, t.FW, table(), n, *net["p1w"], None, None, 0, s) < 0      # FR_E_INVALID
    torch.cuda.synchronize()
    assert bool((tbuf.raw == -7).all()) and bool((tiles.raw == -7).all())
    for b in levels:
        for k in ("x1", "xs", "head", "wsp", "bc", "boxes", "scores", "regs", "counts"):
            if not (k == "wsp"):
                assert bool(_sentinel(b[k].raw).all()), k
        assert bool((b["wsp"].raw[GUARD + b["lay"]["cells"]:] == -7).all()) and bool(_sentinel(b["wsp"].t[:b["lay"]["cells"]].view(torch.float32)).all())
