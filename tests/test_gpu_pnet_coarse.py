"""The fused P-Net in two tiers (csrc/pnet_fused.hip: the coarse pass pnet23_body<true> over every cell, the split re-evaluation
pnet23_reeval_body of its list) against the one-tier split kernel of the same build, through the C ABI and end to end:

1. fr_pnet23_coarse_f16 against fr_pnet23_split_f16 per level: with coarse_margin = +inf every cell carries the split kernel's
   bits; with the default margin every cell the split kernel lists or keeps does, every other cell stays below the threshold, and
   the second tier visits fewer cells than there are;
2. non-finite operands: the same lists, the same non-finite cells;
3. fr_pnet_pyramid_p23_coarse against fr_pnet_pyramid_p23 on a hand-built table (one tile per frame, a ragged edge, more than
   512 tiles), sentinels and guard zones intact;
4. detect_batch with ``coarse_p23`` on and off, both launch plans: the same bits from the candidate lists to the faces;
5. the envelope: the hi-only format's error of the logit difference by operand scale, against ``coarse_margin`` / 20.

Inputs of 1 - 3: seeded random conv1 maps and the mixed-slope weights of tests/helpers/pyramid_ref.py; the head bias is chosen, on
the host emulation of tests/helpers/pnet_coarse_ref.py, so that the split kernel's own output then holds cells at or above the
threshold, cells inside [thr - coarse_margin, thr) and a majority below - asserted on that output before anything is compared.
Run with -s for the measured lines."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

from facerecognition_infrenceengine_amd import _lib, weights
from facerecognition_infrenceengine_amd.mtcnn import DetectSettings, MTCNNHIP
from tests.helpers import detect_ref as ref
from tests.helpers import pnet_coarse_ref as C
from tests.helpers import pyramid_ref as P

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

MARGIN = DetectSettings.coarse_margin
INF = float("inf")
GUARD = 64
THR = 0.6
LT = math.log(THR / (1.0 - THR))
LO, HI = float(np.float32(LT - P.REFINE_MARGIN)), float(np.float32(LT + P.REFINE_MARGIN))
MAP_RMS = 0.45               # no smaller than the RMS of the synthetic frames' conv1 maps (0.42 over all levels, tests/test_pnet_coarse_host.py)


class Buf:
    """a device buffer pre-filled with a sentinel (NaN / -7), GUARD elements of it in front and behind; ``t`` is the payload"""

    def __init__(self, n, dtype):
        self.fill = float("nan") if dtype == torch.float32 else -7
        self.raw = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device="cuda")
        self.t = self.raw[GUARD:GUARD + n]

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def guards_intact(self):
        g = torch.cat([self.raw[:GUARD], self.raw[-GUARD:]])
        return bool(torch.isnan(g).all()) if self.raw.dtype == torch.float32 else bool((g == -7).all())


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _split_bytes(x):
    """f32 [.., 12] -> the split map's rows [hi 16 | lo 16] f16, as uint8 [.., 64]"""
    xp = torch.zeros((*x.shape[:-1], 16), device=x.device)
    xp[..., :x.shape[-1]] = x
    hi = xp.half()
    return torch.cat([hi, (xp - hi.float()).half()], -1).contiguous().view(torch.uint8)


def _p23(L2, L3):
    hw, hb = L3.head
    w2p = torch.zeros((16, 10, 16)); w2p[:, :9, :10] = L2.w.float().permute(0, 2, 3, 1).reshape(16, 9, 10)
    w3p = torch.zeros((32, 10, 16)); w3p[:, :9, :16] = L3.w.float().permute(0, 2, 3, 1).reshape(32, 9, 16)
    return tuple(t.float().contiguous().cuda() for t in (w2p, L2.b, L2.slope, w3p, L3.b, L3.slope, hw.t(), hb))


def _maps(shapes, B, seed, amp):
    g = torch.Generator().manual_seed(seed)
    out = []
    for H1, W1 in shapes:
        x = torch.zeros((B, H1, W1, 12))
        x[..., :10] = torch.randn((B, H1, W1, 10), generator=g) * amp
        out.append(x)
    return out


def _need(ncell):
    """cells a case must hold at or above the threshold, and inside the margin below it: 10, or - a case of a handful of cells
    (the 5 x 5 map: one cell per frame) - one"""
    return 10 if ncell >= 100 else 1


def _case(shapes, B, L):
    """Seeded maps and a head bias for them: (maps, layers 1 / 2 with the bias).  On the host emulation the cells are spread over
    ~0.1 logit (the maps' amplitude is halved until they are) and the bias puts a quarter of them (one of three) at or above the
    threshold; the first seed whose emulated counts hold with 1e-3 to spare is taken."""
    for seed in range(40):
        amp = MAP_RMS
        while True:
            maps = _maps(shapes, B, 7000 + seed, amp)
            d = torch.cat([C.dl_hi_only(x[..., :10].permute(0, 3, 1, 2), L[1], L[2]).flatten() for x in maps]).double()
            if float(d.std()) <= 0.12 or amp < 1e-3:
                break
            amp *= 0.5
        n, need = d.numel(), _need(d.numel())
        ds = d.sort(descending=True).values
        k = max(need, n // 4) if n >= 100 else 1
        delta = (LO - MARGIN / 2 - float(ds[1])) if n < 100 else (LO - float(ds[k - 1] + ds[k]) / 2)
        e = d + delta
        above, inside = int((e >= LO + 1e-3).sum()), int(((e >= LO - MARGIN + 1e-3) & (e < LO - 1e-3)).sum())
        below = int((e < LO - 1e-3).sum())
        if above >= need and inside >= need and 2 * below > n:
            hw, hb = L[2].head
            hb = hb.clone(); hb[1] += delta
            L3 = ref.Layer(L[2].w, L[2].b, L[2].slope, 0, (hw, hb))
            return maps, L[1], L3
    raise AssertionError("no seed gives the case its cells")


@pytest.fixture(scope="module")
def env():
    return dict(lib=_lib.load(), L=ref.pnet_layers(P.states()[0]), s=_lib.stream_ptr())


# ---------------------------------------------------------------------------------------------------- running a level
def _run_level(env, x1, xs, p23, lo, hi, margin, all_heads=2):
    """one level through fr_pnet23_split_f16 (margin None) or fr_pnet23_coarse_f16 -> its buffers"""
    lib, s = env["lib"], env["s"]
    B, H1, W1, _ = x1.shape
    lay = P.layout(B, H1, W1)
    head, wsp = Buf(lay["cells"] * 6, torch.float32), Buf(lay["workspace_bytes"] // 4, torch.int32)
    wsp.t[:lay["cells"]].view(torch.float32).fill_(float("nan"))
    pp = [_lib.ptr(t) for t in p23]
    out = dict(head=head, wsp=wsp, lay=lay, B=B, H1=H1, W1=W1)
    if margin is None:
        lib.fr_pnet23_split_f16(_lib.ptr(x1), _lib.ptr(xs), B, H1, W1, *pp, head.ptr, all_heads, lo, hi, None, wsp.ptr,
                                lay["workspace_bytes"], s)
    else:
        nb = lib.fr_pnet23_coarse_workspace_bytes(B, H1, W1)
        assert nb == 512 * 4 + lay["grid"] * lay["seg_cap"] * 4
        cws, visited = Buf(nb // 4, torch.int32), torch.zeros(1, dtype=torch.int32, device="cuda")
        lib.fr_pnet23_coarse_f16(_lib.ptr(x1), _lib.ptr(xs), B, H1, W1, *pp, head.ptr, all_heads, lo, hi, None, wsp.ptr,
                                 lay["workspace_bytes"], margin, cws.ptr, nb, _lib.ptr(visited), s)
        out.update(cws=cws, visited=visited)
    return out


def _workspace(b):
    """(dl [cells] f32, the 512 counters, segments [grid, seg_cap], in-segment mask)"""
    lay, w = b["lay"], b["wsp"].t
    dl = w[:lay["cells"]].view(torch.float32)
    counts = w[lay["cells"]:lay["cells"] + 512]
    seg = w[lay["cells"] + 512:].view(lay["grid"], lay["seg_cap"])
    mask = torch.arange(lay["seg_cap"], device="cuda")[None, :] < counts[:lay["grid"], None]
    return dl, counts, seg, mask


def _preconditions(par, lo, tag):
    dl = _workspace(par)[0]
    n, need = dl.numel(), _need(dl.numel())
    above, inside = int((dl >= lo).sum()), int(((dl >= lo - MARGIN) & (dl < lo)).sum())
    assert above >= need and inside >= need and 2 * int((dl < lo).sum()) > n, (tag, n, above, inside)
    return above, inside


def _compare(par, new, lo, every_cell, tag):
    """the post-state of the two-tier entry against the split kernel's.  every_cell: dl in every cell (coarse_margin = +inf);
    else in the cells the split kernel lists or keeps (dl >= lo or non-finite), the others below lo.  Returns the visited count."""
    for k in ("head", "wsp", "cws"):
        assert new[k].guards_intact(), (tag, k)
    dp, cp, sp, mp = _workspace(par)
    dn, cn, sn, mn = _workspace(new)
    keep = (dp >= lo) | ~torch.isfinite(dp)
    assert torch.equal(_bits(dp)[keep], _bits(dn)[keep]), (tag, "dl of the cells that can be kept")
    if every_cell:
        assert torch.equal(_bits(dp), _bits(dn)), (tag, "dl")
    else:
        assert bool((dn[~keep] < lo).all()), (tag, "a cell the split kernel rejects is not below the threshold")
    # head rows: written for the same cells with the same bits, the sentinel everywhere else
    assert torch.equal(_bits(par["head"].t), _bits(new["head"].t)), (tag, "head rows")
    assert torch.equal(cp, cn) and bool((cn[:par["lay"]["grid"]] >= 0).all()), (tag, "counts")      # (past the grid: the sentinel, in both)
    big = torch.iinfo(torch.int32).max
    assert torch.equal(torch.sort(torch.where(mp, sp, big), 1).values, torch.sort(torch.where(mn, sn, big), 1).values), (tag, "lists")
    assert bool((sn[~mn] == -7).all()), (tag, "a segment is written past its count")
    visited = int(new["visited"])
    ccounts = new["cws"].t[:new["lay"]["grid"]]
    assert visited == int(ccounts.sum()) >= int(cn[:par["lay"]["grid"]].sum()), (tag, "visited cells")
    return visited


# ---------------------------------------------------------------------------------------------------- 1. per level
@pytest.mark.parametrize("band", [True, False])
@pytest.mark.parametrize("H1,W1", [(5, 5), (9, 13), (13, 37)])
def test_coarse_level_entry_equals_the_split_kernel(env, H1, W1, band):
    B = 3
    maps, L2, L3 = _case([(H1, W1)], B, env["L"])
    x1 = maps[0].cuda()
    xs, p23 = _split_bytes(x1), _p23(L2, L3)
    hi = HI if band else -INF
    par = _run_level(env, x1, xs, p23, LO, hi, None)
    full = _run_level(env, x1, xs, p23, LO, hi, INF)
    new = _run_level(env, x1, xs, p23, LO, hi, MARGIN)
    torch.cuda.synchronize()
    tag = (H1, W1, band)
    above, inside = _preconditions(par, LO, tag)
    ncell = par["lay"]["cells"]
    assert _compare(par, full, LO, True, tag + ("inf",)) == ncell           # (a) every cell re-evaluated: the split kernel's bits everywhere
    visited = _compare(par, new, LO, False, tag + ("default",))             # (b)
    print(f"coarse level {H1}x{W1} band={band}: {ncell} cells, {above} at or above the threshold, {inside} inside the margin, {visited} visited")
    assert above <= visited < ncell, tag                                    # the skip is exercised


def test_coarse_level_entry_refusals(env):
    """all_heads & 1, a missing or short coarse buffer, a negative margin: FR_E_INVALID before any launch"""
    lib, s = env["lib"], env["s"]
    maps, L2, L3 = _case([(9, 13)], 3, env["L"])
    x1 = maps[0].cuda()
    xs, pp = _split_bytes(x1), [_lib.ptr(t) for t in _p23(L2, L3)]
    lay = P.layout(3, 9, 13)
    head, wsp = Buf(lay["cells"] * 6, torch.float32), Buf(lay["workspace_bytes"] // 4, torch.int32)
    nb = lib.fr_pnet23_coarse_workspace_bytes(3, 9, 13)
    cws = Buf(nb // 4, torch.int32)
    for all_heads, margin, cp, cb, what in ((1, MARGIN, cws.ptr, nb, "all_heads"), (3, MARGIN, cws.ptr, nb, "all_heads"),
                                            (2, MARGIN, None, nb, "coarse buffer"), (2, MARGIN, cws.ptr, nb - 4, "coarse buffer"),
                                            (2, -1.0, cws.ptr, nb, "margin")):
        with pytest.raises(_lib.FrError, match=what):
            lib.fr_pnet23_coarse_f16(_lib.ptr(x1), _lib.ptr(xs), 3, 9, 13, *pp, head.ptr, all_heads, LO, HI, None, wsp.ptr,
                                     lay["workspace_bytes"], margin, cp, cb, None, s)
    torch.cuda.synchronize()
    assert bool(torch.isnan(head.raw).all()) and bool((wsp.raw == -7).all()) and bool((cws.raw == -7).all())


# ---------------------------------------------------------------------------------------------------- 2. non-finite operands
@pytest.mark.parametrize("band", [True, False])
def test_coarse_level_entry_with_non_finite_operands(env, band):
    """one +inf and one NaN as hi halves of the split map, 20 columns apart: the cells whose windows hold them (25 each) are
    non-finite and listed by both entries, and everything else compares as in 1."""
    B, H1, W1 = 3, 13, 37
    maps, L2, L3 = _case([(H1, W1)], B, env["L"])
    x1 = maps[0].cuda()
    xs, p23 = _split_bytes(x1), _p23(L2, L3)
    h = xs.view(torch.float16).view(B, H1, W1, 32)
    h[0, 6, 8, 3] = float("inf")
    h[1, 5, 28, 0] = float("nan")
    hi = HI if band else -INF
    par = _run_level(env, x1, xs, p23, LO, hi, None)
    new = _run_level(env, x1, xs, p23, LO, hi, MARGIN)
    torch.cuda.synchronize()
    dp, dn = (_workspace(r)[0].view(B, H1 - 4, W1 - 4) for r in (par, new))
    for n, y, x in ((0, 6, 8), (1, 5, 28)):
        win = (n, slice(y - 4, y + 1), slice(x - 4, x + 1))                   # the 25 cells whose 5 x 5 windows hold the pixel
        assert dp[win].numel() == 25 and not bool(torch.isfinite(dp[win]).any()), (n, y, x)
        assert torch.equal(torch.isfinite(dp[win]), torch.isfinite(dn[win])), (n, y, x)
    assert torch.equal(torch.isfinite(dp), torch.isfinite(dn))
    _compare(par, new, LO, False, ("non-finite", band))                       # the lists hold all 50 cells in both


# ---------------------------------------------------------------------------------------------------- 3. the pyramid-wide entry
TABLE = [(140, 500), (21, 45), (9, 13)]       # conv1 maps, largest first: 17 x 16 tiles per frame (544 of two frames > 512 blocks: 32 blocks
                                              # walk two tiles), 3 x 2 tiles with ragged edges, one tile per frame


def _run_table(env, maps, splits, p23, lo, hi, margin):
    lib, s = env["lib"], env["s"]
    B = maps[0].shape[0]
    levels, entries = [], []
    for x1, xs in zip(maps, splits):
        _, H1, W1, _ = x1.shape
        lay = P.layout(B, H1, W1)
        b = dict(head=Buf(lay["cells"] * 6, torch.float32), wsp=Buf(lay["workspace_bytes"] // 4, torch.int32), lay=lay, B=B, H1=H1, W1=W1)
        b["wsp"].t[:lay["cells"]].view(torch.float32).fill_(float("nan"))
        if margin is not None:
            b["cws"] = Buf(lib.fr_pnet23_coarse_workspace_bytes(B, H1, W1) // 4, torch.int32)
        levels.append(b)
        entries.append(_lib.PnetLevel(x1.data_ptr(), b["head"].ptr, b["wsp"].ptr, H1, W1, 0.5, None, None, None, None, None, xs.data_ptr(),
                                      2 * H1 + 1, 2 * W1 + 1, 0))
    lv = (_lib.PnetLevel * len(entries))(*entries)
    pp = [_lib.ptr(t) for t in p23]
    if margin is None:
        lib.fr_pnet_pyramid_p23(lv, len(entries), B, *pp, 0, lo, hi, s)
    else:
        visited = torch.zeros(1, dtype=torch.int32, device="cuda")
        cws = (ctypes.c_void_p * len(entries))(*[b["cws"].t.data_ptr() for b in levels])
        lib.fr_pnet_pyramid_p23_coarse(lv, len(entries), B, *pp, 0, lo, hi, margin, cws, _lib.ptr(visited), s)
        for b in levels:
            b["visited"] = visited
    return levels


@pytest.mark.parametrize("band", [True, False])
def test_coarse_pyramid_entry_equals_the_split_launch(env, band):
    B = 2
    assert P.layout(B, *TABLE[0])["tiles"] > 512 and P.layout(B, *TABLE[2])["tiles"] == B
    maps, L2, L3 = _case(TABLE, B, env["L"])
    maps = [m.cuda() for m in maps]
    splits, p23 = [_split_bytes(m) for m in maps], _p23(L2, L3)
    hi = HI if band else -INF
    par = _run_table(env, maps, splits, p23, LO, hi, None)
    full = _run_table(env, maps, splits, p23, LO, hi, INF)
    new = _run_table(env, maps, splits, p23, LO, hi, MARGIN)
    torch.cuda.synchronize()
    above = inside = ncell = 0
    for li, p in enumerate(par):
        dl = _workspace(p)[0]
        above, inside, ncell = above + int((dl >= LO).sum()), inside + int(((dl >= LO - MARGIN) & (dl < LO)).sum()), ncell + dl.numel()
    assert above >= 10 and inside >= 10 and above + inside < ncell // 2, (above, inside, ncell)
    _preconditions(par[0], LO, ("table", 0))                                  # the level whose blocks walk two tiles holds all three kinds
    for run, every in ((full, True), (new, False)):
        visited = 0
        for li, (p, n) in enumerate(zip(par, run)):
            n = dict(n, visited=int(n["cws"].t[:n["lay"]["grid"]].sum()))     # the entry's counter is the table's: a level's share is its counts
            visited += _compare(p, n, LO, every, ("table", li, band, every))
        assert visited == int(run[0]["visited"]), (band, every)
        assert (visited == ncell) if every else (above <= visited < ncell), (band, every, visited)
    print(f"coarse pyramid band={band}: {ncell} cells, {above} at or above the threshold, {inside} inside the margin, {visited} visited")
    with pytest.raises(_lib.FrError, match="all_heads"):
        lv = (_lib.PnetLevel * 1)(_lib.PnetLevel(maps[2].data_ptr(), par[2]["head"].ptr, par[2]["wsp"].ptr, 9, 13, 0.5, None, None, None, None,
                                                 None, splits[2].data_ptr(), 19, 27, 0))
        env["lib"].fr_pnet_pyramid_p23_coarse(lv, 1, B, *[_lib.ptr(t) for t in p23], 1, LO, hi, MARGIN,
                                              (ctypes.c_void_p * 1)(new[2]["cws"].t.data_ptr()), None, env["s"])


# ---------------------------------------------------------------------------------------------------- 4. end to end
def _detect(det, fr, pyramid, coarse):
    det.pyramid_launch, det.coarse_p23 = pyramid, coarse
    det.level_tensors = []
    try:
        out = det.detect_batch(fr)
        torch.cuda.synchronize()
        assert det.exact_list_overflow() == []
        cand = det.level_tensors[-1]["cand"]
    finally:
        det.level_tensors = None
    return out, cand, dict(det._tls.path)


def test_detect_batch_is_unchanged_by_the_coarse_pass():
    from make_golden import synth_frame
    fr = torch.from_numpy(np.ascontiguousarray(np.stack([synth_frame(360, 640, 170 + i) for i in range(8)]))).cuda()
    det = MTCNNHIP(*weights.synth_mtcnn_states(), device="cuda:0", batch_min_pixels=0)
    for pyramid in (True, False):
        (rb, rs, rk, rc), (cb, cs, cr, cc), pa = _detect(det, fr, pyramid, False)
        (nb, ns, nk, nc), (db, ds, dr, dc), pb = _detect(det, fr, pyramid, True)
        assert pa["batch"] and pb["batch"] and pa["coarse_levels"] == 0 and pb["coarse_levels"] == pb["fused_levels"] == pb["band_levels"] >= 6, (pa, pb)
        assert torch.equal(cc, dc) and int(cc.sum()) >= 50
        used = torch.arange(cb.shape[2], device="cuda")[None, None, :] < cc[:, :, None]
        for x, y in ((cb, db), (cs, ds), (cr, dr)):                           # the per-level candidate lists [level, frame, slot]
            assert torch.equal(_bits(x[used]), _bits(y[used])), pyramid
        assert torch.equal(rc, nc) and int(rc.sum()) >= 8
        used = torch.arange(rb.shape[1], device="cuda")[None, :] < rc[:, None]
        for x, y in ((rb, nb), (rs, ns), (rk, nk)):                           # boxes, scores, landmarks
            assert torch.equal(_bits(x[used].contiguous()), _bits(y[used].contiguous())), pyramid
    det.set_exact(True)
    for pyramid in (True, False):
        _, _, p = _detect(det, fr, pyramid, True)
        assert p["coarse_levels"] == 0 and p["band_levels"] == 0 and p["fused_levels"] >= 6, p
    det.set_exact(False)
    det.p23_all_heads = True                                                  # the split heads of every cell: the one-tier kernel's business
    _, _, p = _detect(det, fr, True, True)
    assert p["coarse_levels"] == 0 and p["band_levels"] >= 6, p


# ---------------------------------------------------------------------------------------------------- 5. the envelope
SCALES = tuple(range(-4, 5))         # the P-Net's supported operand scales 2^-4 .. 2^4 round the canonical weight scale


@pytest.mark.parametrize("k", SCALES)
def test_hi_only_format_error_by_operand_scale(env, k):
    """conv2's inputs and weights x 2^k, conv3's weights and the head weights x 2^-k (the network is unchanged, conv2's output is
    4^k its usual size - tests/test_gpu_detect_precision.py test_split_pnet23_vs_split_arithmetic) on conv1 maps of the RMS the
    synthetic frames' maps have; both thresholds at +inf, so no cell is re-evaluated and the dl map of the two-tier entry is the
    coarse pass's.  204 800 cells.  Every scale is inside the supported envelope: 20 x the largest difference from the split kernel's
    dl must fit in coarse_margin."""
    lib, s = env["lib"], 2.0 ** k
    L = ref.pnet_layers(weights.synth_mtcnn_states()[0])
    B, H1, W1 = 4, 164, 324
    g = torch.Generator(device="cuda").manual_seed(9000 + k)
    x1 = torch.zeros((B, H1, W1, 12), device="cuda")
    x1[..., :10] = torch.randn((B, H1, W1, 10), generator=g, device="cuda") * (MAP_RMS * s)
    xs = _split_bytes(x1)
    p23 = _p23(L[1].scaled(s, s * s), L[2].scaled(1.0 / s, s, 1.0 / s))
    par = _run_level(env, x1, xs, p23, INF, -INF, None)
    new = _run_level(env, x1, xs, p23, INF, -INF, MARGIN)
    torch.cuda.synchronize()
    dp, dn = _workspace(par)[0], _workspace(new)[0]
    assert dp.numel() >= 200_000 and bool(torch.isfinite(dp).all()) and bool(torch.isfinite(dn).all())
    assert int(new["visited"]) == 0 and not bool(_workspace(new)[1][:new["lay"]["grid"]].any())
    e = float((dn.double() - dp.double()).abs().max())
    print(f"P-Net conv2/conv3/heads, hi operands only 2^{k:+d}: max |dl0 - dl_split| {e:.3e} over {dp.numel()} cells "
          f"(dl std {float(dp.std()):.2f}); 20 x = {20 * e:.4f} of coarse_margin {MARGIN}")
    assert 20 * e <= MARGIN, (k, e)
