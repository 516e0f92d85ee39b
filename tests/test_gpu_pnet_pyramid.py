"""The batch detector's pyramid-wide P-Net launch plan (MTCNNHIP.pyramid_launch: every layer launched once over all levels,
csrc fr_pnet_pyramid_*) against the per-level plan of the same build: the same bits everywhere, no tolerance.

Inputs are seeded: tests/golden/make_golden.synth_frame (the 4K frames are 2 x 2 mosaics of its 1080p frames)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))


def _frames(kind):
    from make_golden import synth_frame
    if kind == "12x1080p":
        frs = np.stack([synth_frame(1080, 1920, 200 + i) for i in range(12)])
    elif kind == "8x4k":
        q = [synth_frame(1080, 1920, 300 + i) for i in range(8)]
        frs = np.stack([np.concatenate([np.concatenate([q[i], q[(i + 1) % 8]], 1),
                                        np.concatenate([q[(i + 3) % 8], q[(i + 5) % 8]], 1)], 0) for i in range(8)])
    else:
        frs = np.stack([synth_frame(1000, 1777, 400 + i) for i in range(9)])
    return torch.from_numpy(np.ascontiguousarray(frs)).cuda()


def _detector(**attrs):
    from facerecognition_infrenceengine_amd import weights
    from facerecognition_infrenceengine_amd.mtcnn import MTCNNHIP
    det = MTCNNHIP(*weights.synth_mtcnn_states(), device="cuda:0", batch_min_pixels=0)
    for k, v in attrs.items():
        setattr(det, k, v)
    return det


def _run(det, fr, pyramid):
    """one detect_batch under the given plan -> (result, per-level tensors, candidate lists, path)"""
    det.pyramid_launch = pyramid
    det.level_tensors = []
    try:
        out = det.detect_batch(fr)
        torch.cuda.synchronize()
        assert det.exact_list_overflow() == []
        levels = list(det.level_tensors)
    finally:
        det.level_tensors = None
    cand = levels.pop()["cand"]
    return out, levels, cand, dict(det._tls.path)


def _p23_layout(N, h, w):
    """csrc/pnet_fused.hip p23_layout: (cells, grid, seg_cap) of a level's workspace [dl | 512 counts | list segments]"""
    ncell = N * (h - 4) * (w - 4)
    ntiles = N * (-(-(w - 4) // 32)) * (-(-(h - 4) // 8))
    grid = min(ntiles, 512)
    return ncell, grid, -(-ntiles // grid) * 256


def _band_lists(lv, N):
    """(dl, per-block counts, per-block SORTED cell lists padded with -1) of a level"""
    ncell, grid, seg_cap = _p23_layout(N, lv["h"], lv["w"])
    wi = lv["wsp"].view(torch.int32)
    counts = wi[ncell:ncell + grid].clone()
    seg = wi[ncell + 512:ncell + 512 + grid * seg_cap].reshape(grid, seg_cap)
    assert int(counts.min()) >= 0 and int(counts.max()) <= seg_cap
    used = torch.arange(seg_cap, device=seg.device)[None, :] < counts[:, None]
    cells = torch.where(used, seg, torch.full_like(seg, -1)).sort(dim=1).values       # the order inside a block's list is a race
    return lv["wsp"][:ncell], counts, cells


def _tile_mask(tiles, N, h, w):
    """conv1-map pixels [N, h, w] inside the listed 8 x 32-pixel tiles (tile = (frame * regions_y + ry) * regions_x + rx)"""
    ry, rx = (h + 7) // 8, (w + 31) // 32
    m = torch.zeros(N * ry * rx, dtype=torch.bool, device=tiles.device)
    m[tiles.long()] = True
    m = m.reshape(N, ry, rx).repeat_interleave(8, 1).repeat_interleave(32, 2)
    return m[:, :h, :w]


def _tiles_by_level(levels, pyramid):
    """{level index: sorted tile numbers} of the exact conv1 pass"""
    out = {}
    if pyramid:
        if "tiles" not in levels[0]:
            return out
        n = int(levels[0]["tbuf"][0])
        e = levels[0]["tiles"][:n]
        assert n <= levels[0]["tiles"].numel()
        for li, lv in enumerate(levels):
            if lv["f16"]:
                out[li] = (e[(e >> 27) == li] & ((1 << 27) - 1)).sort().values
        assert sum(t.numel() for t in out.values()) == n
    else:
        for li, lv in enumerate(levels):
            if lv["f16"]:
                out[li] = lv["tiles"][:int(lv["tbuf"][0])].sort().values
    return out


def _assert_same(fr, det, expect_f16):
    N = fr.shape[0]
    ra, la, ca, pa = _run(det, fr, False)
    rb, lb, cb, pb = _run(det, fr, True)
    nlev = len(la)
    assert nlev == len(lb) >= 8
    # the path, as the end-to-end tests read it
    for p in (pa, pb):
        assert p["batch"] and p["frames"] == N and p["chunks"] == 1 and p["unfused_levels"] == 0, p
        assert p["fused_levels"] == nlev and p["band_levels"] == (nlev if det.pnet_band else 0), p
    assert pa["pconv1_mfma_levels"] == pb["pconv1_mfma_levels"] == [(lv["h"], lv["w"]) for lv in la if lv["f16"]]
    assert all(h * w >= det.split_pconv1_min_px for h, w in pb["pconv1_mfma_levels"])
    assert [bool(lv["f16"]) for lv in lb] == [bool(lv["f16"]) for lv in la]
    assert expect_f16(sum(bool(lv["f16"]) for lv in lb), nlev)
    ta, tb = _tiles_by_level(la, False), _tiles_by_level(lb, True)
    assert sorted(ta) == sorted(tb)
    t0 = det.thresholds[0]
    thr = math.log(t0 / (1.0 - t0)) - det.refine_margin
    listed = written = 0
    for li, (a, b) in enumerate(zip(la, lb)):
        h, w = a["h"], a["w"]
        assert (h, w) == (b["h"], b["w"])
        assert torch.equal(a["xs"], b["xs"]), ("split conv1 map", li)
        dla, cnta, cella = _band_lists(a, N)
        dlb, cntb, cellb = _band_lists(b, N)
        assert torch.equal(dla.view(torch.int32), dlb.view(torch.int32)), ("logit differences", li)
        assert torch.equal(cnta, cntb) and torch.equal(cella, cellb), ("band lists", li)
        listed += int(cnta.sum())
        rows = ((dla >= thr) | ~torch.isfinite(dla)).reshape(N, h - 4, w - 4)          # the head rows a level writes
        assert torch.equal(a["head"][rows].view(torch.int32), b["head"][rows].view(torch.int32)), ("head rows", li)
        written += int(rows.sum())
        if a["f16"]:
            assert torch.equal(ta[li], tb[li]), ("exact conv1 tiles", li)
            m = _tile_mask(ta[li], N, h, w)
            assert torch.equal(a["x"][m].view(torch.int32), b["x"][m].view(torch.int32)), ("sparse f32 conv1 map", li)
        else:
            assert torch.equal(a["x"].view(torch.int32), b["x"].view(torch.int32)), ("f32 conv1 map", li)
    assert listed >= 50 and written >= listed
    # the candidate lists [level, frame, slot]
    (ab, as_, ar, ac), (bb, bs, br, bc) = ca, cb
    assert torch.equal(ac, bc) and int(ac.sum()) >= 100
    used = torch.arange(ab.shape[2], device="cuda")[None, None, :] < ac[:, :, None]
    for x, y in ((ab, bb), (as_, bs), (ar, br)):
        assert torch.equal(x[used].view(torch.int32), y[used].view(torch.int32))
    # what detect_batch returns
    assert torch.equal(ra[3], rb[3]) and int(ra[3].sum()) >= N
    used = torch.arange(ra[0].shape[1], device="cuda")[None, :] < ra[3][:, None]
    for x, y in zip(ra[:3], rb[:3]):
        assert torch.equal(x[used].view(torch.int32), y[used].view(torch.int32))
    return cb


@pytest.mark.parametrize("kind", ["12x1080p", "8x4k", "9x1000x1777"])
def test_pyramid_plan_equals_per_level_plan(kind):
    """Default gates: per level the split conv1 map, the logit differences, the band lists (as sets per block), the head rows a
    level writes, the f32 conv1 map (inside the exact tiles where it is sparse), then the candidate lists and the final faces."""
    fr = _frames(kind)
    det = _detector()
    _assert_same(fr, det, lambda n16, nlev: 1 <= n16 < nlev)


@pytest.mark.parametrize("kind", ["12x1080p", "9x1000x1777"])
def test_pyramid_plan_every_level_f16_and_none(kind):
    """``split_pconv1_min_px`` = 25 (every level takes conv1's f16 form and the shared exact-tile launches) and ``split_pconv1``
    off (none does): both plans agree bit for bit, and the pyramid plan's candidates stand to an all-exact detector
    (``set_exact(True)``) as test_pnet_conv1_on_matrix_cores_with_exact_tiles_under_the_band states it: the same cells in the
    same order, the cells well inside the band bit-identical, the others within the split format's error."""
    fr = _frames(kind)
    N = fr.shape[0]
    exact = _detector().set_exact(True)
    _, _, (eb, es, er, ec), pe = _run(exact, fr, False)
    assert pe["band_levels"] == 0 and pe["pconv1_mfma_levels"] == []
    lt = math.log(exact.thresholds[0] / (1.0 - exact.thresholds[0]))
    for attrs, expect in ((dict(split_pconv1_min_px=25), lambda n16, nlev: n16 == nlev), (dict(split_pconv1=False), lambda n16, nlev: n16 == 0)):
        det = _detector(**attrs)
        gb, gs, gr, gc = _assert_same(fr, det, expect)
        assert torch.equal(gc, ec)
        used = torch.arange(gb.shape[2], device="cuda")[None, None, :] < gc[:, :, None]
        assert torch.equal(gb[used], eb[used])                                # the same cells in the same order
        s = es[used]
        near = (torch.log(s / (1 - s)) - lt).abs() < 0.5 * det.refine_margin  # well inside the band by the f32 path's own score
        assert int(near.sum()) >= 1
        assert torch.equal(gs[used][near], s[near]) and torch.equal(gr[used][near], er[used][near])
        assert float((gs[used] - s).abs().max()) <= 5e-6 and float((gr[used] - er[used]).abs().max()) <= 2e-5
