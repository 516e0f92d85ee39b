"""GPU: the gallery and frame kernels where offsets pass 2^31 and 2^32 (include/frhip.h promises N < 2^31 rows and frame stacks of any
length; nothing else in the suite leaves the first 2 GiB of a buffer).

1. A contiguous gallery of N = 2^22 + 4173 rows: 2^31 and 2^32 bytes in f32 (rows 2^20, 2^21), 2^31 elements in every type and 2^32
   bytes in f16 (row 2^22), a partial last tile.  The background is filled on the device with values in [-2^-7, 2^-7] and scores
   below 0.18 against any unit query (tests/helpers/large_ref.py); planted rows around every edge must come back, with the bits
   tests/helpers/scan_ref.py gives for the f32 scans and the tolerances tests/test_gpu_match.py holds for the coarse ones.
2. Writes and views at slots around 2^22 of a DeviceGallery of that capacity.
3. Frame stacks whose last frame starts past byte 2^31: every frame kernel on frames 86 and 87 of 88 4K frames against the same call on
   those frames alone (bit for bit) and against its existing CPU reference at its existing tolerance.
4. The two host branches that cut a scan range to 2^20 rows (scan_plan of scan_gemm.hip, pair_plan of pair_scan.hip).
A test skips only when the device reports less free memory than it needs; the largest needs about 22 GB.
tests/test_large_ref_host.py holds the premises on the CPU."""
import numpy as np
import pytest
import torch

from tests.helpers import large_ref as lr
from tests.helpers import scan_ref as sr

pytestmark = pytest.mark.gpu
GIB = 1 << 30
IDX_FILL = -7
SCORE_FILL = 0x7FC0BEEF                                                    # a NaN no kernel produces
COARSE_ATOL = 3e-6                                                         # tests/test_gpu_match.py, tests/test_gpu_view_scan.py


def _need(nbytes, what):
    torch.cuda.empty_cache()                                               # what earlier tests left cached is free memory too
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip(f"{what} needs {nbytes} bytes of device memory, {free} are free")


def _release():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _outputs(*shape):
    idx = torch.full(shape, IDX_FILL, dtype=torch.int64, device="cuda")
    score = torch.full(shape, SCORE_FILL, dtype=torch.int32, device="cuda").view(torch.float32)
    return idx, score


def _same(got, want):
    """indices and score bits, both with torch.equal"""
    wi, ws = torch.from_numpy(np.ascontiguousarray(want[0])), torch.from_numpy(np.ascontiguousarray(want[1]).view(np.int32))
    gi, gs = got[0].cpu(), _bits(got[1]).cpu()
    assert gi.shape == wi.shape and gs.shape == ws.shape
    return torch.equal(gi, wi) and torch.equal(gs, ws)


def _rows_of(T, rows):
    """T[rows] by plain slices: no index arithmetic but the narrow's own"""
    return torch.cat([T[int(r):int(r) + 1] for r in rows]).cpu()


def _put_rows(T, rows, vals):
    for r, v in zip(rows, vals):
        T[int(r):int(r) + 1].copy_(v[None])


def _fill_background(G, seed):
    """i.i.d. uniform in [-2^-7, 2^-7), in place, 2^19 rows (1 GiB of f32) at a time"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    for a in range(0, G.shape[0], 1 << 19):
        G[a:a + (1 << 19)].uniform_(-lr.AMP, lr.AMP, generator=g)


def _convert(lib, X, kind):
    from facerecognition_infrenceengine_amd import _lib
    out = torch.empty(X.shape, dtype=torch.float16 if kind == "f16" else torch.uint8, device="cuda")
    (lib.fr_f32_to_f16 if kind == "f16" else lib.fr_f32_to_f8)(_lib.ptr(X), _lib.ptr(out), X.numel(), _lib.stream_ptr())
    return out


def _raw(t):
    return t.view(torch.int16) if t.dtype == torch.float16 else t


# ---------------------------------------------------------------- 1. a contiguous gallery past 2^31 elements and 2^32 bytes
@pytest.fixture(scope="module")
def slab():
    """f32 [N][512], 8.6 GB: background + the planted rows of large_ref.plant(); no test writes to it"""
    _need(lr.N * 2048 + GIB, "the f32 slab")
    pl = lr.plant()
    G = torch.empty((lr.N, 512), dtype=torch.float32, device="cuda")
    _fill_background(G, 71)
    lo, hi = torch.aminmax(G[(1 << 22) + (1 << 11) + 1:lr.N - 14])         # a stretch without planted rows
    assert -lr.AMP <= float(lo) < -0.99 * lr.AMP and 0.99 * lr.AMP < float(hi) <= lr.AMP
    _put_rows(G, pl.rows, _dev(pl.P))
    assert torch.equal(_rows_of(G, pl.rows), torch.from_numpy(pl.P))
    yield G
    del G
    _release()


def _matcher(kind, slab):
    from facerecognition_infrenceengine_amd.gallery import GalleryMatcher
    m = GalleryMatcher("cuda:0", scan=kind)
    m.set_rows(range(lr.N), slab, normalise=False)
    assert m.G.data_ptr() == slab.data_ptr()
    return m


def test_l2norm_over_all_rows(slab):
    """fr_l2norm_rows_f32 through set_rows(normalise=True): planted rows and their background neighbours around every edge against
    NumPy, the tolerance of test_l2norm_rows_matches_numpy"""
    from facerecognition_infrenceengine_amd.gallery import GalleryMatcher
    _need(lr.N * 2048 + GIB, "the normalised copy")
    m = GalleryMatcher("cuda:0")
    m.set_rows(range(lr.N), slab, normalise=True)
    assert m.G.data_ptr() != slab.data_ptr() and m.G.shape == slab.shape
    rows = lr.check_rows()
    x = _rows_of(slab, rows).numpy()
    ref = x / np.linalg.norm(x, axis=1, keepdims=True)
    np.testing.assert_allclose(_rows_of(m.G, rows).numpy(), ref, rtol=3e-7, atol=1e-8)
    del m
    _release()


@pytest.mark.parametrize("kind", ["f32", "f16", "f8"])
def test_match_returns_the_planted_rows(slab, lib, kind):
    """fr_gallery_match_f32 / _f16 / _f8 through GalleryMatcher, 40 queries off unit length, also with row_offset = 2^33.  f16 / f8: the
    copy is the library's own conversion of the whole slab, read back around every edge against the conversion of those rows alone."""
    pl = lr.plant()
    if kind != "f32":
        _need(lr.N * (1024 if kind == "f16" else 512) + GIB, f"the {kind} copy")
    m = _matcher(kind, slab)
    if kind != "f32":
        rows = lr.check_rows()
        want = _convert(lib, _rows_of(slab, rows).cuda(), kind)
        assert m.G16.shape == slab.shape and torch.equal(_raw(_rows_of(m.G16, rows)), _raw(want).cpu())
    Qd = _dev(pl.Qraw)
    for off in (0, lr.OFFSET):
        idx, score = m.match_device(Qd, row_offset=off)
        wi, ws = lr.expect_match(pl.S, pl.rows, off)
        assert np.array_equal(wi, pl.target + off)
        if kind == "f32":
            assert _same((idx, score), (wi, ws)), (off, idx.tolist(), wi.tolist())
        else:
            assert np.array_equal(idx.cpu().numpy(), wi), (off, idx.tolist(), wi.tolist())
            np.testing.assert_allclose(score.cpu().numpy(), ws, atol=COARSE_ATOL, rtol=0)
    del m
    _release()


def _topk_f32(lib, Qd, Gd, K, row_offset=0):
    from facerecognition_infrenceengine_amd import _lib
    F, N = Qd.shape[0], Gd.shape[0]
    need = lib.fr_gallery_topk_workspace(F, N, K)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    idx, score = _outputs(F, K)
    lib.fr_gallery_topk_f32(_lib.ptr(Qd), _lib.ptr(Gd), F, N, 512, K, row_offset, _lib.ptr(idx), _lib.ptr(score), _lib.ptr(ws), need,
                            None, 0, _lib.stream_ptr())
    return idx, score


def _check_topk(got, pl, K, off=0):
    """The planted rows that score above 0.18 open the list, bit for bit.  Behind them come rows that score below it, planted or
    background, which only a scan of the slab could rank: distinct rows inside the slab, scores in (-1, 0.18) in descending order, and
    a planted row among them carries its own score's bits."""
    wi, ws, n = lr.expect_topk(pl.S, pl.rows, K, off)
    gi, gs = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert gi.shape == wi.shape and gs.shape == ws.shape
    for f in range(len(wi)):
        k = int(n[f])
        assert np.array_equal(gi[f, :k], wi[f, :k]), (f, gi[f], wi[f])
        assert np.array_equal(gs[f, :k].view(np.int32), ws[f, :k].view(np.int32)), (f, gs[f], ws[f])
        tail = gi[f, k:]
        assert ((gs[f, k:] > -1) & (gs[f, k:] < lr.BG_BOUND)).all() and (np.diff(gs[f, k:]) <= 0).all(), (f, gs[f])
        assert ((tail >= off) & (tail < off + lr.N)).all() and len(set(gi[f].tolist())) == K, (f, gi[f])
        for j in range(k, K):
            p = pl.where.get(int(gi[f, j]) - off)
            assert p is None or gs[f, j].view(np.int32) == pl.S[f, p].view(np.int32), (f, j, gi[f, j], gs[f, j], pl.S[f, p])


def test_exact_topk_lists_the_graded_rows_across_every_edge(slab, lib):
    """fr_gallery_topk_f32, K = 16: the graded query's list alternates between rows below 2^20 and above 2^22 and holds an exact tie
    across row 2^22; every other query's list opens with its planted rows"""
    pl = lr.plant()
    Qd = _dev(pl.Qn)
    for off in (0, lr.OFFSET):
        _check_topk(_topk_f32(lib, Qd, slab, 16, off), pl, 16, off)


def test_certified_coarse_topk_gives_the_bits_of_the_exact_scan(slab, lib):
    """a scan="f16" matcher over the slab answers top-16 by the coarse pass (last_topk()), with the exact scan's bits"""
    from facerecognition_infrenceengine_amd.gallery import last_topk
    pl = lr.plant()
    _need(lr.N * 1024 + GIB, "the f16 copy")
    m = _matcher("f16", slab)
    assert len(m) >= m.coarse_topk_min_rows
    got = m.match_topk_device(_dev(pl.Qraw), 16)
    info = last_topk()
    assert info["path"] == "coarse" and info["flags"] is not None
    flags = info["flags"].cpu().numpy()
    print(f"\ncoarse top-16 over {lr.N} rows: {int((flags == 0).sum())} of {len(flags)} queries certified")
    assert set(flags.tolist()) <= {0, 1}
    exact = _topk_f32(lib, _dev(pl.Qn), slab, 16)
    assert torch.equal(got[0], exact[0]) and torch.equal(_bits(got[1]), _bits(exact[1]))
    _check_topk(got, pl, 16)
    del m
    _release()


def test_first_above_finds_the_lowest_planted_row(slab, lib):
    from facerecognition_infrenceengine_amd import _lib
    pl = lr.plant()
    Qd = _dev(pl.Qn)
    F = Qd.shape[0]
    ws = torch.empty(F * 8, dtype=torch.uint8, device="cuda")
    for inclusive in (0, 1):
        for off in (0, lr.OFFSET):
            idx, score = _outputs(F)
            lib.fr_gallery_first_above_f32(_lib.ptr(Qd), _lib.ptr(slab), F, lr.N, 512, lr.THR, inclusive, off, _lib.ptr(idx),
                                           _lib.ptr(score), _lib.ptr(ws), F * 8, _lib.stream_ptr())
            want = lr.expect_first_above(pl.S1, pl.rows, lr.THR, inclusive, off)
            assert _same((idx, score), want), (inclusive, off, idx.tolist(), want[0].tolist())


def test_gmax_over_the_whole_slab_is_the_longest_planted_row(slab, lib):
    """the longest row is N - 13, past every edge; the tolerance is test_gmax_is_the_largest_norm_ever_written's (8 u, derived there)"""
    from facerecognition_infrenceengine_amd import _lib
    pl = lr.plant()
    gmax = torch.zeros(1, dtype=torch.float32, device="cuda")
    lib.fr_gallery_gmax_update(_lib.ptr(slab), None, lr.N, 512, _lib.ptr(gmax), _lib.stream_ptr())
    norms = np.linalg.norm(pl.P.astype(np.float64), axis=1)
    want = float(norms.max())
    assert int(norms.argmax()) == pl.where[lr.N - 13] and abs(want - lr.HEAVY) < 1e-6
    assert abs(float(gmax) - want) <= 8 * 2.0 ** -24 * (1 + 1e-6) * want, (float(gmax), want)


def test_fp8_only_slab_past_2_32_bytes(lib):
    """N8 = 2^23 + 4173 rows of e4m3 codes (4.3 GB), no f32 rows: fr_gallery_match_f8 with G32 == NULL returns the coarse maximum and
    the first row of its 4-row group.  Background: codes of |x| <= 2 = 256 * 2^-7 with random signs, written as bytes."""
    from facerecognition_infrenceengine_amd import _lib
    _need(lr.N8 * 512 + 2 * GIB, "the fp8 slab")
    pf = lr.plant_f8()
    G8 = torch.empty((lr.N8, 512), dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(72)
    for a in range(0, lr.N8, 1 << 21):                                     # 1 GiB of bytes at a time
        part = G8[a:a + (1 << 21)]
        part.random_(0, lr.F8_CODE_MAX + 1, generator=g)
        sign = torch.empty_like(part).random_(0, 2, generator=g)
        part.add_(sign, alpha=128)
        del sign
    assert int((G8[1:64] & 127).max()) == lr.F8_CODE_MAX
    P8 = _convert(lib, _dev(pf.P), "f8")
    _put_rows(G8, pf.rows, P8)
    assert torch.equal(_rows_of(G8, pf.rows), P8.cpu())
    Qd = _dev(pf.P)
    F = Qd.shape[0]
    need = lib.fr_gallery_match_f8_workspace(F, lr.N8)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    for off in (0, lr.OFFSET):
        idx, score = _outputs(F)
        lib.fr_gallery_match_f8(_lib.ptr(Qd), _lib.ptr(G8), None, F, lr.N8, 512, off, _lib.ptr(idx), _lib.ptr(score), _lib.ptr(ws),
                                need, None, 0, _lib.stream_ptr())
        want = lr.expect_coarse_f8(pf.S, pf.rows, off)
        assert _same((idx, score), want), (off, idx.tolist(), want[0].tolist(), score.tolist())
    del G8, ws
    _release()


# ---------------------------------------------------------------- 2. writes and views at high slots
@pytest.mark.parametrize("scan", ["f32", "f16", "f8"])
def test_writes_and_views_around_slot_2_22(scan, lib):
    """A DeviceGallery of N slots whose first upsert lands on slots 2^22 - 150 .. 2^22 + 149: fr_gallery_update_rows_f32 / _shadow and
    fr_gallery_gmax_update at high slots, then a shuffled view of those ids and 700 zero slots from both sides through every view
    entry.  Ids as the literal loop of the oracle (tests/test_gpu_gallery_sync.py::check), top-K and grouped results with the bits of
    the exact scan (tests/helpers/scan_ref.py)."""
    from facerecognition_infrenceengine_amd.gallery import DeviceGallery, last_topk
    from tests.test_gpu_gallery_sync import check
    vc = lr.view_case()
    per = 2048 + {"f32": 0, "f16": 1024, "f8": 512}[scan]
    _need(lr.N * per + GIB, f"a {scan} gallery of {lr.N} slots")
    g = DeviceGallery("cuda:0", capacity=lr.N, scan=scan)
    g._next = lr.FIRST_SLOT
    g.upsert(vc.ids[:lr.NIDS], vc.rows)
    slots = np.array([g.slot_of[i] for i in range(lr.NIDS)])
    assert np.array_equal(slots, lr.FIRST_SLOT + np.arange(lr.NIDS)) and g.capacity == lr.N
    lo, hi = int(slots[0]), int(slots[-1]) + 1
    assert torch.equal(_bits(g.G[lo:hi]).cpu(), torch.from_numpy(vc.rows.view(np.int32)))
    if scan != "f32":
        assert g.S.shape == (lr.N, 512) and torch.equal(_raw(g.S[lo:hi]), _raw(_convert(lib, _dev(vc.rows), scan)))
    for d in (1 << 20, 1 << 21, 1 << 22):                                  # where a slot * 512 that wrapped would have written
        a, b = max(lo - d, 0), hi - d
        assert int(torch.count_nonzero(g.G[a:b])) == 0
        assert scan == "f32" or int(torch.count_nonzero(_raw(g.S[a:b]))) == 0
    if scan == "f16":
        want = float(np.linalg.norm(vc.rows.astype(np.float64), axis=1).max())
        assert abs(float(g.gmax) - want) <= 8 * 2.0 ** -24 * (1 + 1e-6) * want
    for k, s in enumerate(vc.zslots):                                      # never-written slots, named so that a view can list them
        g.slot_of[("z", k)] = int(s)
    view = g.view(vc.idsA)
    assert len(view) == 1000 and int(view.slots.max()) == lr.N - 1 and int(view.slots.min()) == 0
    Qd = _dev(vc.Qraw)
    # top-1 through the view: the oracle's loop over the rows in view order
    check(view, dict(zip(vc.idsA, vc.V)), vc.Qraw)
    idx, score = view.match_device(Qd)
    wi, ws = sr.match_ref(vc.S)
    assert np.array_equal(idx.cpu().numpy(), wi)
    if scan == "f32":
        assert _same((idx, score), (wi, ws))
    # top-16: the exact scan, and once the certified coarse pass through the slot list
    for coarse in ((False, True) if scan == "f16" else (False,)):
        g.coarse_topk_min_rows = 1000 if coarse else 1 << 30
        got = view.match_topk_device(Qd, 16)
        assert last_topk()["path"] == ("coarse" if coarse else "exact")
        assert _same(got, sr.topk_ref(vc.S, 16)), (scan, coarse)
    # the audit: the two planted pairs, the bits of the first-hit dot
    dup = view.find_duplicates(thr=lr.THR)
    assert np.array_equal(dup.pairs, vc.pairs), dup.pairs
    assert np.array_equal(dup.scores.view(np.int32), vc.pair_scores.view(np.int32))
    # two views in one grouped scan
    viewB = g.view(vc.idsB)
    vs = g.view_set([view, viewB])
    view_of = [(f // 3) % 2 for f in range(lr.NQ)]
    SB = np.ascontiguousarray(vc.S[:, vc.posB])
    w1 = [sr.match_ref(vc.S), sr.match_ref(SB)]
    w16 = [sr.topk_ref(vc.S, 16), sr.topk_ref(SB, 16)]
    inA = np.array(view_of) == 0

    def per_view(a, b):
        sel = inA.reshape((-1,) + (1,) * (a[0].ndim - 1))
        return np.where(sel, a[0], b[0]), np.where(sel, a[1], b[1])

    assert _same(vs.match_device(Qd, view_of), per_view(*w1))
    assert _same(vs.match_topk_device(Qd, view_of, 16), per_view(*w16))
    del g, view, viewB, vs
    _release()


# ---------------------------------------------------------------- 3. frame stacks past 2^31 bytes
FH, FW, NF = 2160, 3840, 88                                                # 88 x 24.9 MB: the last frame starts past byte 2^31
LIVE = (0, 86, 87)                                                         # the frames that carry content; the others are zero


@pytest.fixture(scope="module")
def stack():
    """big: u8 [88][2160][3840][3], zero but for synth_frame content in frames 0, 86 and 87; small: those three alone; host: the
    content.  No test writes to either."""
    import os
    import sys
    from types import SimpleNamespace
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import synth_frame
    assert 86 * FH * FW * 3 < 2 ** 31 < 87 * FH * FW * 3 and FH * FW * 3 < 2 ** 31
    _need(2 * NF * FH * FW * 3 + GIB, "the frame stack and a copy of it")
    host = [synth_frame(FH, FW, 900 + f) for f in LIVE]
    big = torch.zeros((NF, FH, FW, 3), dtype=torch.uint8, device="cuda")
    for f, fr in zip(LIVE, host):
        big[f].copy_(torch.from_numpy(fr))
    small = torch.stack([big[f] for f in LIVE])
    yield SimpleNamespace(big=big, small=small, host=host)
    del big, small
    _release()


def test_warps_read_the_frames_past_2_31_bytes(stack, lib):
    """fr_warp_affine_5pt and fr_warp_affine_5pt_slots, three edge faces per live frame (one larger than the frame, one over the
    bottom-right corner: on frame 87 the pulled-back 8-byte load at the end of the buffer, one over the top-left corner):
    the bits of the same call on the three live frames alone, and oracle.align.norm_crop within the bars of
    test_warp_affine_5pt_edges_vs_oracle / test_warp_affine_5pt_slots_edges_vs_oracle"""
    from facerecognition_infrenceengine_amd import _lib
    from oracle import align as oalign
    from tests.test_gpu_detect_kernels import _decode_f16, _u8_bar
    from tests.test_gpu_letterbox import _corner_kps
    per = 3
    kps = np.concatenate([_corner_kps(FH, FW)] * len(LIVE))
    F = len(kps)
    dk = _dev(kps)

    def warp(frames, fidx):
        out = torch.full((F, 112, 112, 8), float("nan"), dtype=torch.float16, device="cuda")
        u8 = torch.full((F, 112, 112, 3), 77, dtype=torch.uint8, device="cuda")
        M = torch.zeros((F, 2, 3), dtype=torch.float32, device="cuda")
        di = _dev(np.repeat(np.array(fidx, np.int32), per))
        lib.fr_warp_affine_5pt(_lib.ptr(frames), frames.shape[0], FH, FW, _lib.ptr(dk), _lib.ptr(di), None, F, 112, _lib.ptr(out),
                               _lib.ptr(u8), _lib.ptr(M), _lib.stream_ptr())
        return out, u8, M

    big, small = warp(stack.big, LIVE), warp(stack.small, range(len(LIVE)))
    assert torch.equal(big[0].view(torch.int16), small[0].view(torch.int16)) and torch.equal(big[1], small[1])
    assert torch.equal(_bits(big[2]), _bits(small[2]))
    got_u8, got_m = big[1].cpu().numpy(), big[2].cpu().numpy()
    dec = _decode_f16(big[0])
    for i in range(F):
        want, Mw = oalign.norm_crop(stack.host[i // per], kps[i])
        diff = np.abs(got_u8[i].astype(int) - want.astype(int))
        print(f"warp face {i}: max |diff| {diff.max()}, fraction differing {(diff > 0).mean():.2e}")
        np.testing.assert_allclose(got_m[i], Mw, rtol=1e-5, atol=1e-4, err_msg=str(i))
        assert _u8_bar(got_u8[i], want), i
        assert np.array_equal(dec[i], got_u8[i]) and got_u8[i].any(), i
    # the slot form: cap 4, three faces in the live frames, none elsewhere
    cap = 4

    def slots(frames, live):
        n = frames.shape[0]
        ks = np.full((n, cap, 5, 2), np.nan, np.float32)
        counts = np.zeros(n, np.int32)
        for j, f in enumerate(live):
            ks[f, :per] = kps[j * per:(j + 1) * per]
            counts[f] = per
        out = torch.full((n * cap, 112, 112, 8), float("nan"), dtype=torch.float16, device="cuda")
        dks, dc = _dev(ks), _dev(counts)
        lib.fr_warp_affine_5pt_slots(_lib.ptr(frames), n, FH, FW, _lib.ptr(dks), _lib.ptr(dc), cap, 112, _lib.ptr(out),
                                     _lib.stream_ptr())
        return out.reshape(n, cap, 112, 112, 8)

    sb, ss = slots(stack.big, LIVE), slots(stack.small, range(len(LIVE)))
    for j, f in enumerate(LIVE):
        assert torch.equal(sb[f].view(torch.int16), ss[j].view(torch.int16)), f
        assert torch.equal(sb[f, :per].view(torch.int16), big[0][j * per:(j + 1) * per].view(torch.int16)) and not bool(sb[f, per:].any())
    idle = [f for f in range(NF) if f not in LIVE]
    assert not bool(sb[idle].any())


def _crop_boxes():
    """four boxes per frame: inside, over the bottom-right corner (the last bytes of the frame), larger than the frame, over the
    top-left corner with fractional corners"""
    return np.array([[1200.0, 700.0, 1500.0, 1060.0], [FW - 90.0, FH - 120.0, FW + 25.0, FH + 18.0],
                     [-40.0, -30.0, FW + 50.0, FH + 35.0], [-20.5, -12.25, 61.75, 86.5]], np.float32)


@pytest.fixture(scope="module")
def ro_layers():
    from facerecognition_infrenceengine_amd import weights
    from tests.helpers import detect_ref as dref
    _, r, o = weights.synth_mtcnn_states(seed=5)
    return {**dref.rnet_layers(r), **dref.onet_layers(o)}


def _slot_args(n, live):
    cap = 4
    boxes = np.full((n, cap, 4), np.nan, np.float32)
    counts = np.zeros(n, np.int32)
    for f in live:
        boxes[f], counts[f] = _crop_boxes(), cap
    return _dev(boxes), _dev(counts), cap


def test_crops_read_the_frames_past_2_31_bytes(stack, lib, ro_layers):
    """fr_crop_resize_norm, fr_crop_conv1_f32, fr_crop_conv1_split (both modes) and fr_crop_conv1_list_f32 on boxes in frames 86 and 87:
    the bits of the same call on the live frames alone; the crops equal oracle.detect.crop_resize bit for bit, the conv1 maps lie
    within C_F32 * A of the float64 layer (tests/test_gpu_detect_precision.py), the split maps are what that module states, the
    list form gives the slot form's rows (tests/test_gpu_detect_kernels.py)."""
    from facerecognition_infrenceengine_amd import _lib
    from oracle import detect as odetect
    from tests.helpers import detect_ref as dref
    from tests.test_gpu_detect_precision import C_F32, _decode
    s = _lib.stream_ptr()
    runs = {}
    for name, frames, live in (("big", stack.big, LIVE), ("small", stack.small, range(len(LIVE)))):
        n = frames.shape[0]
        boxes, counts, cap = _slot_args(n, live)
        r = runs[name] = {}
        for nt, size, P, c in ((0, 24, 11, 28), (1, 48, 23, 32)):
            L = ro_layers[10 if nt == 0 else 20]
            wk = L.w.float().permute(2, 3, 1, 0).reshape(27, c).contiguous().cuda()
            b, sl = L.b.float().cuda(), L.slope.float().cuda()
            crops = torch.full((n * cap, size, size, 4), float("nan"), device="cuda")
            lib.fr_crop_resize_norm(_lib.ptr(frames), n, FH, FW, _lib.ptr(boxes), _lib.ptr(counts), cap, size, _lib.ptr(crops), s)
            f32 = torch.full((n * cap, P, P, c), float("nan"), device="cuda")
            lib.fr_crop_conv1_f32(nt, _lib.ptr(frames), n, FH, FW, _lib.ptr(boxes), _lib.ptr(counts), cap, _lib.ptr(wk), _lib.ptr(b),
                                  _lib.ptr(sl), _lib.ptr(f32), s)
            maps = []
            for mode in (0, 1):
                m = torch.full((n * cap, P * P, 128), 0x7f, dtype=torch.uint8, device="cuda")
                lib.fr_crop_conv1_split(nt, _lib.ptr(frames), n, FH, FW, _lib.ptr(boxes), _lib.ptr(counts), cap, _lib.ptr(wk),
                                        _lib.ptr(b), _lib.ptr(sl), _lib.ptr(m), mode, s)
                maps.append(m)
            lst_h = np.array([f * cap + j for f in reversed(list(live)) for j in (3, 1, 0, 2)], np.int32)
            lst, lc = _dev(lst_h), _dev(np.array([len(lst_h)], np.int32))
            y = torch.full((len(lst_h), P, P, c), float("nan"), device="cuda")
            lib.fr_crop_conv1_list_f32(nt, _lib.ptr(frames), n, FH, FW, _lib.ptr(boxes), cap, _lib.ptr(lst), _lib.ptr(lc), len(lst_h),
                                       _lib.ptr(wk), _lib.ptr(b), _lib.ptr(sl), _lib.ptr(y), s)
            torch.cuda.synchronize()
            rows = torch.tensor([f * cap + j for f in live for j in range(cap)], device="cuda")
            assert torch.equal(_bits(y), _bits(f32[torch.from_numpy(lst_h).long().cuda()])), (name, nt)
            r[nt] = [t[rows] for t in (crops, f32, maps[0], maps[1])] + [y]
    bh = _crop_boxes()
    for nt, size, P, c in ((0, 24, 11, 28), (1, 48, 23, 32)):
        big, small = runs["big"][nt], runs["small"][nt]
        for a, b in zip(big, small):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), nt
        crops, f32, m0, m1, _ = big
        o = crops.cpu()
        for j, f in enumerate(LIVE):
            rgb = stack.host[j][:, :, ::-1].astype(np.float32)
            for k in range(4):
                want = odetect._to_net(odetect.crop_resize(rgb, np.trunc(bh[k]), size))[0].permute(1, 2, 0).contiguous()
                assert torch.equal(o[j * 4 + k, ..., :3].contiguous().view(torch.int32), want.view(torch.int32)), (nt, f, k)
                assert float(o[j * 4 + k, ..., 3].abs().max()) == 0.0
        L = ro_layers[10 if nt == 0 else 20]
        xin = crops.permute(0, 3, 1, 2).double().cpu()[:, :3]
        want, A = dref.apply(L, xin, C_F32)
        got = f32.permute(0, 3, 1, 2).double().cpu()
        ratio = dref.ratio(got, want, A)
        print(f"crop_conv1_f32 net {nt} on frames 0 / 86 / 87: worst err/A {ratio:.3e}")
        assert bool(torch.isfinite(got).all()) and ratio <= C_F32
        hl0 = m0.view(torch.float16).reshape(-1, P, P, 64)
        assert torch.equal(hl0[..., :c], f32.half()) and torch.equal(hl0[..., 32:32 + c], (f32 - f32.half().float()).half()), nt
        dec, hl1 = _decode(m1.reshape(-1, P, P, 128), c)
        S, A = dref.apply(L, xin, C_F32, split=True)
        ratio = dref.ratio(dec.permute(0, 3, 1, 2).double().cpu(), S, A + (2.0 ** -21 * S.abs() + 2.0 ** -24) / C_F32)
        print(f"crop_conv1_split 1 net {nt} on frames 0 / 86 / 87: worst err/A {ratio:.3e}")
        assert ratio <= C_F32


def test_hud_draws_into_the_frames_past_2_31_bytes(stack, lib):
    """fr_hud_draw_u8 on a copy of the stack, two faces in each live frame, one of them over the bottom-right corner: the bits of
    the same call on the live frames alone; inside a window at that corner hud_ref of the window (every clamp of the layout is
    against the right and bottom edges, which the window shares: asserted), outside it the frame as it was; every other frame zero"""
    from facerecognition_infrenceengine_amd import _lib
    from facerecognition_infrenceengine_amd.hud_font import FONT
    from tests.helpers import hud_cases, hud_ref
    wh, ww = 420, 640
    oy, ox = FH - wh, FW - ww
    made = [[hud_cases.face((FW - 300, FH - 330, FW - 150, FH - 190), (0, 255, 0), 40, 90, (b"Name: A", b"Score: 0.71")),
             hud_cases.face((FW - 130, FH - 160, FW + 30, FH + 20), (0, 0, 255), 10, 0, (b"Unknown Person",))] for _ in LIVE]

    def records(n, live):
        per = [[] for _ in range(n)]
        for f, m in zip(live, made):
            per[f] = m
        return hud_cases.pack(per, cap=2, seed=3)

    def draw(frames, live):
        n = frames.shape[0]
        cnt, faces, text = records(n, live)
        c, fa, t, fn = (_dev(a) for a in (cnt, faces, text, np.array(FONT)))
        lib.fr_hud_draw_u8(_lib.ptr(frames), n, FH, FW, _lib.ptr(c), 2, _lib.ptr(fa), _lib.ptr(t), text.shape[3], _lib.ptr(fn), 1,
                           _lib.stream_ptr())
        torch.cuda.synchronize()
        return frames

    big, small = draw(stack.big.clone(), LIVE), draw(stack.small.clone(), range(len(LIVE)))
    idle = [f for f in range(NF) if f not in LIVE]
    assert not bool(big[idle].any())
    cnt, faces, text = records(len(LIVE), range(len(LIVE)))
    for j, f in enumerate(LIVE):
        assert torch.equal(big[f], small[j]), f
        win = faces[j].copy()
        win[:, [0, 2]] -= ox
        win[:, [1, 3]] -= oy
        for rec, wrec in zip(faces[j], win):                               # the window sees the layout the frame sees
            x1, y1, x2, y2, _, _, _, lens = hud_ref.normalise(rec, text.shape[3])
            px, py, pw, ph = hud_ref.panel_rect(x1, y1, x2, y2, lens, FH, FW, 1)
            wx1, wy1, wx2, wy2, _, _, _, _ = hud_ref.normalise(wrec, text.shape[3])
            assert hud_ref.panel_rect(wx1, wy1, wx2, wy2, lens, wh, ww, 1) == (px - ox, py - oy, pw, ph)
            assert min(x1, px) - 20 > ox and min(y1, py) - 20 > oy
        want = hud_ref.draw_records(stack.host[j][oy:, ox:], cnt[j], win, text[j], 1)
        got = big[f].cpu().numpy()
        assert np.array_equal(got[oy:, ox:], want) and not np.array_equal(want, stack.host[j][oy:, ox:])
        outside = np.ones((FH, FW), bool)
        outside[oy:, ox:] = False
        assert np.array_equal(got[outside], stack.host[j][outside])
    del big, small
    _release()


def test_activity_judges_the_frames_past_2_31_bytes(stack, lib):
    """fr_frame_activity_u8 over all 88 frames, twice (the second time frame 87 has a patch inverted): cell means, verdicts and state
    of the live frames against activity_ref and against the same calls on the live frames alone; the zero frames read as zero"""
    from facerecognition_infrenceengine_amd import _lib
    from tests.helpers import activity_ref as ar
    C = (FH // 16) * (FW // 16)
    rule = (4, 2, 0)

    class State:
        def __init__(self, S, N):
            self.grid = torch.zeros((S, C), dtype=torch.uint8, device="cuda")
            self.geom = torch.zeros((S, 2), dtype=torch.int32, device="cuda")
            self.idle = torch.zeros(S, dtype=torch.int32, device="cuda")
            self.cur = torch.full((N, C), 0xA5, dtype=torch.uint8, device="cuda")
            self.changed = torch.full((N,), -77, dtype=torch.int32, device="cuda")
            self.active = torch.full((N,), -77, dtype=torch.int32, device="cuda")
            self.slot = torch.arange(N, dtype=torch.int32, device="cuda").flip(0).contiguous()      # frame n -> slot N - 1 - n

        def run(self, frames):
            n = frames.shape[0]
            lib.fr_frame_activity_u8(_lib.ptr(frames), n, FH, FW, _lib.ptr(self.slot), self.grid.shape[0], _lib.ptr(self.grid),
                                     _lib.ptr(self.geom), _lib.ptr(self.idle), C, _lib.ptr(self.cur), _lib.ptr(self.changed),
                                     _lib.ptr(self.active), *rule, _lib.stream_ptr())
            torch.cuda.synchronize()

    big, small, ref = State(NF, NF), State(len(LIVE), len(LIVE)), ar.GateRef(len(LIVE), C, *rule)
    patch = (slice(1000, 1100), slice(500, 900))
    host = [h.copy() for h in stack.host]
    idle = [f for f in range(NF) if f not in LIVE]
    for turn in range(2):
        if turn == 1:                                                      # invert a patch of frame 87, and put it back below
            stack.big[87][patch].bitwise_not_()
            stack.small[2][patch].bitwise_not_()
            host[2][patch] = ~host[2][patch]
        try:
            big.run(stack.big)
            small.run(stack.small)
        finally:
            if turn == 1:
                stack.big[87][patch].bitwise_not_()
                stack.small[2][patch].bitwise_not_()
        changed, active, cur = ref.judge(host, [2, 1, 0])
        assert changed.tolist() == ([-1, -1, -1] if turn == 0 else [0, 0, int(changed[2])]) and (turn == 0 or changed[2] >= 2)
        for j, f in enumerate(LIVE):
            assert np.array_equal(big.cur[f].cpu().numpy(), cur[j]) and torch.equal(big.cur[f], small.cur[j]), (turn, f)
            assert int(big.changed[f]) == changed[j] == int(small.changed[j]) and int(big.active[f]) == active[j] == int(small.active[j])
            s = NF - 1 - f
            assert np.array_equal(big.grid[s].cpu().numpy(), ref.grid[2 - j]) and torch.equal(big.grid[s], small.grid[2 - j])
            assert big.geom[s].tolist() == [FH, FW] and int(big.idle[s]) == ref.idle[2 - j] == int(small.idle[2 - j])
        assert not bool(big.cur[idle].any()) and not bool(big.grid[[NF - 1 - f for f in idle]].any())
        assert (big.changed[idle] == (-1 if turn == 0 else 0)).all() and (big.active[idle] == (1 if turn == 0 else 0)).all()
        assert (big.idle[[NF - 1 - f for f in idle]] == turn).all()
    assert torch.equal(stack.big[87].cpu(), torch.from_numpy(stack.host[2]))


def test_yuv_conversion_writes_bgr_frames_past_2_31_bytes(lib):
    """fr_yuv420_to_bgr_u8, 88 NV12 frames in (1.1 GB), 88 BGR frames out (2.19 GB): frames 0, 86 and 87 hold random bytes and must
    equal yuv_ref and the same call on those three alone; the zero frames between them give yuv_ref's pixel for (0, 0, 0)"""
    from facerecognition_infrenceengine_amd import _lib, colour
    from tests.helpers import yuv_ref
    per = FH * FW * 3 // 2
    _need(NF * per * 3 + GIB, "the NV12 stack and its BGR stack")
    g = torch.Generator(device="cuda").manual_seed(73)
    src = torch.zeros((NF, FH * 3 // 2, FW), dtype=torch.uint8, device="cuda")
    for f in LIVE:
        src[f].random_(0, 256, generator=g)
    small_src = torch.stack([src[f] for f in LIVE])

    def convert(s):
        n = s.shape[0]
        dst = torch.full((n, FH, FW, 3), 0xA5, dtype=torch.uint8, device="cuda")
        lib.fr_yuv420_to_bgr_u8(_lib.ptr(s), _lib.ptr(dst), n, FH, FW, colour.LAYOUTS["nv12"], *colour.MATRICES["bt601"], _lib.stream_ptr())
        return dst

    big, small = convert(src), convert(small_src)
    for j, f in enumerate(LIVE):
        assert torch.equal(big[f], small[j]), f
        if f:                                                              # frames 86 and 87 against the definition
            want = yuv_ref.yuv420_to_bgr(src[f].cpu().numpy(), "nv12", "bt601")
            assert np.array_equal(big[f].cpu().numpy(), want), f
    zero = torch.tensor([int(v) for v in yuv_ref.convert_triples(0, 0, 0, "bt601")], dtype=torch.uint8, device="cuda")
    idle = [f for f in range(NF) if f not in LIVE]
    assert bool((big[idle] == zero).all())
    del src, small_src, big, small
    _release()


def test_letterbox_writes_canvases_past_2_31_bytes(lib):
    """fr_letterbox_u8, 1750 table entries that all name one 33 x 47 frame, canvases of 640 x 640 (2.15 GB): canvases 0, 1748 and 1749
    equal letterbox_ref.canvas_ref within the canvas bar of tests/test_gpu_letterbox.py, and every canvas equals canvas 0"""
    import os
    import sys
    from facerecognition_infrenceengine_amd import _lib
    from facerecognition_infrenceengine_amd.letterbox import frame_table, letterbox_geometry
    from tests.helpers import letterbox_ref
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import synth_frame
    n, det = 1750, (640, 640)
    assert (n - 1) * 640 * 640 * 3 > 2 ** 31
    _need(n * 640 * 640 * 3 + GIB, "the canvases")
    frame = synth_frame(33, 47, 305)
    fd = _dev(frame)
    tab, _ = frame_table([fd.data_ptr()] * n, [(33, 47)] * n, det)
    table = _dev(tab)
    canvas = torch.full((n, 640, 640, 3), 0xA5, dtype=torch.uint8, device="cuda")
    lib.fr_letterbox_u8(_lib.ptr(table), n, _lib.ptr(canvas), 640, 640, _lib.stream_ptr())
    want, _ = letterbox_ref.canvas_ref(frame, det)
    nh, nw, _ = letterbox_geometry(33, 47, det)
    for i in (0, n - 2, n - 1):
        got = canvas[i].cpu().numpy()
        assert not got[nh:].any() and not got[:, nw:].any()
        d = np.abs(got.astype(np.int16) - want.astype(np.int16))
        assert d.max() <= 1 and int((d.max(axis=2) > 0).sum()) < 1e-3 * nh * nw, i
    assert bool((canvas == canvas[0]).all())
    del canvas
    _release()


# ---------------------------------------------------------------- 4. the two range clamps
def test_scan_plan_clamps_a_range_to_2_20_rows(lib):
    """fr_gallery_match_f16 with G32 == NULL, 8192 queries over 2^23 + 4173 f16 rows: the plan wants 8 ranges of more than 2^20 rows,
    `if (tpr > max_tpr)` of scan_plan cuts them to 2^20 (the workspace size shows 9); planted rows on both sides of every range
    edge come back with their exact coarse scores"""
    from facerecognition_infrenceengine_amd import _lib
    _need(lr.N16 * 1024 + 2 * GIB, "the f16 slab")
    p = lr.plant_f16()
    G16 = torch.empty((lr.N16, 512), dtype=torch.float16, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(74)
    for a in range(0, lr.N16, 1 << 20):
        G16[a:a + (1 << 20)].uniform_(-lr.AMP, lr.AMP, generator=g)
    lo, hi = torch.aminmax(G16[8:1 << 19])
    assert -lr.AMP <= float(lo) and float(hi) <= lr.AMP
    _put_rows(G16, p.rows, _dev(p.P).half())
    F = lr.F16Q
    Qd = _dev(p.P[np.arange(F) % len(p.rows)])
    need = lib.fr_gallery_match_f16_workspace(F, lr.N16)
    per = F * 4 * 4 * 8                                                    # coarse_ref.check_plan: F * nranges * 4 * FR_TOPK * 8 + 256
    assert (need - 256) % per == 0
    nranges = (need - 256) // per
    assert nranges == -(-lr.N16 // lr.CLAMP_ROWS) == 9 > 8
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    for off in (0, lr.OFFSET):
        idx, score = _outputs(F)
        lib.fr_gallery_match_f16(_lib.ptr(Qd), _lib.ptr(G16), None, F, lr.N16, 512, off, _lib.ptr(idx), _lib.ptr(score), _lib.ptr(ws),
                                 need, None, 0, _lib.stream_ptr())
        want = lr.expect_coarse_f16(p.S, p.rows, F, off)
        assert _same((idx, score), want), (off, idx[:20].tolist(), want[0][:20].tolist())
    del G16, ws
    _release()


def test_pair_plan_clamps_a_range_to_2_20_rows(lib):
    """find_duplicates_device(max_ranges=1) over 2^20 + 4173 rows: `if (tpr > PS_MAX_TPR)` of pair_plan outranks max_ranges (two
    ranges are used); the five planted pairs across row 2^20 are found with the bits of the first-hit dot"""
    from facerecognition_infrenceengine_amd.gallery import GalleryMatcher
    pp = lr.plant_pairs()
    _need(lr.NP * 3072 + 2 * GIB, "the rows and the audit's workspace")
    G = torch.empty((lr.NP, 512), dtype=torch.float32, device="cuda")
    _fill_background(G, 75)
    _put_rows(G, pp.rows, _dev(pp.P))
    m = GalleryMatcher("cuda:0")
    m.G, m.ids = G, range(lr.NP)
    keys, scores, counts = m.find_duplicates_device(thr=lr.THR, max_pairs=1 << 12, max_ranges=1)
    seen, found, flags, ranges = counts.tolist()
    assert (found, flags, ranges) == (5, 0, 2) and seen >= 5, counts.tolist()
    k, s = keys[:found].cpu().numpy(), scores[:found].cpu().numpy()
    order = np.argsort(k)
    assert np.array_equal(np.stack([k[order] >> 32, k[order] & 0xFFFFFFFF], 1), pp.pairs)
    assert np.array_equal(s[order].view(np.int32), pp.scores.view(np.int32))
    del G, m, keys, scores
    _release()
