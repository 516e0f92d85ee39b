"""GPU kernel-level tests of the detector's glue and exact pass, and of the alignment, at their edges.

Every reference is written from the oracle (oracle/detect.py, oracle/align.py), never from the .hip sources.  The detector
kernels are built with -ffp-contract=off and mirror the oracle operation for operation, so their results are compared with
np.array_equal; the two exceptions say why beside the assert (the device's expf against numpy's exp; u8 rounding ties at .5)."""
import math
import os
import sys
import threading

import numpy as np
import pytest
import torch

from oracle import align as oalign
from oracle import detect as odetect

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

F32 = np.float32


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


@pytest.fixture(scope="module")
def det():
    from facerecognition_infrenceengine_amd import weights
    from facerecognition_infrenceengine_amd.mtcnn import MTCNNHIP
    return MTCNNHIP(*weights.synth_mtcnn_states(seed=91), device="cuda:0")


# ---------------------------------------------------------------------------------------------------- 1. exact-pass work list
def _margin_heads(rng, nslots, nhead, thr, margin):
    """random heads whose logit differences cluster around thr: about half of them lie within the margin"""
    h = rng.standard_normal((nslots, nhead)).astype(F32)
    h[:, 1] = (h[:, 0] + (thr + rng.uniform(-2, 2, nslots).astype(F32) * margin)).astype(F32)
    return h


def _edge_d(thr, margin, sign):
    """an f32 logit difference d with |d - thr| == margin in f32 arithmetic (the `<=` edge), and the next f32 d outward"""
    d = F32(thr + F32(sign) * margin)
    out = np.nextafter(d, F32(sign * np.inf), dtype=F32)
    assert abs(F32(d - thr)) == margin and abs(F32(out - thr)) > margin
    return d, out


@pytest.mark.parametrize("nhead", [6, 16])
def test_ro_margin_list_vs_numpy(lib, nhead):
    """fr_ro_margin_list over 3 frames x 300 slots (900: not a multiple of 256), counts {300, 0, 171}: the listed set is the
    numpy set of valid slots with |d - thr| <= margin (f32) or any head not finite (NaN, +inf, -inf: the exact pass decides),
    including planted rows exactly on the margin; qualifying heads past
    a frame's count never appear; with a list capacity below the number of qualifying slots the counter still counts them all
    and the list holds list_cap distinct members of the set, nothing past list_cap is written."""
    from facerecognition_infrenceengine_amd import _lib
    rng = np.random.default_rng(nhead)
    nfr, cap = 3, 300
    counts = np.array([300, 0, 171], np.int32)
    # margin ~1e-3 on the grid of thr's ulp (2^-24 in [0.5, 1)): thr +- margin is then an f32, the edge can be planted exactly
    thr, margin = F32(math.log(0.7 / 0.3)), F32(round(1e-3 * 2 ** 24) / 2 ** 24)
    h = _margin_heads(rng, nfr * cap, nhead, thr, margin)
    on_hi, out_hi = _edge_d(thr, margin, +1)
    on_lo, out_lo = _edge_d(thr, margin, -1)
    planted = {3: on_hi, 4: on_lo, 5: out_hi, 6: out_lo, 2 * cap + 170: on_hi, 2 * cap + 169: out_lo}
    for s, d in planted.items():
        h[s, 0] = 0.0
        h[s, 1] = d
    valid = (np.arange(cap)[None, :] < counts[:, None]).reshape(-1)
    h[~valid, 0] = 0.0
    h[~valid, 1] = thr                                           # would qualify, but lie past their frame's count
    # non-finite split heads (an f16 operand overflowed): d = NaN, +inf, -inf must go to the exact pass on valid slots, never
    # past the counts
    nonfinite = {7: (0.0, np.nan), 8: (0.0, np.inf), 9: (np.inf, 0.0), 10: (np.inf, np.inf), 2 * cap + 168: (np.nan, 0.0),
                 cap + 5: (0.0, np.nan), 2 * cap + 200: (0.0, np.inf), 2 * cap + 201: (np.inf, 0.0)}
    for s, (a0, a1) in nonfinite.items():
        h[s, 0], h[s, 1] = a0, a1
    # a finite logit difference far from the threshold, but a regression / landmark head that is not: the exact pass too
    h[11, 0], h[11, 1], h[11, nhead - 1] = 0.0, thr + 5.0, np.nan
    h[12, 0], h[12, 1], h[12, 2] = 0.0, thr - 5.0, -np.inf
    h[2 * cap + 202, 0], h[2 * cap + 202, 1], h[2 * cap + 202, 3] = 0.0, thr + 5.0, np.nan      # past the count: not
    with np.errstate(invalid="ignore"):
        d = (h[:, 1] - h[:, 0]).astype(F32)
        want = set(np.nonzero(valid & (~np.isfinite(h).all(1) | (np.abs((d - thr).astype(F32)) <= margin)))[0].tolist())
    assert {3, 4, 2 * cap + 170, 7, 8, 9, 10, 11, 12, 2 * cap + 168} <= want
    assert not ({5, 6, 2 * cap + 169, cap + 5, 2 * cap + 200, 2 * cap + 201, 2 * cap + 202} & want)
    assert 200 < len(want) < valid.sum()
    hd, cd = _dev(h), _dev(counts)
    for list_cap in (len(want) + 37, len(want), 64):
        lst = torch.full((list_cap + 64,), -7, dtype=torch.int32, device="cuda")
        lc = torch.zeros(1, dtype=torch.int32, device="cuda")
        lib.fr_ro_margin_list(_lib.ptr(hd), nhead, _lib.ptr(cd), nfr, cap, float(thr), float(margin), _lib.ptr(lst), _lib.ptr(lc),
                              list_cap, _lib.stream_ptr())
        torch.cuda.synchronize()
        got = lst.cpu().numpy()
        assert int(lc[0]) == len(want), list_cap
        n = min(len(want), list_cap)
        assert len(set(got[:n].tolist())) == n and set(got[:n].tolist()) <= want
        if list_cap >= len(want):
            assert set(got[:n].tolist()) == want
        assert (got[n:] == -7).all()                              # nothing written past the count / the capacity


@pytest.mark.parametrize("ncols", [6, 16])
def test_ro_scatter_rows_vs_numpy(lib, ncols):
    """fr_ro_scatter_rows: row i < min(count, list_cap) of src lands in dst[list[i]]; every other dst row keeps its sentinel,
    with the counter below the capacity, equal to it and above it (an overflowed list)."""
    from facerecognition_infrenceengine_amd import _lib
    rng = np.random.default_rng(ncols)
    nslots, list_cap = 900, 97
    lst = rng.permutation(nslots)[:list_cap].astype(np.int32)
    src = rng.standard_normal((list_cap, ncols)).astype(F32)
    for count in (0, 41, list_cap, list_cap + 300):
        dst = torch.full((nslots, ncols), -3.5, dtype=torch.float32, device="cuda")
        lib.fr_ro_scatter_rows(_lib.ptr(_sd := _dev(src)), _lib.ptr(_ld := _dev(lst)), _lib.ptr(_cd := _i32([count])), list_cap, ncols,
                               _lib.ptr(dst), _lib.stream_ptr())
        torch.cuda.synchronize()
        want = np.full((nslots, ncols), -3.5, F32)
        n = min(count, list_cap)
        want[lst[:n]] = src[:n]
        assert np.array_equal(dst.cpu().numpy(), want), count


def test_crop_conv1_list_equals_slot_form(det):
    """fr_crop_conv1_list_f32: row i equals, bit for bit, fr_crop_conv1_f32's row of slot list[i] (that entry is pinned to the
    crop + layer by test_crop_conv1_equals_crop_then_layer), for boxes sticking out of every side, larger than the frame, one
    pixel wide, and covering the last frame's bottom-right corner (the 8-byte loads pulled back at the buffer's end); rows past
    the counter stay unwritten, a counter above list_cap computes list_cap rows."""
    from facerecognition_infrenceengine_amd import _lib
    lib = det.lib
    N, H, W, cap = 3, 97, 131, 40
    g = torch.Generator(device="cuda").manual_seed(23)
    frames = torch.randint(0, 256, (N, H, W, 3), generator=g, device="cuda", dtype=torch.uint8)
    x1 = torch.rand((N, cap), generator=g, device="cuda") * (W + 40) - 30
    y1 = torch.rand((N, cap), generator=g, device="cuda") * (H + 40) - 30
    sz = torch.rand((N, cap), generator=g, device="cuda") * 70 + 1
    boxes = torch.stack([x1, y1, x1 + sz, y1 + sz * 1.3], -1).contiguous()
    boxes[2, 0] = torch.tensor([W - 3.0, H - 3.0, W + 10.0, H + 9.0])     # last frame, bottom-right corner
    boxes[2, 1] = torch.tensor([W - 20.0, H - 20.0, W + 0.0, H + 0.0])    # ends on the last pixel of the last frame
    boxes[0, 2] = torch.tensor([-20.0, -20.0, W + 20.0, H + 20.0])        # larger than the frame
    boxes[1, 3] = torch.tensor([7.0, 5.0, 7.0, 60.0])                     # one pixel wide
    boxes[0, 4] = torch.tensor([-50.0, 10.0, -5.0, 40.0])                 # entirely left of the frame
    counts = _i32([cap, cap, cap])
    lst_h = np.array([2 * cap + 0, 2 * cap + 1, 2, cap + 3, 4] + list(np.random.default_rng(3).permutation(N * cap)[:40]), np.int32)
    lst = _dev(lst_h)
    d = det
    d._s = _lib.stream_ptr()
    for net, (p, c) in ((0, (11, 28)), (1, (23, 32))):
        full = d.crop_conv1(net, frames, boxes, counts, cap)
        w, b, s = d._rc1 if net == 0 else d._oc1
        for list_cap, count in ((len(lst_h), 31), (len(lst_h), len(lst_h)), (20, len(lst_h))):
            y = torch.full((list_cap, p, p, c), float("nan"), dtype=torch.float32, device="cuda")
            lc = _i32([count])
            lib.fr_crop_conv1_list_f32(net, _lib.ptr(frames), N, H, W, _lib.ptr(boxes), cap, _lib.ptr(lst), _lib.ptr(lc), list_cap,
                                       _lib.ptr(w), _lib.ptr(b), _lib.ptr(s), _lib.ptr(y), _lib.stream_ptr())
            torch.cuda.synchronize()
            n = min(count, list_cap)
            want = full[torch.from_numpy(lst_h[:n]).long().cuda()]
            assert torch.equal(y[:n].view(torch.int32), want.view(torch.int32)), (net, list_cap, count)
            assert bool(torch.isnan(y[n:]).all()), (net, list_cap, count)


# -------------------------------------------------------------------------------------- 2. overflow of the exact lists
def _eight_360p():
    from make_golden import synth_frame
    frs = np.ascontiguousarray(np.stack([synth_frame(360, 640, 40 + i) for i in range(8)]))
    frs[5] = 0
    return torch.from_numpy(frs).cuda()


def _split_detector():
    from facerecognition_infrenceengine_amd import weights
    from facerecognition_infrenceengine_amd.mtcnn import MTCNNHIP
    return MTCNNHIP(*weights.synth_mtcnn_states(), device="cuda:0", batch_min_pixels=0)


def test_forced_exact_list_overflow_is_reported_and_names_the_net():
    """The split R-/O-Net cascade of test_split_ro_cascade_vs_f32_cascade_and_exact_pass with every crop sent to the exact pass
    (ro_margin 1e9) and work lists too small for them: MTCNNHIP.exact_list_overflow() names exactly the net whose list overflowed,
    exact_lists() gives both lists' full counts and capacities; lists that fit report nothing.  bench.py's _ro_lists still holds the
    same counters."""
    x = _eight_360p()
    det = _split_detector()
    det.detect_batch(x)
    fit = det.exact_lists()
    assert [e["net"] for e in fit] == ["rnet", "onet"] and det.exact_list_overflow() == []
    assert all(0 <= e["count"] <= e["cap"] for e in fit) and [e["cap"] for e in fit] == list(det.ro_list_cap)
    det.ro_margin = 1e9
    det.ro_list_cap = (8 * 512, 8 * 64)                               # every valid crop fits
    det.detect_batch(x)
    everyone = det.exact_lists()
    nr, no = everyone[0]["count"], everyone[1]["count"]
    assert det.exact_list_overflow() == [] and nr > 16 and no > 2, everyone
    det.ro_list_cap = (16, 8 * 64)
    det.detect_batch(x)
    assert det.exact_list_overflow() == ["rnet"]
    rec = det.exact_lists()
    assert rec[0] == {"net": "rnet", "count": nr, "cap": 16} and rec[1]["net"] == "onet" and rec[1]["count"] <= rec[1]["cap"], rec
    assert int(det._ro_lists[0][0]) == nr and int(det._ro_lists[1][0]) == rec[1]["count"]
    det.ro_list_cap = (8 * 512, 2)
    det.detect_batch(x)
    assert det.exact_list_overflow() == ["onet"]
    assert det.exact_lists() == [{"net": "rnet", "count": nr, "cap": 8 * 512}, {"net": "onet", "count": no, "cap": 2}]
    det.ro_list_cap = (16, 2)
    det.detect_batch(x)
    assert det.exact_list_overflow() == ["rnet", "onet"]


def test_exact_list_record_is_per_thread():
    """Two threads share one detector (wide margin, small lists) and run at the same time: one on frames whose lists overflow,
    the other on blank frames with no candidate at all.  Each thread's exact_lists() / exact_list_overflow() describe its own
    call only - the shared _ro_lists attribute would show whichever call finished last."""
    x = _eight_360p()
    blank = torch.zeros_like(x)
    det = _split_detector()
    det.ro_margin = 1e9
    det.ro_list_cap = (16, 2)
    det.detect_batch(x)
    want_busy = det.exact_lists()
    assert det.exact_list_overflow() == ["rnet", "onet"]
    det.detect_batch(blank)
    assert det.exact_lists() == [{"net": "rnet", "count": 0, "cap": 16}, {"net": "onet", "count": 0, "cap": 2}]
    torch.cuda.synchronize()
    rounds, errors = 4, []
    barrier = threading.Barrier(2)

    def work(frames, want, over):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for _ in range(rounds):
                    barrier.wait()
                    det.detect_batch(frames)
                    barrier.wait()                      # both calls issued before either thread reads its record
                    assert det.exact_lists() == want
                    assert det.exact_list_overflow() == over
        except BaseException as e:                      # noqa: BLE001 - re-raised in the main thread
            errors.append(e)
            barrier.abort()

    t = [threading.Thread(target=work, args=(x, want_busy, ["rnet", "onet"])),
         threading.Thread(target=work, args=(blank, [{"net": "rnet", "count": 0, "cap": 16}, {"net": "onet", "count": 0, "cap": 2}], []))]
    for th in t:
        th.start()
    for th in t:
        th.join(timeout=300)
    assert not any(th.is_alive() for th in t)
    if errors:
        raise errors[0]


# -------------------------------------------------------------------------------------------------- 3. box and stage glue
def _boxes(rng, n):
    """wide, tall, negative and 4K-scale boxes, and some that are empty after trunc"""
    kind = rng.integers(0, 5, n)
    x1 = rng.uniform(-60, 3800, n); y1 = rng.uniform(-60, 2100, n)
    w = np.where(kind == 0, rng.uniform(60, 900, n), rng.uniform(2, 120, n))           # wide
    h = np.where(kind == 1, rng.uniform(60, 900, n), rng.uniform(2, 120, n))           # tall
    x1 = np.where(kind == 2, -x1 / 20 - 5, x1)                                          # negative
    b = np.stack([x1, y1, x1 + w, y1 + h], 1)
    e = kind == 4                                                                       # trunc(x2) < trunc(x1)
    b[e, 2] = np.floor(b[e, 0]) - rng.uniform(0.05, 0.95, e.sum()) - rng.integers(0, 3, e.sum())
    return b.astype(F32)


def _stage1_reg(b, r):
    """oracle/detect.py stage 1: regression with w = x2 - x1 (no +1)"""
    rw = b[:, 2] - b[:, 0]; rh = b[:, 3] - b[:, 1]
    return np.stack([b[:, 0] + r[:, 0] * rw, b[:, 1] + r[:, 1] * rh,
                     b[:, 2] + r[:, 2] * rw, b[:, 3] + r[:, 3] * rh], 1).astype(F32)


@pytest.mark.parametrize("naux", [4, 14])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_box_refine_vs_oracle(lib, mode, naux):
    """fr_box_refine on 3 lists x 300 slots, counts {300, 0, 17}: mode 0 = the oracle's stage-1 regression + rerec, 1 = bbreg +
    rerec, 2 = bbreg; equal to the oracle's float32 arithmetic; slots past the count untouched."""
    from facerecognition_infrenceengine_amd import _lib
    rng = np.random.default_rng(10 * mode + naux)
    L, cap = 3, 300
    counts = np.array([300, 0, 17], np.int32)
    b = _boxes(rng, L * cap)
    aux = rng.uniform(-0.6, 0.6, (L * cap, naux)).astype(F32)
    bd = _dev(b)
    lib.fr_box_refine(_lib.ptr(bd), _lib.ptr(ad := _dev(aux)), naux, _lib.ptr(cd := _dev(counts)), L, cap, mode, _lib.stream_ptr())
    got = bd.cpu().numpy()
    r = aux[:, :4]
    want = {0: lambda: odetect.rerec(_stage1_reg(b, r)), 1: lambda: odetect.rerec(odetect.bbreg(b, r)),
            2: lambda: odetect.bbreg(b, r)}[mode]()
    valid = (np.arange(cap)[None, :] < counts[:, None]).reshape(-1)
    assert np.array_equal(got[valid], want[valid])
    assert np.array_equal(got[~valid], b[~valid])


def _stage_ref(b, head, counts, cap, thr, naux):
    """oracle/detect.py's stage decision on each list: score = softmax face prob (0 for crops empty after trunc), kept iff
    score > thr in slot order, emitting trunc(box), score, regs [, landmarks mapped into the frame]"""
    bi = np.trunc(b).astype(F32)
    ok = ((bi[:, 2] - bi[:, 0] + F32(1)) > 0) & ((bi[:, 3] - bi[:, 1] + F32(1)) > 0)
    a0, a1 = head[:, 0], head[:, 1]                              # the oracle's softmax, in float32 op for op
    m = np.maximum(a0, a1)
    e0, e1 = np.exp(a0 - m), np.exp(a1 - m)
    p = np.where(ok, e1 / (e0 + e1), F32(0)).astype(F32)
    out = []
    for l, n in enumerate(counts):
        s = slice(l * cap, l * cap + n)
        keep = np.nonzero(p[s] > F32(thr))[0]
        bl, hl = bi[s][keep], head[s][keep]
        aux = hl[:, 2:6]
        if naux == 14:
            w = (bl[:, 2] - bl[:, 0] + F32(1))[:, None]; hh = (bl[:, 3] - bl[:, 1] + F32(1))[:, None]
            px = w * hl[:, 6:11] + bl[:, 0:1] - F32(1)
            py = hh * hl[:, 11:16] + bl[:, 1:2] - F32(1)
            aux = np.concatenate([aux, np.stack([px, py], 2).reshape(-1, 10)], 1).astype(F32)
        out.append((keep, bl, p[s][keep], aux))
    return p, out


def _ulps(got, want):
    """|got - want| in units of want's f32 ulp"""
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    return d / np.spacing(np.abs(want.astype(F32))).astype(np.float64) if d.size else d


@pytest.mark.parametrize("thr", [0.5, 0.7])
@pytest.mark.parametrize("cap,counts", [(64, (64, 0, 13)), (300, (300, 0, 257)), (512, (257, 512, 0))])
@pytest.mark.parametrize("nh", [6, 16])
def test_stage_select_vs_oracle(lib, nh, cap, counts, thr):
    """fr_stage_select against the oracle's stage decision, with counts that cross the kernel's 256-slot chunks (257, 512) and
    an empty list: kept slots and their order, trunc'ed boxes, regressions and landmarks equal; scores and prob_out within
    2 ulp of the float32 reference (expf against exp); prob_out 0 past the count.  Two equal logits give p = 0.5 exactly, which
    thr = 0.5 must NOT keep (strict >); crops empty after trunc score 0 and are never kept.  The scores' reference is the
    oracle's softmax in float32 numpy (max-subtracted exp, e1 / (e0 + e1))."""
    from facerecognition_infrenceengine_amd import _lib
    naux = 4 if nh == 6 else 14
    rng = np.random.default_rng(cap + nh + int(thr * 10))
    L = 3
    b = _boxes(rng, L * cap)
    head = rng.standard_normal((L * cap, nh)).astype(F32)
    head[:, 6:] = rng.uniform(0, 1, (L * cap, nh - 6))             # landmarks (nh 16): fractions of the box
    lt = math.log(thr / (1 - thr))
    d = rng.uniform(-3, 3, L * cap)
    d = np.where(np.abs(d - lt) < 1e-3, d + 0.01, d)               # every p more than 1e-6 from thr ...
    head[:, 1] = (head[:, 0] + d).astype(F32)
    ties = np.arange(L * cap) % 37 == 5
    head[ties, 1] = head[ties, 0]                                  # ... but these: p == 0.5 exactly
    p64 = 1.0 / (1.0 + np.exp(head[:, 0].astype(np.float64) - head[:, 1].astype(np.float64)))
    far = ~ties
    assert np.all(np.abs(p64[far] - thr) > 1e-6)
    cnt = np.array(counts, np.int32)
    out_b = torch.full((L, cap, 4), -9.0, device="cuda"); out_s = torch.full((L, cap), -9.0, device="cuda")
    out_a = torch.full((L, cap, naux), -9.0, device="cuda"); out_c = _i32([-1] * L)
    prob = torch.full((L, cap), -9.0, device="cuda")
    lib.fr_stage_select(_lib.ptr(bd := _dev(b)), _lib.ptr(hd := _dev(head)), nh, _lib.ptr(cd := _dev(cnt)), L, cap, thr,
                        _lib.ptr(out_b), _lib.ptr(out_s), _lib.ptr(out_a), naux, _lib.ptr(out_c), _lib.ptr(prob), _lib.stream_ptr())
    torch.cuda.synchronize()
    p_ref, ref = _stage_ref(b, head, cnt, cap, thr, naux)
    gb, gs, ga, gc, gp = (t.cpu().numpy() for t in (out_b, out_s, out_a, out_c, prob))
    tied_kept = 0
    for l, (keep, bl, sl, al) in enumerate(ref):
        k = len(keep)
        assert gc[l] == k, (l, gc[l], k)
        assert np.array_equal(gb[l, :k], bl) and np.array_equal(ga[l, :k], al)
        # expf on the device against numpy's exp: the same formula, a last-bit difference of e0 / e1 moves p by <= 2 ulp
        assert k == 0 or _ulps(gs[l, :k], sl).max() <= 2, (l, _ulps(gs[l, :k], sl).max())
        n = cnt[l]
        pl = p_ref[l * cap:l * cap + n]
        assert n == 0 or _ulps(gp[l, :n], pl).max() <= 2, (l, np.bincount(np.ceil(_ulps(gp[l, :n], pl)).astype(int)))
        assert np.array_equal(gp[l, n:], np.zeros(cap - n, F32))
        tied_kept += int(np.isin(keep, np.nonzero(ties[l * cap:l * cap + n])[0]).sum())
        assert np.all(gp[l, :n][_empty(b)[l * cap:l * cap + n]] == 0)
    assert tied_kept == 0
    if thr == 0.5:
        assert np.all(gp.reshape(-1)[ties & (np.arange(L * cap) % cap < np.repeat(cnt, cap)) & ~_empty(b)] == F32(0.5))


def _empty(b):
    return ~(((np.trunc(b[:, 2]) - np.trunc(b[:, 0]) + 1) > 0) & ((np.trunc(b[:, 3]) - np.trunc(b[:, 1]) + 1) > 0))


@pytest.mark.parametrize("k,s", [(3, 2), (2, 2)])
def test_maxpool_vs_torch_ceil_mode(lib, k, s):
    """fr_maxpool_f32 (NHWC, ceil mode) equal to torch's max_pool2d(ceil_mode=True) for H, W in {k, k+1, 2k-1, 24, 47}."""
    from facerecognition_infrenceengine_amd import _lib
    rng = np.random.default_rng(k)
    B, C = 2, 5
    for H in (k, k + 1, 2 * k - 1, 24, 47):
        for W in (k, k + 1, 2 * k - 1, 24, 47):
            x = rng.standard_normal((B, H, W, C)).astype(F32) - 2.0
            want = torch.nn.functional.max_pool2d(torch.from_numpy(x).permute(0, 3, 1, 2), k, s, ceil_mode=True)
            want = want.permute(0, 2, 3, 1).contiguous().numpy()
            y = torch.full((B,) + want.shape[1:], float("nan"), device="cuda")
            lib.fr_maxpool_f32(_lib.ptr(xd := _dev(x)), _lib.ptr(y), B, H, W, C, k, s, _lib.stream_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(y.cpu().numpy(), want), (H, W)


# ------------------------------------------------------------------------------------------------- 4. alignment at the edges
T = oalign.ARCFACE_DST


def _face(scale=1.0, centre=(56.0, 72.0), rot=0.0, mirror=False):
    """the template scaled about its centre, rotated by `rot` degrees, moved to `centre` (frame coordinates)"""
    c = T - T.mean(0)
    if mirror:
        c = c[[1, 0, 2, 4, 3]]                                   # left and right landmarks swapped
    a = math.radians(rot)
    R = np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
    return (c @ R.T * scale + np.asarray(centre)).astype(F32)


def _faces(H, W):
    """[(kps f32 [5,2], frame index)] - the edge cases of the alignment for a frame of H x W (3 frames)"""
    cx, cy = W / 2, H / 2
    return [
        (_face(1.3, (cx, cy)), 0),                                # interior
        (_face(2.0, (8.0, cy)), 1),                               # cut by the left border
        (_face(2.0, (W - 6.0, cy)), 2),                           # right
        (_face(2.0, (cx, 5.0)), 0),                               # top
        (_face(2.0, (cx, H - 4.0)), 1),                           # bottom
        (_face(1.0, (-300.0, H + 250.0)), 2),                     # entirely outside
        (_face(1.0, (W - 1.0, H - 1.0)), 2),                      # covers the last pixel of the last frame (unit steps: the
                                                                  # samples between its last two columns and in its last row)
        (_face(1.2, (cx + 13, cy - 7), mirror=True), 0),          # mirrored landmarks (Umeyama's det < 0 branch)
        (_face(1.1, (cx - 20, cy + 9), rot=90), 1),
        (_face(1.1, (cx + 21, cy + 3), rot=180), 2),
        (_face(4.0 / 35.2, (cx, cy)), 0),                         # eye distance ~4 px
        (_face(400.0 / 35.2, (cx, cy)), 1),                       # ~400 px
        ((T + np.array([17.0, 11.0])).astype(F32), 2),            # template + an integer shift: integer sampling positions
                                                                  # (to the f32 rounding of the landmarks, ~1e-6 px)
    ]


def _umeyama_det(kps):
    """det of the cross-covariance oracle.align.umeyama tests for its reflection branch"""
    s, d = kps.astype(np.float64), T
    return np.linalg.det((d - d.mean(0)).T @ (s - s.mean(0)) / 5)


def _frames(H, W, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 256, (3, H, W, 3), generator=g, device="cuda", dtype=torch.uint8)


def _u8_bar(got, want):
    """the existing bar (test_align_vs_golden): u8 crops differ by at most 1, at no more than 1e-3 of the pixels - rounding
    ties at .5, where the closed-form geometry and the float64 SVD land on either side"""
    diff = np.abs(got.astype(int) - want.astype(int))
    return diff.max() <= 1 and (diff > 0).mean() <= 1e-3


def _decode_f16(out):
    """f16 NHWC8 (x - 127.5) / 127.5 RGB -> u8 BGR; checks the f16 values ARE that encoding of the decoded bytes"""
    x = out.cpu().numpy()
    u = np.round(x[..., :3].astype(np.float64) * 127.5 + 127.5).astype(np.int64)
    assert u.min() >= 0 and u.max() <= 255
    enc = ((u.astype(F32) - F32(127.5)) / F32(127.5)).astype(np.float16)
    assert np.array_equal(x[..., :3], enc)
    assert not x[..., 3:].any()                                   # channels 3 - 7 are zero
    return u[..., ::-1].astype(np.uint8)


@pytest.mark.parametrize("H,W", [(241, 319), (1080, 1920)])
def test_warp_affine_5pt_edges_vs_oracle(lib, H, W):
    """fr_warp_affine_5pt on three frames (frame_idx across them, a device count) against oracle.align.norm_crop for the edge
    faces of _faces(): u8 crops within the u8 bar, the f16 output the normalised RGB of the same bytes, M_out = Umeyama's
    similarity; the faces at index >= count are zero."""
    from facerecognition_infrenceengine_amd import _lib
    frames = _frames(H, W, H)
    fr_h = frames.cpu().numpy()
    faces = _faces(H, W)
    extra = [(_face(1.3, (W / 2, H / 2)), 1), (_face(1.0, (30.0, 40.0)), 0)]       # past the count: zero
    kps = np.stack([k for k, _ in faces + extra])
    fidx = np.array([f for _, f in faces + extra], np.int32)
    F, cnt = len(kps), len(faces)
    out = torch.full((F, 112, 112, 8), float("nan"), dtype=torch.float16, device="cuda")
    u8 = torch.full((F, 112, 112, 3), 77, dtype=torch.uint8, device="cuda")
    M = torch.zeros((F, 2, 3), dtype=torch.float32, device="cuda")
    lib.fr_warp_affine_5pt(_lib.ptr(frames), 3, H, W, _lib.ptr(kd := _dev(kps)), _lib.ptr(fd := _dev(fidx)), _lib.ptr(cd := _i32([cnt])),
                           F, 112, _lib.ptr(out), _lib.ptr(u8), _lib.ptr(M), _lib.stream_ptr())
    torch.cuda.synchronize()
    got_u8, got_m = u8.cpu().numpy(), M.cpu().numpy()
    dec = _decode_f16(out[:cnt])
    for i, (k, f) in enumerate(faces):
        want, Mw = oalign.norm_crop(fr_h[f], k)
        np.testing.assert_allclose(got_m[i], Mw, rtol=1e-5, atol=1e-4, err_msg=str(i))    # closed form == Umeyama's SVD
        assert _u8_bar(got_u8[i], want), i
        assert np.array_equal(dec[i], got_u8[i]), i
    assert _umeyama_det(faces[7][0]) < 0 < _umeyama_det(faces[0][0])   # the mirrored face does take the det < 0 branch
    assert not got_u8[5].any()                                    # the face outside the frame samples the zero border only
    assert not out[cnt:].float().abs().sum().item() and not got_u8[cnt:].any()


def _slot_layout(faces, nframes, cap):
    kps = np.full((nframes * cap, 5, 2), np.nan, F32)            # invalid slots: NaN landmarks
    counts = np.zeros(nframes, np.int32)
    where = []
    for k, f in faces:
        kps[f * cap + counts[f]] = k
        where.append(f * cap + counts[f])
        counts[f] += 1
    return kps, counts, where


@pytest.mark.parametrize("H,W", [(241, 319), (1080, 1920)])
def test_warp_affine_5pt_slots_edges_vs_oracle(lib, H, W):
    """fr_warp_affine_5pt_slots (the alignment of detect_embed_slots): the edge faces of _faces() in per-frame slots, decoded
    from f16 back to u8 and held to the u8 bar against oracle.align.norm_crop; channels 3 - 7 zero; the invalid slots (NaN
    landmarks) zero.  Then 3 frames x cap 4 with counts {4, 0, 2}: every slot past its frame's count is all zero."""
    from facerecognition_infrenceengine_amd import _lib
    frames = _frames(H, W, H + 1)
    fr_h = frames.cpu().numpy()
    faces = _faces(H, W)
    cap = max(sum(1 for _, f in faces if f == g) for g in range(3)) + 1
    kps, counts, where = _slot_layout(faces, 3, cap)
    out = torch.full((3 * cap, 112, 112, 8), float("nan"), dtype=torch.float16, device="cuda")
    lib.fr_warp_affine_5pt_slots(_lib.ptr(frames), 3, H, W, _lib.ptr(kd := _dev(kps)), _lib.ptr(cd := _dev(counts)), cap, 112,
                                 _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    dec = _decode_f16(out[torch.tensor(where, device="cuda")])
    for i, ((k, f), s) in enumerate(zip(faces, where)):
        want, _ = oalign.norm_crop(fr_h[f], k)
        assert _u8_bar(dec[i], want), s
    invalid = np.setdiff1d(np.arange(3 * cap), where)
    assert len(invalid) >= 3 and not out[torch.from_numpy(invalid).cuda()].float().abs().sum().item()
    # 3 frames, cap 4, counts {4, 0, 2}
    six = [(faces[i][0], 0) for i in (0, 1, 3, 7)] + [(faces[i][0], 2) for i in (6, 9)]
    kps, counts, where = _slot_layout(six, 3, 4)
    assert counts.tolist() == [4, 0, 2]
    out = torch.full((12, 112, 112, 8), float("nan"), dtype=torch.float16, device="cuda")
    lib.fr_warp_affine_5pt_slots(_lib.ptr(frames), 3, H, W, _lib.ptr(kd := _dev(kps)), _lib.ptr(cd := _dev(counts)), 4, 112,
                                 _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    dec = _decode_f16(out[torch.tensor(where, device="cuda")])
    for i, ((k, f), s) in enumerate(zip(six, where)):
        assert _u8_bar(dec[i], oalign.norm_crop(fr_h[f], k)[0]), s
    assert sorted(where) == [0, 1, 2, 3, 8, 9]
    for s in (4, 5, 6, 7, 10, 11):
        assert not out[s].float().abs().sum().item(), s
