"""Pins for the coarse gallery scan (csrc/scan_gemm.hip) and for the two premises of the certified coarse top-K.

A. The coarse scores themselves, through the one window that shows them: fr_gallery_match_f16 / _f8 with G32 == NULL return the coarse
   maximum and the first row of the first group that attains it.  Operands are small integers times a dyadic quantum, every row is the
   winner of some query, the result is compared bit for bit with tests/helpers/coarse_ref.py.  The view forms refuse a NULL G32 and are
   pinned through their exact re-rank over f32 rows that hold the same integers.
B. |coarse - exact| <= eps on operands built to approach each term of eps; the bound is DESIGN.md's, nothing is measured to set it.
C. Every row the candidate lists do not name has a coarse score <= B: galleries where coarse and exact order disagree by less than eps,
   one per path on which the scan lets a group go, and positive controls so that "always flag" cannot pass.
tests/test_coarse_ref_host.py shows on the CPU that these instruments fail planted faults."""
import numpy as np
import pytest
import torch

from tests.helpers import coarse_ref as cr

gpu = pytest.mark.gpu
NEVER = 1 << 40
IDX_FILL = -7777
SCORE_FILL = 0x7FC0BEEF                                                    # a NaN no kernel produces


def _bits(t):
    return t.contiguous().view(torch.int32)


def _outputs(F):
    idx = torch.full((F,), IDX_FILL, dtype=torch.int64, device="cuda")
    score = torch.full((F,), SCORE_FILL, dtype=torch.int32, device="cuda").view(torch.float32)
    return idx, score


def _coarse_rows(lib, Gd, kind):
    from facerecognition_infrenceengine_amd import _lib
    Gc = torch.empty(Gd.shape, dtype=torch.float16 if kind == "f16" else torch.uint8, device="cuda")
    (lib.fr_f32_to_f16 if kind == "f16" else lib.fr_f32_to_f8)(_lib.ptr(Gd), _lib.ptr(Gc), Gd.numel(), _lib.stream_ptr())
    return Gc


def _scan_null(lib, kind, Qd, Gc, N, row_offset=0):
    """fr_gallery_match_f16 / _f8 with G32 == NULL -> (idx, score) from prefilled outputs; the plan is held to the workspace size"""
    from facerecognition_infrenceengine_amd import _lib
    F = Qd.shape[0]
    wsz, fn = ((lib.fr_gallery_match_f16_workspace, lib.fr_gallery_match_f16) if kind == "f16" else
               (lib.fr_gallery_match_f8_workspace, lib.fr_gallery_match_f8))
    need = wsz(F, N)
    pl = cr.check_plan(need, F, N, kind)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    idx, score = _outputs(F)
    fn(_lib.ptr(Qd), _lib.ptr(Gc), None, F, N, 512, row_offset, _lib.ptr(idx), _lib.ptr(score), _lib.ptr(ws), need, None, 0,
       _lib.stream_ptr())
    return idx, score, pl


def _equal(idx, score, want):
    return (torch.equal(idx.cpu(), torch.from_numpy(want[0])) and
            torch.equal(_bits(score).cpu(), torch.from_numpy(want[1].view(np.int32))))


def _variants(N, F, kind):
    v = [("plain", pi, 0) for pi in cr.launches(N, F)]
    v[1] = ("plain", v[1][1], (1 << 33) + 5)                               # out_idx carries row_offset
    if kind == "f8" and F == N:
        v.append(("offgrid", cr.launches(N, F)[1], 0))                     # conversion roundings, ties and saturation at +-448
    if (N, F) == (63, 63):
        v += [("negative", pi, 0) for pi in cr.launches(N, F)[:2]]         # the masked zero rows of the partial tile would win
    return v


# ---------------------------------------------------------------- A
@gpu
@pytest.mark.parametrize("kind", ["f16", "f8"])
@pytest.mark.parametrize("N,F", cr.SCAN_SHAPES)
def test_coarse_scores_bit_for_bit(lib, N, F, kind):
    """Query f = row pi(f): its own row must win with |row|^2, an integer that any dropped, doubled or misplaced contribution changes."""
    done = {}
    for variant, pi, off in _variants(N, F, kind):
        Q, G, S = cr.planted(N, kind, pi, variant)
        want = cr.pick(S, kind, off)
        if variant not in done:
            done[variant] = _coarse_rows(lib, torch.tensor(G).cuda(), kind)
        Qd = torch.from_numpy(Q).cuda()
        idx, score, pl = _scan_null(lib, kind, Qd, done[variant], N, off)
        if (N, F) in cr.SCAN_PLANS:
            assert (pl.nqt, pl.nranges, pl.tiles_per_range) == cr.SCAN_PLANS[(N, F)]
        assert _equal(idx, score, want), (variant, int((idx.cpu() != torch.from_numpy(want[0])).sum()),
                                          int((_bits(score).cpu() != torch.from_numpy(want[1].view(np.int32))).sum()))
        if variant == "negative":
            assert bool((score < 0).all()) and bool((score > -1).all())


@gpu
@pytest.mark.parametrize("kind", ["f16", "f8"])
def test_null_g32_reports_nothing_at_or_below_minus_one(lib, kind):
    """(-1, -1.0) when no coarse score exceeds -1; a score of exactly -1 does not; N == 0 likewise"""
    G = np.zeros((8, 512), np.float32); G[:, 0] = [1, 1, 1, 1, 0.5, 1, 1, 1]
    Q = np.zeros((3, 512), np.float32); Q[:, 0] = [-1.0, -0.5, -1.5]
    Qd = torch.from_numpy(Q).cuda()
    for n in (4, 8):
        Gc = _coarse_rows(lib, torch.from_numpy(G[:n].copy()).cuda(), kind)
        idx, score, _ = _scan_null(lib, kind, Qd, Gc, n)
        want = cr.coarse_ref(Q, G[:n], kind)
        assert _equal(idx, score, want)
        assert idx.tolist() == ([-1, 0, -1] if n == 4 else [4, 4, 4])
        assert score.tolist() == ([-1.0, -0.5, -1.0] if n == 4 else [-0.5, -0.25, -0.75])
    idx, score, _ = _scan_null(lib, kind, Qd, None, 0)
    assert idx.tolist() == [-1] * 3 and score.tolist() == [-1.0] * 3


@gpu
@pytest.mark.parametrize("kind", ["f16", "f8"])
@pytest.mark.parametrize("N", [1, 63, 67, 16448])
def test_view_scan_over_a_shuffled_slab(lib, N, kind):
    """The same integers behind a view: capacity > Nview, slots out of order, unused slots NaN in both slabs.  The f32 slab holds the
    same integers, so the exact re-rank's score is the coarse one: idx (first row of the maximum) and score bits equal the reference."""
    from facerecognition_infrenceengine_amd import _lib
    from facerecognition_infrenceengine_amd.gallery import DeviceGallery
    F = min(N, 256)
    G = cr.exact_gallery(N, kind)[0]
    g = DeviceGallery("cuda:0", capacity=N + 37, scan=kind)
    g.G.fill_(float("nan"))
    if kind == "f16":
        g.S.fill_(float("nan"))
    else:
        g.S.fill_(0x7F)                                                    # the e4m3 NaN code
    order = np.random.default_rng(N).permutation(N)
    g.upsert(order.tolist(), G[order])
    view = g.view(range(N))
    unused = torch.ones(g.capacity, dtype=torch.bool, device="cuda")
    unused[view.slots] = False
    assert g.capacity > N and int(unused.sum()) == g.capacity - N and bool(torch.isnan(g.G[unused]).all())
    assert N == 1 or not torch.equal(view.slots, torch.arange(N, device="cuda"))
    wsz, fn = ((lib.fr_gallery_match_view_f16_workspace, lib.fr_gallery_match_view_f16) if kind == "f16" else
               (lib.fr_gallery_match_view_f8_workspace, lib.fr_gallery_match_view_f8))
    need = wsz(F, N)
    cr.check_plan(need, F, N, kind)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    slots = view.slots
    for pi in cr.launches(N, F):
        Q, _, S = cr.planted(N, kind, pi)
        want = cr.rerank_ref(S, kind)
        assert np.array_equal(want[0], pi) and np.array_equal(cr.pick(S, kind)[0], pi // 4 * 4)
        Qd = torch.from_numpy(Q).cuda()
        idx, score = _outputs(F)
        fn(_lib.ptr(Qd), _lib.ptr(g.S), _lib.ptr(g.G), _lib.ptr(slots), F, N, g.capacity, 512, _lib.ptr(idx), _lib.ptr(score),
           _lib.ptr(ws), need, _lib.stream_ptr())
        assert _equal(idx, score, want)


# ---------------------------------------------------------------- B
@gpu
def test_coarse_minus_exact_stays_inside_eps(lib):
    """One launch per probe: 64 rows, the row under test planted at (7 j + 3) mod 64, every other row zero (score 0 < the probe's).
    Required: the bound of DESIGN.md 4.6b (tests/helpers/coarse_ref.eps_bound) with the row's own norm for Gmax - for operands that f16
    holds exactly the accumulation term alone - and bit-equality where every partial sum is an f32 number in any order (subnormal
    operands: a flushing matrix instruction returns 0 there).  Printed, not asserted: the worst err / bound per family and the smallest s at
    which 1 + 31 * 2^-s per 32 columns stops coming back exactly.  On an MI355X (KERNEL_NOTES 4.14): 0.924, 0.676, 0.0039, 0.072 for families
    1 .. 4; the window probes bit-exact up to s = 23 with alternating signs and up to s = 20 with positive ones (then <= 2 ulp of the result,
    the accumulator's own rounding)."""
    from facerecognition_infrenceengine_amd import _lib
    fam = cr.eps_families()
    P, N = len(fam), 64
    Qd = torch.from_numpy(np.stack([p.q for p in fam])).cuda()
    G16 = _coarse_rows(lib, torch.from_numpy(np.stack([p.g for p in fam])).cuda(), "f16")
    Z = torch.zeros((N, 512), dtype=torch.float16, device="cuda")
    need = lib.fr_gallery_match_f16_workspace(1, N)
    assert cr.check_plan(need, 1, N).nranges == 1
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    idx, score = _outputs(P)
    s = _lib.stream_ptr()
    where = [(7 * j + 3) % N for j in range(P)]
    for j in range(P):
        Z[where[j]].copy_(G16[j])
        qj, ij, sj = Qd[j:j + 1], idx[j:j + 1], score[j:j + 1]
        lib.fr_gallery_match_f16(_lib.ptr(qj), _lib.ptr(Z), None, 1, N, 512, 0, _lib.ptr(ij), _lib.ptr(sj), _lib.ptr(ws), need, None, 0, s)
        Z[where[j]].zero_()
    got = score.cpu().numpy()
    assert idx.tolist() == [w // 4 * 4 for w in where]
    worst, inexact, fails = {}, {}, []
    for p, v in zip(fam, got.astype(np.float64)):
        r = abs(v - p.d) / cr.eps_bound(p.q, p.g, p.full)
        if r > worst.get(p.family, (-1, ""))[0]:
            worst[p.family] = (r, p.name)
        if p.family == 3 and v != p.d:
            key = ("alt" if "-alt-" in p.name else "pos", p.s)
            n, e = inexact.get(key, (0, 0.0))
            inexact[key] = (n + 1, max(e, abs(v - p.d) * 2.0 ** p.s))
        if not r <= 1.0 or (p.exact and v != p.d):
            fails.append((p.name, float(v), p.d, r))
    for k in sorted(worst):
        print(f"family {k}: worst err / bound {worst[k][0]:.4f} ({worst[k][1]})")
    print("f16 MFMA window probe, (signs, s): (positions of 32 not bit-exact, worst error in units of 2^-s):", inexact or "exact up to s = 23")
    assert not fails, fails[:8]


# ---------------------------------------------------------------- C
def _same(a, b):
    return a[0].shape == b[0].shape and torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1]))


def _poison(F, K):
    """match_topk_device allocates its own outputs: leave sentinels in blocks of their size for the allocator to hand out next (best effort)"""
    a = torch.full((F, K), IDX_FILL, dtype=torch.int64, device="cuda")
    b = torch.full((F, K), SCORE_FILL, dtype=torch.int32, device="cuda")
    del a, b


def _both(m, Qd, K):
    """(coarse result, exact result, flags) of one matcher or view, the path of each call asserted (as tests/test_gpu_topk_coarse.py)"""
    from facerecognition_infrenceengine_amd.gallery import last_topk
    owner = m.gallery if hasattr(m, "gallery") else m
    owner.coarse_topk_min_rows = 0
    _poison(Qd.shape[0], K)
    got = m.match_topk_device(Qd, K, renormalise=False)
    rec = last_topk()
    assert rec["path"] == "coarse"
    flags = rec["flags"]
    owner.coarse_topk_min_rows = NEVER
    _poison(Qd.shape[0], K)
    want = m.match_topk_device(Qd, K, renormalise=False)
    assert last_topk()["path"] == "exact"
    owner.coarse_topk_min_rows = 0
    return got, want, flags


@pytest.fixture(scope="module")
def topk_base():
    """the background rows on the device and a DeviceGallery holding them in shuffled slots (ids = rows 0 .. 32 770)"""
    from facerecognition_infrenceengine_amd.gallery import DeviceGallery
    n = cr.TOPK_N + 3
    base = cr.background(n)
    g = DeviceGallery("cuda:0", capacity=64, scan="f16")
    order = np.random.default_rng(9).permutation(n)
    g.upsert(order.tolist(), base[order])
    assert g.capacity > n
    return torch.from_numpy(base).cuda(), g


@gpu
@pytest.mark.parametrize("name", cr.TOPK_GROUPS)
def test_unseen_rows_are_bounded(lib, topk_base, name):
    """Background rows score exactly 0; row B = 0.7 on the f16 grid, row A rounds to it but scores 2.3e-4 more exactly, row X scores more
    coarsely and less exactly than A.  A is the true top-1 of every case and the lists never hold it, so the query must be flagged (and
    then answered exactly); with the seen rows raised by 5.5e-3 (> 2 eps) it must be certified.  Layouts: 1 a tile refused at the door,
    2 a group refused inside the insert, 3 a group pushed off the end, 4 the (C+1)-th candidate (K = 1, 5, 16); last*: A (layout 3: the
    fourth X) in rows N - 4 .. N - 1; partial: N = 32 771, A = N - 1 alone in a tile of 3 rows."""
    from facerecognition_infrenceengine_amd.gallery import GalleryMatcher
    base, g = topk_base
    grp = cr.topk_group(name)
    N, F = grp.N, len(grp.cases)
    pl = cr.check_plan(lib.fr_gallery_match_f16_workspace(F, N), F, N)
    assert (pl.nranges, pl.rows_per_range) == (grp.plan.nranges, grp.plan.rows_per_range) == ((171, 192) if name == "partial" else (256, 128))
    rows = sorted(grp.rows)
    vec = torch.from_numpy(np.stack([grp.rows[r] for r in rows])).cuda()
    rix = torch.tensor(rows, device="cuda")
    Gd = base[:N].clone()
    Gd[rix] = vec
    m = GalleryMatcher("cuda:0", scan="f16")
    m.set_rows(list(range(N)), Gd, normalise=False)
    g.upsert(rows, vec)
    try:
        view = g.view(range(N))
        assert float(m.gmax) == 1.0 and float(g.gmax) == 1.0               # eps is the formula's at |q| = sqrt(1 + QC^2), Gmax = 1
        Qd = torch.from_numpy(grp.Q).cuda()
        eps = cr.cert_eps(float(np.linalg.norm(grp.Q[0].astype(np.float64))), 1.0)
        assert cr.PC - cr.P16 > 2 * eps > 2 * (cr.PA - cr.P16)             # the controls' gap is beyond eps, the cases' disagreement inside it
        for K in sorted({c.K for c in grp.cases}):
            for who in (m, view):
                got, want, flags = _both(who, Qd, K)
                assert _same(got, want), (name, K)
                for f, c in enumerate(grp.cases):
                    if c.K != K:
                        continue
                    truth = cr.topk_truth(grp, f, K)
                    assert got[0][f].tolist() == truth and (c.control or truth[0] == c.a_row), (c.name, got[0][f].tolist(), truth)
                    assert int(flags[f]) == (0 if c.control else 1), (c.name, who is view, flags.tolist())
    finally:
        g.upsert(rows, base[rix])                                          # the shared slab gets its background rows back
