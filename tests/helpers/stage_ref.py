"""Float64 references for WHOLE RUNS of the f16 stage kernels (fr_conv_stage14_f16: 14x14x256, fr_conv_stage28_f16: 28x28x128), the
operand generators, the checks and the float32 emulation with planted faults that tests/test_gpu_stage_pins.py (GPU) and
tests/test_stage_ref_host.py (CPU) share.  The single conv, its layouts and `conv_bound` are embed_ref's.

A run is 2 * nblocks convs: block b = conv 2b (9-class bias, PReLU -> f16 map `mid`) and conv 2b + 1 (bias, + the block's input ->
f16).  Parameters are the kernels' own layout, [2 * nblocks][10][C]: rows 0 .. 8 the border-class biases (a second conv repeats its
bias nine times), row 9 the slope (1 for a second conv).

Instruments:
  * exact_stage_run_f16: integer operands with a FIXED number of +-1 weights per row, so the map grows from block to block instead
    of dying out; every value before a rounding is an integer below 2^24 in every partial sum (asserted), so the result does not
    depend on the order of summation, and once the values pass 2048 the f32 -> f16 rounding of each conv is exercised, ties included.
  * selector_block: float operands, one conv of the block a signed channel permutation on the centre tap, so that the other
    conv's every element stands in the output, against float64 within conv_bound.
  * emulate_stage_run: the run in float32 with one fault planted, to show that the two instruments would notice."""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from tests.helpers import embed_ref as er

GEOM = {14: SimpleNamespace(C=256, steps=72), 28: SimpleNamespace(C=128, steps=36)}
EVENTS = ("unrounded", "rounded_non_tie", "tie_up", "tie_down")


def step_of_column(HW):
    """K step of each column of a [tap][C] weight row, as the pack kernels lay the stream out: 14x14 slot = tap * 8 + 32-channel
    group; 28x28 slot = plane * 18 + tap * 2 + 32-channel group of the plane (plane = 64 channels, K is plane-major)."""
    C = GEOM[HW].C
    col = np.arange(9 * C)
    tap, c = col // C, col % C
    return tap * 8 + c // 32 if HW == 14 else (c // 64) * 18 + tap * 2 + (c % 64) // 32


def covers_every_step(w, HW):
    """A non-zero weight for every (K step, wave group of 64 couts): no step of no wave multiplies by zeros only."""
    step, S = step_of_column(HW), GEOM[HW].steps
    nz = np.zeros((w.shape[0] // 64, S), bool)
    for g in range(w.shape[0] // 64):
        nz[g, step[np.flatnonzero(np.any(w[g * 64:(g + 1) * 64] != 0, 0))]] = True
    return bool(nz.all())


def covering_weights(rng, HW, per_row):
    """[C][9 C] weights with exactly per_row entries of +-1 per row, placed so that covers_every_step holds by construction: the
    64 * per_row entries of a group of 64 rows are dealt over the K steps, every step at least once."""
    C, S = GEOM[HW].C, GEOM[HW].steps
    step = step_of_column(HW)
    cols_of = [np.flatnonzero(step == s) for s in range(S)]
    w = np.zeros((C, 9 * C))
    for g in range(C // 64):
        steps = rng.permutation(np.concatenate([np.arange(S), rng.integers(0, S, 64 * per_row - S)])).reshape(64, per_row)
        for i in range(64):
            cols = [rng.choice(cols_of[s]) for s in steps[i]]
            while len(set(cols)) < per_row:
                cols = [rng.choice(cols_of[s]) for s in steps[i]]
            w[g * 64 + i, cols] = rng.choice([-1.0, 1.0], per_row)
    assert ((w != 0).sum(1) == per_row).all() and covers_every_step(w, HW)
    return w


def f16(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def class_map(HW):
    """[HW][HW] border class 0 .. 8 = 3 * (first / inner / last row) + (first / inner / last column)."""
    c = er.border_class(HW)
    return c[:, None] * 3 + c[None, :]


def conv_of_run(h, w, prm, j, residual):
    """Conv j of a run in float64 from the kernels' parameter rows -> (want before the rounding, mag)."""
    if j % 2 == 0:
        return er.conv_ref(h, w, prm[:9].reshape(-1), 1, prm[9], None, 1, 1)
    return er.conv_ref(h, w, prm[0], 0, None, residual, 1, 1)


def stage_run_ref(x, w, prm):
    """The run block by block in float64 with a cast to f16 after each conv -> per conv the unrounded value and mag, per block the
    f16 maps `mid` and `out` (as float64)."""
    r = SimpleNamespace(raw=[], mag=[], mids=[], outs=[])
    h = np.asarray(x, np.float64)
    for b in range(len(w) // 2):
        v, m = conv_of_run(h, w[2 * b], prm[2 * b], 2 * b, None)
        r.raw.append(v), r.mag.append(m), r.mids.append(f16(v))
        v, m = conv_of_run(r.mids[-1], w[2 * b + 1], prm[2 * b + 1], 2 * b + 1, h)
        h = f16(v)
        r.raw.append(v), r.mag.append(m), r.outs.append(h)
    return r


def rounding_events(v):
    """Which f32 -> f16 roundings the integers v exercise -> {event: mask}.  A tie is a value exactly between two neighbouring
    f16 numbers; "up" / "down" is the direction the even neighbour lies in."""
    r = f16(v)
    d = r - v
    other = np.nextafter(r.astype(np.float16), np.where(d > 0, -np.inf, np.inf).astype(np.float16)).astype(np.float64)
    tie = (d != 0) & (np.abs(d) == np.abs(other - v))
    return {"unrounded": (d == 0) & (v != 0), "rounded_non_tie": (d != 0) & ~tie, "tie_up": tie & (d > 0), "tie_down": tie & (d < 0)}


def exact_stage_run_f16(rng, B, HW, nblocks, per_row, rounds=None, slope_p=None):
    """Operands of a whole run on which every conv is exact, with the reference and the conditions asserted on it.

    x in {-2 .. 2}; per conv covering_weights(per_row); first convs: integer 9-class bias in [-8, 8] and slopes in {-1, 0, 1, 2}
    (with the probabilities slope_p, default uniform); second convs: an integer bias; all of them drawn anew for every conv.  Asserted per conv: the value before the rounding is an
    integer, mag < 2^24 (every f32 partial sum exact in any order), |v| <= 65504, a non-zero weight for every (K step, cout group).
    Asserted over the run, in a `mid` map AND in a block output: an element that needs no rounding, and - if `rounds` (default:
    the run is deep enough for values past 2048: 7 blocks at 2 per row, 4 at 4) - a rounded non-tie, a tie resolved upwards and one
    downwards; a negative pre-activation under a slope != 1 (first convs: second convs have no slope); every border class holds a
    rounded element.  Runs of 2 and 3 blocks at 2 per row stay below 2048 (max |v| 106 .. 139 and 249 .. 374 in the cases used): they pin the
    mechanisms of the second and third block without a rounding, and assert that too."""
    C = GEOM[HW].C
    o = SimpleNamespace(B=B, HW=HW, C=C, nblocks=nblocks, per_row=per_row)
    o.x = rng.integers(-2, 3, (B, HW, HW, C)).astype(np.float64)
    o.w = [covering_weights(rng, HW, per_row) for _ in range(2 * nblocks)]
    o.prm = np.empty((2 * nblocks, 10, C))
    for j in range(2 * nblocks):
        if j % 2 == 0:
            o.prm[j, :9], o.prm[j, 9] = rng.integers(-8, 9, (9, C)), rng.choice([-1.0, 0.0, 1.0, 2.0], C, p=slope_p)
        else:
            o.prm[j, :9], o.prm[j, 9] = rng.integers(-8, 9, C)[None], 1.0
    assert all(not np.array_equal(o.w[j], o.w[j - 2]) and not np.array_equal(o.prm[j], o.prm[j - 2]) for j in range(2, 2 * nblocks))
    r = stage_run_ref(o.x, o.w, o.prm)
    o.mids, o.outs, o.want = r.mids, r.outs, r.outs[-1]
    for j in range(2 * nblocks):
        assert np.array_equal(r.raw[j], np.round(r.raw[j])), ("not integral", j)
        assert r.mag[j].max() < 2.0 ** 24 and np.abs(r.raw[j]).max() <= 65504, (j, r.mag[j].max(), np.abs(r.raw[j]).max())
        assert covers_every_step(o.w[j], HW), j
    o.growth = [float(np.abs(h).max()) for h in o.outs]
    o.events = {kind: {e: 0 for e in EVENTS} for kind in ("mid", "out")}
    cls, classes = class_map(HW), set()
    for j in range(2 * nblocks):
        kind = "mid" if j % 2 == 0 else "out"
        ev = rounding_events(r.raw[j])
        for e in EVENTS:
            o.events[kind][e] += int(ev[e].sum())
        classes |= set(np.unique(cls[np.nonzero(~ev["unrounded"] & (r.raw[j] != 0))[1:3]]).tolist())
    # a first conv's value before PReLU: negative under a slope != 1
    pre = [er.conv_ref(o.x if b == 0 else o.outs[b - 1], o.w[2 * b], o.prm[2 * b, :9].reshape(-1), 1, None, None, 1, 1)[0]
           for b in range(min(nblocks, 2))]
    o.neg_slope = [int(((p < 0) & (o.prm[2 * b, 9] != 1)).sum()) for b, p in enumerate(pre)]
    assert all(n > 0 for n in o.neg_slope), o.neg_slope
    o.rounds = (nblocks, per_row) in ((7, 2), (4, 4)) if rounds is None else rounds
    for kind in ("mid", "out"):
        assert o.events[kind]["unrounded"] > 0
        if o.rounds:
            assert all(o.events[kind][e] > 0 for e in EVENTS), (kind, o.events[kind])
        else:
            assert all(o.events[kind][e] == 0 for e in EVENTS[1:]), (kind, o.events[kind])
    if o.rounds:
        assert classes == set(range(9)), classes
    return o


# The exact cases of the GPU test: (HW, nblocks, per_row, faces) -> seed of the draw.  A seed other than 0 is the first one whose
# draw reaches every event of the list above (they are conditions on the inputs: a draw that misses one is replaced, nothing is
# skipped).  At 4 per row the `mid` map of block 4 passes 4096 - where an integer can be rounded without being a tie - only when
# the slopes lean towards 2 and -1, hence SLOPE_P4; all four slopes still occur in every conv.
SLOPE_P4 = (0.2, 0.05, 0.05, 0.7)
EXACT_SEEDS = {(14, 7, 2, 1): 6, (14, 7, 2, 3): 3, (28, 7, 2, 1): 13, (28, 7, 2, 3): 10,
               (14, 4, 4, 1): 2, (14, 4, 4, 3): 2, (28, 4, 4, 1): 6, (28, 4, 4, 3): 1}
DEPTHS = ((2, 2), (3, 2), (7, 2), (4, 4))               # (nblocks, per_row)
WIDE_FACES = 7                                          # distinct faces behind the 256- and 257-face launches
_exact_cache = {}


def exact_case(HW, nblocks, per_row, faces):
    """exact_stage_run_f16 of a case of the table, made once per process and shared (nobody may change it)."""
    key = (HW, nblocks, per_row, faces)
    if key not in _exact_cache:
        rng = np.random.default_rng(EXACT_SEEDS.get(key, 0))
        _exact_cache[key] = exact_stage_run_f16(rng, faces, HW, nblocks, per_row, slope_p=SLOPE_P4 if per_row == 4 else None)
    return _exact_cache[key]


def gather_faces(a, B):
    """B faces from the distinct faces of `a` in the order i % len(a): every neighbour differs."""
    return a[np.arange(B) % a.shape[0]]


# ---------------------------------------------------------------- a selecting partner conv
def selector_weights(rng, C):
    """One centre-tap weight of +-1 per row, the rows a permutation of the channels -> (w [C][9 C], perm, sign)."""
    perm, sign = rng.permutation(C), rng.choice([-1.0, 1.0], C)
    w = np.zeros((C, 9 * C))
    w[np.arange(C), 4 * C + perm] = sign
    return w, perm, sign


def selector_block(rng, HW, which, x):
    """A block on float operands whose conv `which` ("conv1" / "conv2") is a selector and whose other conv is random (f16 weights,
    f32 parameters; a first conv's slopes include zeros and negatives) -> .w (2), .prm [2][10][C], and for the input x the
    float64 reference: .want / .bound of the block's output per element, .want_mid / .bound_mid of the f16 map between the convs.

    conv2 the selector: out = sign * mid[perm] + x.  Where x == 0 that is mid's element itself, exactly, under conv1's own
    conv_bound (K + 2 roundings at 2^-24 mag max(1, |slope|), half an f16 ulp).  Where x != 0 the selecting conv adds its own
    conv_bound with K = 1 on the magnitude |mid| + |x| (mid taken at the far end of its own bound) and its half ulp.
    conv1 the selector: mid = sign * x[perm] exactly; conv2 + bias + x against float64 under conv_bound with slope 1."""
    C, K = GEOM[HW].C, 9 * GEOM[HW].C
    o = SimpleNamespace(HW=HW, C=C, which=which, x=np.asarray(x, np.float64))
    wsel, o.perm, o.sign = selector_weights(rng, C)
    wr = er._f16(rng.standard_normal((C, K)) * (2.0 / K) ** 0.5)
    o.prm = np.zeros((2, 10, C))
    o.prm[:, 9] = 1.0
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    if which == "conv2":
        o.w = [wr, wsel]
        o.prm[0, :9] = f32(rng.standard_normal((9, C)) * 0.3)
        o.prm[0, 9] = f32(rng.random(C) - 0.25)
        o.prm[0, 9, ::7] = 0.0
        assert (o.prm[0, 9] < 0).any() and (o.prm[0, 9] > 0).any()
        o.want_mid, mag = conv_of_run(o.x, wr, o.prm[0], 0, None)
        o.bound_mid = er.conv_bound(K, mag, o.want_mid)
        wm, bm = o.want_mid[..., o.perm], o.bound_mid[..., o.perm]
        o.want = o.sign * wm + o.x
        own = er.conv_bound(1, np.abs(wm) + bm + np.abs(o.x), o.want)
        o.bound = bm + np.where(o.x != 0, own, 0.0)
    else:
        o.w = [wsel, wr]
        o.prm[1, :9] = f32(rng.standard_normal(C) * 0.1)[None]
        o.want_mid = o.sign * o.x[..., o.perm]
        o.bound_mid = np.zeros_like(o.want_mid)
        o.want, mag = conv_of_run(o.want_mid, wr, o.prm[1], 1, o.x)
        o.bound = er.conv_bound(K, mag, o.want)
    return o


def selector_seed(HW, which, variant):
    return HW * 100 + 10 * (which == "conv1") + ("even", "odd", "none", "late").index(variant)


def selector_input(rng, B, HW, zero):
    """f16 normal input with the channels of one parity ("even" / "odd") zero: there the block's residual is zero, and a selecting
    second conv shows the first conv's element untouched; every K step of the first conv still has 16 non-zero inputs."""
    C = GEOM[HW].C
    x = er._f16(rng.standard_normal((B, HW, HW, C)))
    x[..., 0::2] *= zero != "even"
    x[..., 1::2] *= zero != "odd"
    return x


def selector_ratio(o, y, mid=None):
    """Worst err / bound of the output y of a selector block and, where the kernel shows it (28x28), of the `mid` map: exact for a
    selecting first conv, under the first conv's own bound otherwise."""
    y = np.asarray(y, np.float64)
    assert np.isfinite(y).all()
    worst = er.worst_ratio(np.abs(y - o.want), o.bound)
    if mid is not None:
        mid = np.asarray(mid, np.float64)
        if o.which == "conv1":
            assert np.array_equal(mid, o.want_mid)
        else:
            worst = max(worst, er.worst_ratio(np.abs(mid - o.want_mid), o.bound_mid))
    return worst


def late_selector_run(rng, B, HW, which):
    """The selector block as the LAST block of a 3-block run whose first two blocks are exact integers: its input is the known
    integer map of block 1, its parameters ride at conv index 4 / 5 -> (run operands, selector block)."""
    run = exact_stage_run_f16(rng, B, HW, 3, 2)
    blk = selector_block(rng, HW, which, run.outs[1])
    run.w[4:6] = blk.w
    run.prm[4:6] = blk.prm
    return run, blk


def selector_cases(HW, which, B=3):
    """The cases of the selector pins: (name, x of the run, w, prm, selector block, conv index of the block's first conv) - the
    block alone (a selecting second conv twice: even, then odd channels of x zero) and as the last of three."""
    out = []
    for zero in (("even", "odd") if which == "conv2" else ("none",)):
        rng = np.random.default_rng(selector_seed(HW, which, zero))
        x = selector_input(rng, B, HW, zero)
        blk = selector_block(rng, HW, which, x)
        out.append((f"block 0, zero channels {zero}", x, blk.w, blk.prm, blk, 0))
    run, blk = late_selector_run(np.random.default_rng(selector_seed(HW, which, "late")), B, HW, which)
    out.append(("last of 3", run.x, run.w, run.prm, blk, 4))
    return out


# ---------------------------------------------------------------- float operands of a run at the network's depth
def float_run_operands(HW, nblocks, B, seed):
    """torch tensors: x [B][HW][HW][C] f16, w [2 n][C][9 C] f16, prm [2 n][10][C] f32, drawn as test_stage14_kernel_vs_torch draws
    them but with conv2 scaled by (0.02 / K)^0.5, so that the map's variance grows by ~2 % a block and stays O(1) over 29 blocks."""
    C, K = GEOM[HW].C, 9 * GEOM[HW].C
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, HW, HW, C), generator=g).to(torch.float16)
    w = torch.randn((2 * nblocks, C, K), generator=g)
    w[0::2] *= (2.0 / K) ** 0.5
    w[1::2] *= (0.02 / K) ** 0.5
    prm = torch.empty((2 * nblocks, 10, C))
    prm[0::2, :9] = torch.randn((nblocks, 9, C), generator=g) * 0.3
    prm[0::2, 9] = torch.rand((nblocks, C), generator=g) * 0.5
    prm[1::2, :9] = (torch.randn((nblocks, 1, C), generator=g) * 0.1).expand(nblocks, 9, C)
    prm[1::2, 9] = 1.0
    return x, w.to(torch.float16), prm


# ---------------------------------------------------------------- float32 emulation with planted faults
def _conv_f32(h, w):
    B, H, W, C = h.shape
    w4 = torch.from_numpy(np.ascontiguousarray(w.astype(np.float32).reshape(-1, 3, 3, C))).permute(0, 3, 1, 2)
    return F.conv2d(er._nchw(h.astype(np.float32)), w4, None, 1, 1).permute(0, 2, 3, 1).numpy()


def _to_f16(v, trunc):
    v = np.asarray(v, np.float32)
    if not trunc:
        return v.astype(np.float16)
    r = v.astype(np.float16)
    over = np.abs(r.astype(np.float32)) > np.abs(v)                        # rounded away from zero: one step back
    return np.where(over, np.nextafter(r, np.float16(0)), r).astype(np.float16)


def emulate_stage_run(x, w, prm, HW, fault=None, at=None, prefill=np.nan):
    """A stage run in float32 (f16 maps, f32 products, sums, bias, PReLU, residual; the order of the sums is the BLAS's: the exact
    cases do not depend on it) -> (y, last mid) as float16.  `prefill` stands in for a NaN-filled buffer.  Faults, planted at
    conv `at` where one is named (default: every conv the fault can apply to):
      "prm_prev"       conv j >= 1 uses conv j - 1's parameter rows
      "res_from_x"     block b >= 1 takes its residual from the run's input
      "in_from_x"      block b >= 1 reads its input from the run's input (the residual stays right)
      "first_slot"     conv j >= 1 multiplies its first K step by conv j - 1's first weight slot
      "drop_last"      conv j loses its last K step
      "halo15"         28x28: output row 13 of conv j >= 2 reads input row 14 as the buffer held it before conv j - 1 stored
      "half_unwritten" 28x28: rows 14 .. 27 of the last conv are not written (the buffer keeps the block's input)
      "slope_prev", "bias_prev"   the slope / the bias classes of channel c - 1
      "border_192"     14x14: pixels 192 .. 195 take the border class of the column to their left
      "trunc"          f32 -> f16 by truncation
      "mid_unrounded"  the second conv reads the first conv's f32 values"""
    x = np.asarray(x, np.float64)
    n, step = len(w), step_of_column(HW)
    cls = class_map(HW)
    hit = lambda j: at is None or at == j
    h = x
    mid = np.full(x.shape, prefill)
    bufs = {0: None, 1: None}                     # what conv j's INPUT buffer held before conv j - 1 stored into it
    for j in range(n):
        b, second = j // 2, j % 2 == 1
        wj = w[j].copy()
        if fault == "first_slot" and j >= 1 and hit(j):
            wj[:, step == 0] = w[j - 1][:, step == 0]
        if fault == "drop_last" and hit(j):
            wj[:, step == step.max()] = 0.0
        p = prm[j - 1] if fault == "prm_prev" and j >= 1 and hit(j) else prm[j]
        bias, slope = p[:9].copy(), p[9].copy()
        if fault == "slope_prev" and hit(j):
            slope = np.roll(slope, 1)
        if fault == "bias_prev" and hit(j):
            bias = np.roll(bias, 1, 1)
        src = mid_in if second else h
        if fault == "in_from_x" and not second and b >= 1 and hit(j):
            src = x
        v = _conv_f32(src, wj)
        if fault == "halo15" and j >= 2 and hit(j):
            stale = src.copy()
            stale[:, 14] = bufs[j % 2][:, 14]
            v[:, 13] = _conv_f32(stale, wj)[:, 13]
        c = cls.copy()
        if fault == "border_192" and HW == 14 and hit(j):
            c[13, 10:] = cls[13, 9:13]
        v = v + bias.astype(np.float32)[c][None]
        if not second:
            v = np.where(v > 0, v, v * slope.astype(np.float32)).astype(np.float32)
        else:
            res = x if fault == "res_from_x" and b >= 1 and hit(j) else h
            v = v + res.astype(np.float32)
        out16 = _to_f16(v, fault == "trunc" and hit(j))
        out = out16.astype(np.float64)
        if not second:
            bufs[1] = mid.copy()                  # the mid buffer before this store: conv j + 1's stale view
            mid = out
            mid_in = v.astype(np.float64) if fault == "mid_unrounded" and hit(j) else out
        else:
            bufs[0] = h.copy()                    # the x buffer before this store
            if fault == "half_unwritten" and j == n - 1:
                out = out.copy()
                out[:, 14:] = h[:, 14:]
            h = out
    return h.astype(np.float16), mid.astype(np.float16)
