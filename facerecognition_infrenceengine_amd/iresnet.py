"""ArcFace IResNet embed network on the HIP conv kernels.

Stands in for the recognition half of ``FaceAnalysis.get`` / ``face.normed_embedding``
(/root/reference/infrenceServer.py:528,532).  Host side = weight folding + launch plan;
all arithmetic runs in libfrhip.so (``fr_conv_nhwc_f16``, ``fr_fc_reduce_l2norm``).

Folding (inference BN):  s = gamma / sqrt(var + eps),  t = beta - mean * s.
  block:  y = bn3(conv2(prelu(bn2(conv1(bn1(x)))))) + shortcut(x)
  conv1':  w = s2[co] * w1 * s1[ci];  the bn1 shift t1 cannot be a plain bias because the
           zero padding is applied AFTER bn1, so it becomes a border-class bias
           bias9[rc][cc][co] = t2[co] + s2[co] * sum_{valid taps} sum_ci w1 * t1[ci]
           (exact; 9 classes = top/mid/bottom x left/mid/right), epilogue PReLU.
  conv2':  w = s3[co] * w2, bias t3, epilogue += shortcut (f16 residual stream).
  shortcut (first block of a stage): 1x1/s2 conv with sd folded, bias td.
  tail:    bn2 -> flatten(NCHW) -> fc -> features(BN1d) folds into one 25088->512 GEMM
           (columns permuted to NHWC order), run split-K on the same MFMA kernel.
"""
import ctypes
import functools
import logging
import threading
import types
from collections import namedtuple

import torch

from . import _lib
from .weights import IRESNET_LAYERS, IRESNET_WIDTHS

BN_EPS = 1e-5
FC_SPLITK = 28
# up to this many faces the 3x3 convs run split along K (see IResNetHIP._small_batch_splitk)
SMALL_BATCH = 48      # measured crossover: 32 faces 2.7 vs 3.3 ms, 64 faces 4.6 vs 3.7 ms
# up to this many faces the 3x3 / stride-1 convs with >= 128 input channels run split along K INSIDE a workgroup, one launch
# per conv (fr_conv_inblock_f16) instead of the partials launch + fr_conv_splitk_epilogue (see IResNetHIP._inblock)
INBLOCK_BATCH = 8      # measured (tools/bench_inblock.py, forward ms): 1 face 0.89 vs 1.30, 2: 0.95 / 1.41, 4: 1.23 / 1.65, 5: 1.25 / 1.78,
                       # 6: 1.82 / 1.88, 8: 1.85 / 2.19, 12: 2.94 / 2.11 (one, two or four pixel tiles per workgroup by the workgroup count)
# up to this many faces (single frames) every K slice is at most 3 K steps long: a slice's steps are dependent HBM
# round trips (the weights are cold: 130 MB per forward), so a launch takes ~1.2 us per step + ~3 us
LOW_BATCH = 8
# single-frame plans (4 x 12.8 MB of activations + ~40 MB of split-K scratch per HIP stream) are kept for this many streams
MAX_PLAN_STREAMS = 8
# from this many faces up the stride-1 blocks of the 14x14 stage run as ONE launch with the image resident in LDS
# (fr_conv_stage14_f16: one workgroup per image, one image per CU); below, the per-layer path fills the CUs better
# (measured r100 forward ALONE, stage / layer by layer: 128 faces 4.62 / 4.44 ms, 160: 5.16 / 5.74, 192: 5.49 / 6.17, 256: 6.8 / 7.6).
# Taken from 128 faces all the same: in a pipeline the CUs a 128-workgroup launch leaves free are the detector's - config C3 (8 x 4K
# frames, 128 faces per step; tools/ab_c3_stage_min.py, same box): 19 640 - 19 820 faces/s with the threshold at 144, 20 430 - 20 550 at 128
STAGE14_MIN_BATCH = 128
# fr_conv_walk64_f16: one workgroup per (face, 64-cout group), a face's walk cut into 2 / 4 / 8 pieces while that fills <= 256
# CUs.  Measured (tools/bench_walk64_crossover.py, r100 forward): it beats the per-tile kernel at 64 / 96 / 128 faces (cut walks) and
# from 160 up; between 129 and 159 faces an uncut walk leaves 40 % of the CUs idle and loses by 1 %.
WALK64_SKIP = range(129, 160)
STAGE28_MIN_BATCH = 144     # fr_conv_stage28_f16: one workgroup per face, as the 14x14 stage kernel


def _bn_fold(st, prefix, n, conv=None):
    """(scale, shift) of an inference BatchNorm; the identity when the state dict has no such BN (an exporter folded
    it into the conv before it: onnx_import.py).  ``conv``: name of the conv feeding it - its bias, if any, joins
    the shift."""
    if prefix + ".weight" in st:
        s = st[prefix + ".weight"].double() / torch.sqrt(st[prefix + ".running_var"].double() + BN_EPS)
        t = st[prefix + ".bias"].double() - st[prefix + ".running_mean"].double() * s
    else:
        s, t = torch.ones(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    if conv is not None and conv + ".bias" in st:
        t = t + s * st[conv + ".bias"].double()
    return s, t


def _pack_w(w):
    """[Cout,Cin,KH,KW] -> [Cout, KH*KW*Cin] f16 (K contiguous, tap-major)."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).to(torch.float16).contiguous()


F8_MAX = 448.0                 # largest finite OCP e4m3 value
F8_MARGIN = 1.5                # activation scale head-room over the calibration batch's absmax


def f8_eligible(c, H):
    """Layers fr_conv_nhwc_f8 takes: 3x3 / stride 1 at 28x28 and 14x14 with 128-multiple channels (78 % of r100)."""
    return c.k == 3 and c.stride == 1 and H in (14, 28) and c.cin % 128 == 0 and c.cout % 128 == 0


def round_e4m3(t):
    """Round a float tensor to the nearest OCP e4m3 VALUE (ties to even, saturating at +-448; subnormal step 2^-9) in
    plain float arithmetic - device- and dtype-independent (the GPTQ loop runs in f64 on the GPU)."""
    a = t.abs().clamp(max=F8_MAX)
    _, e = torch.frexp(a.clamp_min(2.0 ** -9))                    # a = m * 2^e, m in [0.5, 1)
    step = torch.ldexp(torch.ones_like(a), (e - 1).clamp_min(-6) - 3)
    return torch.copysign(torch.round(a / step) * step, t)


def gptq_factor(hm, damp=0.01):
    """Upper Cholesky factor U of the inverse of the (damped) second-moment matrix hm [K,K], f64."""
    K = hm.shape[0]
    hm = hm.double() + damp * hm.diagonal().mean().double() * torch.eye(K, dtype=torch.float64, device=hm.device)
    return torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(hm)), upper=True).contiguous()


def gptq_e4m3_torch(w, hm, sw, block=128, damp=0.01):
    """GPTQ rounding (Frantar et al. 2022) of folded weights ``w`` [Cout, K] to the per-row e4m3 grid ``sw[co] * e4m3``
    given the second-moment matrix ``hm`` [K, K] of the conv's (centred) input patches, K order as ``w``'s columns:
    columns are rounded one after the other and each column's rounding error is pushed onto the columns still to
    come along the inverse Hessian, so that the OUTPUT error ||(W - Wq) X|| - not the weight error - is what is
    minimised.  Returns the rounded weights divided by sw (values on the e4m3 grid), f32.  Plain-torch form (blocked):
    the cross-check of fr_gptq_round_e4m3, which the product uses."""
    W = w.double().clone()
    K = W.shape[1]
    U = gptq_factor(hm, damp)
    sw = sw.double()
    Q = torch.empty_like(W)
    for i0 in range(0, K, block):
        i1 = min(i0 + block, K)
        W1, U1 = W[:, i0:i1].clone(), U[i0:i1, i0:i1]
        E1 = torch.empty_like(W1)
        for j in range(i1 - i0):
            q = round_e4m3(W1[:, j] / sw)
            Q[:, i0 + j] = q
            err = (W1[:, j] - q * sw) / U1[j, j]
            W1[:, j:] -= err[:, None] * U1[j, j:][None, :]
            E1[:, j] = err
        if i1 < K:
            W[:, i1:] -= E1 @ U[i0:i1, i1:]
    return Q.to(torch.float32)


def quantise_weights_f8(w):
    """[Cout, K] (f64/f32, folded) -> (uint8 e4m3 bytes [Cout, K], per-output-channel scale sw f32 [Cout]):
    w8 = fp8(w / sw), sw = max|w[co]| / 448."""
    w = w.to(torch.float32)
    sw = (w.abs().amax(dim=1) / F8_MAX).clamp_min(1e-30)
    q = (w / sw[:, None]).clamp(-F8_MAX, F8_MAX).to(torch.float8_e4m3fn)
    return q.view(torch.uint8).contiguous(), sw


def border_bias9(base, tap):
    """base ([Cout], or [3,3,Cout] by border class) + per border class (top / mid / bottom x left / mid / right) the sum of
    ``tap`` [Cout,3,3] over the taps that fall inside the image -> f64 [3,3,Cout]"""
    valid = {0: [1, 2], 1: [0, 1, 2], 2: [0, 1]}
    base = base.expand(3, 3, tap.shape[0])
    b9 = torch.empty(3, 3, tap.shape[0], dtype=torch.float64)
    for rc in range(3):
        for cc in range(3):
            b9[rc, cc] = base[rc, cc] + tap[:, valid[rc]][:, :, valid[cc]].sum((1, 2))
    return b9


def fold_iresnet(state, arch="r100"):
    """Inference-BN folding of an IResNet state dict in f64 on the host (module docstring).  Pure: no device, no
    library - ``IResNetHIP`` packs the result for the kernels, ``tools/fp8_sim.py`` replays it on the CPU.
    Returns {"stem": conv, "blocks": [{"c1", "c2", "sc"}], "fc_w" [512, 49*512] (NHWC K order), "fc_bias"}; a conv is
    {"w" f64 [Cout,Cin,KH,KW] (stem: packed [64,128]), "bias" (c1: bias9 flattened [9*Cout]), "slope", "cin", "cout",
    "stride"}."""
    layers = IRESNET_LAYERS[arch]
    st = {k: torch.as_tensor(v).detach().to("cpu") for k, v in state.items()}
    # stem: conv1 + bn1 + prelu, packed K = 16 taps x 8 channels
    s, t = _bn_fold(st, "bn1", 64, conv="conv1")
    w = st["conv1.weight"].double() * s[:, None, None, None]
    wp = torch.zeros(64, 16, 8, dtype=torch.float64)
    wp[:, :9, :3] = w.permute(0, 2, 3, 1).reshape(64, 9, 3)
    out = {"stem": {"w": wp.reshape(64, 128), "w4": w, "bias": t, "slope": st["prelu.weight"], "cin": 8, "cout": 64,
                    "stride": 1}, "blocks": []}
    cin = 64
    for li, (n, cout) in enumerate(zip(layers, IRESNET_WIDTHS), start=1):
        for bi in range(n):
            p = f"layer{li}.{bi}"
            stride = 2 if bi == 0 else 1
            s1, t1 = _bn_fold(st, p + ".bn1", cin)
            s2, t2 = _bn_fold(st, p + ".bn2", cout, conv=p + ".conv1")
            s3, t3 = _bn_fold(st, p + ".bn3", cout, conv=p + ".conv2")
            w1 = st[p + ".conv1.weight"].double()
            w1f = w1 * s2[:, None, None, None] * s1[None, :, None, None]
            tap = (w1 * t1[None, :, None, None]).sum(1) * s2[:, None, None]      # [co,kh,kw]
            c1 = {"w": w1f, "bias": border_bias9(t2, tap).reshape(9 * cout), "slope": st[p + ".prelu.weight"], "cin": cin,
                  "cout": cout, "stride": 1}
            w2f = st[p + ".conv2.weight"].double() * s3[:, None, None, None]
            c2 = {"w": w2f, "bias": t3, "slope": None, "cin": cout, "cout": cout, "stride": stride}
            sc = None
            if bi == 0:
                sd, td = _bn_fold(st, p + ".downsample.1", cout, conv=p + ".downsample.0")
                wd = st[p + ".downsample.0.weight"].double() * sd[:, None, None, None]
                sc = {"w": wd, "bias": td, "slope": None, "cin": cin, "cout": cout, "stride": stride}
            out["blocks"].append({"c1": c1, "c2": c2, "sc": sc})
            cin = cout
    # tail
    sb, tb = _bn_fold(st, "bn2", 512)
    sf, tf = _bn_fold(st, "features", 512)
    W = st["fc.weight"].double().reshape(512, 512, 49)                   # [o, c, hw]
    out["fc_bias"] = sf * (st["fc.bias"].double() + (W * tb[None, :, None]).sum((1, 2))) + tf
    out["fc_w"] = (W * sb[None, :, None] * sf[:, None, None]).permute(0, 2, 1).reshape(512, 49 * 512)   # NHWC K order
    return out


# ---- the route: which kernel every conv of the net takes at a batch size (the table of the modes: DESIGN.md section 4.2).
# Pure: shapes and flags in, steps out - no weights, no device, no library.
PLAIN, SPLITK, INBLOCK, WALK64 = "plain", "splitk", "inblock", "walk64"    # one f16 conv: fr_conv_nhwc_f16 / partials + epilogue / ...
STAGE28, STAGE14, STAGE14_F8, CONV_F8, QUANTISE = "stage28", "stage14", "stage14_f8", "conv_f8", "quantise"    # a run of blocks; fp8
_SEQ_KIND = {PLAIN: 0, SPLITK: 1, INBLOCK: 2}    # fr_conv_step.kind of the routes fr_conv_sequence replays


# Shape of one conv (no weights).  key: "stem", (block, "c1" | "c2" | "sc"), (block, "fz") = the stage-entry c2 with its block's
# 1x1 shortcut conv as extra K rows, "fc".  H: input map (H = W).  fuses: a c2 whose block has the "fz" form.  walk64:
# fr_conv_walk64_f16 takes it (3x3 / s1, 64 input channels: 112x112, 56x56).  c2: channels of the second input that enters
# through a 1x1 tap (fr_conv_args.x2), "fz" only.  flops: algorithmic, per face (stem: 3 real channels).
ConvRec = namedtuple("ConvRec", "key k stride pad cin cout bias_mode H fuses walk64 c2 flops")
# convs: key -> ConvRec in network order; run28 / run14: longest_run of the 128- / 256-wide stride-1 blocks; flops: per face
ConvTable = namedtuple("ConvTable", "arch convs nblocks run28 run14 flops_per_face")


def longest_run(convs, nblocks, width):
    """(first, n) of the longest run of consecutive stride-1 width -> width blocks (r100: 128 -> blocks 4..15 behind stage
    2's entry block, 256 -> blocks 17..45 behind stage 3's); None when shorter than two blocks."""
    run, best = [], []
    for i in range(nblocks):
        c1, c2 = convs[i, "c1"], convs[i, "c2"]
        ok = (i, "sc") not in convs and c1.cin == width and c1.cout == width and c2.stride == 1 and c2.cout == width
        run = run + [i] if ok else []
        if len(run) > len(best):
            best = run
    return (best[0], len(best)) if len(best) >= 2 else None


@functools.lru_cache(maxsize=None)
def conv_table(arch):
    """The static shape table of an IResNet: stem, then per block c1, c2, sc (and fz), then the FC as a 1x1 conv over a
    1x1 image with Cin = 25088."""
    R = ConvRec
    convs = {"stem": R("stem", 3, 1, 1, 8, 64, 0, 112, False, False, 0, 2 * 112 * 112 * 27 * 64)}
    cin, hw, bi = 64, 112, 0
    for n, cout in zip(IRESNET_LAYERS[arch], IRESNET_WIDTHS):
        for j in range(n):
            stride = 2 if j == 0 else 1
            ho = hw // stride
            fuses = j == 0 and cin % 64 == 0 and cout % 64 == 0
            convs[bi, "c1"] = R((bi, "c1"), 3, 1, 1, cin, cout, 1, hw, False, cin == 64 and cout % 64 == 0, 0, 2 * hw * hw * cin * cout * 9)
            convs[bi, "c2"] = R((bi, "c2"), 3, stride, 1, cout, cout, 0, hw, fuses, stride == 1 and cout == 64, 0, 2 * ho * ho * cout * cout * 9)
            if j == 0:
                convs[bi, "sc"] = R((bi, "sc"), 1, stride, 0, cin, cout, 0, hw, False, False, 0, 2 * ho * ho * cin * cout)
            if fuses:
                convs[bi, "fz"] = R((bi, "fz"), 3, stride, 1, cout, cout, 0, hw, False, False, cin, 2 * ho * ho * cout * (9 * cout + cin))
            cin, hw, bi = cout, ho, bi + 1
    convs["fc"] = R("fc", 1, 1, 0, 25088, 512, 0, 1, False, False, 0, 2 * 25088 * 512)
    flops = sum(c.flops for c in convs.values() if not c.c2)                # "fz" counts as its c2 and sc
    return ConvTable(arch, convs, bi, longest_run(convs, bi, 128), longest_run(convs, bi, 256), flops)


# Everything but the batch size that the route decision reads.  fp8: keys of the convs that carry an fp8 form (empty: the f16
# net); stage14_f8: the 14x14 run has its fp8 stream (fr_conv_stage14_f8).
# A profiled, tapped or calibrating forward takes the plain path at small batch sizes ON PURPOSE: none of them replays the
# prepared sequence (one C call has no per-conv events, taps or statistics); a profiled one also runs neither split-K form -
# one launch per conv on fr_conv_nhwc_f16, so bench.py's instrumented pass names one kernel per conv - and a tapped or
# calibrating one runs no stage kernel (the maps inside a run never reach HBM).
RouteMode = namedtuple("RouteMode", "small_batch low_batch inblock_batch use_stage14 use_stage28 use_walk64 fuse_shortcut fp8 "
                       "stage14_f8 profiled tapped calibrating",
                       defaults=(SMALL_BATCH, LOW_BATCH, INBLOCK_BATCH, True, True, True, True, frozenset(), False, False, False, False))
# One launch (SPLITK: two).  conv: key of its conv; of a stage run (first block, blocks); of QUANTISE the conv that reads the codes.
# slices: K slices (SPLITK, the FC), else 1.  x2: the block input enters as second input (fr_conv_args.x2).  src: "x" | "h" | "mid",
# the tensor it reads (CONV_F8, STAGE14_F8: that tensor's fp8 codes); dst: "h" | "mid" | "short" | "emb" (QUANTISE: the codes of src);
# res: None | "h" | "short", the residual its epilogue adds.  want16 / nxt (CONV_F8): the output is written as f16 and / or as fp8
# codes centred and scaled for the consumer nxt.  variant: the kernel its launch ends in (None: no profiled forward takes the route).
Step = namedtuple("Step", "route conv H W Ho Wo slices x2 src dst res want16 nxt tap variant flops")


def step_variant(route, c, H):
    """Mirror of the C dispatch (fr_conv_nhwc_f16 -> fr_conv_halo_try: halo kernel for the 3x3 / s1 body convs).
    bench.py and profiles/r05_pmc_traffic.json key on these strings."""
    if route in (STAGE28, STAGE14, STAGE14_F8):
        return {STAGE28: "conv_stage28_kernel", STAGE14: "conv_stage14_kernel<0, 0>", STAGE14_F8: "conv_stage14_f8_kernel<0>"}[route]
    if route == CONV_F8:
        return "conv_halo_kernel<2, 13, %d, 1, 4, false, true, 4, true, 8, 0>" % (256 if H == 14 else 320)
    if route == WALK64:
        return "conv_walk64_kernel %dx%d -> %d" % (H, H, c.cout)
    if route != PLAIN:
        return None
    if c.k == 3 and c.stride == 1 and c.cin % 64 == 0:
        if H in (7, 14, 28) and c.cout % 128 == 0:       # lean variant: BN = 128, two blocks per CU
            return "conv_halo_kernel<2, 13, %d, 1, 4, false, true, 4, false, 8, 0>" % {7: 384, 14: 256, 28: 320}[H]
        if H == 56 and c.cin == 64:
            return "conv_halo_kernel<1, 14, 384, 1, 4, false, false, 4, false, 8, 0>"
        if H == 112 and c.cin == 64 and c.cout == 64:
            return "conv_halo_kernel<1, 14, 512, 1, 4, false, false, 4, false, 8, 0>"
    return "conv_stem_kernel<112>" if c.cin == 8 else "conv_mfma_kernel<%d, false, true>" % (2 if c.cout % 128 == 0 else 1)


def step_cost(table, route, conv, B):
    """(profile variant, algorithmic FLOPs) of a step at B faces"""
    run = route in (STAGE28, STAGE14, STAGE14_F8)                     # n blocks of two equal convs
    c = table.convs[(conv[0], "c1") if run else conv]
    return step_variant(route, c, c.H), float(B * c.flops * (2 * conv[1] if run else 1))


def conv_step(table, B, mode, rules, key, src, dst, res=None, x2=False, tap=None):
    """The route of ONE f16 conv at B faces.  ``rules``: whose ``_small_batch_splitk`` / ``_inblock`` decide."""
    c = table.convs[key]
    Ho = (c.H + 2 * c.pad - c.k) // c.stride + 1
    route, slices = PLAIN, 1
    if key == "fc":
        slices = FC_SPLITK                       # split-K into f32 partials that fr_fc_reduce_l2norm sums
    elif not mode.profiled:
        if not x2 and rules._inblock(c, B):
            route = INBLOCK
        else:
            slices = rules._small_batch_splitk(c, B)
            route = SPLITK if slices > 1 else PLAIN
    if route == PLAIN and c.walk64 and mode.use_walk64 and not x2 and B > mode.small_batch and B not in WALK64_SKIP:
        route = WALK64
    return Step(route, key, c.H, c.H, Ho, Ho, slices, x2, src, dst, res, True, None, tap, *step_cost(table, route, key, B))


def embed_route(table, B, mode, rules=None):
    """The launches of a B-face forward, in order: an immutable tuple of Step, the FC last.  ``rules``: the network whose
    ``_small_batch_splitk`` / ``_inblock`` decide (default: IResNetHIP's, over the mode's own batch sizes)."""
    if rules is None:
        rules = types.SimpleNamespace(**{n: functools.partial(getattr(IResNetHIP, n), mode) for n in ("_small_batch_splitk", "_inblock")})
    cv, fp8 = table.convs, mode.fp8
    conv = functools.partial(conv_step, table, B, mode, rules)

    def special(route, key, H, src, dst, res=None, want16=True, nxt=None, tap=None):
        cost = (None, 0.0) if route == QUANTISE else step_cost(table, route, key, B)
        return Step(route, key, H, H, H, H, 1, False, src, dst, res, want16, nxt, tap, *cost)

    staged = not (mode.tapped or mode.calibrating)
    run14 = table.run14 if staged and mode.use_stage14 and B >= STAGE14_MIN_BATCH and (not fp8 or mode.stage14_f8) else None
    run28 = None
    if staged and mode.use_stage28 and B >= STAGE28_MIN_BATCH and table.run28 is not None:
        # the 28x28 run: its leading blocks that hold no fp8 conv (enable_fp8 "accurate": all but the last two)
        first, n = table.run28
        lead = next((i - first for i in range(first, first + n) if (i, "c1") in fp8 or (i, "c2") in fp8), n)
        run28 = (first, lead) if lead >= 2 else None
    steps = [conv("stem", "x", "h", tap="stem")]
    bi, li = 0, 0
    h8 = False                                   # h has an fp8 copy, scaled for the conv that will read it
    while bi < table.nblocks:
        k1, k2, ksc, n1 = (bi, "c1"), (bi, "c2"), (bi, "sc"), (bi + 1, "c1")
        f1, f2, entry, H = k1 in fp8, k2 in fp8, ksc in cv, cv[k1].H
        run = next((r for r in (run28, run14) if r is not None and bi == r[0]), None)
        if run is not None:                      # all its blocks in one launch
            if run is run14 and fp8:
                if not h8:
                    steps.append(special(QUANTISE, k1, H, "h", "h"))
                h8 = False                       # the run's consumer quantises the f16 output itself
            steps.append(special(STAGE28 if run is run28 else STAGE14_F8 if fp8 else STAGE14, run, H, "h", "h"))
            bi += run[1]
            continue
        li += 1 if entry else 0
        tap = "layer%d.0.mid" % li if entry else None
        if f1:
            if not h8:
                steps.append(special(QUANTISE, k1, H, "h", "h"))
            steps.append(special(CONV_F8, k1, H, "h", "mid", want16=not f2 or mode.tapped, nxt=k2 if f2 else None, tap=tap))
        else:
            steps.append(conv(k1, "h", "mid", tap=tap))
        fz = mode.fuse_shortcut and not f2 and cv[k2].fuses
        if entry and not fz:
            steps.append(conv(ksc, "h", "short"))
        res = "short" if entry else "h"
        if fz:                                   # stride-2 conv + 1x1 shortcut of the block input as one implicit GEMM
            steps.append(conv((bi, "fz"), "mid", "h", x2=True))
        elif f2:
            if not f1:
                steps.append(special(QUANTISE, k2, H, "mid", "mid"))
            steps.append(special(CONV_F8, k2, H, "mid", "h", res, nxt=n1 if n1 in fp8 else None))
        else:
            steps.append(conv(k2, "mid", "h", res))
        h8 = f2 and not fz and n1 in fp8
        bi += 1
    steps.append(conv("fc", "h", "emb"))
    return tuple(steps)


class _Conv:
    __slots__ = ("key", "w", "bias", "slope", "cin", "cout", "k", "stride", "pad", "bias_mode", "w32", "w8", "sw", "sx",
                 "oscale", "mu", "bias8", "c2", "w64")

    def __init__(self, rec, w, bias, slope, device):
        self.key, self.k, self.stride, self.pad, self.cin, self.cout, self.bias_mode = rec[:7]
        self.c2 = rec.c2             # channels of a second input that enters through a 1x1 tap (fr_conv_args.x2): fused shortcut
        self.w = w.to(device)
        self.w32 = self.w8 = self.sw = self.sx = self.oscale = self.mu = self.bias8 = None      # fp8 form, filled by IResNetHIP.enable_fp8
        self.bias = None if bias is None else bias.to(torch.float32).contiguous().to(device)
        self.slope = None if slope is None else slope.to(torch.float32).contiguous().to(device)
        self.w64 = None              # fr_conv_walk64_pack'ed weights (3x3 / s1, 64 input channels), IResNetHIP._pack_walk64


class IResNetHIP:
    """Folded IResNet resident on one GPU.  ``forward`` takes the packed stem input
    f16 [B,112,112,8] (RGB in channels 0..2, (x-127.5)/127.5, rest zero) produced by
    ``fr_warp_affine_5pt`` and returns (embedding, normed_embedding) f32 [B,512] on device."""

    def __init__(self, state, arch="r100", device="cuda:0", max_chunk=256, small_batch=SMALL_BATCH, low_batch=LOW_BATCH,
                 inblock_batch=INBLOCK_BATCH):
        """``small_batch`` / ``low_batch``: batch-size modes of the split-K single-frame path (module constants above;
        arguments, not environment variables: the product reads no environment)."""
        _lib.require_gpu()
        self.small_batch, self.low_batch, self.inblock_batch = int(small_batch), int(low_batch), int(inblock_batch)
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.arch = arch
        self.max_chunk = max_chunk
        dev = self.device
        f = fold_iresnet(state, arch)
        self.table = conv_table(arch)
        rec, cv = self.table.convs, {}
        self._convs = cv                                         # the table's keys -> the convs
        self.stem = cv["stem"] = _Conv(rec["stem"], f["stem"]["w"].to(torch.float16).contiguous(), f["stem"]["bias"], f["stem"]["slope"], dev)
        self.blocks = []
        # A stage-entry block's 1x1 / stride-2 shortcut conv joins its stride-2 3x3 conv as extra K rows of ONE implicit GEMM
        # (f32 accumulation, biases summed): no shortcut launch, no f16 shortcut map written and read back.
        self.fused_sc = {}
        self.fuse_shortcut = True    # False: shortcut conv as its own launch (A/B, tests)
        for i, b in enumerate(f["blocks"]):
            d1, d2, ds = b["c1"], b["c2"], b["sc"]
            c1 = cv[i, "c1"] = _Conv(rec[i, "c1"], _pack_w(d1["w"]), d1["bias"], d1["slope"], dev)
            c2 = cv[i, "c2"] = _Conv(rec[i, "c2"], _pack_w(d2["w"]), d2["bias"], None, dev)
            if d1["cin"] % 128 == 0 and d1["cout"] % 128 == 0:        # folded f32 weights kept on the host for enable_fp8()
                c1.w32 = d1["w"].permute(0, 2, 3, 1).reshape(d1["cout"], -1).to(torch.float32)
            if d2["stride"] == 1 and d2["cout"] % 128 == 0:
                c2.w32 = d2["w"].permute(0, 2, 3, 1).reshape(d2["cout"], -1).to(torch.float32)
            sc = None
            if ds is not None:
                sc = cv[i, "sc"] = _Conv(rec[i, "sc"], _pack_w(ds["w"]), ds["bias"], None, dev)
            if (i, "fz") in rec:
                w = torch.cat([c2.w.reshape(c2.cout, -1), sc.w.reshape(sc.cout, -1)], 1).contiguous()
                self.fused_sc[i] = cv[i, "fz"] = _Conv(rec[i, "fz"], w, c2.bias + sc.bias, None, dev)
            self.blocks.append((c1, c2, sc))
        # the FC as a 1x1 conv over a 1x1 image with Cin = 25088, split-K -> f32 partials
        self.fc = cv["fc"] = _Conv(rec["fc"], f["fc_w"].to(torch.float16).contiguous(), None, None, dev)
        self.fc_bias = f["fc_bias"].to(torch.float32).contiguous().to(dev)
        self.stage14 = self._pack_stage(self.table.run14, 14)    # the 14x14 stage's stride-1 blocks as one launch (fr_conv_stage14_f16)
        self.stage28 = self._pack_stage(self.table.run28, 28)    # the 28x28 stage's (fr_conv_stage28_f16)
        self._pack_walk64()
        self.flops_per_face = self.table.flops_per_face
        self._routes = {}            # (B, RouteMode) -> embed_route: the route is pure, the walk per forward is not free
        self._plans = {}             # (B, stream) -> prepared fr_conv_sequence of the single-frame forward
        self._plan_bufs = {}         # stream -> (4 activation buffers, split-K scratch) shared by that stream's plans
        self._plan_lock = threading.Lock()       # engines cloned with clone_with() share this network across threads
        self._plan_limit_logged = False
        self.profile = None          # bench.py: list collecting (kernel variant, flops, ev0, ev1) per conv launch
        self.fp8, self._fp8_keys = False, frozenset()    # enable_fp8(): eligible body convs (these keys) run on the fp8 matrix cores
        self.use_stage28 = self.use_stage14 = True      # False: that stage runs layer by layer whatever the batch (A/B, tests)
        self.stage14_f8 = None       # enable_fp8(): the run's fp8 form (fr_conv_stage14_f8)
        self._calib = None

    def _pack_stage(self, run, hw):
        """A stage run (``longest_run``) for its one-launch kernel: the weights of its convs as ONE pre-swizzled stream in kernel
        order + [10][width] f32 parameters per conv (nine border-class biases - a plain bias nine times - and the PReLU slope, 1.0 = none)."""
        if run is None:
            return None
        first, n = run
        width = self.blocks[first][0].cin
        pack = getattr(self.lib, "fr_conv_stage%d_pack" % hw)
        per = getattr(self.lib, "fr_conv_stage%d_weight_bytes" % hw)(1) // 2
        stream = torch.empty(2 * n * per, dtype=torch.float16, device=self.device)
        prm = torch.empty((2 * n, 10, width), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            for k, c in enumerate(c for b in self.blocks[first:first + n] for c in b[:2]):
                pack(_lib.ptr(c.w), _lib.ptr(stream[k * per:]), _lib.stream_ptr())
                prm[k, :9] = c.bias.reshape(9, width) if c.bias_mode == 1 else c.bias[None, :]
                prm[k, 9] = c.slope if c.slope is not None else 1.0
            torch.cuda.synchronize(self.device)
        return {"first": first, "n": n, "w": stream, "prm": prm.contiguous()}

    def _pack_walk64(self):
        """Weights of the 3x3 / s1 convs with 64 input channels (112x112, 56x56) in fr_conv_walk64_f16's stream order."""
        self.use_walk64 = True       # False: these convs on the per-tile halo kernel whatever the batch (A/B, tests)
        with torch.cuda.device(self.device):
            for key, c in self._convs.items():
                if self.table.convs[key].walk64:
                    c.w64 = torch.empty(self.lib.fr_conv_walk64_weight_bytes(c.cout) // 2, dtype=torch.float16, device=self.device)
                    self.lib.fr_conv_walk64_pack(_lib.ptr(c.w), _lib.ptr(c.w64), c.cout, _lib.stream_ptr())
            torch.cuda.synchronize(self.device)

    def _run_stage(self, s, h):
        """A STAGE28 / STAGE14 step -> its output; the 28x28 kernel works in place: ``h`` (the run's input, nobody else's) comes back."""
        st, fn = (self.stage28, self.lib.fr_conv_stage28_f16) if s.route == STAGE28 else (self.stage14, self.lib.fr_conv_stage14_f16)
        y = torch.empty_like(h)
        self._launch(fn, (_lib.ptr(h), _lib.ptr(y), _lib.ptr(st["w"]), _lib.ptr(st["prm"]), h.shape[0], s.conv[1], _lib.stream_ptr()),
                     s.variant, s.flops)
        return h if s.route == STAGE28 else y

    # ---- fp8 path (BASELINE config C5)
    def fp8_candidates(self):
        """[(conv, H)] of the layers fr_conv_nhwc_f8 takes, in network order."""
        sized = [(c, self.table.convs[c.key].H) for b in self.blocks for c in b[:2]]
        return [(c, hw) for c, hw in sized if c.w32 is not None and f8_eligible(c, hw)]

    def enable_fp8(self, calib_crops, select="accurate", centre=True, gptq=True):
        """Switch body convs to fr_conv_nhwc_f8 (3x3/s1 at 28x28 and 14x14: up to 82 % of the r100 FLOPs).

        e4m3 carries 3 mantissa bits: every fp8 conv adds rounding noise of ~3 % of its output's random part, from the
        weights and from the activations in equal shares, and the noise of the convs adds up in the residual stream
        (measured, tools/fp8_sim.py: 1 - cos of the embedding grows by ~4e-5 per fp8 conv, 3.4e-3 for all 84).  What
        this method does about it, from ONE f16 calibration forward of ``calib_crops`` (f16 [B,112,112,8]):
          * ``centre``: a conv's input is rounded as (x - mu[c]) / sx with mu the per-channel calibration mean; the
            exact term W.mu - which depends on the taps that fall inside the image - joins the 9-class border bias.
            |x - mu| < |x| on average and e4m3's error is relative: halves both noise shares.
          * ``gptq``: the weights are rounded column by column with error feedback along the inverse second-moment
            matrix of the (centred) input patches (``gptq_e4m3``), which removes most of the weight share.
          * ``select``: "accurate" (default) = every eligible 14x14 conv + the last four eligible 28x28 convs (61 % of
            the r100 FLOPs; 1 - cos < 1e-3, north_star's bound); "all" = every eligible conv (82 %; ~1.1e-3).
        Activation scales stay static per tensor: sx = 1.5 * absmax|x - mu| / 448 (e4m3 is a floating format: finer
        scale granularity buys nothing).  The residual stream, stem, stride-2 convs, 1x1 shortcuts, the 7x7 stage and
        the FC stay f16."""
        assert calib_crops.dtype == torch.float16 and calib_crops.shape[1:] == (112, 112, 8)
        cands = self.fp8_candidates()
        if select == "all":
            chosen = [c for c, _ in cands]
        elif select == "accurate":
            chosen = [c for c, hw in cands if hw == 14] + [c for c, hw in cands if hw == 28][-4:]
        else:
            chosen = [c for i, (c, _) in enumerate(cands) if select(i, len(cands))]
        self.fp8 = False
        for c, _ in cands:
            c.oscale = None
        self._calib = {"want": {id(c) for c in chosen}, "centre": centre, "gptq": gptq, "stats": {}}
        self.forward(calib_crops.contiguous())
        stats, self._calib = self._calib["stats"], None
        n = 0
        for c in chosen:
            st = stats.get(id(c))
            if st is None:
                continue
            c.sx = max(st["absmax"] * F8_MARGIN / F8_MAX, 1e-12)
            c.mu = st["mu"]
            w8, sw = quantise_weights_f8(c.w32)
            if st.get("wq") is not None:                  # GPTQ-rounded values on the same per-row grid
                w8 = st["wq"].cpu().to(torch.float8_e4m3fn).view(torch.uint8).contiguous()
            c.w8, c.sw = w8.to(self.device), sw.to(self.device)
            c.oscale = (c.sw * c.sx).contiguous()
            # exact W.mu through the zero padding: 9 border classes (c1's bias is one already; c2's plain bias widens)
            base = c.bias.double().cpu()
            tap = (c.w32.double().reshape(c.cout, 9, c.cin) * (c.mu.double().cpu()[None, None, :] if c.mu is not None else 0.0)).sum(2)
            b9 = border_bias9(base.reshape(3, 3, c.cout) if c.bias_mode == 1 else base, tap.reshape(c.cout, 3, 3))
            c.bias8 = b9.reshape(9 * c.cout).to(torch.float32).contiguous().to(self.device)
            n += 1
        self.fp8 = n > 0
        self._fp8_keys = frozenset(key for key, c in self._convs.items() if c.oscale is not None)
        self._pack_stage14_f8()
        return n

    def _pack_stage14_f8(self):
        """fp8 form of the 14x14 run (fr_conv_stage14_f8) when every conv of the run was switched to fp8: the e4m3 weights
        as one pre-swizzled stream + f32 [14][256] parameters per conv (oscale, 1 / oscale, nine border-class biases,
        PReLU slope, the NEXT conv's input centre mu and 1 / sx: a conv's epilogue writes its consumer's codes)."""
        self.stage14_f8 = None
        st = self.stage14
        if st is None or not self.fp8:
            return
        convs = [c for b in self.blocks[st["first"]:st["first"] + st["n"]] for c in b[:2]]
        if any(c.oscale is None or c.mu is None for c in convs):
            return
        after = self.blocks[st["first"] + st["n"]][0] if st["first"] + st["n"] < len(self.blocks) else None
        if after is not None and (after.oscale is None or after.cin != 256):
            after = None                                  # the run's consumer is not an fp8 conv: the last codes are unused
        per = self.lib.fr_conv_stage14_f8_weight_bytes(1)
        rows = self.lib.fr_conv_stage14_f8_param_floats() // 256
        stream = torch.empty(len(convs) * per, dtype=torch.uint8, device=self.device)
        prm = torch.zeros((len(convs), rows, 256), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            for k, c in enumerate(convs):
                self.lib.fr_conv_stage14_f8_pack(_lib.ptr(c.w8), _lib.ptr(stream[k * per:]), _lib.stream_ptr())
                nxt = convs[k + 1] if k + 1 < len(convs) else after
                prm[k, 0] = c.oscale
                prm[k, 1] = (1.0 / c.oscale.double()).to(torch.float32)
                prm[k, 2:11] = c.bias8.reshape(9, 256)
                prm[k, 11] = c.slope if c.slope is not None else 1.0
                if nxt is not None:
                    prm[k, 12] = nxt.mu
                    prm[k, 13, 0] = 1.0 / nxt.sx
                else:
                    prm[k, 13, 0] = 1.0
            torch.cuda.synchronize(self.device)
        self.stage14_f8 = {"w": stream, "prm": prm.contiguous()}

    def _run_stage14_f8(self, h, h8, B):
        st, f8 = self.stage14, self.stage14_f8
        y = torch.empty_like(h)
        args = (_lib.ptr(h8), _lib.ptr(h), _lib.ptr(y), _lib.ptr(f8["w"]), _lib.ptr(f8["prm"]), B, st["n"], _lib.stream_ptr())
        self._launch(self.lib.fr_conv_stage14_f8, args, *self._cost(STAGE14_F8, (st["first"], st["n"]), B))
        return y

    def _calib_observe(self, c, x, H):
        """calibration forward: statistics of the tensor ``x`` (f16 NHWC) an fp8 candidate reads"""
        cal = self._calib
        if cal is None or id(c) not in cal["want"] or not f8_eligible(c, H) or c.w32 is None:
            return
        xf = x.float()
        mu = xf.mean(dim=(0, 1, 2)) if cal["centre"] else None
        xc = xf - mu if mu is not None else xf
        st = {"absmax": float(xc.abs().max()), "mu": mu.contiguous() if mu is not None else None, "wq": None}
        if cal["gptq"]:
            import torch.nn.functional as F
            P = F.unfold(xc.permute(0, 3, 1, 2), 3, padding=1)                  # [B, Cin*9 (ci, kh, kw), L]
            P = P.permute(1, 0, 2).reshape(P.shape[1], -1)
            hm = (P @ P.t()) / P.shape[1]
            del P
            perm = (torch.arange(c.cin, device=x.device)[None, :] * 9 + torch.arange(9, device=x.device)[:, None]).reshape(-1)
            hm = hm[perm][:, perm]                                               # (tap, ci): the column order of w32
            w = c.w32.to(x.device)
            sw = (w.abs().amax(dim=1) / F8_MAX).clamp_min(1e-30).contiguous()
            U = gptq_factor(hm)
            wd = w.double().contiguous()
            st["wq"] = torch.empty(w.shape, dtype=torch.float32, device=x.device)
            self.lib.fr_gptq_round_e4m3(_lib.ptr(wd), _lib.ptr(U), _lib.ptr(sw), _lib.ptr(st["wq"]), w.shape[0], w.shape[1],
                                        _lib.stream_ptr())
        cal["stats"][id(c)] = st

    def _conv_f8(self, x8, c, B, H, W, residual=None, want16=True, nxt=None):
        """``nxt``: the fp8 conv that reads this one's output (its fp8 copy is written centred and scaled for it)"""
        y16 = torch.empty((B, H, W, c.cout), dtype=torch.float16, device=self.device) if want16 else None
        y8 = torch.empty((B, H, W, c.cout), dtype=torch.uint8, device=self.device) if nxt is not None else None
        a = _lib.ConvF8Args(_lib.ptr(x8), _lib.ptr(c.w8), _lib.ptr(y16), _lib.ptr(y8), _lib.ptr(c.oscale),
                            _lib.ptr(c.bias8), _lib.ptr(c.slope), _lib.ptr(residual), B, H, W, c.cin, c.cout,
                            1, float(1.0 / nxt.sx) if nxt is not None else 0.0,
                            _lib.ptr(nxt.mu) if nxt is not None else None)
        self._launch(self.lib.fr_conv_nhwc_f8, (ctypes.byref(a), _lib.stream_ptr()), *self._cost(CONV_F8, c.key, B))
        return y16, y8

    def _quantise(self, x16, c):
        """fp8 input of conv ``c`` from an f16 tensor: (x - mu[channel]) / sx, saturating"""
        out = torch.empty(x16.shape, dtype=torch.uint8, device=self.device)
        if c.mu is not None:
            self.lib.fr_quantize_f16_f8_centred(_lib.ptr(x16), _lib.ptr(out), x16.numel(), c.cin, _lib.ptr(c.mu),
                                                float(1.0 / c.sx), _lib.stream_ptr())
        else:
            self.lib.fr_quantize_f16_f8(_lib.ptr(x16), _lib.ptr(out), x16.numel(), float(1.0 / c.sx), _lib.stream_ptr())
        return out

    # ---- the two rules of the small-batch modes
    def _small_batch_splitk(self, c, B):
        """Small batches (single frames: a handful of faces) leave most CUs without an output tile and every block
        runs its whole K loop alone (measured: 16 faces 3.06 ms, 29 us per conv launch).  Their 3x3 convs are cut
        along K into slices that run side by side, followed by ``fr_conv_splitk_epilogue``.  The slice count
        depends on the layer and on the MODE only (B <= LOW_BATCH: slices of 3 K steps; B <= SMALL_BATCH: of 9), so
        results do not depend on the batch size inside a mode (between modes they differ by f32 summation order)."""
        if B > self.small_batch or c.k != 3 or c.cin % 64:
            return 1
        nk = 9 * c.cin // 64
        if nk < 18:                  # Cin = 64 (the 112x112 / 56x56 layers): one pass
            return 1
        if B <= self.low_batch:
            return -(-nk // 3)
        return min(8, nk // 9)

    def _inblock(self, c, B):
        """Up to eight faces (single frames): a 3x3 / stride-1 conv with >= 128 input channels is ONE launch that splits K
        among the sixteen waves of a workgroup (csrc/conv_inblock.hip) - the split-K form is two launches at their
        latency floor, 89 times per forward.  A mode of its own: inside it a face's embedding does not depend on its
        batch mates, against the other modes it differs by f32 summation order."""
        return (B <= self.inblock_batch and c.k == 3 and c.stride == 1 and c.pad == 1 and c.cin % 32 == 0
                and 128 <= c.cin <= 512 and c.cout % 32 == 0)

    # ---- launches
    def _cost(self, route, conv, B):
        return step_cost(self.table, route, conv, B) if self.profile is not None else ()

    def _launch(self, fn, args, variant=None, flops=0.0):
        """The one place a launch is bracketed by HIP events (on the stream it goes to: torch's current one) when ``profile`` collects."""
        if self.profile is None or variant is None:
            return fn(*args)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(*args)
        e1.record()
        self.profile.append((variant, flops, e0, e1))

    @staticmethod
    def _conv_args(s, c, B, x, y, residual, partial, x2):
        return _lib.ConvArgs(_lib.ptr(x), _lib.ptr(c.w), _lib.ptr(y), _lib.ptr(c.bias), _lib.ptr(c.slope), _lib.ptr(residual),
                             _lib.ptr(partial), B, s.H, s.W, c.cin, c.cout, c.k, c.k, c.stride, c.pad, s.Ho, s.Wo, c.bias_mode,
                             s.slices, _lib.ptr(x2), c.c2 if x2 is not None else 0)

    def _issue(self, s, c, x, residual=None, x2=None, partial=None):
        """One f16 conv step, launch by launch: allocates the output, builds the arguments, launches -> y (None when the
        output is ``partial``, the FC's f32 slices)."""
        B, stream = x.shape[0], _lib.stream_ptr()
        y = None if partial is not None else torch.empty((B, s.Ho, s.Wo, c.cout), dtype=torch.float16, device=self.device)
        if s.route == WALK64:
            self._launch(self.lib.fr_conv_walk64_f16, (_lib.ptr(x), _lib.ptr(c.w64), _lib.ptr(y), _lib.ptr(c.bias), c.bias_mode,
                                                       _lib.ptr(c.slope), _lib.ptr(residual), B, s.H, c.cout, stream), s.variant, s.flops)
        elif s.route == SPLITK:
            M = B * s.Ho * s.Wo
            part = torch.empty((s.slices, M, c.cout), dtype=torch.float32, device=self.device)
            a = _lib.ConvArgs(_lib.ptr(x), _lib.ptr(c.w), None, None, None, None, _lib.ptr(part), B, s.H, s.W, c.cin, c.cout,
                              c.k, c.k, c.stride, c.pad, s.Ho, s.Wo, 0, s.slices, _lib.ptr(x2), c.c2)
            self.lib.fr_conv_nhwc_f16(ctypes.byref(a), stream)
            self.lib.fr_conv_splitk_epilogue(_lib.ptr(part), s.slices, M, c.cout, s.Ho, s.Wo, _lib.ptr(c.bias), c.bias_mode,
                                             _lib.ptr(c.slope), _lib.ptr(residual), _lib.ptr(y), stream)
        else:
            a = self._conv_args(s, c, B, x, y, residual, partial, x2)
            self._launch(self.lib.fr_conv_inblock_f16 if s.route == INBLOCK else self.lib.fr_conv_nhwc_f16,
                         (ctypes.byref(a), stream), s.variant, s.flops)
        return y

    def _mode(self, taps=None):
        return RouteMode(self.small_batch, self.low_batch, self.inblock_batch, self.use_stage14, self.use_stage28,
                         self.use_walk64, self.fuse_shortcut, self._fp8_keys if self.fp8 else frozenset(),
                         self.stage14_f8 is not None, self.profile is not None, taps is not None, self._calib is not None)

    def _conv(self, x, c, B, H, W, residual=None, x2=None):
        """One conv of the net on its own, through the forward's route and dispatch (tools/debug_race3.py) -> (y, Ho, Wo)"""
        s = conv_step(self.table, B, self._mode(), self, c.key, "x", "h", x2=x2 is not None)
        assert (H, W) == (s.H, s.W)
        return self._issue(s, c, x, residual, x2), s.Ho, s.Wo

    def forward(self, x, taps=None):
        assert x.dtype == torch.float16 and x.shape[1:] == (112, 112, 8) and x.is_contiguous()
        B = x.shape[0]
        emb = torch.empty((B, 512), dtype=torch.float32, device=self.device)
        normed = torch.empty_like(emb)
        with torch.cuda.device(self.device):
            for b0 in range(0, B, self.max_chunk):
                b1 = min(B, b0 + self.max_chunk)
                self._forward_chunk(x[b0:b1], emb[b0:b1], normed[b0:b1], taps)
        return emb, normed

    # ---- single frames: the whole conv stack as ONE C call over persistent buffers
    def _splitk_floats(self, route, B):
        """split-K scratch of the largest SPLITK conv of a B-face route (floats)"""
        return max([s.slices * B * s.Ho * s.Wo * self.table.convs[s.conv].cout for s in route if s.route == SPLITK] + [1])

    def release_plans(self):
        """Drop every prepared single-frame plan and its per-stream buffers (they are otherwise kept for the life of
        the network: a captured HIP graph may replay them).  Call only when no captured graph of this network is
        alive - ``FaceAnalysis.enable_graphs(False)`` does, after dropping its graphs."""
        with self._plan_lock:
            self._plans.clear()
            self._plan_bufs.clear()
            self._plan_limit_logged = False

    def _plan(self, B, mode, route):
        """Up to LOW_BATCH faces the forward is ~200 launches of a few microseconds each and the Python / ctypes work
        per launch (argument structs, allocations, stream look-ups) is what the GPU waits for.  The conv steps of the
        route ``_forward_chunk`` walks are laid out once per (B, stream) - four rotating activation buffers, one
        split-K scratch - and replayed by ``fr_conv_sequence``.  Per stream: launches on one stream run in order, so
        they can share the buffers; another stream gets its own."""
        sid = torch.cuda.current_stream(self.device).cuda_stream
        key = (B, sid)
        plan = self._plans.get(key)
        if plan is not None:
            return plan
        if any(s.route not in _SEQ_KIND for s in route[:-1]):
            return None                          # a batch kernel in the route (low_batch above small_batch): launch by launch
        dev = self.device
        # buffers are per STREAM and sized for LOW_BATCH faces: every batch size of the mode lays its steps over them
        # (never freed: a captured HIP graph may hold them); past 8 streams, launch by launch
        shared = self._plan_bufs.get(sid)
        if shared is None:
            if len(self._plan_bufs) >= MAX_PLAN_STREAMS:
                if not self._plan_limit_logged:
                    self._plan_limit_logged = True
                    logging.getLogger(__name__).warning(
                        "IResNetHIP: single-frame plans exist for %d streams already; further streams run the conv stack "
                        "launch by launch (slower single-frame latency).  release_plans() frees them.", MAX_PLAN_STREAMS)
                return None
            shared = self._plan_bufs[sid] = (
                [torch.empty(self.low_batch * 112 * 112 * 64, dtype=torch.float16, device=dev) for _ in range(4)],
                torch.empty(self._splitk_floats(self._route(self.low_batch, mode), self.low_batch), dtype=torch.float32, device=dev))
        bufs, partial = shared
        assert self._splitk_floats(route, B) <= partial.numel()
        free, own, t = list(bufs), {}, {"x": None}                # x (the crops) is patched in per call
        arr = (_lib.ConvStep * (len(route) - 1))()
        for st, s in zip(arr, route):
            c = self._convs[s.conv]
            buf = free.pop()
            if s.dst == "h":                     # a block's output: its input, mid and shortcut buffers rotate back
                free += [own.pop(name) for name in ("h", "mid", "short") if name in own]
            own[s.dst] = buf
            x, residual, x2 = t[s.src], t.get(s.res), t["h"] if s.x2 else None
            t[s.dst] = y = buf[:B * s.Ho * s.Wo * c.cout].view(B, s.Ho, s.Wo, c.cout)
            st.kind = _SEQ_KIND[s.route]
            st.args = self._conv_args(s, c, B, x, y, residual, partial if s.route == SPLITK else None, x2)
        plan = self._plans[key] = (arr, len(arr), t["h"], bufs, partial)
        return plan

    def _route(self, B, mode):
        route = self._routes.get((B, mode))
        if route is None:
            route = self._routes[B, mode] = embed_route(self.table, B, mode, self)
        return route

    def _forward_chunk(self, x, emb, normed, taps):
        B = x.shape[0]
        mode = self._mode(taps)
        route = self._route(B, mode)
        plan = None
        if B <= self.low_batch and not (mode.profiled or mode.tapped or mode.calibrating or mode.fp8):
            with self._plan_lock:
                plan = self._plan(B, mode, route)
        if plan is not None:
            arr, n, h, _, _ = plan
            with self._plan_lock:                # the input pointer is patched into the shared step array
                arr[0].args.x = x.data_ptr()
                self.lib.fr_conv_sequence(arr, n, _lib.stream_ptr())
                self._fc(route[-1], h, emb, normed)
            return
        t, t8 = {"x": x}, {}                     # the f16 tensors / fp8 codes alive, by the names the steps use
        for s in route[:-1]:
            if s.route == QUANTISE:
                t8[s.src] = self._quantise(t[s.src], self._convs[s.conv])
            elif s.route == STAGE14_F8:
                t["h"] = self._run_stage14_f8(t["h"], t8["h"], B)
            elif s.route == STAGE28 or s.route == STAGE14:
                t["h"] = self._run_stage(s, t["h"])
            elif s.route == CONV_F8:             # the hand-over (who quantises, whose codes are written, want16) is the route's
                y, y8 = self._conv_f8(t8[s.src], self._convs[s.conv], B, s.H, s.W, residual=t.get(s.res), want16=s.want16,
                                      nxt=self._convs.get(s.nxt))
                t[s.dst], t8[s.dst] = y, y8
            else:
                c, xs = self._convs[s.conv], t[s.src]
                if mode.calibrating:             # enable_fp8(): statistics of the tensors the candidates read
                    self._calib_observe(c, xs, s.H)
                t[s.dst] = self._issue(s, c, xs, t.get(s.res), t["h"] if s.x2 else None)
            if taps is not None and s.tap is not None:
                taps[s.tap] = t[s.dst]
        if taps is not None:
            taps["final"] = t["h"]
        self._fc(route[-1], t["h"], emb, normed)

    def _fc(self, s, h, emb, normed):
        B = h.shape[0]
        partial = torch.empty((FC_SPLITK, B, 512), dtype=torch.float32, device=self.device)
        self._issue(s, self.fc, h, partial=partial)
        self.lib.fr_fc_reduce_l2norm(_lib.ptr(partial), FC_SPLITK, B, 512, _lib.ptr(self.fc_bias),
                                     _lib.ptr(emb), _lib.ptr(normed), _lib.stream_ptr())
