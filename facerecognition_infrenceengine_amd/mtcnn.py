"""MTCNN cascade on the HIP detector kernels.

Detector half of ``FaceAnalysis.get`` (/root/reference/infrenceServer.py:528).  The host side is
a launch plan only: every stage works on fixed-capacity per-frame slot lists with device-side
counts, so a whole batch of frames runs without a host synchronisation.  Conventions (resize,
ordering, thresholds, capacities) are those written down in ``oracle/detect.py``.
"""
import contextlib
import ctypes
import functools
import logging
import math
import threading
from types import SimpleNamespace
from typing import NamedTuple

import torch

from . import _lib


def pyramid_scales(h, w, minsize=20, factor=0.709):
    m = 12.0 / minsize
    minl = min(h, w) * m
    scales, k = [], 0
    while minl >= 12:
        scales.append(m * factor ** k)
        minl *= factor
        k += 1
    return scales


def _pool_out(n, k, s):
    o = -(-(n - k) // s) + 1
    if (o - 1) * s >= n:
        o -= 1
    return o


# layer id -> (cin, cout, kh, kw, ntb): must mirror the table in csrc/dconv_mfma.hip
MFMA_LAYERS = {0: (3, 12, 3, 3, 1), 1: (12, 16, 3, 3, 1), 2: (16, 32, 3, 3, 2),
               10: (4, 28, 3, 3, 2), 11: (28, 48, 3, 3, 3), 12: (48, 64, 2, 2, 4), 13: (64, 128, 3, 3, 4),
               14: (128, 6, 1, 1, 1),
               20: (4, 32, 3, 3, 1), 21: (32, 64, 3, 3, 2), 22: (64, 64, 3, 3, 4), 23: (64, 128, 2, 2, 4),
               24: (128, 256, 3, 3, 4), 25: (256, 16, 1, 1, 1)}


class _MConv:
    """Detector layer packed for fr_dconv_mfma_f32: w [cout_group][tap][CinP][CP] f32 where
    CinP = Cin rounded up to 4 and CP = NTB*16 (+16 when NTB is even: LDS bank spread)."""

    def __init__(self, layer, w, b, slope, device, head=None):
        cin, cout, kh, kw, ntb = MFMA_LAYERS[layer]      # packed sizes: real channels are zero-padded up to them
        rcout, rcin = w.shape[0], w.shape[1]
        assert tuple(w.shape[2:]) == (kh, kw) and rcout <= cout and rcin <= cin, (layer, tuple(w.shape))
        wfull = torch.zeros((cout, cin, kh, kw), dtype=torch.float32)
        wfull[:rcout, :rcin] = w
        w = wfull
        bfull = torch.zeros(cout); bfull[:rcout] = b; b = bfull
        if slope is not None:
            sfull = torch.zeros(cout); sfull[:rcout] = slope; slope = sfull
        self.layer, self.cin, self.cout, self.kh, self.kw = layer, cin, cout, kh, kw
        cinp = -(-cin // 4) * 4
        cp = ntb * 16 + (16 if ntb % 2 == 0 else 0)
        gsz = ntb * 16
        ngroups = -(-cout // gsz)
        wp = torch.zeros((ngroups, kh * kw, cinp, cp), dtype=torch.float32)
        wt = w.permute(2, 3, 1, 0).reshape(kh * kw, cin, cout)              # [tap][ci][co]
        for g in range(ngroups):
            n = min(gsz, cout - g * gsz)
            wp[g, :, :cin, :n] = wt[:, :, g * gsz:g * gsz + n]
        self.w = wp.contiguous().to(device)
        bp = torch.zeros(ngroups * gsz); bp[:cout] = b
        self.b = bp.to(device)
        self.slope = None
        if slope is not None:
            sp = torch.zeros(ngroups * gsz); sp[:cout] = slope
            self.slope = sp.to(device)
        self.head_w = self.head_b = None
        self.nhead = 0
        if head is not None:
            self.head_w = head[0].t().contiguous().to(torch.float32).to(device)      # [cout][nh]
            self.head_b = head[1].to(torch.float32).contiguous().to(device)
            self.nhead = head[0].shape[0]
        self.pool = {0: 2, 10: 3, 11: 3, 20: 3, 21: 3, 22: 2}.get(layer, 0)     # fused ceil-mode max pool, stride 2

    def out_hw(self, h, w):
        hc, wc = h - self.kh + 1, w - self.kw + 1
        return (_pool_out(hc, self.pool, 2), _pool_out(wc, self.pool, 2)) if self.pool else (hc, wc)


# consecutive layers of each net: (layer, the layers that read its output)
_CHAINS = {"pnet": (("conv1", ("conv2",)), ("conv2", ("conv3",)), ("conv3", ("conv4_1", "conv4_2"))),
           "rnet": (("conv1", ("conv2",)), ("conv2", ("conv3",)), ("conv3", ("dense4",)), ("dense4", ("dense5_1", "dense5_2"))),
           "onet": (("conv1", ("conv2",)), ("conv2", ("conv3",)), ("conv3", ("conv4",)), ("conv4", ("dense5",)),
                    ("dense5", ("dense6_1", "dense6_2", "dense6_3")))}


def canonical_scale(state, net, dead_zone=2):
    """The state dict rescaled, layer pair by layer pair, so that every layer's weights have about the He-init RMS
    sqrt(2 / fan_in): layer l's weights and bias x 2^e, the weights of the layers reading it x 2^-e (e an integer, 0 while the
    RMS is within 2^dead_zone of He init).  PReLU and max pool commute with a positive scale, so the network is unchanged, and
    in f32 arithmetic bit for bit while nothing under- or overflows.  Why: the split-precision operands (x = hi + lo in f16) are
    accurate only near that scale - below it lo, then hi, are f16 subnormals - and a checkpoint may
    carry its scale anywhere along the chain.  The heads take what is left."""
    st = dict(state)
    for name, readers in _CHAINS[net]:
        w = st[name + ".weight"]
        rms = float(w.double().pow(2).mean().sqrt())
        if rms == 0.0:
            continue
        e = math.log2(math.sqrt(2.0 / w[0].numel()) / rms)
        k = int(round(e)) if abs(e) > dead_zone else 0
        if k:
            st[name + ".weight"] = w * 2.0 ** k
            st[name + ".bias"] = st[name + ".bias"] * 2.0 ** k
            for n in readers:
                st[n + ".weight"] = st[n + ".weight"] * 2.0 ** -k
    return st


def _dense_as_conv(w, k, c):
    """MTCNN dense layer over a k x k x c map flattened (w, h, c) -> conv weight [o, c, kh, kw]."""
    o = w.shape[0]
    return w.reshape(o, k, k, c).permute(0, 3, 2, 1).contiguous()      # [o, w, h, c] -> [o, c, h, w]


class DetectSettings:
    """What the launch plan of a call (``detect_plan``) is decided from, with the defaults; MTCNNHIP carries them as attributes."""
    # level streams of a single-frame call while it is captured into a HIP graph (tools/bench_latency_streams.py, get() + match under replay,
    # 24 / 4 hardware queues: 0 streams 1.81 - 1.84 / 1.80 - 1.84 ms, 2: 1.67 - 1.69 / 1.66 - 1.74, 4: 1.59 - 1.65 / 1.58 - 1.64, 11: 1.70 - 1.74 / 1.57 - 1.66)
    SINGLE_FRAME_LEVEL_STREAMS = 4
    one_stream = False              # True (profiling): every pyramid level on the caller's stream, per-kernel times add up
    # Side streams (1 or 2) the pyramid levels 1.. are dealt over, detect_batch's default.  2 since round 4 (split-precision R-/O-Net,
    # band-only exact P-Net pass: a 64 x 1080p batch alone 5.30 ms with one side stream, 4.9 - 5.1 with two; inside the bench C2 24 150 ->
    # 25 400 faces/s, C5 25 470 -> 27 070, C3 20 780 -> 20 880: tools/ab_bench_knobs.sh).  The round-3 figures are in DESIGN.md 4.3.
    level_streams = 2
    phase_marks = None              # tools: a list -> (name, event on the caller's stream) at the cascade's phase ends
    solo_max_frames = 7             # up to this many frames a call that is not a batch runs on ONE stream, eagerly, and is recorded
    # The batch path (batch_min_pixels): only the cells within ``refine_margin`` of the face threshold are re-evaluated exactly (every
    # keep / reject decision is that of f32 arithmetic); kept cells above the band carry the split-precision heads (~2e-6 from
    # the f32 ones) - as the R-/O-Net crops do (``split_ro``).  False: every cell that can be kept carries the f32 path's bits.
    pnet_band = True
    split_pconv1 = True             # with pnet_band: conv1 on the f16 matrix cores too; the exact pass gets an exact f32 map
                                    # under its cells' windows from the f32 conv1 kernel run over just those tiles
    # ... on levels whose conv1 map has at least this many pixels: levels 0 - 4 of a 1080p pyramid (11.7 k pixels and more), 0 - 6 of a 4K
    # one.  Their exact tiles share one list and one launch (pyramid_launch); 64 x 1080p, detector alone, is flat within +- 0.05 ms from
    # three such levels on (0: 5.01 ms, 3: 4.86, 5: 4.83, all 12: 4.82; profiles/pnet_pyramid_ab.txt)
    split_pconv1_min_px = 10000
    pyramid_launch = True           # batches: every P-Net layer launched ONCE over the whole pyramid, on the caller's stream
                                    # (_pnet_pyramid); False: the per-level launches (pnet_level) dealt over the level streams
    refined_cells = None            # optional device int32[1]: cells re-evaluated exactly (diagnostics)
    use_sequence = True             # eager single-frame calls of a known frame shape replay a recorded C call list (fr_detect_sequence)
    fused_crop = True               # first R-/O-Net layer fused with the crop (csrc/ro_conv1.hip)
    # second R-/O-Net layer on the f16 matrix cores with split-precision operands (csrc/ro_conv2.hip; the batch path), the small
    # tail layers as split-precision GEMMs (csrc/ro_gemm.hip); the crops whose logit lies within ``ro_margin`` of the stage
    # threshold are re-evaluated by the all-f32 layers, so every keep / reject decision is that of f32 arithmetic
    split_ro = True
    # The batch path's conv2 / conv3 / heads in two tiers (csrc/pnet_fused.hip): a coarse pass over every cell with the hi halves of the
    # split operands only (one MFMA per product instead of three), then the split-precision form over just the cells whose coarse logit
    # difference is within ``coarse_margin`` of the exact pass's pre-filter (~1 %) - which then carry the bits the one-tier kernel gives
    # them; no other cell's value is ever read beyond "below the pre-filter".  With pnet_band only; False: the one-tier split kernel.
    coarse_p23 = True
    coarse_margin = 0.05            # in logit units; >= 20x the hi-only format's error inside the envelope of DESIGN.md 4.3a
    visited_cells = None            # optional device int32[1]: cells the second tier re-evaluated (diagnostics)

    def __init__(self, minsize=20, factor=0.709, fused_pnet=True, batch_min_pixels=None):
        self.minsize, self.factor = minsize, factor
        # conv2 -> conv3 -> heads in one kernel on split-precision f16 operands + exact f32 re-evaluation (csrc/pnet_fused.hip)
        self.fused_pnet = bool(fused_pnet)
        # From this many PIXELS per call (frames x H x W) the BATCH arithmetic runs: the band-only exact P-Net pass, P-Net conv1 /
        # R-Net / O-Net on the f16 matrix cores with split-precision operands + exact f32 passes at the thresholds.  Below it the
        # all-f32 detector (and, under ``solo_max_frames`` + 1 frames, its recorded call list).  The batch path's extra launches (tile
        # lists, exact chains) cost a fixed ~0.4 ms: measured crossover on MI355X between 8 and 12 x 1080p frames (8: 1.71 against
        # 1.51 ms, 12: 1.80 / 1.90, 16: 1.93 / 2.18, 32: 2.88 / 3.56; profiles/r05_detector_crossover.txt, tools/crossover_det.py),
        # i.e. ~ 22 Mpixel - 8 x 4K frames (66 Mpx) are far on the batch side, 8 x 1080p (16.6 Mpx) are not.
        self.batch_min_pixels = 22_000_000 if batch_min_pixels is None else int(batch_min_pixels)
        self.single_frame_level_streams = self.SINGLE_FRAME_LEVEL_STREAMS      # level_streams of a captured call of <= solo_max_frames frames


class DetectPlan(NamedTuple):
    """Every decision of one ``detect_batch`` call (``detect_plan``)."""
    N: int
    scales: tuple       # the pyramid's scales, largest level first
    geo: tuple          # per level (hs, ws, h, w): the level's size and its conv1 map's
    batch: bool         # the batch arithmetic (batch_min_pixels)
    few: bool           # <= solo_max_frames frames and not a batch
    band: bool          # the P-Net's exact pass takes only the cells in the band round the threshold
    fused: tuple        # per level: the fused P-Net (its split conv1 map fits 32-bit offsets)
    f16: tuple          # per level: conv1 on the f16 matrix cores
    pyramid: bool       # every P-Net layer as ONE launch over all levels
    solo: bool          # every level on the caller's stream: nothing to fork, nothing to join
    nside: int          # side streams the levels 1.. are dealt over otherwise
    cache: bool         # the work tensors of the last call of this frame shape are used again ...
    recorder: bool      # ... and the call may be recorded and replayed as one C call list
    split: bool         # R-/O-Net on the f16 matrix cores + exact pass at the thresholds
    coarse: float       # the fused P-Net in two tiers: the coarse pass's margin (> 0), or 0.0 - the one-tier split kernel
    chunks: tuple       # ((first frame, end frame), ...) when the call must be cut into groups of frames, else ()


def _is_batch(cfg, N, H, W):
    return N * H * W >= cfg.batch_min_pixels


def _level_geo(H, W, scale):
    """(hs, ws, h, w) of a pyramid level: its size and its conv1 map's (3x3 conv + ceil-mode 2x2 / stride-2 pool: _MConv.out_hw of
    layer 0).  The level is resized inside conv1's tile load: there is no f32 level image in HBM."""
    hs, ws = int(math.ceil(H * scale)), int(math.ceil(W * scale))
    return hs, ws, _pool_out(hs - 2, 2, 2), _pool_out(ws - 2, 2, 2)


def _frames32(h, w):
    """How many frames of an h x w conv1 map the fused P-Net takes at once: it addresses the level's split map [N, h, w, 64 B] with
    32-bit buffer offsets."""
    return (2 ** 31 - 1) // (h * w * 64)


def _f16_conv1(cfg, band, h, w):
    return bool(band and cfg.split_pconv1 and h * w >= cfg.split_pconv1_min_px)


def detect_plan(N, H, W, cfg, trace=False, level_streams=None, out=False, capturing=False):
    """The launch plan of a ``detect_batch`` call over N frames of H x W, from ``cfg`` (a DetectSettings), whether the call traces,
    its ``level_streams`` argument, whether it writes into result tensors it was given (a chunk of a larger call) and whether the
    current stream is capturing a graph.  Pure - no device, no library - and remembered: computed on every call it cost a replayed
    single frame 0.035 ms until done and the eager 8 / 12 x 1080p calls 0.03 - 0.04 ms of host issue (profiles/detector_host_refactor.txt)."""
    return _plan(N, H, W, tuple([getattr(cfg, k) for k in _PLAN_READS]), cfg.phase_marks is None and cfg.refined_cells is None,
                 trace, level_streams, out, capturing)


_PLAN_READS = ("minsize", "factor", "fused_pnet", "batch_min_pixels", "solo_max_frames", "pnet_band", "split_pconv1", "split_pconv1_min_px",
               "pyramid_launch", "one_stream", "level_streams", "single_frame_level_streams", "split_ro", "fused_crop", "use_sequence",
               "coarse_p23", "coarse_margin")


@functools.lru_cache(maxsize=256)
def _plan(N, H, W, settings, recordable, trace, level_streams, out, capturing):
    cfg = SimpleNamespace(**dict(zip(_PLAN_READS, settings)))
    scales = tuple(pyramid_scales(H, W, cfg.minsize, cfg.factor))
    geo = tuple(_level_geo(H, W, s) for s in scales)
    batch = _is_batch(cfg, N, H, W)
    few = N <= cfg.solo_max_frames and not batch
    fusable = bool(cfg.fused_pnet) and not trace
    # A batch whose largest level exceeds the fused P-Net's offsets (64 x 4K frames: 3.05e9 B) is cut into the fewest equal groups
    # of frames that fit - frames are independent, every group's final NMS writes its rows of the result tensors - rather than
    # dropping that level to the layer-by-layer f32 path.
    chunks, per = (), N
    if fusable and not out and N > 1 and geo and 1 <= _frames32(*geo[0][2:]) < N:
        per = -(-N // -(-N // _frames32(*geo[0][2:])))
        chunks = tuple((n0, min(N, n0 + per)) for n0 in range(0, N, per))
    band = bool(cfg.pnet_band and batch and not trace)
    fused = tuple(bool(cfg.fused_pnet) and per <= _frames32(h, w) for _, _, h, w in geo)       # (of a call that is cut: its groups')
    f16 = tuple(fu and _f16_conv1(cfg, band, h, w) for fu, (_, _, h, w) in zip(fused, geo))
    pyramid = bool(cfg.pyramid_launch and batch and fusable and all(fused))
    # Level 0 holds half of the pyramid's pixels; the remaining levels are small launches that cannot fill 256 CUs on their own, so
    # they are dealt round-robin over side HIP streams beside level 0 (joined before the NMS).
    nside = max(1, min(2, level_streams if level_streams is not None else cfg.level_streams))
    own = few and level_streams is None
    if own and capturing and cfg.single_frame_level_streams > 0:
        # A single frame is a chain of launch latencies.  While a HIP graph is being captured, every level goes to a stream of its
        # own: the graph then holds the levels' five-kernel chains side by side (640x480 get() + match under replay 2.21 -> 2.01
        # ms).  Not in eager calls: the host issues the launches one by one anyway and the extra fork / join events cost it 0.1 ms.
        nside = min(cfg.single_frame_level_streams, max(1, len(scales) - 1))
    # An EAGER single-frame call is bound by the interpreter (host issue 0.73 ms against 0.85 ms until the GPU is done,
    # tools/host_time_c1.py): side streams would only add their fork / join events and a stream switch per level
    eager = bool(trace or cfg.one_stream or (own and not capturing))
    cache = bool(eager and few and not trace and not out and not capturing)
    # Only the default configuration is recorded: fr_detect_sequence replays the entry points of _lib.SEQ_FN, and the stand-alone
    # crop / the f32 P-Net layers on generic shapes go through others (the recorder refuses such a list as well:
    # Lib.stop_recording); ``one_stream`` asks for every level on the caller's stream, which a recorded list (levels on side
    # streams) would not honour.
    recorder = bool(cache and recordable and cfg.use_sequence and cfg.fused_pnet and cfg.fused_crop and not cfg.one_stream)
    split = bool(cfg.split_ro and cfg.fused_crop and batch and not trace)
    coarse = float(cfg.coarse_margin) if cfg.coarse_p23 and band else 0.0
    return DetectPlan(N, scales, geo, batch, few, band, fused, f16, pyramid, eager or pyramid, nside, cache, recorder, split, coarse, chunks)


# What differs between R-Net / stage 2 and O-Net / stage 3; the row index is the kernels' net id and picks the stage's threshold
# (thresholds[1 + net]), its exact list's capacity, its phase mark and its trace keys.  name: the bound method that runs the net; cap_in,
# cap_out: attributes, slots per frame the stage reads and writes; map1, map2: (side, channels) of conv1's and conv2's pooled maps; w1, w2:
# attributes, conv1's weights for the crop kernels and conv2's for its split form; layers: attributes, the f32 layers conv1, conv2, the tail
# (split GEMMs behind a split conv2), the heads; nhead: 2 logits + 4 regressions (+ 10 landmark coordinates); naux: what a kept box carries
# along of them; refine: fr_box_refine's mode
_RO = (SimpleNamespace(name="rnet", cap_in="cap_p", cap_out="cap_r", crop=24, map1=(11, 28), map2=(4, 48), w1="_rc1", w2="_rc2",
                       layers=("r1", "r2", "r3", "r4", "r5"), nhead=6, naux=4, refine=1),
       SimpleNamespace(name="onet", cap_in="cap_r", cap_out="cap_o", crop=48, map1=(23, 32), map2=(10, 64), w1="_oc1", w2="_oc2",
                       layers=("o1", "o2", "o3", "o4", "o5", "o6"), nhead=16, naux=14, refine=2))


class MTCNNHIP(DetectSettings):
    def __init__(self, pstate, rstate, ostate, device="cuda:0", minsize=20, factor=0.709,
                 thresholds=(0.6, 0.7, 0.7), cap_scale=2048, keep_scale=256, cap_p=512, cap_r=64, cap_o=16,
                 fused_pnet=True, batch_min_pixels=None, canonical=True):
        _lib.require_gpu()
        DetectSettings.__init__(self, minsize, factor, fused_pnet, batch_min_pixels)
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.thresholds = tuple(float(t) for t in thresholds)
        self.cap_scale, self.keep_scale, self.cap_p, self.cap_r, self.cap_o = cap_scale, keep_scale, cap_p, cap_r, cap_o
        assert cap_scale <= 4096 and cap_p <= 1024 and cap_r <= 1024 and cap_o <= 1024
        self._sides = {}                   # caller's stream -> its side streams: independent pipelines (bench --pipes) do not couple
        self._tls = threading.local()      # per-thread launch stream: detect_batch is re-entrant across threads
        self._unfused_logged = False
        d = self.device
        p, r, o = ({k: v.detach().float().cpu() for k, v in s.items()} for s in (pstate, rstate, ostate))
        # canonical: every path runs the nets rescaled to the He-init weight scale (canonical_scale: the same f32 results, and
        # split-precision operands inside the envelope the batch path's margins are sized for).  False: the weights as given.
        if canonical:
            p, r, o = (canonical_scale(s, n) for s, n in ((p, "pnet"), (r, "rnet"), (o, "onet")))
        self.p1 = _MConv(0, p["conv1.weight"], p["conv1.bias"], p["prelu1.weight"], d)
        self.p2 = _MConv(1, p["conv2.weight"], p["conv2.bias"], p["prelu2.weight"], d)
        hw = torch.cat([p["conv4_1.weight"].reshape(2, 32), p["conv4_2.weight"].reshape(4, 32)])
        hb = torch.cat([p["conv4_1.bias"], p["conv4_2.bias"]])
        self.p3 = _MConv(2, p["conv3.weight"], p["conv3.bias"], p["prelu3.weight"], d, head=(hw, hb))
        # the fused P-Net's conv2 / conv3 / head weights as (cout, tap, channel), 10 taps x 16 channels
        w2p = torch.zeros((16, 10, 16)); w2p[:, :9, :10] = p["conv2.weight"].permute(0, 2, 3, 1).reshape(16, 9, 10)
        w3p = torch.zeros((32, 10, 16)); w3p[:, :9, :16] = p["conv3.weight"].permute(0, 2, 3, 1).reshape(32, 9, 16)
        self._p23 = tuple(t.to(torch.float32).contiguous().to(d) for t in (
            w2p, p["conv2.bias"], p["prelu2.weight"], w3p, p["conv3.bias"], p["prelu3.weight"], hw.t().contiguous(), hb))
        self.refine_margin = 2e-3           # in logit units; >= 20x the split format's error inside the envelope of DESIGN.md 4.3a
        self.level_tensors = None           # tests: a list -> one dict per pyramid level of the last batch call (its maps, heads, workspace)
        self.p23_all_heads = False          # True: the fused kernel also writes the approximate heads of the cells it rules out
        # first R-/O-Net layer fused with the crop (fused_crop): weights as [k = (kh, kw, channel)][cout]
        self._rc1 = tuple(t.to(torch.float32).contiguous().to(d) for t in (
            r["conv1.weight"].permute(2, 3, 1, 0).reshape(27, 28), r["conv1.bias"], r["prelu1.weight"]))
        self._oc1 = tuple(t.to(torch.float32).contiguous().to(d) for t in (
            o["conv1.weight"].permute(2, 3, 1, 0).reshape(27, 32), o["conv1.bias"], o["prelu1.weight"]))
        self.split_conv1 = True             # with split_ro: the first layer's conv on the f16 matrix cores too (csrc/ro_conv1.hip, F16)
        self.ro_margin = 1e-3               # in logit units; >= 20x the split format's error inside the envelope of DESIGN.md 4.3a
        self.ro_list_cap = (1024, 256)      # slots of the exact pass's work list (R-Net, O-Net); entries past it keep the split values
        # second R-/O-Net layer in its split-precision form (split_ro): weights as [cout][tap][32 channels] f32
        def c2w(w):
            o, c = w.shape[0], w.shape[1]
            wp = torch.zeros((o, 9, 32))
            wp[:, :, :c] = w.permute(0, 2, 3, 1).reshape(o, 9, c)
            return wp
        self._rc2 = tuple(t.to(torch.float32).contiguous().to(d) for t in (c2w(r["conv2.weight"]), r["conv2.bias"], r["prelu2.weight"]))
        self._oc2 = tuple(t.to(torch.float32).contiguous().to(d) for t in (c2w(o["conv2.weight"]), o["conv2.bias"], o["prelu2.weight"]))
        self.r1 = _MConv(10, r["conv1.weight"], r["conv1.bias"], r["prelu1.weight"], d)
        self.r2 = _MConv(11, r["conv2.weight"], r["conv2.bias"], r["prelu2.weight"], d)
        self.r3 = _MConv(12, r["conv3.weight"], r["conv3.bias"], r["prelu3.weight"], d)
        self.r4 = _MConv(13, _dense_as_conv(r["dense4.weight"], 3, 64), r["dense4.bias"], r["prelu4.weight"], d)
        self.r5 = _MConv(14, torch.cat([r["dense5_1.weight"], r["dense5_2.weight"]]).reshape(6, 128, 1, 1),
                         torch.cat([r["dense5_1.bias"], r["dense5_2.bias"]]), None, d)
        self.o1 = _MConv(20, o["conv1.weight"], o["conv1.bias"], o["prelu1.weight"], d)
        self.o2 = _MConv(21, o["conv2.weight"], o["conv2.bias"], o["prelu2.weight"], d)
        self.o3 = _MConv(22, o["conv3.weight"], o["conv3.bias"], o["prelu3.weight"], d)
        self.o4 = _MConv(23, o["conv4.weight"], o["conv4.bias"], o["prelu4.weight"], d)
        self.o5 = _MConv(24, _dense_as_conv(o["dense5.weight"], 3, 128), o["dense5.bias"], o["prelu5.weight"], d)
        # the small tail layers as split-precision GEMMs on the f16 matrix cores (csrc/ro_gemm.hip; batch path): f32 weights
        # [cout][K], K = (kh, kw, channel) ascending = the input map's memory order, packed into MFMA fragment order
        self._gemm = {}
        for lid, wconv, b, sl in ((12, r["conv3.weight"], r["conv3.bias"], r["prelu3.weight"]),
                                  (13, _dense_as_conv(r["dense4.weight"], 3, 64), r["dense4.bias"], r["prelu4.weight"]),
                                  (22, o["conv3.weight"], o["conv3.bias"], o["prelu3.weight"]),
                                  (23, o["conv4.weight"], o["conv4.bias"], o["prelu4.weight"]),
                                  (24, _dense_as_conv(o["dense5.weight"], 3, 128), o["dense5.bias"], o["prelu5.weight"])):
            wk = wconv.permute(0, 2, 3, 1).reshape(wconv.shape[0], -1).to(torch.float32).contiguous().to(d)
            packed = torch.empty(self.lib.fr_ro_gemm_weight_bytes(lid), dtype=torch.uint8, device=d)
            with torch.cuda.device(d):
                self.lib.fr_ro_gemm_pack(lid, _lib.ptr(wk), _lib.ptr(packed), _lib.stream_ptr())
                torch.cuda.synchronize(d)
            self._gemm[lid] = (packed, b.to(torch.float32).contiguous().to(d), sl.to(torch.float32).contiguous().to(d))
        self.o6 = _MConv(25, torch.cat([o["dense6_1.weight"], o["dense6_2.weight"], o["dense6_3.weight"]]).reshape(16, 256, 1, 1),
                         torch.cat([o["dense6_1.bias"], o["dense6_2.bias"], o["dense6_3.bias"]]), None, d)

    def set_exact(self, on=True):
        """All-exact switch of the batch path: with ``on`` every value a kept candidate carries - P-Net cell scores / regressions,
        R-/O-Net heads - is the all-f32 kernels', bit for bit (pnet_band and split_ro off: the exact P-Net pass re-evaluates every
        cell that can be kept, R-/O-Net run their f32 layers), so that NMS ORDER, box truncation and crop coordinates are those of
        f32 arithmetic too, not only the threshold decisions.  Costs the batch path its round-4 gain (64 x 1080p: 4.9 -> 6.5 ms).
        Default off: threshold decisions exact, kept values within ~5e-6 (DESIGN.md 4.3a says what that can and cannot change)."""
        self.pnet_band = self.split_ro = not on
        return self

    @property
    def _dl(self):
        return getattr(self._tls, "dl", (None, 0.0))

    @property
    def _s(self):
        return self._tls.s

    @_s.setter
    def _s(self, v):
        self._tls.s = v

    # ---- thin launch helpers (all on the current stream)
    def _new(self, shape, dtype):
        """A work tensor.  Inside an eager single-frame call (``_begin`` sets ``_tls.cache``) the k-th allocation of a
        call returns the tensor the k-th allocation of the previous call with the same frame shape, stream and thread
        made: ~90 ``torch.empty`` per call were 0.15 ms of an interpreter-bound 0.73 ms."""
        c = getattr(self._tls, "cache", None)
        if c is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        lst, i = c
        c[1] = i + 1
        if i < len(lst) and lst[i].shape == tuple(shape) and lst[i].dtype == dtype:
            return lst[i]
        t = torch.empty(shape, dtype=dtype, device=self.device)
        self._tls.cache_grew = True             # a recorded call list of this frame shape would hold stale pointers
        if i < len(lst):
            lst[i] = t
        else:
            lst.append(t)
        return t

    def _f32(self, *shape):
        return self._new(shape, torch.float32)

    def _i32(self, *shape):
        return self._new(shape, torch.int32)

    def _fptr(self, frames):
        """The frame batch's pointer, tagged with its role for the call recorder (_lib.RolePtr): a replayed call list
        patches exactly the slots recorded through here."""
        return _lib.ptr(frames, role="frame")

    def _dconv(self, x, c, B, H, W, frames=None, counts=None, cap=0, y_split=None, y=None):
        ho, wo = c.out_hw(H, W)
        if y is None:                               # (else: the output map, made by the caller)
            y = self._f32(B, ho, wo, c.nhead if c.nhead else c.cout)
        fh, fw = (frames.shape[1], frames.shape[2]) if frames is not None else (0, 0)
        self.lib.fr_dconv_mfma_f32(c.layer, _lib.ptr(x), _lib.ptr(c.w), _lib.ptr(c.b), _lib.ptr(c.slope), _lib.ptr(y),
                                   B, H, W, _lib.ptr(c.head_w), _lib.ptr(c.head_b), self._fptr(frames), fh, fw,
                                   _lib.ptr(counts), cap, _lib.ptr(y_split), self._s)
        return y, ho, wo

    def _gemm_split(self, lid, x, B, shape, counts, cap):
        w, b, sl = self._gemm[lid]
        y = self._f32(B, *shape)
        self.lib.fr_ro_gemm_split(lid, _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(sl), _lib.ptr(y), B, _lib.ptr(counts), cap, self._s)
        return y

    def _nms(self, boxes, scores, aux, naux, counts, L, nseg, seg_cap, seg_major, thr, mode, keep, out=None, results=False):
        """results: the four outputs are what detect_batch returns - their pointers carry the roles "out0".."out3" for the
        call recorder."""
        if out is None:
            bo, so, co = self._f32(L, keep, 4), self._f32(L, keep), self._i32(L)
            ao = self._f32(L, keep, max(naux, 1))
        else:
            bo, so, ao, co = out
        po = [_lib.ptr(t, role="out%d" % i if results else None) for i, t in enumerate((bo, so, ao, co))]
        self.lib.fr_sort_nms(_lib.ptr(boxes), _lib.ptr(scores), _lib.ptr(aux), naux, _lib.ptr(counts), L, nseg, seg_cap,
                             seg_major, thr, mode, keep, *po, keep, self._s)
        return bo, so, ao, co

    # ---- P-Net
    def _band_logits(self, band=True):
        """(lo, hi) in logit units: cells at or above lo can be kept (the exact pass's pre-filter), those below hi are re-evaluated
        exactly - all of them without ``band``."""
        lt = math.log(self.thresholds[0] / (1.0 - self.thresholds[0]))
        return lt - self.refine_margin, lt + self.refine_margin if band else float("-inf")

    def _coarse(self, margin):
        """The coarse pass's margin for this call's fused levels, or 0.0: ``p23_all_heads`` asks for the split heads of every cell."""
        return 0.0 if self.p23_all_heads else margin

    def _level_buffers(self, N, scale, geo, band, f16, cand, coarse=0.0):
        """The work tensors of one fused P-Net level - the split-f16 copy ``xs`` of conv1's map, the f32 map ``x`` (a level with ``f16``:
        SPARSE, written only in the 16 x 64-pixel tiles the band-tile list names, where the exact pass needs a 5x5 window, uninitialised
        elsewhere), the heads, the fused kernel's workspace, the candidate kernel's block counts - as a dict (``level_tensors``), and the
        level's fr_pnet_level entry; cand: its candidate list (boxes, scores, regs, counts) or None.  coarse: the level runs in two tiers and
        gets the coarse pass's buffer ``cws`` too.  Notes the level in ``_tls.path``."""
        hs, ws, h, w = geo
        path = getattr(self._tls, "path", None)
        if path is not None:
            path["fused_levels"] += 1
            path["band_levels"] += int(band)
            path["coarse_levels"] += int(coarse > 0.0)
            if f16:
                path["pconv1_mfma_levels"].append((h, w))
        xs = self._new((N, h, w, 64), torch.uint8)
        x = self._f32(N, h, w, 12)
        head = self._f32(N, h - 4, w - 4, 6)
        wsp = self._new((self.lib.fr_pnet23_workspace_bytes(N, h, w) // 4,), torch.float32)
        bc = self._i32(N * (-(-(h - 4) * (w - 4) // 256)))
        cws = self._i32(self.lib.fr_pnet23_coarse_workspace_bytes(N, h, w) // 4) if coarse > 0.0 else None
        entry = None
        if cand is not None:
            entry = _lib.PnetLevel(x.data_ptr(), head.data_ptr(), wsp.data_ptr(), h, w, float(scale), *[t.data_ptr() for t in cand],
                                   bc.data_ptr(), xs.data_ptr(), hs, ws, int(f16))
        return dict(h=h, w=w, f16=f16, x=x, xs=xs, head=head, wsp=wsp, bc=bc, cws=cws), entry

    def _level(self, frames, scale, geo, fused, band, f16, trace, cand, coarse=0.0):
        """One pyramid level's P-Net -> (head, hc, wc, bc, dl, dl_min, keep): the heads f32 [N,hc,wc,6]; the block counts,
        logit-difference map and pre-filter for fr_pnet_candidates; keep: None, or - the level has extracted its candidates itself
        (``f16``) - its tensors (x, xs, head, wsp, tbuf, tiles, bc), to be kept alive until the level's stream has been joined."""
        N, H, W, _ = frames.shape
        hs, ws, h, w = geo
        lib, p1 = self.lib, self.p1
        if not fused:
            # A level too large for 32-bit offsets into the split map (detect_batch cuts batches so that this does not happen; what is
            # left is a single frame beyond ~ 8K x 16K): the three P-Net layers as generic f32 launches.  Same results, slower - said aloud.
            if self.fused_pnet and not self._unfused_logged:
                self._unfused_logged = True
                logging.getLogger(__name__).warning("MTCNNHIP: a %d x %d pyramid level of %d frame(s) exceeds the fused P-Net's 32-bit map "
                                                    "offsets; it runs layer by layer (f32)", hs, ws, N)
            if getattr(self._tls, "path", None) is not None:
                self._tls.path["unfused_levels"] += 1
            x, h, w = self._dconv(None, p1, N, hs, ws, frames=frames)
            x, h, w = self._dconv(x, self.p2, N, h, w)
            head, h, w = self._dconv(x, self.p3, N, h, w)
            return head, h, w, self._i32(N * (-(-h * w // 256))), None, 0.0, None
        lo, hi = self._band_logits(band)
        coarse = self._coarse(coarse)
        t, entry = self._level_buffers(N, scale, geo, band, f16, cand[3:] if f16 else None, coarse)
        x, xs, head, wsp, cws = t["x"], t["xs"], t["head"], t["wsp"], t["cws"]
        p1w, p23 = (_lib.ptr(p1.w), _lib.ptr(p1.b), _lib.ptr(p1.slope)), [_lib.ptr(v) for v in self._p23]
        if f16:         # conv1 on the f16 matrix cores: the split map only (csrc/pnet_conv1.hip F16)
            lib.fr_pnet_conv1_band(0, self._fptr(frames), N, H, W, hs, ws, *p1w, None, _lib.ptr(xs), None, None, 0, self._s)
        else:
            self._dconv(None, p1, N, hs, ws, frames=frames, y_split=xs, y=x)
        if coarse > 0.0:
            lib.fr_pnet23_coarse_f16(_lib.ptr(x), _lib.ptr(xs), N, h, w, *p23, _lib.ptr(head), 2 if f16 else 0, lo, hi,
                                     _lib.ptr(self.refined_cells), _lib.ptr(wsp), wsp.numel() * 4, coarse, _lib.ptr(cws), cws.numel() * 4,
                                     _lib.ptr(self.visited_cells), self._s)
        else:
            lib.fr_pnet23_split_f16(_lib.ptr(x), _lib.ptr(xs), N, h, w, *p23, _lib.ptr(head),
                                    (1 if (self.p23_all_heads or trace is not None) else 0) | (2 if f16 else 0), lo, hi,
                                    _lib.ptr(self.refined_cells), _lib.ptr(wsp), wsp.numel() * 4, self._s)
        keep = None
        if f16:         # -> the conv1 tiles under the band cells' windows, EXACTLY (LIST) -> the exact pass + the candidates
            nt = lib.fr_pnet_band_tiles_count(N, h, w)
            tbuf, tiles = self._i32(1 + (nt + 31) // 32), self._i32(nt)
            lib.fr_pnet_band_tiles(_lib.ptr(wsp), N, h, w, _lib.ptr(tbuf), _lib.ptr(tiles), self._s)
            lib.fr_pnet_conv1_band(1, self._fptr(frames), N, H, W, hs, ws, *p1w, _lib.ptr(x), None, _lib.ptr(tiles), _lib.ptr(tbuf), nt, self._s)
            lib.fr_pnet_finish_levels((_lib.PnetLevel * 1)(entry), 1, N, *p23, cand[1], cand[2], lo, _lib.ptr(self.refined_cells), self._s)
            t.update(tbuf=tbuf, tiles=tiles)
            keep = (x, xs, head, wsp, tbuf, tiles, t["bc"])      # (cws: read by the two launches above only, on the stream it was allocated on)
        if self.level_tensors is not None:
            self.level_tensors.append(t)
        return head, h - 4, w - 4, t["bc"], wsp, lo, keep

    def pnet_level(self, frames, scale, trace=None, cand=None):
        """frames u8 [N,H,W,3] -> (head f32 [N,hc,wc,6], hc, wc) of one pyramid level.
        cand (batches): (scale, thr, cap, boxes, scores, regs, counts) of the level's candidate list - with conv1 on the f16 matrix
        cores (``split_pconv1``) the level extracts its candidates itself: ``_tls.level_done``, its tensors in ``_tls.keep``.
        ``_dl``: the logit-difference map and pre-filter fr_pnet_candidates takes otherwise."""
        N, H, W, _ = frames.shape
        geo = _level_geo(H, W, scale)
        fused = bool(self.fused_pnet) and N <= _frames32(*geo[2:])
        band = bool(self.pnet_band and _is_batch(self, N, H, W) and trace is None)
        f16 = fused and cand is not None and _f16_conv1(self, band, *geo[2:])
        coarse = self.coarse_margin if self.coarse_p23 and band else 0.0
        head, hc, wc, _, dl, dl_min, keep = self._level(frames, scale, geo, fused, band, f16, trace, cand, coarse)
        self._tls.dl, self._tls.level_done, self._tls.keep = (dl, dl_min), keep is not None, keep
        return head, hc, wc

    def _pnet_pyramid(self, frames, plan, cand):
        """The P-Net of ALL pyramid levels of a batch with every layer launched once, on the current stream
        (fr_pnet_pyramid_*: a block finds its level in a table, largest level first): conv1 (its f16 form over the levels
        ``split_pconv1`` selects, its f32 form over the rest) -> conv2/3/heads -> the exact conv1 tiles under the band cells of
        the f16 levels -> the exact pass + the candidates of every level.  The values are those of ``pnet_level`` per level, bit
        for bit; twelve levels are 9 launches instead of 64.  cand: (boxes, scores, regs, counts) with a leading level axis."""
        N, H, W, _ = frames.shape
        lib, p1, nlev = self.lib, self.p1, len(plan.scales)
        lo, hi = self._band_logits(plan.band)
        lv = (_lib.PnetLevel * nlev)()
        keep, ntile, words, coarse = [], 0, 0, self._coarse(plan.coarse)
        for li, (s, geo, f16) in enumerate(zip(plan.scales, plan.geo, plan.f16)):
            t, lv[li] = self._level_buffers(N, s, geo, plan.band, f16, [c[li] for c in cand], coarse)
            keep.append(t)
            if f16:
                nt = lib.fr_pnet_band_tiles_count(N, t["h"], t["w"])
                ntile, words = ntile + nt, words + (nt + 31) // 32
        p1w, p23 = (_lib.ptr(p1.w), _lib.ptr(p1.b), _lib.ptr(p1.slope)), [_lib.ptr(t) for t in self._p23]
        lib.fr_pnet_pyramid_conv1(0, self._fptr(frames), N, H, W, lv, nlev, *p1w, None, None, 0, self._s)
        if coarse > 0.0:
            cws = (ctypes.c_void_p * nlev)(*[t["cws"].data_ptr() for t in keep])
            lib.fr_pnet_pyramid_p23_coarse(lv, nlev, N, *p23, 0, lo, hi, coarse, cws, _lib.ptr(self.visited_cells), self._s)
        else:
            lib.fr_pnet_pyramid_p23(lv, nlev, N, *p23, 1 if self.p23_all_heads else 0, lo, hi, self._s)
        if ntile:
            tbuf, tiles = self._i32(1 + words), self._i32(ntile)
            lib.fr_pnet_pyramid_band_tiles(lv, nlev, N, _lib.ptr(tbuf), _lib.ptr(tiles), self._s)
            lib.fr_pnet_pyramid_conv1(1, self._fptr(frames), N, H, W, lv, nlev, *p1w, _lib.ptr(tiles), _lib.ptr(tbuf), ntile, self._s)
            keep[0].update(tbuf=tbuf, tiles=tiles)
        lib.fr_pnet_finish_levels(lv, nlev, N, *p23, self.thresholds[0], self.cap_scale, lo, _lib.ptr(self.refined_cells), self._s)
        if self.level_tensors is not None:
            self.level_tensors.extend(keep)

    @contextlib.contextmanager
    def _forked(self, main, n, events=None):
        """n side streams of the caller's stream ``main``, forked from it on entry and joined to it on exit: by ``wait_stream``, or -
        events: n + 1 of them, a call that is being recorded - by event pairs of the call's own that the call list notes down
        (FR_FN_EVENT_RECORD = 8 / FR_FN_STREAM_WAIT = 9)."""
        note = self.lib.note
        sides = self._sides.setdefault(main.cuda_stream, [])
        while len(sides) < n:
            sides.append(torch.cuda.Stream(device=self.device))
        sides = sides[:n]
        if events is None:
            for side in sides:
                side.wait_stream(main)
        else:
            events[0].record(main)
            note(8, events[0].cuda_event, main.cuda_stream)
            for side in sides:
                side.wait_event(events[0])
                note(9, side.cuda_stream, events[0].cuda_event)
        yield sides
        if events is None:
            for side in sides:
                main.wait_stream(side)
        else:
            for side, ev in zip(sides, events[1:]):
                ev.record(side)
                note(8, ev.cuda_event, side.cuda_stream)
                main.wait_event(ev)
                note(9, main.cuda_stream, ev.cuda_event)
        self._s = ctypes.c_void_p(main.cuda_stream)

    def _pnet_levels(self, frames, plan, trace, cand):
        """The P-Net and the candidates of every pyramid level, one launch chain per level: on the caller's stream (``plan.solo``), or level 0
        there and the levels 1.. dealt over side streams - of a recorded call without switching torch's stream: its work tensors are cached."""
        N, lib, t0, cs = plan.N, self.lib, self.thresholds[0], self.cap_scale
        events = (self._tls.rec or {}).get("events")
        forked = events is not None or not plan.solo
        main, keep = torch.cuda.current_stream(), []
        with (self._forked(main, len(events) - 1 if events else plan.nside, events) if forked else contextlib.nullcontext()) as sides:
            for li, s in enumerate(plan.scales):
                stream = sides[(li - 1) % len(sides)] if forked and li else main
                with (contextlib.nullcontext() if plan.solo else torch.cuda.stream(stream)):
                    if forked:
                        self._s = ctypes.c_void_p(stream.cuda_stream)
                    lcand = [c[li] for c in cand]
                    head, hc, wc, bc, dl, dl_min, done = self._level(
                        frames, s, plan.geo[li], plan.fused[li], plan.band, plan.f16[li], trace,
                        (float(s), t0, cs, *lcand) if plan.batch and trace is None else None, plan.coarse)
                    prob = self._f32(N, hc, wc) if trace is not None else None
                    if done is not None:                            # the level extracted its candidates itself
                        keep.append(done)
                    else:
                        lib.fr_pnet_candidates(_lib.ptr(head), N, hc, wc, float(s), t0, cs, *[_lib.ptr(c) for c in lcand], _lib.ptr(bc),
                                               _lib.ptr(prob), _lib.ptr(dl), dl_min, self._s)
                    if trace is not None:
                        trace.setdefault("pnet_head", []).append(head)
                        trace.setdefault("pnet_prob", []).append(prob)
        for grp in keep:                                    # allocated on a level stream, must outlive the kernels queued there
            for t in grp:
                t.record_stream(main)

    def _stage1(self, frames, plan, trace):
        """Pyramid + P-Net -> candidates per level -> per-level NMS 0.5 (keep_scale survivors; all levels in one launch) ->
        cross-level NMS 0.7 -> cap_p refined boxes per frame: (boxes, scores, regs, counts)."""
        N, nlev, cs, ksz = plan.N, len(plan.scales), self.cap_scale, self.keep_scale
        lb, ls, lr, lc = self._f32(nlev, N, cs, 4), self._f32(nlev, N, cs), self._f32(nlev, N, cs, 4), self._i32(nlev, N)
        kb, ks, ka, kc = self._f32(nlev, N, ksz, 4), self._f32(nlev, N, ksz), self._f32(nlev, N, ksz, 4), self._i32(nlev, N)
        if self.level_tensors is not None:
            del self.level_tensors[:]
        if plan.pyramid:
            self._pnet_pyramid(frames, plan, (lb, ls, lr, lc))
        else:
            self._pnet_levels(frames, plan, trace, (lb, ls, lr, lc))
        self._mark("pnet")
        if self.level_tensors is not None:
            self.level_tensors.append(dict(cand=(lb, ls, lr, lc)))      # the candidate lists [level, frame, slot]
        self._nms(lb, ls, lr, 4, lc, nlev * N, 1, cs, 0, 0.5, 0, ksz, out=(kb, ks, ka, kc))
        b1, s1, a1, c1 = self._nms(kb, ks, ka, 4, kc, N, nlev, ksz, 1, 0.7, 0, self.cap_p)
        self.lib.fr_box_refine(_lib.ptr(b1), _lib.ptr(a1), 4, _lib.ptr(c1), N, self.cap_p, 0, self._s)
        self._mark("stage1_nms")
        if trace is not None:
            trace.update(stage1_boxes=b1, stage1_scores=s1, stage1_counts=c1)
        return b1, s1, a1, c1

    # ---- R-Net, O-Net
    def crop_conv1(self, net, frames, boxes, counts, cap):
        """frames u8 [N,H,W,3], boxes f32 [N,cap,4], counts i32 [N] -> the net's pooled conv1 map of every valid slot."""
        N, H, W, _ = frames.shape
        t = _RO[net]
        w, b, s = getattr(self, t.w1)
        y = self._f32(N * cap, t.map1[0], t.map1[0], t.map1[1])
        self.lib.fr_crop_conv1_f32(net, self._fptr(frames), N, H, W, _lib.ptr(boxes), _lib.ptr(counts), cap, _lib.ptr(w),
                                   _lib.ptr(b), _lib.ptr(s), _lib.ptr(y), self._s)
        return y

    def crop_conv12_split(self, net, frames, boxes, counts, cap):
        """crop -> conv1 -> pool (map written as split f16) -> conv2 -> pool on the f16 matrix cores: the net's pooled conv2
        map of every valid slot, f32 [N*cap, 4, 4, 48] / [N*cap, 10, 10, 64]."""
        N, H, W, _ = frames.shape
        t = _RO[net]
        (w1, b1, s1), (w2, b2, s2) = getattr(self, t.w1), getattr(self, t.w2)
        xs = self._new((N * cap, t.map1[0] ** 2, 128), torch.uint8)
        self.lib.fr_crop_conv1_split(net, self._fptr(frames), N, H, W, _lib.ptr(boxes), _lib.ptr(counts), cap, _lib.ptr(w1),
                                     _lib.ptr(b1), _lib.ptr(s1), _lib.ptr(xs), 1 if self.split_conv1 else 0, self._s)
        y = self._f32(N * cap, t.map2[0], t.map2[0], t.map2[1])
        lc = self._i32(1)                   # the exact pass's list counter: cleared by the conv2 kernel, filled by fr_ro_margin_list
        self.lib.fr_ro_conv2_split(net, _lib.ptr(xs), _lib.ptr(w2), _lib.ptr(b2), _lib.ptr(s2), _lib.ptr(y), N * cap,
                                   _lib.ptr(counts), cap, _lib.ptr(lc), self._s)
        return y, lc

    def exact_pass(self, net, frames, boxes, counts, cap, head, thr, lc):
        """The split-precision heads ``head`` [N*cap, 6 | 16] of the crops whose logit difference lies within ``ro_margin`` of
        the stage threshold are replaced by those of the all-f32 layers (compact work list, device-side count: no sync)."""
        N, H, W, _ = frames.shape
        t = _RO[net]
        w1, b1, s1 = getattr(self, t.w1)
        lcap, nh = self.ro_list_cap[net], head.shape[1]
        lst = self._i32(lcap)
        self.lib.fr_ro_margin_list(_lib.ptr(head), nh, _lib.ptr(counts), N, cap, math.log(thr / (1.0 - thr)), self.ro_margin,
                                   _lib.ptr(lst), _lib.ptr(lc), lcap, self._s)
        x1 = self._f32(lcap, t.map1[0], t.map1[0], t.map1[1])
        self.lib.fr_crop_conv1_list_f32(net, self._fptr(frames), N, H, W, _lib.ptr(boxes), cap, _lib.ptr(lst), _lib.ptr(lc), lcap,
                                        _lib.ptr(w1), _lib.ptr(b1), _lib.ptr(s1), _lib.ptr(x1), self._s)
        exact = getattr(self, t.name)(None, lcap, lc, lcap, x1=x1)
        self.lib.fr_ro_scatter_rows(_lib.ptr(exact), _lib.ptr(lst), _lib.ptr(lc), lcap, nh, _lib.ptr(head), self._s)
        # diagnostics / bench.py (``_ro_lists``): how many crops the exact pass took, THIS thread's last call (or last chunk of it)
        self._tls.__dict__.setdefault("ro_lists", {})[net] = lc
        # this thread's record of the call (every chunk of it): the device counter beside its capacity, read by exact_lists()
        self._tls.path["exact_lists"].append((net, lcap))
        self._tls.exact_counters.append(lc)

    @property
    def _ro_lists(self):
        """{net: device counter of its exact work list} of this thread's last split R-/O-Net pass; {} before the first."""
        return getattr(self._tls, "ro_lists", {})

    def exact_lists(self):
        """The exact R-/O-Net work lists of this thread's last ``detect_batch`` call, one entry per list in launch order (R-Net,
        O-Net, for every chunk of the call): dicts {"net": "rnet" | "onet", "count": crops that qualified, "cap": list capacity}.
        Synchronises the device.  A count above its cap is an overflow: the crops past the cap kept their split-precision
        heads (include/frhip.h fr_ro_margin_list)."""
        path = getattr(self._tls, "path", None)
        if not path:
            return []
        torch.cuda.synchronize(self.device)
        return [{"net": _RO[net].name, "count": int(lc[0]), "cap": cap}
                for (net, cap), lc in zip(path["exact_lists"], self._tls.exact_counters)]

    def exact_list_overflow(self):
        """The nets ("rnet", "onet") whose exact work list overflowed in this thread's last call (any chunk); [] when none did.
        Synchronises the device."""
        return sorted({e["net"] for e in self.exact_lists() if e["count"] > e["cap"]}, key=("rnet", "onet").index)

    def _net(self, t, x, B, counts, cap, x1, x2):
        """R-Net / O-Net (``t``: its row of _RO) from the crops ``x``, from conv1's pooled map ``x1`` or from conv2's ``x2`` -
        then the tail layers are the split-precision GEMMs of the batch path (csrc/ro_gemm.hip) - to the heads [B, 6 | 16]."""
        k = dict(counts=counts, cap=cap)
        layers = [getattr(self, n) for n in t.layers]
        if x2 is not None:
            x, h, w = x2, t.map2[0], t.map2[0]
        else:
            x, h, w = (x1, t.map1[0], t.map1[0]) if x1 is not None else self._dconv(x, layers[0], B, t.crop, t.crop, **k)
            x, h, w = self._dconv(x, layers[1], B, h, w, **k)
        for c in layers[2:-1]:
            if x2 is not None:
                h, w = c.out_hw(h, w)
                x = self._gemm_split(c.layer, x, B, (h, w, c.cout), counts, cap)
            else:
                x, h, w = self._dconv(x, c, B, h, w, **k)
        x, _, _ = self._dconv(x, layers[-1], B, 1, 1, **k)
        return x.reshape(B, t.nhead)

    def rnet(self, x, B, counts=None, cap=0, x1=None, x2=None):
        """counts / cap: only the first counts[frame] of a frame's cap crop slots are computed (device-side).
        x1: conv1's pooled map when it was computed straight from the frames (crop_conv1); x2: conv2's (crop_conv12_split)."""
        return self._net(_RO[0], x, B, counts, cap, x1, x2)

    def onet(self, x, B, counts=None, cap=0, x1=None, x2=None):
        return self._net(_RO[1], x, B, counts, cap, x1, x2)

    def _refine_stage(self, net, frames, boxes, counts, plan, trace, out=None):
        """Stage 2 (net 0: R-Net) / stage 3 (net 1: O-Net) over the boxes [N, cap, 4] of the stage before: crops -> net -> the
        crops at or above the stage's threshold -> (boxes, scores, aux, counts) with the stage's output capacity."""
        t = _RO[net]
        N, H, W, _ = frames.shape
        lib, run, thr, crops = self.lib, getattr(self, t.name), self.thresholds[1 + net], None
        cap, cap_out = getattr(self, t.cap_in), getattr(self, t.cap_out)
        if plan.split:                              # conv2 on the f16 matrix cores (split precision) + exact pass at the threshold
            y, lc = self.crop_conv12_split(net, frames, boxes, counts, cap)
            head = run(None, N * cap, counts, cap, x2=y)
            self.exact_pass(net, frames, boxes, counts, cap, head, thr, lc)
        elif self.fused_crop and trace is None:     # crop + conv1 + pool in one kernel: no crop tensor in HBM
            head = run(None, N * cap, counts, cap, x1=self.crop_conv1(net, frames, boxes, counts, cap))
        else:
            crops = self._f32(N * cap, t.crop, t.crop, 4)
            lib.fr_crop_resize_norm(self._fptr(frames), N, H, W, _lib.ptr(boxes), _lib.ptr(counts), cap, t.crop, _lib.ptr(crops), self._s)
            head = run(crops, N * cap, counts, cap)
        sb, ss, sa, sc = self._f32(N, cap, 4), self._f32(N, cap), self._f32(N, cap, t.naux), self._i32(N)
        prob = self._f32(N, cap) if trace is not None else None
        lib.fr_stage_select(_lib.ptr(boxes), _lib.ptr(head), t.nhead, _lib.ptr(counts), N, cap, thr, _lib.ptr(sb), _lib.ptr(ss),
                            _lib.ptr(sa), t.naux, _lib.ptr(sc), _lib.ptr(prob), self._s)
        if net == 0:                                # select -> NMS -> refine
            res = self._nms(sb, ss, sa, t.naux, sc, N, 1, cap, 0, 0.7, 0, cap_out)
            lib.fr_box_refine(_lib.ptr(res[0]), _lib.ptr(res[2]), t.naux, _lib.ptr(res[3]), N, cap_out, t.refine, self._s)
        else:                                       # select -> refine -> the final NMS, into the call's result tensors
            lib.fr_box_refine(_lib.ptr(sb), _lib.ptr(sa), t.naux, _lib.ptr(sc), N, cap, t.refine, self._s)
            self._tls.cache = None                  # what is returned to the caller is never a cached work tensor
            res = self._nms(sb, ss, sa, t.naux, sc, N, 1, cap, 0, 0.7, 1, cap_out, out=out, results=True)
        self._mark("stage%d" % (2 + net))
        if trace is not None:
            trace.update({t.name + "_head": head, t.name + "_prob": prob})
            if net == 0:
                trace.update(rnet_crops=crops, stage2_boxes=res[0], stage2_scores=res[1], stage2_counts=res[3])
        return res

    def _mark(self, name):
        if self.phase_marks is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.phase_marks.append((name, e))

    # ---- the work-tensor cache and the call recorder of eager few-frame calls
    def _begin(self, frames, plan):
        """An eager call of few frames (``plan.cache``) takes its work tensors from ``_new``'s cache (the four most recent frame shapes are
        kept).  From the second call of a shape on every work tensor is the cached one, so the call is the same list of C calls with the same
        arguments - but for the frame and the four result tensors.  It is recorded once (on the second call: the first filled the cache) and
        replayed by ONE C call from the third on (fr_detect_sequence): an eager single-frame call waited for the interpreter's ~50 ctypes calls.
        -> the recorded list to replay instead of running the cascade, or None; ``_tls.rec``: the call's key, configuration, ``events`` while recording."""
        tls = self._tls
        tls.rec = None
        if not plan.cache:
            return None
        caches, seqs = tls.__dict__.setdefault("caches", {}), tls.__dict__.setdefault("seqs", {})
        key = (*frames.shape[:3], torch.cuda.current_stream().cuda_stream)
        if key not in caches and len(caches) >= 4:
            old_key = next(iter(caches))                    # oldest frame shape of this thread
            caches.pop(old_key); seqs.pop(old_key, None)
        known = key in caches
        tls.cache = [caches.setdefault(key, []), 0]
        cfg = (self.fused_pnet, self.fused_crop, self.p23_all_heads, self.thresholds, self.refine_margin,
               self.cap_scale, self.keep_scale, self.cap_p, self.cap_r, self.cap_o, self.minsize, self.factor, self.coarse_p23, self.coarse_margin)
        seq = seqs.get(key)
        if seq is not None and (not plan.recorder or seq["cfg"] != cfg):
            seqs.pop(key)                                   # recorded under another configuration: never replayed again
            seq = None
        if seq is not None:
            tls.cache = None
            return seq
        tls.rec = {"key": key, "cfg": cfg, "events": None}
        if plan.recorder and known:
            self.lib.start_recording()
            # The recorded call deals the levels 1.. over side streams, forked and joined by events of its own (_forked; the call list carries
            # their record / wait): replayed by one C call the host is no longer what the GPU waits for, the serial chain of ten levels is
            tls.rec["events"] = [torch.cuda.Event() for _ in range(1 + min(4, max(1, len(plan.scales) - 1)))]

    def _end(self, frames, outs):
        """Closes what ``_begin`` opened: a recording becomes this frame shape's call list, unless it is unusable."""
        tls = self._tls
        rec, tls.rec = tls.rec, None
        if rec is None:
            return
        if rec["events"] is not None:
            calls = self.lib.stop_recording()           # None: a launch the list cannot express happened (Lib.recording_invalid)
            if calls and not tls.cache_grew:
                seq = self._make_sequence(calls, frames, outs, rec["cfg"])
                if seq is not None:
                    seq["events"] = rec["events"]               # the call list holds their handles
                    tls.seqs[rec["key"]] = seq
        if tls.cache_grew:
            # a work tensor was replaced in this call (recording or not): a list recorded earlier for this frame shape
            # holds the freed tensor's pointer
            tls.seqs.pop(rec["key"], None)

    # ---- cascade
    def detect_batch(self, frames, trace=None, level_streams=None, _out=None):
        """frames: uint8 [N,H,W,3] BGR device tensor (contiguous).

        level_streams: side HIP streams (1 or 2) the pyramid levels 1.. are dealt over; level 0 stays on the caller's
        stream.  (Per-level launches only: a batch under ``pyramid_launch`` runs its whole P-Net on the caller's stream.)
        Default ``self.level_streams``.  _out: the result tensors' rows of a group of frames of a larger call (``plan.chunks``).

        Returns device tensors: boxes f32 [N,cap_o,4], scores f32 [N,cap_o], kps f32 [N,cap_o,5,2],
        counts i32 [N] (faces per frame, in descending-score order).

        ``_tls.path`` (this thread's last call): which arithmetic ran - {"frames", "batch", "chunks", "fused_levels", "band_levels", "coarse_levels" [fused levels run in two tiers, ``coarse_p23``],
        "pconv1_mfma_levels" [(h, w) of the conv1 maps computed on the f16 matrix cores], "unfused_levels", "split_ro",
        "exact_lists" [(net, list capacity) of every exact R-/O-Net pass, all chunks]} - so that a test can assert the path it means
        to test was the one taken (the decisions are ``detect_plan``'s); ``exact_lists()`` / ``exact_list_overflow()`` read the lists' counters."""
        assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3 and frames.is_contiguous()
        N, H, W, _ = frames.shape
        with torch.cuda.device(self.device):
            plan = detect_plan(N, H, W, self, trace is not None, level_streams, _out is not None, torch.cuda.is_current_stream_capturing())
            if _out is None:
                self._tls.path = {"frames": N, "batch": plan.batch, "chunks": max(1, len(plan.chunks)), "fused_levels": 0, "band_levels": 0, "coarse_levels": 0,
                                  "pconv1_mfma_levels": [], "unfused_levels": 0, "split_ro": False, "exact_lists": []}
                self._tls.exact_counters = []       # device counters of the exact lists of path["exact_lists"] (no sync here)
            if plan.chunks:
                out = tuple(torch.empty(sh, dtype=dt, device=self.device) for sh, dt in (
                    ((N, self.cap_o, 4), torch.float32), ((N, self.cap_o), torch.float32), ((N, self.cap_o, 14), torch.float32), ((N,), torch.int32)))
                for n0, n1 in plan.chunks:
                    self.detect_batch(frames[n0:n1], None, level_streams, _out=tuple(t[n0:n1] for t in out))
                return out[0], out[1], out[2][..., 4:14].unflatten(-1, (5, 2)), out[3]
            self._s = _lib.stream_ptr()
            self._tls.cache, self._tls.cache_grew = None, False         # (a call that raised may have left these set)
            self.lib.stop_recording()
            self._mark("start")
            if not plan.scales:                 # frame smaller than one 12-px cell at the coarsest usable scale
                z = torch.zeros((N, self.cap_o, 14), dtype=torch.float32, device=self.device)
                return (z[..., :4].contiguous(), z[..., 0].contiguous(), z[..., 4:14].unflatten(-1, (5, 2)),
                        torch.zeros(N, dtype=torch.int32, device=self.device))
            assert len(plan.scales) * self.keep_scale <= 4096, "too many pyramid levels for the merged NMS list"
            seq = self._begin(frames, plan)
            if seq is not None:
                return self._replay(seq, frames)
            b1, _, _, c1 = self._stage1(frames, plan, trace)
            self._tls.path["split_ro"] = plan.split
            b2, _, _, c2 = self._refine_stage(0, frames, b1, c1, plan, trace)
            b3, s3, a3, c3 = self._refine_stage(1, frames, b2, c2, plan, trace, out=_out)
            self._end(frames, (b3, s3, a3, c3))
            # aux = (reg4, (x1,y1)..(x5,y5)): kps is a strided view, no copy
            return b3, s3, a3[..., 4:14].unflatten(-1, (5, 2)), c3

    def _make_sequence(self, calls, frames, outs, cfg):
        """The recorded C calls of one eager single-frame detect_batch as an fr_call array.  The slots a replay patches -
        the frame and the four result tensors - are those the call sites passed WITH that role (_lib.RolePtr: ``_fptr``,
        ``_nms(results=True)``), noted by the recorder beside the call; no slot is found by comparing pointer values.  The
        values only serve as a check: a slot that holds the frame's or a result's address without the role would be a
        call site that forgot it, and the list is refused: None is returned, nothing is cached for the frame shape, the call
        that was being recorded has already produced its (valid, eager) results and later calls stay eager."""
        log = logging.getLogger(__name__)
        arr = (_lib.Call * len(calls))()
        want = {"frame": frames.data_ptr(), **{"out%d" % i: t.data_ptr() for i, t in enumerate(outs)}}
        fpos, opos = [], [[] for _ in outs]
        for k, (fid, slots, roles) in enumerate(calls):
            arr[k].fn, arr[k].nargs = fid, len(slots)
            for i, v in enumerate(slots):
                arr[k].a[i] = v
            tagged = dict(roles)
            for i, role in roles:
                if slots[i] != want[role]:
                    log.warning("MTCNNHIP: recorded call %d: slot %d carries the role '%s' but holds another tensor; call list refused", k, i, role)
                    return None
                (fpos if role == "frame" else opos[int(role[3:])]).append((k, i))
            if fid < 8:                              # (event / stream handles of the pseudo calls are not tensors)
                for i, v in enumerate(slots):
                    if i not in tagged and v in want.values():
                        log.warning("MTCNNHIP: recorded call %d: slot %d holds a patched tensor without its role; call list refused", k, i)
                        return None
        if not fpos or not all(opos):
            log.warning("MTCNNHIP: the recorded call list does not mention the frame and every result tensor; refused")
            return None
        return {"arr": arr, "n": len(calls), "fpos": fpos, "opos": opos, "cfg": cfg,
                "meta": [(tuple(t.shape), t.dtype) for t in outs]}

    def _replay(self, seq, frames):
        arr = seq["arr"]
        outs = [torch.empty(shape, dtype=dtype, device=self.device) for shape, dtype in seq["meta"]]
        fptr = frames.data_ptr()
        for k, i in seq["fpos"]:
            arr[k].a[i] = fptr
        for t, pos in zip(outs, seq["opos"]):
            p = t.data_ptr()
            for k, i in pos:
                arr[k].a[i] = p
        self.lib.fr_detect_sequence(arr, seq["n"])
        b3, s3, a3, c3 = outs
        return b3, s3, a3[..., 4:14].unflatten(-1, (5, 2)), c3
