"""The premise of the P-Net's coarse pass (csrc/pnet_fused.hip pnet23_body<true>), on the host: with only the hi
halves of the split operands - every operand of conv2, conv3 and the heads rounded to f16, f32 sums - the logit difference of a
cell moves by far less than ``coarse_margin``, and few cells lie within the margin below the exact pass's pre-filter.

Two synthetic 270 x 480 frames over all pyramid levels, the synthetic weights at the scale the detector runs them (canonical_scale),
the conv1 map in float64 rounded to f32 as the kernels' input; the emulation is tests/helpers/pnet_coarse_ref.py."""
import math
import os
import sys

import numpy as np
import torch

from facerecognition_infrenceengine_amd import weights
from facerecognition_infrenceengine_amd.mtcnn import DetectSettings, canonical_scale, pyramid_scales
from oracle import detect as odetect
from tests.helpers import detect_ref as ref
from tests.helpers import pnet_coarse_ref as C

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))


def test_hi_only_error_and_extra_cells_on_synthetic_frames():
    from make_golden import synth_frame
    p = weights.synth_mtcnn_states()[0]
    L = ref.pnet_layers(canonical_scale({k: v.detach().float().cpu() for k, v in p.items()}, "pnet"))
    H, W = 270, 480
    errs, dls, rms = [], [], []
    for f in range(2):
        rgb = synth_frame(H, W, 600 + f)[:, :, ::-1].astype(np.float32)
        for s in pyramid_scales(H, W, 20, 0.709):
            hs, ws = int(math.ceil(H * s)), int(math.ceil(W * s))
            x = torch.as_tensor(odetect._to_net(odetect.resize_bilinear(rgb, hs, ws)))
            x1 = ref.apply(L[0], (x[None] if x.dim() == 3 else x).double(), 0.0)[0].float()
            if min(x1.shape[2:]) < 5:
                continue
            d64 = C.dl_f64(x1, L[1], L[2])
            errs.append((C.dl_hi_only(x1, L[1], L[2]).double() - d64).abs().flatten())
            dls.append(d64.flatten())
            rms.append((float(x1.double().pow(2).sum()), x1.numel()))
    err, dl = torch.cat(errs), torch.cat(dls)
    thr = math.log(0.6 / 0.4) - 2e-3                       # mtcnn.py _band_logits: the exact pass's pre-filter
    kept = float((dl >= thr).double().mean())
    extra = float(((dl >= thr - 0.05) & (dl < thr)).double().mean())
    pooled = math.sqrt(sum(q for q, _ in rms) / sum(n for _, n in rms))
    lo, hi = (f(math.sqrt(q / n) for q, n in rms) for f in (min, max))
    print(f"{err.numel()} cells over {len(errs)} levels: hi-only error of dl max {float(err.max()):.3e}, median {float(err.median()):.3e}; "
          f"dl std {float(dl.std()):.2f}; kept {100 * kept:.2f} %, within 0.05 below {100 * extra:.2f} %; conv1 map RMS {pooled:.3f} ({lo:.2f} - {hi:.2f} by level)")
    assert err.numel() >= 30_000 and 0.001 < kept < 0.05
    assert 20 * float(err.max()) <= 0.05 <= DetectSettings.coarse_margin
    assert extra < 0.01
    assert pooled <= 0.45                                  # tests/test_gpu_pnet_coarse.py MAP_RMS: the envelope's maps are no smaller
