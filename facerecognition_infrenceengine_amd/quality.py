"""Face quality: judge each aligned face on the device, so that the embed net and the gallery scan run for the fit ones only.

The engine spends the embed net and a gallery scan on every detected face, whatever it looks like: a motion-blurred face, a
20-pixel speck, a blown-out crop or a near-profile is not recognisable, yet its embedding is matched, counted and enrolled as if
it meant something (the reference embeds every face too, infrenceServer.py:528-532).  ``warp_affine_5pt`` writes every face as a
112 x 112 crop in fixed geometry, so sharpness, exposure and contrast measured on the crop compare between a 30-pixel and a
600-pixel face, and pose and resolution follow from the five landmarks.  One launch (csrc/face_quality.hip) measures all of it
in exact integers and float32 terms without a division; the arithmetic and the verdict bits are include/frhip.h
fr_face_quality_f16 and DESIGN.md 4.5e.
"""
import numpy as np
import torch

from . import _lib

SMALL, DARK, BRIGHT, FLAT, BLURRED, CLIPPED, YAW, PITCH = 1, 2, 4, 8, 16, 32, 64, 128
REASONS = ((SMALL, "small"), (DARK, "dark"), (BRIGHT, "bright"), (FLAT, "flat"), (BLURRED, "blurred"), (CLIPPED, "clipped"),
           (YAW, "yaw"), (PITCH, "pitch"))
WINDOW_PIXELS = 6400


class FaceQuality:
    """The thresholds of the verdict and the launch that measures a batch of aligned faces.

    Every default is a judgment, not a measurement: the tree has only synthetic weights, and real faces have not been measured
    against any of these numbers.  ``min_eye=12``: an eye distance below 12 frame pixels is a face some 30 pixels wide, enlarged
    more than three times into the crop.  ``mean_lo=40, mean_hi=215``: the mean luma of the face interior.  ``contrast_min=100``:
    a luma variance of 100 is a standard deviation of 10 grey levels.  ``sharp_min=50``: the variance of the 4-neighbour
    Laplacian.  ``clip_max=1600``: a quarter of the 6400 window pixels at or below 15 or at or above 240.  ``yaw_max=0.5``: the
    nose's projection on the eye line may leave the middle by a quarter of the eye distance.  ``pitch_lo=0.25, pitch_hi=0.75``: the
    nose's distance below the eye line as a share of the mouth's (0.495 on the template).

    The object validates its arguments and holds no device state: one may be shared by every caller and thread."""

    def __init__(self, device="cuda:0", min_eye=12, mean_lo=40, mean_hi=215, contrast_min=100, sharp_min=50, clip_max=1600,
                 yaw_max=0.5, pitch_lo=0.25, pitch_hi=0.75):
        min_eye, yaw_max, pitch_lo, pitch_hi = float(min_eye), float(yaw_max), float(pitch_lo), float(pitch_hi)
        if not (0.0 <= min_eye and float(np.float32(min_eye) * np.float32(min_eye)) <= 3.0e38):
            raise ValueError("min_eye must be a finite, non-negative number of pixels")
        if not (0 <= int(mean_lo) <= 255 and 0 <= int(mean_hi) <= 255):
            raise ValueError("mean_lo and mean_hi lie in 0 .. 255")
        if int(contrast_min) < 0 or int(sharp_min) < 0:
            raise ValueError("contrast_min and sharp_min are not negative")
        if not 0 <= int(clip_max) <= WINDOW_PIXELS:
            raise ValueError(f"clip_max lies in 0 .. {WINDOW_PIXELS}")
        if not yaw_max >= 0.0:
            raise ValueError("yaw_max is not negative (infinity switches the test off)")
        if not pitch_lo <= pitch_hi:
            raise ValueError("pitch_lo must not exceed pitch_hi")
        self.device = torch.device(device)
        self.min_eye, self.min_eye2 = min_eye, float(np.float32(min_eye) * np.float32(min_eye))
        self.mean_lo, self.mean_hi, self.contrast_min = int(mean_lo), int(mean_hi), int(contrast_min)
        self.sharp_min, self.clip_max = int(sharp_min), int(clip_max)
        self.yaw_max, self.pitch_lo, self.pitch_hi = yaw_max, pitch_lo, pitch_hi

    def limits(self):
        """the scalar arguments of fr_face_quality_f16, in its order"""
        return (self.min_eye2, self.mean_lo, self.mean_hi, self.contrast_min, self.sharp_min, self.clip_max, self.yaw_max,
                self.pitch_lo, self.pitch_hi)

    def measure_device(self, crops, kps, counts=None, cap=None):
        """``crops``: f16 ``[S,112,112,8]`` as the alignment writes them; ``kps``: f32 ``[S,5,2]`` (or ``[N,cap,5,2]``) in frame
        pixels, both contiguous and on the device of the crops.  ``counts`` i32 ``[S / cap]`` with ``cap``: the slot form - slot
        ``s`` holds a face iff ``s % cap < counts[s // cap]``, and a slot without one is not read (verdict -1, zeros).  Without
        them every row holds a face.  Returns ``(qi i32 [S,8], qf f32 [S,4], verdict i32 [S])``, device tensors written on the
        current stream; no synchronisation."""
        if not (torch.is_tensor(crops) and crops.dtype == torch.float16 and crops.dim() == 4
                and tuple(crops.shape[1:]) == (112, 112, 8) and crops.is_contiguous() and crops.is_cuda):
            raise ValueError("crops must be a contiguous f16 [S,112,112,8] device tensor")
        S = crops.shape[0]
        if not (torch.is_tensor(kps) and kps.dtype == torch.float32 and kps.numel() == S * 10 and kps.is_contiguous()
                and kps.device == crops.device):
            raise ValueError("kps must be a contiguous f32 [S,5,2] tensor on the crops' device")
        if (counts is None) != (cap is None):
            raise ValueError("counts and cap come together")
        if counts is not None:
            cap = int(cap)
            if cap < 1 or S % cap or not (torch.is_tensor(counts) and counts.dtype == torch.int32 and counts.numel() == S // cap
                                          and counts.is_contiguous() and counts.device == crops.device):
                raise ValueError("counts must be a contiguous i32 [S / cap] tensor on the crops' device, cap a divisor of S")
        lib = _lib.load()
        with torch.cuda.device(crops.device):
            qi = torch.empty((S, 8), dtype=torch.int32, device=crops.device)
            qf = torch.empty((S, 4), dtype=torch.float32, device=crops.device)
            verdict = torch.empty(S, dtype=torch.int32, device=crops.device)
            lib.fr_face_quality_f16(_lib.ptr(crops), _lib.ptr(kps), _lib.ptr(counts), cap or 0, S, _lib.ptr(qi), _lib.ptr(qf),
                                    _lib.ptr(verdict), *self.limits(), _lib.stream_ptr())
        return qi, qf, verdict

    @staticmethod
    def describe(qi_row, qf_row, verdict):
        """One face's row on the host -> the dict callers see.  ``ok`` is False for a slot without a face (verdict -1) too."""
        v = int(verdict)
        return {"mean": int(qi_row[0]), "contrast": int(qi_row[1]), "sharp": int(qi_row[2]), "dark": int(qi_row[3]),
                "bright": int(qi_row[4]), "eye_dist": float(np.sqrt(max(float(qf_row[0]), 0.0))), "ok": v == 0,
                "reasons": [name for bit, name in REASONS if v > 0 and v & bit]}
