"""The DEFINITION of the eight EXIF orientations (tag 0x0112), as plain NumPy views: what a decoder that honours the tag returns
for a picture coded as ``img``.  ``jpeg_decode.orient`` in the package is its independent twin; the kernel
(csrc/jpeg_decode.hip jpegd_colour_oriented) is compared against this one."""
import numpy as np


def orient(img, o):
    """``[H,W,C]`` -> ``[H,W,C]`` for 1 .. 4, ``[W,H,C]`` for 5 .. 8"""
    x = np.asarray(img)
    if o == 1:
        return x
    if o == 2:
        return x[:, ::-1]
    if o == 3:
        return x[::-1, ::-1]
    if o == 4:
        return x[::-1]
    if o == 5:
        return x.transpose(1, 0, 2)
    if o == 6:
        return np.rot90(x, -1)
    if o == 7:
        return x[::-1, ::-1].transpose(1, 0, 2)
    if o == 8:
        return np.rot90(x, 1)
    raise ValueError(f"EXIF orientation {o} is not 1 .. 8")
