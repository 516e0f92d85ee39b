"""The DEFINITION of the device JPEG encoder's bytes (csrc/jpeg_encode.hip), in NumPy, integers only.

Baseline JPEG, 4:2:0, the Annex K Huffman tables, one restart interval per MCU row.  ``encode(bgr, quality)`` returns the file's
bytes; the kernel reproduces them byte for byte.  The tables come from the package's jpeg_tables module; everything else - the
header, the colour transform, libjpeg's integer forward DCT, the quantiser and the entropy coder of T.81 F.1.2 - is written out
here.  PIL decodes what this writes (tests/test_jpeg_ref_host.py), which is the independent judgement that it is a JPEG of the
picture."""
import struct

import numpy as np

from facerecognition_infrenceengine_amd import jpeg_tables as T

C = (2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172)
CONST_BITS, PASS1_BITS = 13, 2


def header(h, w, quality):
    """SOI .. SOS for an h x w picture"""
    q = T.quant_tables(quality)
    out = [b"\xff\xd8", b"\xff\xe0" + struct.pack(">H5sBBBHHBB", 16, b"JFIF\0", 1, 1, 0, 1, 1, 0, 0)]
    for tid in (0, 1):
        out.append(b"\xff\xdb" + struct.pack(">HB", 67, tid) + bytes(int(v) for v in q[tid][T.ZIGZAG]))
    out.append(b"\xff\xc0" + struct.pack(">HBHHB", 17, 8, h, w, 3) + bytes((1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for tc_th in (0x00, 0x10, 0x01, 0x11):
        bits, vals = T.HUFFMAN[tc_th]
        out.append(b"\xff\xc4" + struct.pack(">HB", 19 + len(vals), tc_th) + bytes(bits) + bytes(vals))
    out.append(b"\xff\xdd" + struct.pack(">HH", 4, (w + 15) // 16))
    out.append(b"\xff\xda" + struct.pack(">HB", 12, 3) + bytes((1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))
    return b"".join(out)


def ycbcr(bgr):
    """JFIF full-range Y, Cb, Cr planes (int32) of a uint8 [H, W, 3] BGR picture, libjpeg's 16-bit fixed point"""
    b, g, r = (bgr[..., k].astype(np.int32) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _pass(d, first):
    """one 1-D pass of jfdctint over the last axis of int32 [..., 8]"""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., k] for k in range(8))
    tmp0, tmp7, tmp1, tmp6 = d0 + d7, d0 - d7, d1 + d6, d1 - d6
    tmp2, tmp5, tmp3, tmp4 = d2 + d5, d2 - d5, d3 + d4, d3 - d4
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    n = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS
    out = [None] * 8
    if first:
        out[0], out[4] = (tmp10 + tmp11) << PASS1_BITS, (tmp10 - tmp11) << PASS1_BITS
    else:
        out[0], out[4] = _descale(tmp10 + tmp11, PASS1_BITS), _descale(tmp10 - tmp11, PASS1_BITS)
    z1 = (tmp12 + tmp13) * C[2]
    out[2] = _descale(z1 + tmp13 * C[3], n)
    out[6] = _descale(z1 - tmp12 * C[7], n)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * C[5]
    tmp4, tmp5, tmp6, tmp7 = tmp4 * C[0], tmp5 * C[9], tmp6 * C[11], tmp7 * C[6]
    z1, z2, z3, z4 = -z1 * C[4], -z2 * C[10], -z3 * C[8] + z5, -z4 * C[1] + z5
    out[7], out[5] = _descale(tmp4 + z1 + z3, n), _descale(tmp5 + z2 + z4, n)
    out[3], out[1] = _descale(tmp6 + z2 + z3, n), _descale(tmp7 + z1 + z4, n)
    return np.stack(out, axis=-1)


def fdct(blocks):
    """libjpeg's integer "islow" forward DCT of int32 [..., 8, 8] (samples - 128): rows, then columns; scaled by 8"""
    rows = _pass(blocks.astype(np.int32), True)
    return np.swapaxes(_pass(np.swapaxes(rows, -1, -2), False), -1, -2)


def quantise(coef, table):
    """int32 [..., 64] natural order; table int32 [64]: sign(c) * ((|c| + (qv >> 1)) // qv) with qv = t << 3"""
    qv = table.astype(np.int32) << 3
    mag = (np.abs(coef) + (qv >> 1)) // qv
    return np.where(coef < 0, -mag, mag).astype(np.int32)


def _blocks(plane):
    """int32 [h, w] (multiples of 8) -> [h/8, w/8, 8, 8]"""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).swapaxes(1, 2)


def _category(v):
    return int(abs(int(v))).bit_length()


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length

    def flush(self):
        """the bits so far, padded with 1-bits to a whole byte, 0x00 stuffed behind every 0xFF; (bytes, stuffed)"""
        pad = -self.n % 8
        self.put((1 << pad) - 1, pad)
        raw = self.acc.to_bytes(self.n // 8, "big")
        return raw.replace(b"\xff", b"\xff\x00"), raw.count(b"\xff")


def _code_block(bits, zz, pred, dc, ac, stats):
    """one block's 64 quantised coefficients in zigzag order -> bits (T.81 F.1.2)"""
    diff = int(zz[0]) - pred
    cat = _category(diff)
    stats["max_dc_category"] = max(stats["max_dc_category"], cat)
    bits.put(*dc[cat])
    bits.put(diff & ((1 << cat) - 1) if diff >= 0 else (diff - 1) & ((1 << cat) - 1), cat)
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bits.put(*ac[0xF0])
            stats["zrl"] += 1
            run -= 16
        cat = _category(v)
        stats["max_ac_category"] = max(stats["max_ac_category"], cat)
        bits.put(*ac[run << 4 | cat])
        bits.put(v & ((1 << cat) - 1) if v >= 0 else (v - 1) & ((1 << cat) - 1), cat)
        run = 0
    if run:
        bits.put(*ac[0x00])
    else:
        stats["blocks_without_eob"] += 1


def new_stats():
    return {"zrl": 0, "stuffed": 0, "blocks_without_eob": 0, "max_dc_category": 0, "max_ac_category": 0, "row_bytes": []}


def encode(bgr, quality, stats=None):
    """``bgr``: uint8 [H, W, 3]; ``quality``: 1 .. 95.  Returns the JPEG file's bytes.  ``stats`` (a dict, see ``new_stats``) is
    filled with what the tests need to see that the hard cases occurred: counts of ZRL symbols, stuffed bytes and blocks
    without EOB, the largest DC and AC categories, and ``row_bytes`` - the entropy-coded length of every MCU row."""
    bgr = np.asarray(bgr)
    if bgr.ndim != 3 or bgr.shape[2] != 3 or bgr.dtype != np.uint8:
        raise ValueError("bgr must be uint8 [H, W, 3]")
    h, w = bgr.shape[:2]
    if not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError("H and W must be 1 .. 65535")
    stats = new_stats() if stats is None else stats
    for k, v in new_stats().items():
        stats.setdefault(k, v)
    qt = T.quant_tables(quality)
    mh, mw = (h + 15) // 16, (w + 15) // 16
    padded = np.pad(bgr, ((0, mh * 16 - h), (0, mw * 16 - w), (0, 0)), mode="edge")
    y, cb, cr = ycbcr(padded)
    cb, cr = ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2 for p in (cb, cr))
    zz = []
    for plane, table in ((y, qt[0]), (cb, qt[1]), (cr, qt[1])):
        coef = fdct(_blocks(plane - 128)).reshape(plane.shape[0] // 8, plane.shape[1] // 8, 64)
        zz.append(quantise(coef, table)[..., T.ZIGZAG])
    codes = {k: T.huffman_codes(*v) for k, v in T.HUFFMAN.items()}
    out = [header(h, w, quality)]
    for my in range(mh):
        bits, pred = _Bits(), [0, 0, 0]
        for mx in range(mw):
            for by, bx in ((0, 0), (0, 1), (1, 0), (1, 1)):
                blk = zz[0][2 * my + by, 2 * mx + bx]
                _code_block(bits, blk, pred[0], codes[0x00], codes[0x10], stats)
                pred[0] = int(blk[0])
            for c in (1, 2):
                blk = zz[c][my, mx]
                _code_block(bits, blk, pred[c], codes[0x01], codes[0x11], stats)
                pred[c] = int(blk[0])
        row, stuffed = bits.flush()
        stats["stuffed"] += stuffed
        stats["row_bytes"].append(len(row))
        out.append(row)
        if my + 1 < mh:
            out.append(bytes((0xFF, 0xD0 + (my & 7))))
    out.append(b"\xff\xd9")
    return b"".join(out)
