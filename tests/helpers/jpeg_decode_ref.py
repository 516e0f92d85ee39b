"""The DEFINITION of the device JPEG decoder's pixels (csrc/jpeg_decode.hip), in NumPy, integers only, a
sequential scan.

``decode(data)`` returns ``(bgr uint8 [H, W, 3], stats)``; the kernels reproduce the picture byte for byte.  The arithmetic is
libjpeg's: the Huffman decoding of T.81 F.2.2 with the file's own tables, ``coef * q``, the "islow" inverse DCT (jidctint: the
mirror of jpeg_ref._pass, the same twelve constants), the "fancy" triangle filter for the chroma planes, the 16-bit fixed-point
colour transform.  PIL's decode of the same file is the same bytes (tests/test_jpeg_decode_ref_host.py), with no tolerance.

Baseline sequential (SOF0), 8 bit, one interleaved scan; 3 components at 4:4:4 / 4:2:2 / 4:2:0 or 1 component; any DQT / DHT
contents; any restart interval or none.  Everything else raises ``Unsupported``; a stream that breaks off, holds a code no
table has or runs a coefficient index past 63 raises ``BadStream``.

``stats`` also holds a simulation of the kernel's self-synchronising entropy decoder (Weissenberger & Schmidt) at its
subsequence size ``S``: a restart interval is walked in chunks of ``LANES`` subsequences of ``S`` raw bytes, every lane decodes
its subsequence from a guessed state and then from its predecessor's end state until nothing changes."""
import struct

import numpy as np

from facerecognition_infrenceengine_amd import jpeg_tables as T

from .jpeg_ref import C, CONST_BITS, PASS1_BITS, _descale

S, LANES = 32, 256                               # csrc/jpeg_decode.hip JD_S, JD_LANES
MCU_BLOCKS = {"444": (0, 1, 2), "422": (0, 0, 1, 2), "420": (0, 0, 0, 0, 1, 2), "gray": (0,)}
SAMPLING = {(0x11, 0x11, 0x11): "444", (0x21, 0x11, 0x11): "422", (0x22, 0x11, 0x11): "420"}


class Unsupported(ValueError):
    pass


class BadStream(ValueError):
    pass


def new_stats():
    return {"intervals": 0, "rst_wraps": 0, "stuffed": 0, "zrl": 0, "blocks_without_eob": 0, "long_codes": 0,
            "chunks": 0, "sync_rounds_max": 0}


# ---------------------------------------------------------------- the header
def parse(data):
    """SOI .. SOS of ``data`` -> a dict: H, W, sampling, restart, qtables {id: int32 [64] natural order}, huffman
    {class << 4 | id: (bits, vals)}, components [(quant id, dc id, ac id)], scan (offset of the entropy data)"""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise Unsupported("no SOI")
    pos, qt, huff, restart, frame = 2, {}, {}, 0, None
    while True:
        if pos + 4 > len(data) or data[pos] != 0xFF:
            raise BadStream("header cut or no marker")
        marker = data[pos + 1]
        if marker == 0xFF:
            pos += 1
            continue
        length = struct.unpack(">H", data[pos + 2:pos + 4])[0]
        seg = data[pos + 4:pos + 2 + length]
        if length < 2 or len(seg) != length - 2:
            raise BadStream("segment cut")
        pos += 2 + length
        if marker == 0xDB:
            while seg:
                if seg[0] >> 4:
                    raise Unsupported("16-bit DQT")
                qt[seg[0] & 15] = np.frombuffer(seg[1:65], np.uint8).astype(np.int32)[np.argsort(T.ZIGZAG)]
                seg = seg[65:]
        elif marker == 0xC4:
            while seg:
                bits = tuple(seg[1:17])
                huff[seg[0]] = (bits, tuple(seg[17:17 + sum(bits)]))
                seg = seg[17 + sum(bits):]
        elif marker == 0xC0:
            prec, h, w, nc = struct.unpack(">BHHB", seg[:6])
            frame = (prec, h, w, [tuple(seg[6 + 3 * i:9 + 3 * i]) for i in range(nc)])
        elif marker in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise Unsupported("SOF%d" % (marker - 0xC0))
        elif marker == 0xDD:
            restart = struct.unpack(">H", seg[:2])[0]
        elif marker == 0xDA:
            break
    if frame is None:
        raise BadStream("SOS before SOF")
    prec, h, w, comps = frame
    if prec != 8 or len(comps) not in (1, 3) or h == 0 or w == 0:
        raise Unsupported("precision, component count or DNL height")
    if seg[0] != len(comps) or tuple(seg[1 + 2 * len(comps):4 + 2 * len(comps)]) != (0, 63, 0):
        raise Unsupported("not one interleaved baseline scan")
    sampling = "gray" if len(comps) == 1 else SAMPLING.get(tuple(c[1] for c in comps))
    if sampling is None:
        raise Unsupported("sampling factors")
    components = []
    for i, (cid, _, tq) in enumerate(comps):
        sid, tables = seg[1 + 2 * i], seg[2 + 2 * i]
        if sid != cid:
            raise Unsupported("scan order")
        components.append((tq, tables >> 4, tables & 15))
    return {"H": h, "W": w, "sampling": sampling, "restart": restart, "qtables": qt, "huffman": huff, "components": components,
            "scan": pos}


# ---------------------------------------------------------------- the entropy data
def _lut(bits, vals):
    """list [65536]: the next 16 bits -> length << 8 | symbol, 0 where no code matches"""
    lut = np.zeros(65536, np.int32)
    for sym, (code, length) in T.huffman_codes(bits, vals).items():
        lut[code << (16 - length):(code + 1) << (16 - length)] = length << 8 | sym
    return lut.tolist()


def _peek16(u, p):
    k = p >> 3
    return ((u[k] << 16 | u[k + 1] << 8 | u[k + 2]) >> (8 - (p & 7))) & 0xFFFF


def _walk(u, nbits, luts, blocks, p, b, z, limit, coef=None, blk=0, stats=None, strict=True):
    """Decodes the symbols that START before bit ``limit`` of the unstuffed bytes ``u`` (``nbits`` of them real, four zero
    bytes behind) from the state (bit ``p``, block ``b`` of the MCU, zigzag index ``z``).  Returns the end state and the number
    of blocks completed, ``(p, b, z, n)``; None for a code no table has, a DC category past 11 or an index past 63.  A symbol
    that would end past ``nbits``, or bits that are no code with fewer than 16 of them left, are the padding of the interval's
    last byte (or a stream that broke off): the walk ends AT ``nbits``.  ``coef`` (int32 [blocks, 64], natural order) receives the values, DC as differences, from block ``blk`` on."""
    n = 0
    while p < limit:
        dc, ac = luts[blocks[b]]
        e = (dc if z == 0 else ac)[_peek16(u, p)]
        if e == 0:
            if nbits - p < 16:
                return nbits, b, z, n
            if strict:
                return None
            p += 1
            continue
        length, sym = e >> 8, e & 255
        run, size = (0, sym) if z == 0 else (sym >> 4, sym & 15)
        if z == 0 and size > 11:
            if strict:
                return None
            size &= 15
        if p + length + size > nbits:
            return nbits, b, z, n
        if stats is not None and length > 9:
            stats["long_codes"] += 1
        v = (_peek16(u, p + length) >> (16 - size)) if size else 0
        if size and v < 1 << (size - 1):
            v -= (1 << size) - 1
        p += length + size
        if z == 0:
            if coef is not None:
                if blk + n >= len(coef):
                    return None
                coef[blk + n, 0] = v
            z = 1
        elif size == 0:
            if run == 15:
                z += 16
                if stats is not None:
                    stats["zrl"] += 1
                if z > 64:
                    if strict:
                        return None
                    z = 64
                if z == 64 and stats is not None:
                    stats["blocks_without_eob"] += 1
            else:
                z = 64
        else:
            z += run
            if z > 63:
                if strict:
                    return None
                z = 63
            if coef is not None:
                coef[blk + n, T.ZIGZAG[z]] = v
            z += 1
            if z == 64 and stats is not None:
                stats["blocks_without_eob"] += 1
        if z == 64:
            z, b, n = 0, (b + 1) % len(blocks), n + 1
    return p, b, z, n


def _simulate(raw, u, nbits, luts, blocks, stats):
    """the self-synchronising walk over one restart interval; returns the blocks it counts"""
    stuffed = np.zeros(len(raw) + 1, np.int64)
    arr = np.frombuffer(raw, np.uint8)
    stuffed[2:] = np.cumsum((arr[1:] == 0) & (arr[:-1] == 0xFF))          # stuffed[k]: stuffed zeros in raw[:k]
    # the unstuffed bit a subsequence starts at (a stuffed zero is skipped: it maps to the byte behind it)
    bound = [8 * int(min(k, len(raw)) - stuffed[min(k, len(raw))]) for k in range(0, len(raw) + S * LANES + S, S)]
    entry, total = (0, 0, 0), 0
    subs = max((len(raw) + S - 1) // S, 1)
    for c0 in range(0, subs, LANES):
        stats["chunks"] += 1
        lanes = min(LANES, subs - c0)                 # the subsequences that begin inside the interval
        start = [entry] + [(bound[c0 + i], 0, 0) for i in range(1, lanes)]
        end = [None] * lanes
        todo, rounds = list(range(lanes)), 0
        while True:
            for i in todo:
                st = start[i]
                end[i] = None if st is None else _walk(u, nbits, luts, blocks, *st, min(bound[c0 + i + 1], nbits), strict=False)
            todo = []
            for i in range(1, lanes):
                want = None if end[i - 1] is None else end[i - 1][:3]
                if want != start[i]:
                    start[i] = want
                    todo.append(i)
            if not todo:
                break
            rounds += 1
        stats["sync_rounds_max"] = max(stats["sync_rounds_max"], rounds)
        if any(e is None for e in end):
            raise BadStream("code, category or index")
        total += sum(e[3] for e in end)
        entry = end[-1][:3]
    return total, entry


def coefficients(data, stats=None, simulate=True):
    """``(header dict, int32 [blocks, 64])``: the quantised coefficients in scan order (MCU by MCU), natural order inside a
    block, DC as values"""
    data = bytes(data)
    stats = new_stats() if stats is None else stats
    for k, v in new_stats().items():
        stats.setdefault(k, v)
    hd = parse(data)
    blocks = MCU_BLOCKS[hd["sampling"]]
    mw, mh = {"444": (8, 8), "422": (16, 8), "420": (16, 16), "gray": (8, 8)}[hd["sampling"]]
    mcus = ((hd["W"] + mw - 1) // mw) * ((hd["H"] + mh - 1) // mh)
    luts = []
    for _, td, ta in hd["components"]:
        if td not in hd["huffman"] or 0x10 | ta not in hd["huffman"]:
            raise BadStream("a Huffman table the scan names is missing")
        luts.append((_lut(*hd["huffman"][td]), _lut(*hd["huffman"][0x10 | ta])))
    scan = data[hd["scan"]:]
    # the scan ends at the first marker that is no RSTm; the intervals lie between the RSTm
    cuts, end = [], len(scan)
    k = scan.find(b"\xff")
    while k != -1 and k + 1 < len(scan):
        nxt = scan[k + 1]
        if 0xD0 <= nxt <= 0xD7:
            if nxt - 0xD0 != len(cuts) & 7:
                raise BadStream("RST out of order")
            cuts.append(k)
        elif nxt != 0:
            end = k
            break
        k = scan.find(b"\xff", k + 2 if nxt else k + 1)
    per = hd["restart"] or mcus
    want = (mcus + per - 1) // per
    if len(cuts) + 1 != want:
        raise BadStream("%d restart intervals for %d" % (len(cuts) + 1, want))
    stats["intervals"] += want
    stats["rst_wraps"] = max(stats["rst_wraps"], len(cuts) // 8)
    coef = np.zeros((mcus * len(blocks), 64), np.int32)
    comp = np.tile(np.array(blocks), mcus)
    for i, (a, z) in enumerate(zip([0] + [c + 2 for c in cuts], cuts + [end])):
        raw = scan[a:z]
        stats["stuffed"] += raw.count(b"\xff\x00")
        u = raw.replace(b"\xff\x00", b"\xff")
        nbits, u = 8 * len(u), u + bytes(4)
        first, count = i * per * len(blocks), (min(per, mcus - i * per)) * len(blocks)
        res = _walk(u, nbits, luts, blocks, 0, 0, 0, nbits, coef[:first + count], first, stats)
        if res is None or res[1:] != (0, 0, count):
            raise BadStream("interval %d" % i)
        if simulate and _simulate(raw, u, nbits, luts, blocks, stats)[0] != count:
            raise AssertionError("the self-synchronising walk disagrees with the sequential one")
        for c in set(blocks):
            sel = first + np.flatnonzero(comp[first:first + count] == c)
            coef[sel, 0] = np.cumsum(coef[sel, 0])
    return hd, coef


# ---------------------------------------------------------------- the pixels
def _idct_pass(d, n):
    """one 1-D pass of jidctint over the last axis of int32 [..., 8]"""
    i0, i1, i2, i3, i4, i5, i6, i7 = (d[..., k] for k in range(8))
    z1 = (i2 + i6) * C[2]
    tmp2, tmp3 = z1 - i6 * C[7], z1 + i2 * C[3]
    tmp0, tmp1 = (i0 + i4) << CONST_BITS, (i0 - i4) << CONST_BITS
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = i7, i5, i3, i1
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * C[5]
    tmp0, tmp1, tmp2, tmp3 = tmp0 * C[0], tmp1 * C[9], tmp2 * C[11], tmp3 * C[6]
    z1, z2, z3, z4 = -z1 * C[4], -z2 * C[10], -z3 * C[8] + z5, -z4 * C[1] + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    out = (tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3)
    return np.stack([_descale(o, n) for o in out], axis=-1)


def idct(blocks):
    """libjpeg's integer "islow" inverse DCT of dequantised int32 [..., 8, 8] -> samples 0 .. 255: columns, then rows"""
    cols = np.swapaxes(_idct_pass(np.swapaxes(blocks.astype(np.int32), -1, -2), CONST_BITS - PASS1_BITS), -1, -2)
    return np.clip(_idct_pass(cols, CONST_BITS + PASS1_BITS + 3) + 128, 0, 255)


def _planes(hd, coef):
    """the component planes, each cropped to its real size ceil(H v / vmax) x ceil(W h / hmax)"""
    blocks = MCU_BLOCKS[hd["sampling"]]
    hs, vs = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "gray": (1, 1)}[hd["sampling"]]
    mx, my = (hd["W"] + 8 * hs - 1) // (8 * hs), (hd["H"] + 8 * vs - 1) // (8 * vs)
    coef = coef.reshape(my, mx, len(blocks), 8, 8)
    planes = []
    for c, (tq, _, _) in enumerate(hd["components"]):
        if tq not in hd["qtables"]:
            raise BadStream("a quantisation table the frame names is missing")
        px = idct(coef[:, :, [j for j, b in enumerate(blocks) if b == c]] * hd["qtables"][tq].reshape(8, 8))
        ch, cv = (hs, vs) if c == 0 else (1, 1)
        px = px.reshape(my, mx, cv, ch, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(my * cv * 8, mx * ch * 8)
        planes.append(px[:(hd["H"] * cv + vs - 1) // vs, :(hd["W"] * ch + hs - 1) // hs])
    return planes


def _shift(x, d, axis):
    """x moved by d along axis, the edge replicated"""
    idx = np.clip(np.arange(x.shape[axis]) + d, 0, x.shape[axis] - 1)
    return np.take(x, idx, axis=axis)


def upsample(plane, sampling, h, w):
    """libjpeg's chroma upsampling to h x w: the "fancy" triangle filter, or replication for a component at most 2 wide"""
    if sampling in ("444", "gray"):
        return plane
    if plane.shape[1] <= 2:
        return np.repeat(np.repeat(plane, 2 if sampling == "420" else 1, axis=0), 2, axis=1)[:h, :w]
    if sampling == "422":
        out = np.empty((plane.shape[0], 2 * plane.shape[1]), np.int32)
        out[:, 0::2] = (3 * plane + _shift(plane, -1, 1) + 1) >> 2
        out[:, 1::2] = (3 * plane + _shift(plane, 1, 1) + 2) >> 2
        return out[:h, :w]
    s = np.empty((2 * plane.shape[0], plane.shape[1]), np.int32)
    s[0::2] = 3 * plane + _shift(plane, -1, 0)
    s[1::2] = 3 * plane + _shift(plane, 1, 0)
    out = np.empty((s.shape[0], 2 * s.shape[1]), np.int32)
    out[:, 0::2] = (3 * s + _shift(s, -1, 1) + 8) >> 4
    out[:, 1::2] = (3 * s + _shift(s, 1, 1) + 7) >> 4
    return out[:h, :w]


def decode(data, stats=None, simulate=False):
    """``data``: a JPEG file's bytes.  Returns ``(bgr uint8 [H, W, 3], stats)``; ``simulate``: also walk every restart interval
    the way the kernel does and fill ``chunks`` and ``sync_rounds_max``."""
    stats = new_stats() if stats is None else stats
    hd, coef = coefficients(data, stats, simulate)
    h, w = hd["H"], hd["W"]
    planes = _planes(hd, coef)
    y = planes[0]
    if hd["sampling"] == "gray":
        return np.repeat(y[..., None], 3, axis=-1).astype(np.uint8), stats
    cb, cr = (upsample(p, hd["sampling"], h, w) - 128 for p in planes[1:])
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8), stats
