"""The HUD in NumPy, integers only: the definition the device drawing (csrc/hud_draw.hip) is pinned to, byte for byte.

OpenCV is not a dependency, and its anti-aliased lines and Hershey font cannot be pinned; so the layout of the reference's
HUD (a blended box, corner ticks, two confidence bars, an info panel) is restated here with this project's own constants,
and THIS file is what the kernel has to reproduce.  Written from the specification, not from the kernel.

Every layer is a predicate on the pixel's own (x, y) plus a colour rule; no layer reads a neighbouring pixel.  The picture is
therefore a fold, per pixel, over the frame's faces in order and, within a face, over the layers in the order below.  All
rectangles are inclusive on both ends; pixels outside the frame do not exist (that is the clipping).  With s = ``scale``:

1. box      [x1,x2] x [y1,y2] minus [x1+2s,x2-2s] x [y1+2s,y2-2s]            p = (102 c + 154 p + 128) >> 8
2. ticks    opaque c; L = 15 s, h = s; per corner (cx, cy) of (x1,y1) (x2,y1) (x1,y2) (x2,y2), u = x - cx, v = y - cy:
            [cx,cx+L] x [cy-h,cy+h],  [cx-h,cx+h] x [cy,cy+L],  0 <= u,v <= L and |u + v - L| <= h
3. bars     bx = x2 + 10 s; detection bar: outline [bx,bx+6s] x [y1,y2] of thickness s inward in (100,100,100), fill
            [bx,bx+6s] x [y2-dh,y2] in (255,140,0), glyph 'D' (scale s, white) at (bx-2s, y1-12s); recognition bar: the same at
            bx + 12 s, filled in c over rh rows, glyph 'R' at (bx+10s, y1-12s)
4. panel    g = 2 s; pw = maxlen 6 g + 20 s, ph = nlines 18 s + 10 s; px = max(0, min(x1, W - pw)); py = max(0, y2 + 10 s), and
            if py + ph > H: py = max(0, y1 - ph - 10 s); background [px,px+pw] x [py,py+ph]: p = (205*30 + 51 p + 128) >> 8;
            border of thickness s inward in c; line i (white, glyph scale g) at (px + 10 s, py + s + 18 s i)

Text: a glyph pixel covers g x g output pixels, a character cell is 6 g wide (its last g columns empty); a byte outside
0x20 .. 0x7E is drawn as '?'.  The font is ``uint8 [95, 7]`` row masks, bit 4 the leftmost column (hud_font.py).

A face record (``K`` int32): x1 y1 x2 y2 | B G R | dh rh | nlines | len0 len1 len2 len3 | 0 0.  What a record holds is
normalised before it is drawn, here and in the kernel alike: coordinates clamped to +-2^20, colours taken modulo 256,
dh / rh clamped to [0, y2 - y1] (0 when that is negative), nlines to 0 .. 4, lengths to 0 .. max_chars.
"""
import math

import numpy as np

K = 16
MAX_LINES = 4
COORD_LIMIT = 1 << 20
GREY, ORANGE, WHITE, PANEL = (100, 100, 100), (255, 140, 0), (255, 255, 255), (30, 30, 30)
COLOURS = {"employee": (0, 255, 0), "visitor": (0, 255, 255)}
UNKNOWN_COLOUR = (0, 0, 255)


def default_font():
    from facerecognition_infrenceengine_amd.hud_font import FONT
    return FONT


# ---------------------------------------------------------------- the layers
def _rect(X, Y, xa, ya, xb, yb):
    return (X >= xa) & (X <= xb) & (Y >= ya) & (Y <= yb)


def _ring(X, Y, xa, ya, xb, yb, t):
    """the rectangle's outline, ``t`` pixels thick, inward"""
    return _rect(X, Y, xa, ya, xb, yb) & ~_rect(X, Y, xa + t, ya + t, xb - t, yb - t)


def _blend(img, m, colour, wc, wp):
    for ch in range(3):
        plane = img[..., ch]
        plane[m] = (wc * colour[ch] + wp * plane[m] + 128) >> 8


def _paint(img, m, colour):
    for ch in range(3):
        img[..., ch][m] = colour[ch]


def _glyphs(X, Y, tx, ty, g, chars, font):
    """mask of the lit pixels of the byte string ``chars`` drawn with its top-left corner at (tx, ty), glyph scale g"""
    n = len(chars)
    u, v = X - tx, Y - ty
    inside = (u >= 0) & (v >= 0) & (v < 7 * g) & (u < n * 6 * g)
    if n == 0 or not inside.any():
        return np.zeros(inside.shape, bool)
    uu, vv = np.where(inside, u, 0), np.where(inside, v, 0)          # only non-negative values are ever divided
    ci = uu // (6 * g)
    cu = (uu - ci * 6 * g) // g
    row = vv // g
    codes = np.array([c if 0x20 <= c <= 0x7E else 0x3F for c in chars], np.int64) - 0x20
    bits = np.asarray(font, np.int64)[codes[ci], row]
    lit = (cu < 5) & (((bits >> (4 - np.minimum(cu, 4))) & 1) == 1)
    return inside & lit


def normalise(rec, max_chars):
    """One record as both implementations read it: (x1, y1, x2, y2, colour, dh, rh, line lengths)."""
    rec = [int(v) for v in rec]
    x1, y1, x2, y2 = (max(-COORD_LIMIT, min(COORD_LIMIT, v)) for v in rec[:4])
    colour = tuple(v & 255 for v in rec[4:7])
    span = max(y2 - y1, 0)
    dh, rh = (max(0, min(v, span)) for v in rec[7:9])
    nlines = max(0, min(rec[9], MAX_LINES))
    lens = [max(0, min(v, max_chars)) for v in rec[10:10 + nlines]]
    return x1, y1, x2, y2, colour, dh, rh, lens


def panel_rect(x1, y1, x2, y2, lens, H, W, s):
    """(px, py, pw, ph) of the info panel"""
    g = 2 * s
    pw = (max(lens) if lens else 0) * 6 * g + 20 * s
    ph = len(lens) * 18 * s + 10 * s
    px = max(0, min(x1, W - pw))
    py = max(0, y2 + 10 * s)
    if py + ph > H:
        py = max(0, y1 - ph - 10 * s)
    return px, py, pw, ph


def draw_face(img, rec, text, max_chars, s, font):
    """Folds ONE face into ``img`` (int64 [H,W,3], in place).  ``rec``: the K ints, ``text``: uint8 [4, max_chars]."""
    H, W = img.shape[:2]
    Y, X = np.mgrid[0:H, 0:W]
    x1, y1, x2, y2, c, dh, rh, lens = normalise(rec, max_chars)
    # 1. box
    _blend(img, _ring(X, Y, x1, y1, x2, y2, 2 * s), c, 102, 154)
    # 2. corner ticks (all four point right / down)
    L, h = 15 * s, s
    for cx, cy in ((x1, y1), (x2, y1), (x1, y2), (x2, y2)):
        u, v = X - cx, Y - cy
        _paint(img, _rect(X, Y, cx, cy - h, cx + L, cy + h), c)
        _paint(img, _rect(X, Y, cx - h, cy, cx + h, cy + L), c)
        _paint(img, (u >= 0) & (v >= 0) & (u <= L) & (v <= L) & (np.abs(u + v - L) <= h), c)
    # 3. bars
    bx = x2 + 10 * s
    for b0, fill, height, letter in ((bx, ORANGE, dh, b"D"), (bx + 12 * s, c, rh, b"R")):
        _paint(img, _ring(X, Y, b0, y1, b0 + 6 * s, y2, s), GREY)
        _paint(img, _rect(X, Y, b0, y2 - height, b0 + 6 * s, y2), fill)
        _paint(img, _glyphs(X, Y, b0 - 2 * s, y1 - 12 * s, s, letter, font), WHITE)
    # 4. panel
    px, py, pw, ph = panel_rect(x1, y1, x2, y2, lens, H, W, s)
    _blend(img, _rect(X, Y, px, py, px + pw, py + ph), PANEL, 205, 51)
    _paint(img, _ring(X, Y, px, py, px + pw, py + ph, s), c)
    for i, n in enumerate(lens):
        _paint(img, _glyphs(X, Y, px + 10 * s, py + s + 18 * s * i, 2 * s, bytes(bytearray(text[i][:n])), font), WHITE)


def draw_records(frame, count, faces, text, scale=1, font=None):
    """``frame`` uint8 [H,W,3] -> a new uint8 frame with the first ``count`` records of ``faces`` int32 [cap, K] /
    ``text`` uint8 [cap, 4, max_chars] drawn, in order.  Records behind ``count`` are not looked at."""
    font = default_font() if font is None else font
    faces, text = np.asarray(faces), np.asarray(text)
    img = np.asarray(frame).astype(np.int64)
    for j in range(max(0, min(int(count), len(faces)))):
        draw_face(img, faces[j], text[j], text.shape[2], int(scale), font)
    assert img.min() >= 0 and img.max() <= 255
    return img.astype(np.uint8)


# ---------------------------------------------------------------- result dicts -> records
def clean(s, max_chars):
    """a text line as the bytes that are drawn: one byte per character, cut to ``max_chars``, everything outside
    0x20 .. 0x7E a '?'"""
    return bytes(ord(ch) if 0x20 <= ord(ch) <= 0x7E else 0x3F for ch in str(s)[:max_chars])


def lines_of(result):
    info = result["person_info"]
    t = info.get("type")
    if t == "employee":
        return ["Name: %s" % info.get("name", ""), "ID: %s" % info.get("employeeId", ""), "Type: Employee",
                "Score: %.2f" % float(result["recognition_score"])]
    if t == "visitor":
        return ["Name: %s" % info.get("name", ""), "Type: Visitor", "Score: %.2f" % float(result["recognition_score"])]
    return ["Unknown Person", "Detection: %.2f" % float(result["det_score"])]


def bar_height(span, score):
    score = float(score)
    if math.isnan(score):
        return 0
    return max(0, min(int(span * min(score, 1.0)), span))


def pack(results, frame_hw, out_hw=None, max_chars=40):
    """One frame's result dicts -> (faces int32 [m, K], text uint8 [m, 4, max_chars]).  With ``out_hw = (nh, nw)`` a box
    corner maps to floor(x nw / W), floor(y nh / H)."""
    results = list(results or ())
    faces = np.zeros((len(results), K), np.int32)
    text = np.zeros((len(results), MAX_LINES, max_chars), np.uint8)
    H, W = frame_hw
    for j, r in enumerate(results):
        xa, ya, xb, yb = (int(v) for v in r["bbox"])
        if out_hw is not None:
            nh, nw = out_hw
            xa, xb = xa * nw // W, xb * nw // W
            ya, yb = ya * nh // H, yb * nh // H
        x1, x2, y1, y2 = min(xa, xb), max(xa, xb), min(ya, yb), max(ya, yb)
        x1, y1, x2, y2 = (max(-COORD_LIMIT, min(COORD_LIMIT, v)) for v in (x1, y1, x2, y2))
        lines = [clean(s, max_chars) for s in lines_of(r)]
        faces[j, :4] = x1, y1, x2, y2
        faces[j, 4:7] = COLOURS.get(r["person_info"].get("type"), UNKNOWN_COLOUR)
        faces[j, 7] = bar_height(y2 - y1, r["det_score"])
        faces[j, 8] = bar_height(y2 - y1, r["recognition_score"])
        faces[j, 9] = len(lines)
        for i, b in enumerate(lines):
            faces[j, 10 + i] = len(b)
            text[j, i, :len(b)] = np.frombuffer(b, np.uint8)
    return faces, text


def draw_results(frame, results, scale=1, out_hw=None, frame_hw=None, max_chars=40, font=None):
    """``frame`` with the HUD of ``results`` (what ``recognize_batch`` returns for it; None or empty: the frame as it is).
    ``out_hw`` / ``frame_hw``: ``frame`` is a preview of a ``frame_hw`` frame whose picture fills ``out_hw``."""
    if not results:
        return np.array(frame, copy=True)
    faces, text = pack(results, frame_hw or frame.shape[:2], out_hw, max_chars)
    return draw_records(frame, len(faces), faces, text, scale, font)
