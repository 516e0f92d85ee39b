"""The definition of the device JPEG decoder's pixels (tests/helpers/jpeg_decode_ref.py) IS libjpeg's decode: equal to Pillow's,
byte for byte, on every supported file (no GPU needed).  If a libjpeg build disagrees, that is a finding for DESIGN.md 4.5j, not
a reason for a tolerance."""
import io

import numpy as np
import pytest
from PIL import Image

from facerecognition_infrenceengine_amd import jpeg_decode, jpeg_tables as T
from tests.helpers import jpeg_decode_cases as cases, jpeg_decode_ref as ref, jpeg_ref

GRID_SIZES = [(1, 1), (2, 3), (8, 8), (15, 2), (5, 4), (7, 5), (16, 6), (17, 33), (24, 40), (37, 51)]     # widths 2 .. 7 among them


@pytest.mark.parametrize("h,w", GRID_SIZES)
def test_definition_equals_pillow(h, w):
    n = 0
    for kind in ("noise", "ramp", "flats"):
        bgr = cases.picture(kind, h, w)
        for quality in (10, 50, 75, 95, 100):
            for sampling in ("444", "422", "420"):
                for writer in cases.WRITERS:
                    data = cases.pil_file(bgr, quality, sampling, writer)
                    got, _ = ref.decode(data)
                    assert np.array_equal(got, cases.pil_decode(data)), (kind, quality, sampling, writer)
                    n += 1
    assert n == 180


def test_definition_equals_pillow_gray():
    for h, w in ((1, 1), (17, 33), (37, 51)):
        for writer in cases.WRITERS:
            data = cases.pil_file(cases.picture("noise", h, w), 80, "gray", writer)
            got, _ = ref.decode(data)
            assert got.shape == (h, w, 3) and np.array_equal(got, cases.pil_decode(data))


def _encoder_coefficients(bgr, quality):
    """what jpeg_ref.encode codes: the quantised coefficients in scan order (Y00 Y01 Y10 Y11 Cb Cr per MCU), natural order"""
    h, w = bgr.shape[:2]
    mh, mw = (h + 15) // 16, (w + 15) // 16
    padded = np.pad(bgr, ((0, mh * 16 - h), (0, mw * 16 - w), (0, 0)), mode="edge")
    y, cb, cr = jpeg_ref.ycbcr(padded)
    cb, cr = ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2 for p in (cb, cr))
    qt = T.quant_tables(quality)
    q = [jpeg_ref.quantise(jpeg_ref.fdct(jpeg_ref._blocks(p - 128)).reshape(p.shape[0] // 8, p.shape[1] // 8, 64), t)
         for p, t in ((y, qt[0]), (cb, qt[1]), (cr, qt[1]))]
    out = np.empty((mh, mw, 6, 64), np.int32)
    for j, (by, bx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        out[:, :, j] = q[0][by::2, bx::2]
    out[:, :, 4], out[:, :, 5] = q[1], q[2]
    return out.reshape(-1, 64)


@pytest.mark.parametrize("h,w,quality", [(1, 1, 50), (16, 16, 10), (37, 51, 75), (40, 56, 95), (144, 176, 90)])
def test_the_encoders_own_files(h, w, quality):
    for kind in ("noise", "flats"):
        bgr = cases.picture(kind, h, w)
        data = jpeg_ref.encode(bgr, quality)
        got, stats = ref.decode(data)
        assert np.array_equal(got, cases.pil_decode(data))
        assert stats["intervals"] == (h + 15) // 16
        # the entropy half on its own: the coefficients recovered are the ones the encoder's definition coded
        hd, coef = ref.coefficients(data, simulate=False)
        assert hd["sampling"] == "420" and hd["restart"] == (w + 15) // 16
        assert np.array_equal(coef, _encoder_coefficients(bgr, quality))


def _save(bgr, **kw):
    buf = io.BytesIO()
    Image.fromarray(bgr[..., ::-1].copy()).save(buf, **kw)
    return buf.getvalue()


def test_parse_says_what_it_does_not_take():
    bgr = cases.picture("ramp", 24, 40)
    good = cases.pil_file(bgr, 80, "420")
    hd = jpeg_decode.parse(good)
    assert isinstance(hd, jpeg_decode.Header)
    assert (hd.H, hd.W, hd.sampling, hd.restart, hd.segments) == (24, 40, jpeg_decode.S420, 0, 1)
    assert good[hd.scan - 14:hd.scan - 12] == b"\xff\xda" and hd.scan == ref.parse(good)["scan"]
    assert "progressive" in jpeg_decode.parse(_save(bgr, format="JPEG", progressive=True))
    buf = io.BytesIO()
    Image.fromarray(np.zeros((8, 8, 4), np.uint8), "CMYK").save(buf, "JPEG")
    assert "4 components" in jpeg_decode.parse(buf.getvalue())
    assert "no SOI" in jpeg_decode.parse(_save(bgr, format="PNG"))
    assert "no SOI" in jpeg_decode.parse(b"")
    assert jpeg_decode.parse(None) == "not bytes"
    for cut in (2, 3, 20, 100, hd.scan - 1):
        assert "cut short" in jpeg_decode.parse(good[:cut]), cut
    assert isinstance(jpeg_decode.parse(good[:hd.scan]), jpeg_decode.Header)       # the scan is the device's to judge
    # segments the decoder has no use for are skipped; a restart interval is counted
    with_com = good[:2] + b"\xff\xfe\x00\x05abc" + b"\xff\xe1\x00\x04xy" + good[2:]
    assert jpeg_decode.parse(with_com)[:4] == hd[:4]
    dri = jpeg_decode.parse(cases.pil_file(bgr, 80, "444", "dri_3"))
    assert dri.restart == 3 and dri.segments == 5 and dri.sampling == jpeg_decode.S444
    gray = jpeg_decode.parse(cases.pil_file(bgr, 80, "gray"))
    assert gray.sampling == jpeg_decode.GRAY and len(gray.qtables) == 1
    # the same tables in every frame of a camera: the same cache keys
    again = jpeg_decode.parse(cases.pil_file(cases.picture("noise", 24, 40), 80, "420"))
    assert again.qtables == hd.qtables and again.huffman == hd.huffman


def test_huffman_rows_decode_every_code():
    """jpeg_decode.huffman_row (what the kernel reads) against the canonical codes of jpeg_tables, Annex K and optimised tables"""
    tables = [bytes(bits) + bytes(vals) for bits, vals in T.HUFFMAN.values()]
    hd = jpeg_decode.parse(cases.pil_file(cases.picture("noise", 37, 51), 100, "444", "optimize"))
    tables += [t for pair in hd.huffman for t in pair]
    for table in tables:
        row = jpeg_decode.huffman_row(table)
        assert row.shape == (jpeg_decode.HUFF_ROW,) and row.dtype == np.int32
        codes = T.huffman_codes(tuple(table[:16]), tuple(table[16:]))
        assert len(codes) == len(table) - 16
        for sym, (code, length) in codes.items():
            win = code << (16 - length) | ((1 << (16 - length)) - 1 if sym & 1 else 0)        # any bits behind the code
            e = int(row[win >> 7])
            if length <= 9:
                assert e == length << 8 | sym
            else:
                assert e == 0
                hit = [l for l in range(10, 17) if (win >> (16 - l)) <= row[512 + l]][0]
                assert hit == length and row[548 + row[530 + length] + code] == sym


def test_stats_show_the_hard_cases():
    stats = ref.new_stats()
    ref.decode(cases.pil_file(cases.picture("noise", 37, 51), 100, "444"), stats)          # long codes, stuffing, full blocks
    assert stats["long_codes"] > 0 and stats["stuffed"] > 0 and stats["blocks_without_eob"] > 0
    flats = ref.new_stats()
    data = cases.pil_file(cases.picture("flats", 37, 51), 50, "420")
    ref.decode(data, flats)
    assert flats["blocks_without_eob"] == 0 and flats["zrl"] == 0                          # EOB-only blocks
    zrl = ref.new_stats()
    ref.decode(cases.pil_file(cases.picture("noise", 37, 51), 50, "422"), zrl)
    assert zrl["zrl"] > 0
    wrap = ref.new_stats()
    ref.decode(cases.pil_file(cases.picture("ramp", 37, 51), 75, "444", "dri_3"), wrap)    # 35 MCUs in intervals of 3
    assert wrap["intervals"] == 12 and wrap["rst_wraps"] == 1
    sync = ref.new_stats()
    data = cases.pil_file(cases.picture("noise", *cases.LARGE), 90, "420")
    assert jpeg_decode.parse(data).restart == 0
    ref.decode(data, sync, simulate=True)
    assert sync["intervals"] == 1 and sync["chunks"] >= 3 and sync["sync_rounds_max"] > 1
    assert sync["chunks"] == (len(data) - jpeg_decode.parse(data).scan - 2 + ref.S * ref.LANES - 1) // (ref.S * ref.LANES)


def test_broken_scans_raise_in_the_definition():
    good = cases.pil_file(cases.picture("noise", 37, 51), 90, "420")
    scan = jpeg_decode.parse(good).scan
    for data in (good[:scan], good[:scan + 100], good[:scan] + b"\xff" * 300, good[:scan] + bytes(300)):
        with pytest.raises(ref.BadStream):
            ref.decode(data)
    with pytest.raises(ref.Unsupported):
        ref.decode(_save(cases.picture("ramp", 16, 16), format="JPEG", progressive=True))
