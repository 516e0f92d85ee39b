"""EXIF orientation on the host (no GPU): the definition tests/helpers/orient_ref.py against Pillow's ``exif_transpose``,
``jpeg_decode.exif_orientation`` against Pillow's reading of hand-built Exif segments, its robustness on prefixes and mutations,
``parse`` untouched by the segment, and ``ingest.decode_image(..., orient=True)``."""
import io
import struct

import numpy as np
import pytest
from PIL import Image, ImageOps

from facerecognition_infrenceengine_amd import jpeg_decode as J
from facerecognition_infrenceengine_amd.ingest import decode_image
from tests.helpers import exif_cases as X, jpeg_decode_cases as cases, orient_ref


def _file(h, w):
    return cases.pil_file(cases.picture("noise", h, w), 90, "444")


def _pil_orientation(data):
    with Image.open(io.BytesIO(data)) as im:
        return im.getexif().get(0x0112)


def _pil_turned(data):
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(ImageOps.exif_transpose(im).convert("RGB"), dtype=np.uint8)


def _pil_plain(data):
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


@pytest.mark.parametrize("h,w", [(17, 33), (1, 5)])
def test_definition_is_pillows_exif_transpose(h, w):
    plain = _file(h, w)
    coded = _pil_plain(plain)
    for o in range(10):
        data = X.with_orientation(plain, o)
        assert _pil_orientation(data) == o
        assert np.array_equal(_pil_plain(data), coded)
        want = _pil_turned(data)
        got = orient_ref.orient(coded, o) if 1 <= o <= 8 else coded       # 0 and 9 leave the picture alone
        assert got.shape == want.shape == ((w, h, 3) if 5 <= o <= 8 else (h, w, 3)), o
        assert np.array_equal(got, want), o
    for o in (0, 9):
        with pytest.raises(ValueError):
            orient_ref.orient(coded, o)


def test_package_orient_is_the_definition():
    img = cases.picture("noise", 5, 7)
    for o in range(1, 9):
        got = J.orient(img, o)
        assert np.array_equal(got, orient_ref.orient(img, o)), o
        assert J.oriented_shape((5, 7), o) == got.shape[:2]


def _hand_built(plain):
    """name -> file: every case of the issue"""
    out = {}
    for order, oname in (("<", "II"), (">", "MM")):
        for kind, kname in ((X.SHORT, "SHORT"), (X.LONG, "LONG")):
            out[f"{oname} {kname} 6"] = X.splice(plain, X.exif(X.tiff(order, value=6, kind=kind)), front=False)
        out[f"{oname} SHORT count 2"] = X.splice(plain, X.exif(X.tiff(order, value=6, count=2)), front=False)
        out[f"{oname} BYTE"] = X.splice(plain, X.exif(X.tiff(order, value=6, kind=X.BYTE)), front=False)
        other = X.entry(order, 0x010F, X.SHORT, 1, 3)                     # a tag in front of 0x0112 (tags ascend in an IFD)
        out[f"{oname} another tag in front"] = X.splice(plain, X.exif(X.tiff(order, entries=[other, X.entry(order, 0x0112, X.SHORT, 1, 8)])),
                                                        front=False)
        out[f"{oname} IFD0 at 16"] = X.splice(plain, X.exif(X.tiff(order, value=5, ifd=16)), front=False)
    six, three = X.exif(X.tiff("<", value=6)), X.exif(X.tiff(">", value=3))
    out["Exif in front of APP0"] = X.splice(plain, six, front=True)
    out["XMP APP1 in front"] = X.splice(plain, X.app1(b"http://ns.adobe.com/xap/1.0/\0<x:xmpmeta/>") + six, front=False)
    out["two Exif segments"] = X.splice(plain, six + three, front=False)
    out["value 0"] = X.with_orientation(plain, 0)
    out["value 9"] = X.with_orientation(plain, 9)
    out["LONG count 2"] = X.splice(plain, X.exif(X.tiff("<", value=6, kind=X.LONG, count=2)), front=False)
    out["IFD offset beyond the segment"] = X.splice(plain, X.exif(X.tiff("<", value=6)[:4] + struct.pack("<I", 4000) + X.tiff("<", value=6)[8:]),
                                                    front=False)
    out["entry count beyond the segment"] = X.splice(plain, X.exif(X.tiff("<", value=6)[:8 + 2 + 4]), front=False)   # ends inside entry 0
    out["bad magic"] = X.splice(plain, X.exif(X.tiff("<", value=6, magic=43)), front=False)
    out["no EXIF"] = plain
    for o in range(1, 9):
        out[f"value {o}"] = X.with_orientation(plain, o)
    return out


EXPECT = {"II SHORT 6": 6, "MM LONG 6": 6, "II SHORT count 2": 6, "MM BYTE": 1, "II another tag in front": 8, "MM IFD0 at 16": 5,
          "Exif in front of APP0": 6, "XMP APP1 in front": 6, "two Exif segments": 6, "value 0": 1, "value 9": 1,
          "IFD offset beyond the segment": 1, "entry count beyond the segment": 1, "bad magic": 1, "no EXIF": 1, "value 7": 7}


def test_exif_orientation_on_hand_built_segments():
    files = _hand_built(_file(17, 33))
    for name, data in files.items():
        ours = J.exif_orientation(data)
        assert ours in range(1, 9), name
        try:
            pil = _pil_orientation(data)
        except Exception:                                # Pillow gives up on the segment: nothing to turn by
            pil = None
        if isinstance(pil, int) and 1 <= pil <= 8:
            assert ours == pil, (name, ours, pil)
        else:
            assert ours == 1, (name, ours, pil)
        if name in EXPECT:
            assert ours == EXPECT[name], (name, ours)
        # what Pillow then does to the picture is what our value does to it
        coded = _pil_plain(files["no EXIF"])
        assert np.array_equal(_pil_turned(data), orient_ref.orient(coded, ours)), name
        for view in (bytearray(data), memoryview(data), np.frombuffer(data, np.uint8)):
            assert J.exif_orientation(view) == ours
    # The rule is about the COUNT: an IFD that declares more entries than the segment holds is not walked at all.  Pillow reads
    # the entries that are there and gives up at the first one that is not, so here - and only here - it turns and we do not.
    liar = X.splice(files["no EXIF"], X.exif(X.tiff("<", value=6, declared=200)), front=False)
    assert J.exif_orientation(liar) == 1
    assert J.exif_orientation(b"") == 1 and J.exif_orientation(None) == 1 and J.exif_orientation(b"\x89PNG\r\n") == 1


def test_prefixes_and_mutations_never_raise():
    data = X.with_orientation(_file(17, 33), 6)
    assert J.exif_orientation(data) == 6
    for k in range(len(data) + 1):
        assert J.exif_orientation(data[:k]) in range(1, 9), k
    lo = data.index(b"\xff\xe1")
    hi = lo + 2 + (data[lo + 2] << 8 | data[lo + 3])
    rng = np.random.default_rng(20261)
    seen = set()
    for _ in range(2000):
        at, byte = int(rng.integers(lo, hi)), int(rng.integers(256))
        got = J.exif_orientation(data[:at] + bytes([byte]) + data[at + 1:])
        assert got in range(1, 9), (at, byte)
        seen.add(got)
    assert {1, 6} <= seen                                # some mutations broke the segment, some left it whole


def test_parse_is_untouched_by_the_segment():
    plain = _file(17, 33)
    data = X.with_orientation(plain, 6)
    a, b = J.parse(plain), J.parse(data)
    assert isinstance(a, J.Header) and isinstance(b, J.Header)
    assert a._replace(scan=0) == b._replace(scan=0)
    assert b.scan - a.scan == len(data) - len(plain) > 0


def test_decode_image_orient():
    plain = _file(17, 33)
    coded = decode_image(plain)
    assert np.array_equal(coded, cases.pil_decode(plain))
    for o in range(10):
        data = X.with_orientation(plain, o)
        assert np.array_equal(decode_image(data), coded), o                              # the default: as coded
        assert np.array_equal(decode_image(data, orient=False), coded), o
        got = decode_image(data, orient=True)
        assert got.flags["C_CONTIGUOUS"] and got.dtype == np.uint8
        assert np.array_equal(got, _pil_turned(data)[..., ::-1]), o
    # a PNG that carries EXIF
    rgb = np.ascontiguousarray(cases.picture("ramp", 9, 14)[..., ::-1])
    ex = Image.Exif()
    ex[0x0112] = 8
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "PNG", exif=ex)
    png = buf.getvalue()
    assert _pil_orientation(png) == 8
    assert np.array_equal(decode_image(png), rgb[..., ::-1])
    got = decode_image(png, orient=True)
    assert got.shape == (14, 9, 3) and np.array_equal(got, _pil_turned(png)[..., ::-1])
    assert np.array_equal(got, orient_ref.orient(rgb[..., ::-1], 8))
    assert decode_image(b"not an image", orient=True) is None
