"""Exif ``APP1`` segments built by hand with ``struct`` and spliced into JPEG files, for the orientation tests (host and GPU)."""
import struct

BYTE, SHORT, LONG = 1, 3, 4


def entry(order, tag, kind, count, value):
    """one 12-byte IFD entry whose value sits in the value field, left-justified as TIFF asks"""
    field = {BYTE: "B", SHORT: "H", LONG: "I"}[kind]
    raw = struct.pack(order + field, value)
    if kind == SHORT and count == 2:
        raw += struct.pack(order + "H", 3)               # a second value nobody should read
    return struct.pack(order + "HHI", tag, kind, count) + raw.ljust(4, b"\0")


def tiff(order="<", entries=None, value=6, kind=SHORT, count=1, ifd=8, magic=42, declared=None):
    """a TIFF structure with one IFD at offset ``ifd``; ``entries``: ready-made entry bytes (default: tag 0x0112 alone);
    ``declared``: the entry count written, when it is to differ from the entries present"""
    if entries is None:
        entries = [entry(order, 0x0112, kind, count, value)]
    head = (b"II" if order == "<" else b"MM") + struct.pack(order + "HI", magic, ifd)
    body = struct.pack(order + "H", len(entries) if declared is None else declared) + b"".join(entries) + struct.pack(order + "I", 0)
    return head.ljust(ifd, b"\0") + body


def app1(payload):
    return b"\xff\xe1" + struct.pack(">H", 2 + len(payload)) + payload


def exif(tiff_bytes):
    return app1(b"Exif\0\0" + tiff_bytes)


def splice(jpeg, segments, front=True):
    """``segments`` (bytes) put behind SOI (``front``) or behind the file's first segment (its JFIF ``APP0``)"""
    assert jpeg[:2] == b"\xff\xd8"
    at = 2
    if not front and jpeg[2] == 0xFF and jpeg[3] == 0xE0:
        at = 4 + (jpeg[4] << 8 | jpeg[5])
    return jpeg[:at] + segments + jpeg[at:]


def with_orientation(jpeg, o):
    """the file with an Exif segment that carries orientation ``o`` (little-endian SHORT) behind its APP0"""
    return splice(jpeg, exif(tiff("<", value=o)), front=False)
