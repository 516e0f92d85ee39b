"""chips.FaceChips, the host half (no GPU): the square of a face, who is chipped, the fail-safe beside a redactor, the padding of the
records and the arguments that are refused."""
import numpy as np
import pytest

from facerecognition_infrenceengine_amd.chips import COORD_LIMIT, FaceChips
from facerecognition_infrenceengine_amd.redact import Redactor


def face(bbox, kind="unknown", **more):
    return dict({"bbox": np.asarray(bbox), "person_info": {"name": "x", "type": kind}}, **more)


def test_square_is_centred_on_the_box_and_grown_by_the_margin():
    c = FaceChips(margin=0, encode=None)
    assert c.square(face([10, 20, 29, 39])) == (10, 20, 20)                  # a 20 x 20 box is its own square
    assert c.square(face([10, 20, 29, 59])) == (0, 20, 40)                   # 20 x 40: the larger side, centred across
    assert c.square(face([29, 59, 10, 20])) == (0, 20, 40)                   # corners in any order
    assert c.square(face([7, 7, 7, 7])) == (7, 7, 1)
    c = FaceChips(margin=30, encode=None)
    assert c.square(face([100, 100, 199, 219])) == (54, 64, 192)              # s0 = 120, side = 120 + 2 * 36
    x0, y0, side = c.square(face([100, 100, 199, 219]))
    assert (2 * x0 + side, 2 * y0 + side) == (100 + 199 + 1, 100 + 219 + 1)   # centred exactly: both sums are even here
    c = FaceChips(margin=400, encode=None)
    assert c.square(face([0, 0, 9, 9])) == (-40, -40, 90)
    # negative coordinates: floor division keeps the square centred left of and above the frame
    c = FaceChips(margin=0, encode=None)
    assert c.square(face([-30, -50, -11, -41])) == (-30, -55, 20)
    assert c.square(face([-30, -50, -10, -41])) == (-30, -56, 21)             # (-30 - 10 + 1 - 21) // 2 = -30; (-50 - 41 + 1 - 21) // 2 = -56
    assert c.square(face([-4, -4, -2, 5])) == ((-4 - 2 + 1 - 10) // 2, -4, 10) == (-8, -4, 10)
    # the clamp to 4096
    c = FaceChips(margin=400, encode=None)
    x0, y0, side = c.square(face([0, 0, 999, 1999]))
    assert side == 4096 and (x0, y0) == ((0 + 999 + 1 - 4096) // 2, (0 + 1999 + 1 - 4096) // 2)
    assert FaceChips(margin=0, encode=None).square(face([0, 0, 9999, 5]))[2] == 4096


def test_who_as_a_set_and_as_a_callable():
    faces = [face([0, 0, 9, 9], "employee"), face([0, 0, 9, 9], "visitor"), face([0, 0, 9, 9], "unknown"),
             face([0, 0, 9, 9], "contractor"), {"bbox": [0, 0, 9, 9]}]
    assert [FaceChips(encode=None).selects(f) for f in faces] == [True] * 5
    assert [FaceChips(who=("unknown",), encode=None).selects(f) for f in faces] == [False, False, True, True, True]
    assert [FaceChips(who="employee", encode=None).selects(f) for f in faces] == [True, False, False, False, False]
    assert [FaceChips(who=(), encode=None).selects(f) for f in faces] == [False] * 5
    fresh = FaceChips(who=lambda r: not r.get("tracked"), encode=None)
    assert fresh.selects(face([0, 0, 1, 1], tracked=False)) and not fresh.selects(face([0, 0, 1, 1], tracked=True))
    with pytest.raises(ValueError, match="who holds"):
        FaceChips(who=("employee", "stranger"), encode=None)


def test_a_face_the_redactor_masks_gets_no_chip_unless_masked():
    res = [[face([0, 0, 9, 9], "employee"), face([20, 0, 29, 9], "unknown"), face([40, 0, 49, 9], "visitor")]]
    red = Redactor(who=("unknown", "visitor"))
    recs, owners = FaceChips(encode=None).records(res, redact=red)
    assert owners == [(0, 0)] and recs[0].tolist() == [0, -3, -3, 16]
    recs, owners = FaceChips(encode=None, masked=True).records(res, redact=red)
    assert owners == [(0, 0), (0, 1), (0, 2)]
    recs, owners = FaceChips(encode=None).records(res)                        # no redactor in the call: everybody the object selects
    assert owners == [(0, 0), (0, 1), (0, 2)]
    recs, owners = FaceChips(encode=None, who=("unknown",)).records(res, redact=Redactor(who=("employee",)))
    assert owners == [(0, 1)]


def test_records_are_padded_to_a_power_of_two_with_records_that_name_no_frame():
    c = FaceChips(margin=0, encode=None)
    unchanged = object()
    res = [[face([1, 2, 10, 11])], None, unchanged, [], [face([5, 5, 6, 6]), face([0, 0, 99, 49])]]
    recs, owners = c.records(res)
    assert recs.dtype == np.int32 and recs.shape == (16, 4)
    assert owners == [(0, 0), (4, 0), (4, 1)]
    assert recs[:3].tolist() == [[0, 1, 2, 10], [4, 5, 5, 2], [4, 0, -25, 100]]
    assert (recs[3:, 0] == -1).all() and not recs[3:, 1:].any()
    for count, padded in ((0, 16), (1, 16), (16, 16), (17, 32), (32, 32), (33, 64), (100, 128)):
        recs, owners = c.records([[face([0, 0, 3, 3])] * count])
        assert len(owners) == count and recs.shape == (padded, 4) and (recs[count:, 0] == -1).all()
    # a coordinate beyond the limit stays beyond it (the kernel answers with fill) and fits an int32
    recs, owners = c.records([[face([1 << 40, 0, (1 << 40) + 9, 9])]])
    assert owners == [(0, 0)] and recs[0, 1] > COORD_LIMIT and recs[0, 3] == 10


def test_arguments_are_validated():
    for size in (15, 257, 0):
        with pytest.raises(ValueError, match="size"):
            FaceChips(size=size, encode=None)
    for margin in (-1, 401):
        with pytest.raises(ValueError, match="margin"):
            FaceChips(margin=margin, encode=None)
    for fill in ((0, 0), (0, 0, 256), (-1, 0, 0)):
        with pytest.raises(ValueError, match="fill"):
            FaceChips(fill=fill, encode=None)
    with pytest.raises(ValueError, match="encode"):
        FaceChips(encode="jpeg")
    c = FaceChips(size=16, margin=0, fill=(1, 2, 3), encode=None)
    assert (c.size, c.margin, c.bgr_word, c.encode, c.masked) == (16, 0, 1 | 2 << 8 | 3 << 16, None, False)
    from facerecognition_infrenceengine_amd import JpegEncoder
    import facerecognition_infrenceengine_amd as pkg
    import app.services as services
    assert pkg.FaceChips is FaceChips and services.FaceChips is FaceChips
    d = FaceChips()
    assert isinstance(d.encode, JpegEncoder) and d.encode.quality == 85 and (d.size, d.margin) == (112, 30)
    assert FaceChips().encode is not d.encode                                 # an encoder of its own: its buffers are not shared
