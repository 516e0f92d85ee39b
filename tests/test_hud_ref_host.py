"""The HUD's definition (tests/helpers/hud_ref.py), its font and the host half of the drawing (``Hud.records``) against values
worked out by hand (no GPU).  The kernel is pinned to hud_ref byte for byte (tests/test_gpu_hud.py); this pins hud_ref."""
import numpy as np
import pytest

from tests.helpers import hud_ref

GREEN = (0, 255, 0)


def _draw(H, W, box, colour=GREEN, dh=0, rh=0, lines=(b"A",), scale=1, fill=200):
    from tests.helpers import hud_cases
    counts, faces, text = hud_cases.pack([[hud_cases.face(box, colour, dh, rh, lines)]], cap=2, seed=3)
    return hud_ref.draw_records(np.full((H, W, 3), fill, np.uint8), counts[0], faces[0], text[0], scale)


def _px(img, x, y):
    return tuple(int(v) for v in img[y, x])


def test_layers_on_a_frame_of_constant_200():
    """One face, box (20,6)-(50,26), green, dh 0, rh 10, one line "A", scale 1, on 64 x 96 of 200."""
    img = _draw(64, 96, (20, 6, 50, 26), dh=0, rh=10)
    # box: (102 c + 154 * 200 + 128) >> 8 = 30928 >> 8 = 120 for c = 0, 56938 >> 8 = 222 for c = 255; two pixels thick
    assert _px(img, 40, 6) == (120, 222, 120) and _px(img, 40, 7) == (120, 222, 120)
    assert _px(img, 40, 8) == (200, 200, 200) and _px(img, 40, 5) == (200, 200, 200)
    assert _px(img, 49, 23) == (120, 222, 120) and _px(img, 48, 23) == (200, 200, 200)
    # ticks of corner (20, 6): the diagonal u + v = 15 +- 1, opaque
    assert _px(img, 27, 14) == GREEN and _px(img, 27, 15) == GREEN and _px(img, 27, 13) == GREEN
    assert _px(img, 27, 16) == (200, 200, 200)
    assert _px(img, 35, 5) == GREEN and _px(img, 36, 5) == (200, 200, 200)          # the horizontal arm ends at cx + 15
    assert _px(img, 19, 21) == GREEN and _px(img, 18, 21) == (200, 200, 200)        # the vertical arm is cx - 1 .. cx + 1
    # corner (50, 6) points right / down too: its horizontal arm leaves the box
    assert _px(img, 65, 5) == GREEN and _px(img, 66, 5) == (200, 200, 200)
    assert _px(img, 65, 6) == (100, 100, 100)          # ... and the bar's outline, a later layer, is drawn over it
    # detection bar at bx = 60: grey outline, dh = 0 still fills one row in orange, the interior is untouched
    assert _px(img, 60, 15) == (100, 100, 100) and _px(img, 66, 15) == (100, 100, 100) and _px(img, 63, 15) == (200, 200, 200)
    assert _px(img, 63, 26) == (255, 140, 0) and _px(img, 60, 26) == (255, 140, 0) and _px(img, 66, 26) == (255, 140, 0)
    assert _px(img, 63, 25) == GREEN                   # the tick of corner (50, 26) under the bar's empty interior
    # recognition bar at 72: filled with the face's colour over rows y2 - 10 .. y2
    assert _px(img, 75, 20) == GREEN and _px(img, 75, 16) == GREEN and _px(img, 75, 15) == (200, 200, 200)
    assert _px(img, 72, 10) == (100, 100, 100)
    # the letters start at y1 - 12 = -6: only their last row is inside the frame ('D' = ###.., 'R' = #...#)
    assert [_px(img, x, 0) == (255, 255, 255) for x in range(57, 63)] == [False, True, True, True, False, False]
    assert [_px(img, x, 0) == (255, 255, 255) for x in range(69, 76)] == [False, True, False, False, False, True, False]
    # panel: pw = 12 + 20, ph = 18 + 10, at (20, 36); background (6150 + 51 * 200 + 128) >> 8 = 64; border in the colour
    assert hud_ref.panel_rect(20, 6, 50, 26, [1], 64, 96, 1) == (20, 36, 32, 28)
    assert _px(img, 45, 50) == (64, 64, 64) and _px(img, 20, 45) == GREEN and _px(img, 52, 45) == GREEN
    assert _px(img, 35, 36) == GREEN and _px(img, 53, 45) == (200, 200, 200) and _px(img, 35, 35) == (200, 200, 200)
    # the tick of corner (20, 26) under the panel: green first, then the background blend (6150 + 51 * 255 + 128) >> 8 = 75
    assert _px(img, 21, 40) == (24, 75, 24)
    # text "A" at (30, 37), glyph pixels 2 x 2: row 0 = .###. lights x 32 .. 37, row 4 = ##### starts at x 30
    assert _px(img, 32, 37) == (255, 255, 255) and _px(img, 37, 38) == (255, 255, 255)
    assert _px(img, 30, 37) == (64, 64, 64) and _px(img, 38, 37) == (64, 64, 64)
    assert _px(img, 30, 45) == (255, 255, 255) and _px(img, 39, 46) == (255, 255, 255) and _px(img, 40, 45) == (64, 64, 64)
    assert _px(img, 30, 51) == (64, 64, 64)                                          # below the seven glyph rows


def test_scale_multiplies_every_length():
    img = _draw(128, 192, (40, 12, 100, 52), dh=0, rh=20, scale=2)
    assert _px(img, 80, 15) == (120, 222, 120) and _px(img, 80, 16) == (200, 200, 200)          # the box is four thick
    assert _px(img, 70, 12) == GREEN and _px(img, 71, 11) == (200, 200, 200)                     # the arm reaches cx + 30
    assert _px(img, 120, 30) == (100, 100, 100) and _px(img, 121, 30) == (100, 100, 100) and _px(img, 122, 30) == (200, 200, 200)
    assert hud_ref.panel_rect(40, 12, 100, 52, [1], 128, 192, 2) == (40, 72, 64, 56)


def test_panel_position():
    # below the box when it fits
    assert hud_ref.panel_rect(50, 10, 90, 30, [5, 3], 100, 200, 1) == (50, 40, 80, 46)
    # it would leave the bottom (95 + 46 > 100): above the box, at y1 - ph - 10
    assert hud_ref.panel_rect(50, 60, 90, 85, [5, 3], 100, 200, 1) == (50, 4, 80, 46)
    # ... and never above the frame
    assert hud_ref.panel_rect(50, 40, 90, 85, [5, 3], 100, 200, 1) == (50, 0, 80, 46)
    # exactly fitting stays below: py + ph == H is not "beyond"
    assert hud_ref.panel_rect(50, 10, 90, 44, [5, 3], 100, 200, 1)[1] == 54
    # px clamps at the right edge, and at 0 for a box left of the frame
    assert hud_ref.panel_rect(150, 10, 190, 30, [5, 3], 100, 200, 1)[0] == 120
    assert hud_ref.panel_rect(-30, 10, 20, 30, [5, 3], 100, 200, 1)[0] == 0
    # a panel wider than the frame starts at 0 and is clipped by the frame
    assert hud_ref.panel_rect(150, 10, 190, 30, [20], 100, 200, 1)[:3] == (0, 40, 260)
    img = _draw(100, 200, (150, 10, 190, 30), lines=(b"x" * 20,))
    assert _px(img, 199, 50) == (64, 64, 64) and _px(img, 0, 50) == GREEN and _px(img, 100, 40) == GREEN
    # the flipped panel is drawn where panel_rect says
    img = _draw(100, 200, (50, 60, 90, 85), lines=(b"abcde", b"abc"))
    assert _px(img, 50, 4) == GREEN and _px(img, 130, 50) == GREEN and _px(img, 100, 3) == (200, 200, 200)


def _result(kind="employee", bbox=(10, 20, 50, 80), det=0.93, rec=0.874, **info):
    base = {"employee": {"name": "Ann", "employeeId": "E7", "type": "employee"}, "visitor": {"name": "Bob", "type": "visitor"},
            "unknown": {"name": "Unknown", "type": "unknown"}}[kind]
    return {"bbox": np.array(bbox), "person_id": None, "person_info": dict(base, **info), "det_score": det,
            "recognition_score": rec}


def _lines(faces, text, j=0):
    return [bytes(text[j, i, :faces[j, 10 + i]]).decode() for i in range(faces[j, 9])]


def test_records_lines_colours_and_heights():
    from facerecognition_infrenceengine_amd.hud import Hud
    hud = Hud()
    faces, text = hud.records([_result("employee"), _result("visitor"), _result("unknown", rec=0)], (120, 160))
    assert faces.shape == (3, 16) and faces.dtype == np.int32 and text.shape == (3, 4, 40) and text.dtype == np.uint8
    assert _lines(faces, text, 0) == ["Name: Ann", "ID: E7", "Type: Employee", "Score: 0.87"]
    assert _lines(faces, text, 1) == ["Name: Bob", "Type: Visitor", "Score: 0.87"]
    assert _lines(faces, text, 2) == ["Unknown Person", "Detection: 0.93"]
    assert faces[:, 4:7].tolist() == [[0, 255, 0], [0, 255, 255], [0, 0, 255]]           # annotate's colours
    assert faces[:, :4].tolist() == [[10, 20, 50, 80]] * 3
    assert faces[:, 7].tolist() == [55, 55, 55]                  # int(60 * 0.93) = int(55.8)
    assert faces[:, 8].tolist() == [52, 52, 0]                   # int(60 * 0.874) = int(52.44); the unknown's score is 0
    assert not faces[:, 14:].any()
    # no employeeId in the metadata: the line is there and empty behind its label
    info = {"name": "Cy", "type": "employee"}
    faces, text = hud.records([dict(_result(), person_info=info)], (120, 160))
    assert _lines(faces, text) == ["Name: Cy", "ID: ", "Type: Employee", "Score: 0.87"]
    assert hud.records(None, (120, 160))[0].shape == (0, 16) and hud.records([], (120, 160))[1].shape == (0, 4, 40)


def test_records_truncation_ascii_scores_and_coordinates():
    from facerecognition_infrenceengine_amd.hud import Hud
    faces, text = Hud().records([_result(name="N" * 50)], (120, 160))
    assert _lines(faces, text)[0] == "Name: " + "N" * 34 and faces[0, 10] == 40
    faces, text = Hud(max_chars=8).records([_result(name="Zoë中")], (120, 160))
    assert _lines(faces, text) == ["Name: Zo", "ID: E7", "Type: Em", "Score: 0"]
    faces, text = Hud().records([_result(name="Zoë 中\x07.")], (120, 160))
    assert _lines(faces, text)[0] == "Name: Zo? ??."                    # one '?' per character that is not printable ASCII
    # a score above 1 fills the bar, NaN and a negative score give 0
    faces, _ = Hud().records([_result(det=1.7, rec=float("nan")), _result(det=-0.5, rec=1.0)], (120, 160))
    assert faces[:, 7].tolist() == [60, 0] and faces[:, 8].tolist() == [0, 60]
    # swapped corners are ordered
    faces, _ = Hud().records([_result(bbox=(50, 80, 10, 20))], (120, 160))
    assert faces[0, :4].tolist() == [10, 20, 50, 80] and faces[0, 7] == 55
    # a preview: floor, not truncation, for negative coordinates (-5 * 80 // 160 = -3, -3 * 60 // 120 = -2)
    faces, _ = Hud().records([_result(bbox=(-5, -3, 7, 9), det=1.0)], (120, 160), out_hw=(60, 80))
    assert faces[0, :4].tolist() == [-3, -2, 3, 4] and faces[0, 7] == 6
    # the helper's own packing of the same dicts agrees with the package's, preview or not
    res = [_result("employee", name="Zoë" * 20), _result("visitor", bbox=(70, 90, -5, -3), det=float("nan")), _result("unknown")]
    for out_hw in (None, (45, 60)):
        a, b = Hud().records(res, (120, 160), out_hw), hud_ref.pack(res, (120, 160), out_hw)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_hud_arguments():
    from facerecognition_infrenceengine_amd.hud import Hud
    for bad in (0, 9, -1):
        with pytest.raises(ValueError, match="scale"):
            Hud(scale=bad)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="max_chars"):
            Hud(max_chars=bad)
    with pytest.raises(ValueError, match="font"):
        Hud(font=np.zeros((96, 7), np.uint8))
    assert Hud(out_size=(80, 60)).out_hw((120, 160)) == (60, 80) and Hud().out_hw((120, 160)) is None
    from facerecognition_infrenceengine_amd.letterbox import letterbox_geometry
    assert Hud(out_size=(80, 60)).out_hw((90, 160)) == letterbox_geometry(90, 160, (80, 60))[:2] == (45, 80)


def test_pack_lays_the_batch_out_for_the_kernel():
    from facerecognition_infrenceengine_amd.hud import Hud
    hud = Hud(max_chars=12)
    per_frame = [[_result("unknown")], None, [_result("employee"), _result("visitor")], []]
    buf, cap, at_faces, at_text = hud.pack(per_frame, [(120, 160)] * 4)
    assert cap == 2 and at_faces == 16 and at_text == 16 + 4 * 4 * 2 * 16 and len(buf) == at_text + 4 * 2 * 4 * 12
    assert buf[:16].view(np.int32).tolist() == [1, 0, 2, 0]
    faces = buf[at_faces:at_text].view(np.int32).reshape(4, 2, 16)
    assert faces[2, 1, 4:7].tolist() == [0, 255, 255] and faces[0, 0, 9] == 2 and not faces[1].any()


def test_font():
    from facerecognition_infrenceengine_amd.hud_font import FONT, probe_font
    assert FONT.shape == (95, 7) and FONT.dtype == np.uint8
    assert int(FONT.max()) < 32                                  # every glyph fits in 5 columns
    empty = [k for k in range(95) if not FONT[k].any()]
    assert empty == [0]                                          # only the space is empty
    assert len({bytes(g) for g in FONT}) == 95                   # all glyphs are distinct
    assert FONT[ord("D") - 32].tolist() == [0x1C, 0x12, 0x11, 0x11, 0x11, 0x12, 0x1C]
    p = probe_font()
    assert p.shape == (95, 7) and [bin(int(v)).count("1") for v in p.reshape(-1)].count(1) == 95 and int((p != 0).sum()) == 95
    with pytest.raises(ValueError):
        FONT[0, 0] = 1                                           # the one table is read-only
