"""tests/helpers/pyramid_ref.py on the host: the layout restatement against the library's own size functions, the entry
contract of every table, and - on the float64 reference alone - that each table's thresholds give the GPU pins
(tests/test_gpu_pnet_pyramid_pins.py) something to decide."""
import math

import numpy as np
import pytest
import torch

from facerecognition_infrenceengine_amd import _lib
from tests.helpers import detect_ref as ref
from tests.helpers import pyramid_ref as P

NAMES = sorted(P.TABLES)


@pytest.fixture(scope="module")
def layers():
    return ref.pnet_layers(P.states()[0])


def test_states_are_the_precision_tests_draw():
    from tests import test_gpu_detect_precision as prec
    a, b = P.states(), prec._states(P.WEIGHT_SEED)
    assert P.C_F32 == prec.C_F32 and P.REFINE_MARGIN == prec.REFINE_MARGIN and P.SLOPES == prec.SLOPES
    for x, y in zip(a, b):
        assert sorted(x) == sorted(y) and all(torch.equal(x[k], y[k]) for k in x)
    assert bool((a[0]["prelu1.weight"] < 0).any()), "no negative conv1 slope: the activate-then-pool branch would not run"


@pytest.mark.parametrize("name", NAMES)
def test_layout_equals_the_librarys_size_functions(name):
    lib = _lib.load()
    t = P.TABLES[name]
    for li in range(len(t.levels)):
        H1, W1 = t.geo(li)
        lay = P.layout(t.N, H1, W1)
        assert lay["workspace_bytes"] == lib.fr_pnet23_workspace_bytes(t.N, H1, W1), (name, li)
        assert lay["band_tiles"] == lib.fr_pnet_band_tiles_count(t.N, H1, W1), (name, li)
        assert lay["band_tiles"] == P.conv1_tiles(t.N, *t.levels[li][:2]), (name, li)      # one conv1 tile = one band tile
        assert lay["grid"] * lay["seg_cap"] >= lay["tiles"] * 256 and lay["grid"] <= 512


@pytest.mark.parametrize("name", NAMES)
def test_tables_obey_the_entry_contract(name):
    t = P.TABLES[name]
    assert 1 <= len(t.levels) <= 16 and t.N >= 1
    for li, (hs, ws, f16, scale) in enumerate(t.levels):
        H1, W1 = t.geo(li)
        assert H1 == (hs - 1) // 2 and W1 == (ws - 1) // 2 and H1 >= 5 and W1 >= 5 and hs >= 3 and ws >= 3
        assert 0 < scale <= 1 and f16 in (0, 1)
        assert t.N * H1 * W1 * 64 < 2 ** 31 and P.conv1_tiles(t.N, hs, ws) < 2 ** 27
        # a cell's box corner names the cell: strictly increasing in the float32 formula
        bx = P.emit_boxes(np.arange(H1 - 4), np.zeros(H1 - 4), scale)[:, 1]
        by = P.emit_boxes(np.zeros(W1 - 4), np.arange(W1 - 4), scale)[:, 0]
        assert (np.diff(bx) > 0).all() and (np.diff(by) > 0).all()
    assert 0 < t.thr < 1 and math.isfinite(t.band(True)[1]) and t.band(False)[1] == float("-inf")


def test_tables_are_what_they_are_named_after():
    T = P.TABLES
    tiles = lambda t, li: P.conv1_tiles(t.N, *t.levels[li][:2])
    lay = lambda t, li: P.layout(t.N, *t.geo(li))
    assert [len(T[n].levels) for n in ("one_f32", "one_f16")] == [1, 1]
    assert T["one_f32"].levels[0][2] == 0 and T["one_f16"].levels[0][2] == 1
    s = T["sixteen"]
    assert len(s.levels) == 16 and [l[2] for l in s.levels] == [1] * 5 + [0] * 11
    assert [l[:2] for l in s.levels[-4:]] == [(11, 11), (12, 12), (11, 140), (140, 11)]
    assert [s.geo(li) for li in (12, 13, 14, 15)] == [(5, 5), (5, 5), (5, 69), (69, 5)]
    assert [l[2] for l in T["interleaved"].levels] == [0, 1, 0, 1, 1, 0]
    a = T["ascending"]
    assert all(x[0] * x[1] < y[0] * y[1] for x, y in zip(a.levels, a.levels[1:])) and {l[2] for l in a.levels} == {0, 1}
    w = T["twins"]
    assert w.levels[0][:2] == w.levels[1][:2] and w.levels[0][2] != w.levels[1][2]
    g = T["grid512"]
    assert [lay(g, li)["tiles"] for li in range(4)] == [512, 1, 518, 1]
    assert lay(g, 2)["grid"] == 512 and lay(g, 2)["seg_cap"] == 512 and lay(g, 0)["seg_cap"] == 256
    r = T["rpb8"]
    assert [tiles(r, li) for li in range(4)] == [4098, 6, 4098, 6] and [l[2] for l in r.levels] == [1, 1, 0, 0]
    for n, N in (("odd_even_1", 1), ("odd_even_3", 3)):
        o = T[n]
        assert o.N == N
        for f in (0, 1):
            assert {(hs % 2, ws % 2) for hs, ws, f16, _ in o.levels[:8] if f16 == f} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for t in T.values():         # every conv1 instantiation choice below the switch except where the table says otherwise
        assert t is r or all(tiles(t, li) < 4096 for li in range(len(t.levels)))


@pytest.mark.parametrize("name", NAMES)
def test_thresholds_give_the_pins_something_to_decide(name, layers):
    t = P.TABLES[name]
    refs = P.reference(t, P.level_images(t, P.frames(t)), layers)
    for li, r in enumerate(refs):
        H1, W1 = t.geo(li)
        assert r["conv1"].shape == (t.N, 10, H1, W1) and r["head"].shape == (t.N, 6, H1 - 4, W1 - 4)
        assert all(bool(torch.isfinite(v).all()) for v in r.values())
        # the band's premise on this table: the split chain's logit difference within margin / 20 of the exact one
        assert float((r["sdl"] - r["dl"]).abs().max()) <= P.REFINE_MARGIN / 20, (name, li)
    P.conditions(t, refs)
