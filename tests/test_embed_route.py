"""The embed net's route table on the CPU - no device, no library: ``embed_route(conv_table(arch), B, mode)`` must imply the C
calls tests/golden/embed_calls.json recorded on the commit before the route table existed (entry points, every shape field,
which pointers are set; tests/test_gpu_embed_calls.py compares what a GPU forward really issues, buffer rotation included),
and the batch-size modes must begin and end where the module constants say."""
import json
import os
import sys

import pytest

from facerecognition_infrenceengine_amd import iresnet
from facerecognition_infrenceengine_amd.iresnet import RouteMode, conv_table, embed_route
from facerecognition_infrenceengine_amd.weights import IRESNET_LAYERS, IRESNET_WIDTHS

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLDEN)
from make_embed_calls import CASES, R100_CASE, unrle  # noqa: E402

P = "P"


@pytest.fixture(scope="module")
def pinned():
    with open(os.path.join(GOLDEN, "embed_calls.json")) as f:
        return json.load(f)


def _mode(pinned, case):
    B, fp8, profiled, attrs = CASES[case]
    keys = frozenset((i, ("c1", "c2")[j]) for i, j in pinned["fp8_convs"]) if fp8 else frozenset()
    return B, RouteMode(fp8=keys, stage14_f8=fp8 and pinned["stage14_f8"], profiled=profiled, **attrs)


def _conv_args(s, c, B, launch_splitk, planned):
    """fr_conv_args as the fixture writes it; ``launch_splitk``: the partials launch of a launch-by-launch SPLITK step"""
    fc = s.conv == "fc"
    slope = P if s.conv == "stem" or s.conv[1] == "c1" else 0             # the convs with a PReLU epilogue
    shape = [B, s.H, s.W, c.cin, c.cout, c.k, c.k, c.stride, c.pad, s.Ho, s.Wo]
    if launch_splitk:
        return [P, P, 0, 0, 0, 0, P] + shape + [0, s.slices, P if s.x2 else 0, c.c2]
    partial = P if fc or (planned and s.route == iresnet.SPLITK) else 0
    return ([P, P, 0 if fc else P, 0 if fc else P, slope, P if s.res else 0, partial] + shape
            + [c.bias_mode, s.slices, P if s.x2 else 0, c.c2 if s.x2 else 0])


def implied_calls(table, route, B, planned):
    """The reduced C calls (make_embed_calls._reduce) of a forward that walks ``route`` on the default stream; in a planned
    one every pointer into the plan buffers reads "P" (``_flat`` does the same to the fixture)."""
    r, calls, seq = iresnet, [], []
    for s in route:
        c = table.convs.get(s.conv)
        slope = P if c is not None and (s.conv == "stem" or s.conv[1] == "c1") else 0
        res = P if s.res else 0
        if planned and s.conv != "fc":
            seq.append([iresnet._SEQ_KIND[s.route], _conv_args(s, c, B, False, True)])
        elif s.route == r.SPLITK:
            M = B * s.Ho * s.Wo
            calls.append(["fr_conv_nhwc_f16", _conv_args(s, c, B, True, False), 0])
            calls.append(["fr_conv_splitk_epilogue", P, s.slices, M, c.cout, s.Ho, s.Wo, P, c.bias_mode, slope, res, P, 0])
        elif s.route in (r.PLAIN, r.INBLOCK):
            calls.append(["fr_conv_inblock_f16" if s.route == r.INBLOCK else "fr_conv_nhwc_f16", _conv_args(s, c, B, False, False), 0])
        elif s.route == r.WALK64:
            calls.append(["fr_conv_walk64_f16", P, P, P, P, c.bias_mode, slope, res, B, s.H, c.cout, 0])
        elif s.route in (r.STAGE28, r.STAGE14):
            calls.append(["fr_conv_stage%d_f16" % s.H, P, P, P, P, B, s.conv[1], 0])
        elif s.route == r.STAGE14_F8:
            calls.append(["fr_conv_stage14_f8", P, P, P, P, P, B, s.conv[1], 0])
        elif s.route == r.CONV_F8:
            calls.append(["fr_conv_nhwc_f8", [P, P, P if s.want16 else 0, P if s.nxt else 0, P, P, slope, res, B, s.H, s.W, c.cin, c.cout,
                                              1, "F", P if s.nxt else 0], 0])
        else:
            assert s.route == r.QUANTISE                                    # the fixture's nets were calibrated centred
            calls.append(["fr_quantize_f16_f8_centred", P, P, B * s.H * s.W * c.cin, c.cin, P, "F", 0])
    if planned:
        calls.insert(0, ["fr_conv_sequence", seq, len(seq), 0])
    return calls + [["fr_fc_reduce_l2norm", P, iresnet.FC_SPLITK, B, 512, P, P, P, 0]]


def _flat(call):
    """a pinned call with its plan-buffer placements ([buffer, offset]) read as plain set pointers"""
    if call[0] != "fr_conv_sequence":
        return call
    return [call[0], [[kind, [P if isinstance(v, list) else v for v in args]] for kind, args in call[1]]] + call[2:]


@pytest.mark.parametrize("case", list(CASES))
def test_route_implies_the_pinned_calls(pinned, case):
    B, mode = _mode(pinned, case)
    table = conv_table(pinned["arch"])
    route = embed_route(table, B, mode)
    want = [_flat(c) for c in unrle(pinned["cases"][case]["calls"])]
    planned = want[0][0] == "fr_conv_sequence"
    assert planned == (B <= mode.low_batch and not (mode.profiled or mode.fp8))
    got = implied_calls(table, route, B, planned)
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "call %d: implied %s, pinned %s" % (k, g, w)


@pytest.mark.parametrize("case, arch", [("profiled_b4", None), ("profiled_b150", None), (R100_CASE, "r100")])
def test_route_gives_the_pinned_profile(pinned, case, arch):
    B, mode = _mode(pinned, case) if arch is None else (256, RouteMode(profiled=True))
    route = embed_route(conv_table(arch or pinned["arch"]), B, mode)
    got = [[s.variant, s.flops] for s in route if s.variant is not None]
    want = unrle(pinned["cases"][case]["profile"])
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "launch %d: route %s, pinned %s" % (k, g, w)


def _shape(route, B):
    """a route without what scales with the batch size"""
    return tuple(s._replace(flops=s.flops / B) for s in route)


def test_modes_begin_and_end_on_the_module_constants():
    table, mode = conv_table("r100"), RouteMode()
    shapes = {B: _shape(embed_route(table, B, mode), B) for B in range(1, 258)}
    last = sorted(B for B in range(1, 257) if shapes[B] != shapes[B + 1])    # the last batch size of every mode but the open one
    skip = iresnet.WALK64_SKIP
    assert last == [8, 48, 127, 128, 143, 159]
    assert last == [iresnet.LOW_BATCH, iresnet.SMALL_BATCH, iresnet.STAGE14_MIN_BATCH - 1, skip.start - 1,
                    iresnet.STAGE28_MIN_BATCH - 1, skip.stop - 1]
    assert iresnet.INBLOCK_BATCH == iresnet.LOW_BATCH          # one mode: the replayed sequence with its in-block convs


def _old_count_flops(arch):
    """IResNetHIP._count_flops as it stood before the table (there over the folded convs)"""
    f, hw, cin = 2 * 112 * 112 * 27 * 64, 112, 64
    for n, cout in zip(IRESNET_LAYERS[arch], IRESNET_WIDTHS):
        for j in range(n):
            f += 2 * hw * hw * cin * cout * 9
            ho = hw // (2 if j == 0 else 1)
            f += 2 * ho * ho * cout * cout * 9
            if j == 0:
                f += 2 * ho * ho * cin * cout
            hw, cin = ho, cout
    return f + 2 * 25088 * 512


def test_table_flops_and_stage_runs(pinned):
    for arch in ("r34", "r50", "r100"):
        assert conv_table(arch).flops_per_face == _old_count_flops(arch)
    for arch, flops in pinned["flops_per_face"].items():                    # what the networks of the fixture's commit reported
        assert conv_table(arch).flops_per_face == flops
    assert abs(conv_table("r50").flops_per_face / 1e9 - 12.6) < 0.2         # 12.62 GFLOP / face
    assert (conv_table("r100").run14, conv_table("r100").run28) == ((17, 29), (4, 12))
    assert (conv_table("r50").run14[1], conv_table("r50").run28[1]) == (13, 3)
    assert conv_table("r18").run14 is None and conv_table("r18").run28 is None
    assert sorted(k[0] for k in conv_table("r100").convs if k[1:] == ("fz",)) == [0, 3, 16, 46]
