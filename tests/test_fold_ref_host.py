"""The embed net's host assembly against its definition, on the CPU in float64 (tests/helpers/fold_ref.py): iresnet.fold_iresnet
(BN fold, nine border-class biases, FC permutation) step by step against the unfolded IResNet, the exporter form, the route
table's shapes - and the proof that these instruments fail planted fold errors which the 1 - cos < 1e-3 of the end-to-end tests
lets pass.  tests/test_gpu_embed_assembly.py holds the device side against the same helper."""
import functools

import numpy as np
import pytest
import torch

from facerecognition_infrenceengine_amd import iresnet, weights
from facerecognition_infrenceengine_amd.iresnet import conv_table, fold_iresnet
from oracle import nets as onets
from tests.helpers import embed_ref as er
from tests.helpers import fold_ref as fr

ARCHS = ("r18", "r34", "r50", "r100")
SEED = 1234


@functools.lru_cache(maxsize=None)
def case(arch):
    """(state, input, unfolded net, fold, clean err / bound per step) of an arch on 2 faces; made once, nobody changes it."""
    state = weights.synth_iresnet_state(arch, seed=SEED)
    x = torch.rand((2, 3, 112, 112), generator=torch.Generator().manual_seed(11), dtype=torch.float64) * 2 - 1
    net = fr.unfolded_blocks(state, arch, x)
    fold = fold_iresnet(state, arch)
    steps = fr.net_steps(net)
    clean = {key: fr.ratio(fr.folded_step(fold, key, inp), want, fr.host_bound(K, mag)) for key, inp, want, mag, K in steps}
    return state, x, net, fold, steps, clean


def step_ratio(fold, step):
    key, inp, want, mag, K = step
    return fr.ratio(fr.folded_step(fold, key, inp), want, fr.host_bound(K, mag))


@pytest.mark.parametrize("arch", ARCHS)
def test_folded_step_equals_unfolded_block(arch):
    """Every folded conv, fed the unfolded net's own input for it, gives the unfolded `mid` / shortcut / block output /
    embedding, every element within HOST_C (K + 2) 2^-53 mag (HOST_C = 3: the rounding count in fold_ref's docstring)."""
    state, x, net, fold, steps, clean = case(arch)
    # the helper is the oracle's net, not a third opinion: the same float64 state through oracle.nets
    ref = onets.iresnet_forward(fr.state64(state), x, weights.IRESNET_LAYERS[arch])
    tie = float((net.emb - ref).abs().max() / ref.abs().max())
    worst = max(clean, key=clean.get)
    print(f"\n{arch}: unfolded vs oracle.nets max rel {tie:.2e}; worst folded step {worst}: err / bound {clean[worst]:.4f}")
    assert tie <= 8 * 2.0 ** -52
    assert len(clean) == 2 + 2 * len(net.blocks) + 4
    assert all(r < 1 for r in clean.values()), {k: r for k, r in clean.items() if r >= 1}
    # the packed stem: 9 taps x 3 channels of [64][16][8], the rest zero
    wp = fold["stem"]["w"].reshape(64, 16, 8)
    assert not wp[:, 9:].any() and not wp[:, :, 3:].any() and wp[:, :9, :3].abs().min() > 0


def test_border_classes_on_small_maps():
    """One c1 (r18 block 1, 64 -> 64) on 5x5 and 6x7 maps, a constant and a ramp input: all nine classes occur, hold distinct
    values, and the folded conv equals bn1 -> zero padding -> conv -> bn2 -> PReLU per element.  The synthetic taps are not
    symmetric (asserted), so top / bottom and left / right differ and a swap exceeds the bound here."""
    state, _, _, fold, _, _ = case("r18")
    st, p, key = fr.state64(state), "layer1.1", (1, "c1")
    c = fold["blocks"][1]["c1"]
    b9 = fr.bias9(c)
    w1, t1 = st[p + ".conv1.weight"], st[p + ".bn1.bias"] - st[p + ".bn1.running_mean"] * st[p + ".bn1.weight"] / torch.sqrt(
        st[p + ".bn1.running_var"] + fr.BN_EPS)
    tap = (w1 * t1[None, :, None, None]).sum(1)                          # [co][kh][kw]: what a tap adds where it is inside
    scale = float(b9.abs().max())
    assert float((tap[:, 0].sum(1) - tap[:, 2].sum(1)).abs().min()) > 1e-6 * scale          # top row of taps != bottom row
    assert float((tap[:, :, 0].sum(1) - tap[:, :, 2].sum(1)).abs().min()) > 1e-6 * scale    # left column != right column
    flat = b9.reshape(9, -1)
    for a in range(9):
        for b in range(a + 1, 9):
            assert float((flat[a] - flat[b]).abs().min()) > 1e-6 * scale, (a, b)         # distinct in EVERY channel
    swaps = {"top/bottom": lambda f: fr.plant_swap_top_bottom(f, 1),
             "left/right": lambda f: f["blocks"][1]["c1"].__setitem__("bias", fr.bias9(f["blocks"][1]["c1"]).flip(1).reshape(-1).clone())}
    worst = 0.0
    for H, W in ((5, 5), (6, 7)):
        ramp = (torch.arange(H * W, dtype=torch.float64).reshape(1, 1, H, W) / (H * W) - 0.4) * torch.linspace(-1, 1, 64,
                                                                                                             dtype=torch.float64).reshape(1, 64, 1, 1)
        for x in (torch.full((1, 64, H, W), 0.37, dtype=torch.float64), ramp):
            blk = fr.unfolded_block(st, p, x, 1)
            step = (key, (x,), blk.mid, blk.mag_mid, 9 * 64)
            cls = er.border_class(H)[:, None] * 3 + er.border_class(W)[None, :]
            assert set(np.unique(cls).tolist()) == set(range(9))
            worst = max(worst, step_ratio(fold, step))
            for name, plant in swaps.items():
                bad = fr.copy_fold(fold)
                plant(bad)
                assert step_ratio(bad, step) > 10, (name, H, W)
    print(f"\nborder classes, 5x5 and 6x7, constant and ramp: worst err / bound {worst:.4f}")
    assert worst < 1


def exporter_state(state, arch):
    """The state as an exporter leaves it (onnx_import.py): bn2 / bn3 / downsample.1 of every block folded into the conv
    before them as weight + bias, their keys removed; bn1 (it precedes its conv) stays."""
    st = fr.state64(state)
    for i in range(sum(fr.LAYERS[arch])):
        p = fr.block_prefix(arch, i)
        for conv, bn in ((".conv1", ".bn2"), (".conv2", ".bn3"), (".downsample.0", ".downsample.1")):
            if p + conv + ".weight" not in st:
                continue
            s = st[p + bn + ".weight"] / torch.sqrt(st[p + bn + ".running_var"] + fr.BN_EPS)
            st[p + conv + ".bias"] = st[p + bn + ".bias"] - st[p + bn + ".running_mean"] * s
            st[p + conv + ".weight"] = st[p + conv + ".weight"] * s[:, None, None, None]
            for n in ("weight", "bias", "running_mean", "running_var"):
                del st[p + bn + "." + n]
    return st


@pytest.mark.parametrize("arch", ("r18", "r50"))
def test_exporter_form_gives_the_same_folded_steps(arch):
    """_bn_fold's identity branch with a conv bias: the same steps within the same bound (the exporter's fold makes the same
    roundings the engine's would: s is 3, the weight product 1, the shift 2)."""
    state, _, net, fold, steps, _ = case(arch)
    est = exporter_state(state, arch)
    assert not any(".bn2." in k or ".bn3." in k or "downsample.1" in k for k in est) and "layer1.0.conv1.bias" in est
    efold = fold_iresnet(est, arch)
    ratios = {s[0]: step_ratio(efold, s) for s in steps}
    worst = max(ratios, key=ratios.get)
    print(f"\n{arch}, exporter form: worst folded step {worst}: err / bound {ratios[worst]:.4f}")
    assert all(r < 1 for r in ratios.values()), {k: r for k, r in ratios.items() if r >= 1}


PLANTS = {
    "top/bottom classes swapped in block 5's conv1": lambda f, st: fr.plant_swap_top_bottom(f, 5),
    "corner classes = edge class in every block": lambda f, st: fr.plant_corner_is_edge(f),
    "no border classes (plain bias) in every block": lambda f, st: fr.plant_plain_bias(f),
    "block 5's PReLU slope from its neighbour": lambda f, st: fr.plant_neighbour_slope(f, 5),
    "eps twice in block 12's bn3": lambda f, st: fr.plant_eps_twice(f, st, 12, fr.block_prefix("r50", 12)),
    "FC columns left in NCHW order": lambda f, st: fr.plant_fc_nchw(f),
}


@pytest.mark.parametrize("name", list(PLANTS), ids=["swap", "corners", "plain", "slope", "eps", "fc"])
def test_the_instrument_notices_planted_fold_errors(name):
    """r50, 2 faces.  Each planted error exceeds the per-step bound by >= 10x at every step it was planted in and at no other
    (the steps are teacher-forced: an unchanged conv on unchanged inputs is the clean check, which passed) - while the embedding
    of the same broken fold, running free, stays within 1 - cos < 1e-3 of the unfolded net's: the end-to-end bound cannot see it.
    The FC permutation is the exception the end-to-end bound DOES see (it scrambles the embedding); that is asserted too."""
    state, x, net, fold, steps, clean = case("r50")
    bad = fr.copy_fold(fold)
    hit = PLANTS[name](bad, state)
    by_key = {s[0]: s for s in steps}
    ratios = {key: step_ratio(bad, by_key[key]) for key in hit}
    first = [s[0] for s in steps].index(hit[0])
    assert all(clean[s[0]] < 1 for s in steps[:first])
    assert all(clean[s[0]] < 1 for s in steps if s[0] not in hit)
    omc = float(fr.one_minus_cos(fr.folded_forward(bad, x), net.emb).max())
    print(f"\nplanted: {name}: err / bound min {min(ratios.values()):.3g} max {max(ratios.values()):.3g} over {len(hit)} steps; "
          f"free-running 1 - cos {omc:.2e}")
    assert min(ratios.values()) >= 10, ratios
    if hit == ["fc"]:
        assert omc > 1e-3
    else:
        assert omc < 1e-3


def test_clean_fold_running_free():
    """the clean fold's free-running embedding: float64 noise (the table of the issue: max rel err ~3e-15)"""
    _, x, net, fold, _, _ = case("r50")
    rel = float((fr.folded_forward(fold, x) - net.emb).abs().max() / net.emb.abs().max())
    print(f"\nr50 clean fold running free: max rel err {rel:.2e}")
    assert rel < 1e-12


@pytest.mark.parametrize("block", (1, 5, 12, 23))
def test_the_gpu_step_bound_notices(block):
    """The device-side bound (fold_ref.step_ref) on an f32 stand-in for the kernel - torch CPU float32 conv of the f16 operands,
    f16 store - at conv1 of one r50 block per width (64 / 128 / 256 / 512): the clean operands stay inside it, operands whose
    top / bottom classes are swapped or whose ONE corner class is its edge's do not."""
    _, _, net, fold, _, _ = case("r50")
    key = (block, "c1")
    x = er._f16(net.blocks[block].x.permute(0, 2, 3, 1).numpy())
    ops = fr.engine_operands(fold, key)
    want, mag, bound = fr.step_ref(key, ops, (x, None, None))
    got = {"clean": fr.ratio(fr.standin_step(key, ops, (x, None, None)), want, bound)}
    for name, plant in (("swap", lambda f: fr.plant_swap_top_bottom(f, block)),
                        ("corner", lambda f: fr.plant_corner_is_edge(f, [block], corners=((2, 2),)))):
        bad = fr.copy_fold(fold)
        plant(bad)
        got[name] = fr.ratio(fr.standin_step(key, fr.engine_operands(bad, key), (x, None, None)), want, bound)
    print(f"\nr50 block {block} conv1 (width {ops.w.shape[0]}), f32 stand-in: err / bound " + ", ".join(f"{k} {v:.3g}" for k, v in got.items()))
    assert got["clean"] < 1 and got["swap"] > 1 and got["corner"] > 1, got


@pytest.mark.parametrize("arch", ARCHS)
def test_route_table_shapes(arch):
    """conv_table's cin / cout / stride / H per key are what the unfolded net's tensors have, and flops_per_face is their sum."""
    _, _, net, _, _, _ = case(arch)
    t = conv_table(arch)
    seen = {"stem": (3, 3, 64, 1, 112, 112), "fc": (1, 25088, 512, 1, 1, 1)}               # k, cin, cout, stride, H, Ho
    for i, b in enumerate(net.blocks):
        assert b.mid.shape[1:] == (b.cout, b.H, b.H) and b.out.shape[1:] == (b.cout, b.H // b.stride, b.H // b.stride)
        seen[i, "c1"] = (3, b.cin, b.cout, 1, b.H, b.H)
        seen[i, "c2"] = (3, b.cout, b.cout, b.stride, b.H, b.out.shape[2])
        if b.sc is not None:
            seen[i, "sc"] = (1, b.cin, b.cout, b.stride, b.H, b.sc.shape[2])
    assert t.nblocks == len(net.blocks)
    flops = 0
    for key, (k, cin, cout, stride, H, Ho) in seen.items():
        c = t.convs[key]
        want_cin = 8 if key == "stem" else cin                              # the stem's input is packed to 8 channels
        assert (c.k, c.cin, c.cout, c.stride, c.H) == (k, want_cin, cout, stride, H), (key, c)
        assert c.flops == 2 * Ho * Ho * k * k * cin * cout, key
        flops += c.flops
    for key, c in t.convs.items():
        if key not in seen:                                                 # (i, "fz"): its block's c2 with the shortcut's rows
            i = key[0]
            assert key[1] == "fz" and c.c2 == seen[i, "sc"][1] and c.flops == t.convs[i, "c2"].flops + t.convs[i, "sc"].flops
            assert (c.k, c.cin, c.cout, c.stride, c.H) == seen[i, "c2"][:5]
    assert t.flops_per_face == flops
    assert iresnet.IRESNET_LAYERS[arch] == fr.LAYERS[arch] and iresnet.IRESNET_WIDTHS == fr.WIDTHS


def case_route(arch, B, fuse, tapped):
    return iresnet.embed_route(conv_table(arch), B, iresnet.RouteMode(fuse_shortcut=fuse, tapped=tapped))


def test_forward_cases_reach_every_route_of_every_conv():
    """The GPU cases (fold_ref.FORWARD_CASES; each asserts that it saw exactly its embed_route) between them take every conv
    of r100's table through every (route, slice count) that a forward of 1 .. 256 faces gives it, and the unfused case adds
    the shortcut convs and the stride-2 c2 apart."""
    t = conv_table("r100")
    possible = set()
    for B in range(1, 257):
        possible |= fr.covered(iresnet.embed_route(t, B, iresnet.RouteMode()))
    seen = set()
    for arch, B, fuse, tapped in fr.FORWARD_CASES:
        if arch == "r100":
            seen |= fr.covered(case_route(arch, B, fuse, tapped))
    assert possible <= seen, sorted(possible - seen, key=str)
    keys = {k for _, _, k in seen}
    assert keys == set(t.convs), set(t.convs) ^ keys
    assert {r for r, _, _ in seen} == {"plain", "splitk", "inblock", "walk64", "stage28", "stage14"}
    r50 = case_route(*fr.FORWARD_CASES[-1])
    assert sorted(s.conv[1] for s in r50 if s.route in fr.RUN_ROUTES) == [3, 13]


@pytest.mark.parametrize("fuse", (True, False))
def test_forward_check_on_the_standin(fuse):
    """fold_ref.check_forward - the GPU test's instrument - on a float32 stand-in forward of r18 over the 50-face route (3 faces
    computed): the clean forward is inside every step's bound; one that adds the wrong residual, or reads a c1 from the wrong
    block's output, misses at those steps and only there (the other steps are teacher-forced by the recorded tensors)."""
    _, _, _, fold, _, _ = case("r18")
    t = conv_table("r18")
    route = case_route("r18", 50, fuse, False)
    g = torch.Generator().manual_seed(3)
    x = np.zeros((3, 112, 112, 8))
    x[..., :3] = er._f16((torch.rand((3, 112, 112, 3), generator=g, dtype=torch.float64) * 2 - 1).numpy())
    rec, emb, normed = fr.standin_forward(fold, t, route, x)
    clean = fr.check_forward(fold, t, route, x, rec, emb, normed)
    worst = max(clean, key=clean.get)
    print(f"\nr18 stand-in forward, fuse_shortcut {fuse}: worst err / bound {clean[worst]:.4f} at {worst}")
    assert len(clean) == len(route) + 1 and all(r < 1 for r in clean.values()), clean
    for fault, kind in (("residual", "c2"), ("source", "c1")):
        rec, emb, normed = fr.standin_forward(fold, t, route, x, fault)
        got = fr.check_forward(fold, t, route, x, rec, emb, normed)
        missed = {k for k, r in got.items() if r >= 1}
        hit = {k for k in got if isinstance(k[2], tuple) and k[2][1] == kind and (i_ok(t, k[2], fault))}
        assert missed == hit and len(hit) >= 2, (fault, missed ^ hit)


def i_ok(table, key, fault):
    """the steps standin_forward's faults change"""
    i = key[0]
    if fault == "residual":
        return (i, "sc") not in table.convs
    return i >= 2 and (i - 1, "sc") not in table.convs               # blocks i - 2 and i - 1 give maps of one shape
