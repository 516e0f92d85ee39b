"""GPU pins of the embed net's ASSEMBLY on real (synthetic-seeded) weights: what IResNetHIP holds on the device after
fold_iresnet / _pack_w / _pack_stage, and every step of real forwards, against tests/helpers/fold_ref.py (tests/test_fold_ref_host.py
ties that helper to the unfolded net and to oracle.nets and shows that it fails planted fold, source and residual errors).

A. Read-back, exact: every conv's weights, bias and slope, the FC bias and the stage runs' parameter rows are torch.equal to
   fold_ref.engine_operands / stage_params.  (The swizzled streams are pinned by their pack entry points elsewhere.)
B. Every step of a real forward, teacher-forced by the network's own dataflow: _issue, _run_stage and _fc are wrapped, the
   output rows of three faces (first, middle, last) cloned straight after each call, and fold_ref.check_forward takes each step's
   inputs from the recorded outputs that the GRAPH names.  Every picked element within the step's bound; the (route, conv)
   multiset seen equals embed_route's; a run taken in one launch equals, bit for bit, its own stream and parameter rows launched
   one block at a time on the recorded input.
C. Every block of both packed runs, launched alone on the previous block's GPU output, 2 faces, within fold_ref.block_ref.

Each test prints its worst err / bound and where; docs/KERNEL_NOTES.md 4.12 ("the embed net's assembly") records them."""
from collections import Counter
from types import SimpleNamespace

import pytest
import torch

from tests.helpers import fold_ref as fr

pytestmark = pytest.mark.gpu
NAN = float("nan")
SEEDS = {"r100": 1234, "r50": 77}


def _engine(arch):
    from facerecognition_infrenceengine_amd import weights
    from facerecognition_infrenceengine_amd.iresnet import IResNetHIP, fold_iresnet
    state = weights.synth_iresnet_state(arch, seed=SEEDS[arch])
    return SimpleNamespace(arch=arch, net=IResNetHIP(state, arch, "cuda:0"), fold=fold_iresnet(state, arch))


@pytest.fixture(scope="module")
def r100():
    return _engine("r100")


@pytest.fixture(scope="module")
def r50():
    return _engine("r50")


@pytest.fixture
def engine(r100, r50):
    return {"r100": r100, "r50": r50}


def _crops(B, seed):
    """f16 [B][112][112][8] on the device: RGB in channels 0 .. 2 in (-1, 1), the rest zero."""
    x = torch.zeros((B, 112, 112, 8), dtype=torch.float16)
    x[..., :3] = (torch.rand((B, 112, 112, 3), generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(torch.float16)
    return x.cuda()


# ---------------------------------------------------------------- A. read-back
@pytest.mark.parametrize("arch", ["r100", "r50"])
def test_device_operands_equal_the_fold(engine, arch):
    e = engine[arch]
    net, fold = e.net, e.fold
    assert set(net._convs) == set(net.table.convs)
    for key, c in net._convs.items():
        want = fr.engine_operands(fold, key)
        assert c.w.dtype == torch.float16 and torch.equal(c.w.cpu(), want.w), key
        for name in ("bias", "slope"):
            got, w = getattr(c, name), getattr(want, name)
            if key == "fc" and name == "bias":
                got = net.fc_bias
                assert c.bias is None
            assert (got is None) == (w is None), (key, name)
            if w is not None:
                assert got.dtype == torch.float32 and torch.equal(got.cpu(), w), (key, name)
        assert (c.k, c.stride, c.pad, c.bias_mode, c.cin, c.c2) == (want.k, want.stride, want.pad, want.bias_mode, want.cin, want.c2), key
    for st, run in ((net.stage14, net.table.run14), (net.stage28, net.table.run28)):
        assert (st["first"], st["n"]) == run
        assert torch.equal(st["prm"].cpu(), fr.stage_params(fold, *run))


# ---------------------------------------------------------------- B. every step of a real forward
def _per(lib, HW):
    return getattr(lib, f"fr_conv_stage{HW}_weight_bytes")(1) // 2


def _block_alone(net, HW, st, j, h):
    """Block j of the packed run `st` alone on h (left unchanged): the stream and the parameter rows start at the block's own
    offset, nblocks = 1 -> (out, the 28x28 kernel's `mid` map or None)."""
    from facerecognition_infrenceengine_amd import _lib
    ws, ps = st["w"][2 * j * _per(net.lib, HW):], st["prm"][2 * j:]
    assert ps.is_contiguous() and 0 <= j < st["n"]
    if HW == 14:
        y, mid = torch.full_like(h, NAN), None
        assert net.lib.fr_conv_stage14_f16(_lib.ptr(h), _lib.ptr(y), _lib.ptr(ws), _lib.ptr(ps), h.shape[0], 1, _lib.stream_ptr()) == 0
    else:
        y, mid = h.clone(), torch.full_like(h, NAN)
        assert net.lib.fr_conv_stage28_f16(_lib.ptr(y), _lib.ptr(mid), _lib.ptr(ws), _lib.ptr(ps), h.shape[0], 1, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    return y, mid


def _record_forward(net, x, pick, taps, monkeypatch):
    """forward(x) with _issue, _run_stage and _fc wrapped -> ({conv key: output rows `pick`, cloned right after the call}, emb,
    normed rows, [(route, conv key)] in call order)."""
    rec, log = {}, []
    issue, run_stage, fc = net._issue, net._run_stage, net._fc

    def keep(s, y):
        torch.cuda.synchronize()
        assert s.conv not in rec
        rec[s.conv] = y[pick].clone()

    def _issue(s, c, x, residual=None, x2=None, partial=None):
        y = issue(s, c, x, residual, x2, partial)
        log.append((s.route, s.conv))
        assert c is net._convs[s.conv]
        if y is not None:
            keep(s, y)
        return y

    def _run_stage(s, h):
        y = run_stage(s, h)
        log.append((s.route, s.conv))
        keep(s, y)
        return y

    def _fc(s, h, emb, normed):
        fc(s, h, emb, normed)
        torch.cuda.synchronize()
        rec["emb"], rec["normed"] = emb[pick].clone(), normed[pick].clone()

    with monkeypatch.context() as m:
        m.setattr(net, "_issue", _issue)
        m.setattr(net, "_run_stage", _run_stage)
        m.setattr(net, "_fc", _fc)
        emb, normed = net.forward(x, taps)
    assert torch.equal(emb[pick], rec["emb"]) and torch.equal(normed[pick], rec["normed"])
    return rec, rec.pop("emb"), rec.pop("normed"), log


@pytest.mark.parametrize("case", fr.FORWARD_CASES, ids=lambda c: f"{c[0]}-{c[1]}{'' if c[2] else '-unfused'}{'-tapped' if c[3] else ''}")
def test_every_step_of_a_forward(engine, monkeypatch, case):
    from facerecognition_infrenceengine_amd import iresnet
    arch, B, fuse, tapped = case
    net, fold = engine[arch].net, engine[arch].fold
    route = iresnet.embed_route(net.table, B, iresnet.RouteMode(fuse_shortcut=fuse, tapped=tapped))
    pick = fr.picked_faces(B)
    x = _crops(B, 1000 + B)
    monkeypatch.setattr(net, "fuse_shortcut", fuse)
    rec, emb, normed, log = _record_forward(net, x, pick, {} if tapped else None, monkeypatch)
    assert Counter(log) == Counter((s.route, s.conv) for s in route)
    assert [k for _, k in log] == [s.conv for s in route]

    def run_check(s, h_in, got):
        """structural: the run's output rows equal its own stream and rows launched block by block on the recorded input"""
        HW = 28 if s.route == iresnet.STAGE28 else 14
        st = net.stage28 if HW == 28 else net.stage14
        assert s.conv == (st["first"], st["n"]) and h_in.shape == got.shape == (len(pick), HW, HW, fr.WIDTHS[1 if HW == 28 else 2])
        h = h_in
        for j in range(st["n"]):
            h, _ = _block_alone(net, HW, st, j, h)
        assert torch.equal(h, got), s.conv

    ratios = fr.check_forward(fold, net.table, route, x[pick].cpu().double().numpy(), rec, emb, normed, run_check)
    assert len(ratios) == len(route) + 1 and fr.covered(route) >= {fr.step_id(s) for s in route if s.route not in fr.RUN_ROUTES}
    worst = max(ratios, key=ratios.get)
    by_route = {}
    for (r, _, k), v in ratios.items():
        name = "emb" if k == "fc" else k if k == "normed" else r
        if r not in fr.RUN_ROUTES:
            by_route[name] = max(by_route.get(name, 0.0), v)
    runs = [s.conv for s in route if s.route in fr.RUN_ROUTES]
    print(f"\n{arch}, {B} faces, fuse_shortcut {fuse}: worst err / bound {ratios[worst]:.4f} at {worst}; by route "
          + ", ".join(f"{r} {v:.4f}" for r, v in sorted(by_route.items())) + (f"; runs {runs} equal their blocks one by one" if runs else ""))
    assert all(v < 1 for v in ratios.values()), {k: v for k, v in ratios.items() if v >= 1}


# ---------------------------------------------------------------- C. every block of the packed runs
@pytest.mark.parametrize("HW", [28, 14])
@pytest.mark.parametrize("arch", ["r100", "r50"])
def test_every_block_of_the_packed_runs(engine, monkeypatch, arch, HW):
    """A block packed out of order, a c1 / c2 parameter row swapped or a slope of 1.0 where a PReLU belongs would show here: block j
    of the engine's own stream and rows against float64 from the FOLD's operands for block first + j."""
    net, fold = engine[arch].net, engine[arch].fold
    st = net.stage28 if HW == 28 else net.stage14
    first, n = st["first"], st["n"]
    x = _crops(2, 77)
    rec, _, _, _ = _record_forward(net, x, [0, 1], {}, monkeypatch)          # tapped: launch by launch, no run
    entry = (first - 1, "fz") if (first - 1, "fz") in rec else (first - 1, "c2")
    h = rec[entry]
    worst = (0.0, None)
    for j in range(n):
        y, mid = _block_alone(net, HW, st, j, h)
        o1, o2 = fr.engine_operands(fold, (first + j, "c1")), fr.engine_operands(fold, (first + j, "c2"))
        prm = fr.stage_params(fold, first + j, 1)
        want_mid, bound_mid, want, bound = fr.block_ref(h, o1.w, o2.w, prm)
        r = fr.ratio(y, want, bound)
        if mid is not None:
            r = max(r, fr.ratio(mid, want_mid, bound_mid))
        worst = max(worst, (r, first + j))
        h = y
    print(f"\n{arch} stage{HW}, blocks {first} .. {first + n - 1} one by one: worst err / bound {worst[0]:.4f} at block {worst[1]}")
    assert worst[0] < 1, worst
