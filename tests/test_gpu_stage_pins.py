"""GPU pins of the two f16 stage kernels, fr_conv_stage14_f16 and fr_conv_stage28_f16, over WHOLE RUNS of residual blocks, against
the float64 references of tests/helpers/stage_ref.py (tests/test_stage_ref_host.py shows on the CPU that these instruments fail a
planted fault).  One workgroup owns a face for the run; what only exists from the second block on - input taken from the kernel's
own output, the weight ring across a block boundary, parameters by LDS-DMA, a second parked residual, the 28x28 kernel's halo
prefetch across a conv boundary - is what these runs are for.

1. Exact runs: integer operands, a fixed number of +-1 weights per row placed so that every K step of every wave group multiplies
   something, parameters new for every conv.  2, 3 and 7 blocks at 2 per row, 4 blocks at 4 per row, 1 and 3 faces; the 3-block run
   also on 256 and 257 faces built from 7 distinct ones.  torch.equal; the output the kernel does not alias is pre-filled with NaN;
   for 28x28 the scratch map must hold the reference's LAST `mid` bit for bit.  The deep runs pass 2048, so every conv's f32 -> f16
   rounding (ties to even, both ways, and non-ties) is part of what is compared.
2. Composition on float operands at the network's depth (29 blocks at 14x14, 12 at 28x28): a run equals its prefix followed by the
   rest, cut at 1, N / 2 and N - 1, and every run of up to 5 blocks equals one-block launches chained - bit for bit, with no
   reference: a block's arithmetic does not depend on its index in the run, so anything that does (ring phase, parameter DMA,
   residual source, stream offsets) shows.
3. Per element against float64 on float operands: one conv of a block is a signed channel permutation on the centre tap, so the
   other conv's every element stands in the output; bound = embed_ref.conv_bound.  Block 0 of a run and the last block of three.

Every float64 test prints its worst err / bound; docs/KERNEL_NOTES.md 4.12 records them."""
import numpy as np
import pytest
import torch

from tests.helpers import stage_ref as sr

pytestmark = pytest.mark.gpu
NAN = float("nan")
DEPTH = {14: 29, 28: 12}                    # IResNet-100's stride-1 blocks at each geometry


def _dev(a, dtype=torch.float16):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _per(lib, HW):
    return getattr(lib, f"fr_conv_stage{HW}_weight_bytes")(1) // 2


def _pack(lib, HW, wd):
    """wd [nconv][C][9 C] f16 on the device -> the kernels' weight stream."""
    from facerecognition_infrenceengine_amd import _lib
    per = _per(lib, HW)
    stream = torch.empty(wd.shape[0] * per, dtype=torch.float16, device="cuda")
    for j in range(wd.shape[0]):
        wj, sj = wd[j], stream[j * per:]
        assert getattr(lib, f"fr_conv_stage{HW}_pack")(_lib.ptr(wj), _lib.ptr(sj), _lib.stream_ptr()) == 0
    return stream


def _run(lib, HW, xd, stream, pd, first, last):
    """Blocks first .. last - 1 of the run on xd (left unchanged) -> (output, the 28x28 kernel's scratch map or None).  The entry
    points take raw pointers: the stream and the parameters of block `first` are where the launch starts."""
    from facerecognition_infrenceengine_amd import _lib
    B, n = xd.shape[0], last - first
    ws, ps = stream[2 * first * _per(lib, HW):], pd[2 * first:]
    assert ps.is_contiguous() and pd.shape[0] >= 2 * last
    if HW == 14:
        y = torch.full_like(xd, NAN)
        assert lib.fr_conv_stage14_f16(_lib.ptr(xd), _lib.ptr(y), _lib.ptr(ws), _lib.ptr(ps), B, n, _lib.stream_ptr()) == 0
        mid = None
    else:
        y, mid = xd.clone(), torch.full_like(xd, NAN)
        assert lib.fr_conv_stage28_f16(_lib.ptr(y), _lib.ptr(mid), _lib.ptr(ws), _lib.ptr(ps), B, n, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    return y, mid


def _operands(lib, HW, x, w, prm):
    return _dev(x), _pack(lib, HW, _dev(np.stack(w))), _dev(prm, torch.float32)


# ---------------------------------------------------------------- 1. exact runs
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("depth", sr.DEPTHS, ids=lambda d: f"{d[0]}x{d[1]}")
@pytest.mark.parametrize("HW", [14, 28])
def test_stage_run_exact(lib, HW, depth, B):
    o = sr.exact_case(HW, *depth, B)                     # asserts exactness, K-step coverage and the events on the reference
    xd, stream, pd = _operands(lib, HW, o.x, o.w, o.prm)
    y, mid = _run(lib, HW, xd, stream, pd, 0, o.nblocks)
    print(f"\nexact run {HW}x{HW}, {depth[0]} blocks at {depth[1]} per row, {B} faces: max |v| per block {o.growth}")
    assert torch.equal(y.cpu(), torch.from_numpy(o.want).to(torch.float16))
    if mid is not None:
        assert torch.equal(mid.cpu(), torch.from_numpy(o.mids[-1]).to(torch.float16))


@pytest.mark.parametrize("B", [256, 257])
@pytest.mark.parametrize("HW", [14, 28])
def test_stage_run_exact_wide(lib, HW, B):
    """More workgroups than CUs (257: a second workgroup on a CU while 255 others still run, the shared L2, the sc1 loads of maps
    the workgroup itself wrote): 7 distinct faces in the order i % 7, so that every neighbour differs; 3 blocks."""
    o = sr.exact_case(HW, 3, 2, sr.WIDE_FACES)
    x7, stream, pd = _operands(lib, HW, o.x, o.w, o.prm)
    idx = (torch.arange(B) % sr.WIDE_FACES).cuda()
    xd = x7[idx].contiguous()
    y, mid = _run(lib, HW, xd, stream, pd, 0, 3)
    assert torch.equal(y, _dev(o.want)[idx])
    if mid is not None:
        assert torch.equal(mid, _dev(o.mids[-1])[idx])


# ---------------------------------------------------------------- 2. composition at the network's depth
@pytest.fixture(scope="module", params=[14, 28])
def deep(request, lib):
    HW = request.param
    N = DEPTH[HW]
    x, w, prm = sr.float_run_operands(HW, N, 3, 1000 + HW)
    xd, wd, pd = x.cuda(), w.cuda(), prm.cuda()
    stream = _pack(lib, HW, wd)
    whole, _ = _run(lib, HW, xd, stream, pd, 0, N)
    return HW, N, xd, stream, pd, whole


def test_deep_run_stays_finite(deep):
    HW, N, xd, stream, pd, whole = deep
    assert torch.isfinite(whole).all() and 0.5 < whole.float().abs().max().item() < 100.0
    assert not torch.equal(whole, xd)


@pytest.mark.parametrize("cut", ["1", "N/2", "N-1"])
def test_deep_run_equals_prefix_then_rest(lib, deep, cut):
    HW, N, xd, stream, pd, whole = deep
    k = {"1": 1, "N/2": N // 2, "N-1": N - 1}[cut]
    head, _ = _run(lib, HW, xd, stream, pd, 0, k)
    tail, _ = _run(lib, HW, head, stream, pd, k, N)
    assert torch.equal(tail, whole)


def test_every_short_run_equals_chained_one_block_launches(lib, deep):
    HW, N, xd, stream, pd, whole = deep
    h = xd
    for n in range(5):
        h, _ = _run(lib, HW, h, stream, pd, n, n + 1)
        run, _ = _run(lib, HW, xd, stream, pd, 0, n + 1)
        assert torch.isfinite(run).all() and torch.equal(run, h), n


# ---------------------------------------------------------------- 3. per element through a selecting partner conv
@pytest.mark.parametrize("which", ["conv2", "conv1"])
@pytest.mark.parametrize("HW", [14, 28])
def test_stage_block_per_element_through_a_selector(lib, HW, which):
    """conv2 the selector: conv1 (9-class bias, PReLU with zero and negative slopes) per element - where the block's input is zero
    (half the channels of the block-0 cases) its f16 element stands in the output untouched; conv1 the selector: conv2 + bias +
    residual per element.  For 28x28 the scratch map shows `mid` itself and is held to the same bound."""
    for name, x, w, prm, blk, j0 in sr.selector_cases(HW, which):
        xd, stream, pd = _operands(lib, HW, x, w, prm)
        y, mid = _run(lib, HW, xd, stream, pd, 0, j0 // 2 + 1)
        r = sr.selector_ratio(blk, y.cpu().numpy(), None if mid is None else mid.cpu().numpy())
        print(f"\nfr_conv_stage{HW}_f16, selector {which}, {name}: worst err / bound {r:.4f}")
        assert r <= 1.0, (name, r)
