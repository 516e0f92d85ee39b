"""The strip form of the O-Net crop + conv1 kernel (csrc/ro_conv1.hip, fr_crop_conv1_split with conv_f16 = 1: a wave walks a
strip of 16 conv columns down the crop and pools the raw MFMA sums in registers) against the tile form it replaces on the
batch path (conv_f16 = 2: bands of conv rows through an LDS tile): the same bytes in every valid slot, nothing written
anywhere else.  The R-Net keeps the tile form under both settings (its strip form measured slower, KERNEL_NOTES 4.3a); its
cases pin that dispatch and the shared entry.

Both launch shapes of each net are reached on 3 small frames: caps 16 (R-Net) / 4 (O-Net) take the several-slots-per-block
launch DIRECTLY, through FR_RC1_BATCH_SHAPE (conv_f16 | 16) - by slot count alone fr_crop_conv1_split takes it from 8192 / 2048
slots on; caps 5 / 3 are not divided by the slots per block and take the one-slot-per-block launch (the tile form under both
settings)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, H, W = 3, 70, 90
BATCH_SHAPE = 16                # FR_RC1_BATCH_SHAPE (include/frhip.h)
FILL = 0x7F
NETS = {0: dict(key=1, cout=28, p=11, caps=(16, 5)), 1: dict(key=2, cout=32, p=23, caps=(4, 3))}

# One list for every case (x1, y1, x2, y2; the kernel truncates, the crop is [x1, x2] x [y1, y2] inclusive).
BOXES = [
    (10.0, 8.0, 21.0, 19.0),                # interior squares of 12, 24, 48, 61 px
    (30.3, 20.7, 53.9, 44.2),
    (20.0, 11.0, 67.0, 58.0),
    (14.5, 4.2, 74.6, 64.9),
    (5.0, 30.0, 60.0, 47.0),                # non-square: wide, tall
    (40.0, 2.0, 52.0, 66.0),
    (-15.5, 20.0, 25.0, 50.0),              # sticking out of the left, top, right, bottom side
    (30.0, -12.0, 58.0, 22.0),
    (70.0, 25.0, 110.0, 60.0),
    (22.0, 50.0, 49.0, 85.0),
    (-9.0, -7.0, 18.0, 21.0),               # ... of the top-left and the bottom-right corner
    (W - 14.0, H - 11.0, W + 12.0, H + 16.0),
    (120.0, 90.0, 150.0, 130.0),            # wholly outside the frame: right / below, left / above
    (-60.0, -50.0, -20.0, -10.0),
    (33.0, 12.0, 33.0, 55.0),               # one pixel wide, one pixel high
    (8.0, 41.0, 70.0, 41.0),
    (50.0, 50.0, 40.0, 60.0),               # empty (x2 < x1)
    (0.0, 0.0, W - 1.0, H - 1.0),           # the whole frame
    (-20.0, -20.0, W + 20.0, H + 20.0),     # larger than the frame on every side
    (W - 30.0, H - 26.0, W - 1.0, H - 1.0),  # ending on the last pixel of the frame
]
LAST_PIXEL_BOX = BOXES[-1]


@pytest.fixture(scope="module")
def env():
    from facerecognition_infrenceengine_amd import _lib, weights
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(41)
    frames = torch.randint(0, 256, (N, H, W, 3), generator=g, device="cuda", dtype=torch.uint8)
    st = weights.synth_mtcnn_states(seed=78)
    packs = {}
    for net, t in NETS.items():
        s = st[t["key"]]
        w = s["conv1.weight"].permute(2, 3, 1, 0).reshape(27, t["cout"])
        packs[net] = tuple(x.to(torch.float32).contiguous().cuda() for x in (w, s["conv1.bias"], s["prelu1.weight"]))
        assert bool((packs[net][2] >= 0).all()), "the synthetic slopes are expected to take the pool-then-activate path"
    return _lib, lib, frames, packs


def _boxes(cap, rot):
    """Slot 0 of the LAST frame always holds the box that ends on the frame's last pixel (the one valid slot of the counts = 1
    case: the 8-byte loads there are pulled back); the other N * cap - 1 slots hold boxes rot, rot + 1, ... of the list, cyclically."""
    idx = (torch.arange(N * cap - 1) + rot) % len(BOXES)
    b = torch.tensor(BOXES, dtype=torch.float32)[idx]
    b = torch.cat([b[:(N - 1) * cap], torch.tensor([LAST_PIXEL_BOX]), b[(N - 1) * cap:]]).reshape(N, cap, 4)
    return b.cuda().contiguous()


def _run(env, net, form, boxes, counts, cap, pack):
    _lib, lib, frames, _ = env
    p = NETS[net]["p"]
    out = torch.full((N * cap, p * p, 128), FILL, dtype=torch.uint8, device="cuda")
    w, b, s = pack
    rc = lib.fr_crop_conv1_split(net, _lib.ptr(frames), N, H, W, _lib.ptr(boxes), _lib.ptr(counts), cap, _lib.ptr(w), _lib.ptr(b),
                                 _lib.ptr(s), _lib.ptr(out), form, _lib.stream_ptr())
    assert rc == 0, (net, form, cap)
    torch.cuda.synchronize()
    return out


def _counts_cases(cap):
    return [("full", [cap, cap, cap]), ("partial, 0, 1", [max(cap - 3, 1), 0, 1]), ("1, partial, full", [1, cap - 1, cap])]


def _cases():
    for net, t in NETS.items():
        for cap in t["caps"]:
            for negate in (False, True):
                yield pytest.param(net, cap, negate, id=f"{'ro'[net]}net-cap{cap}-{'negated' if negate else 'own'}-slopes")


@pytest.mark.parametrize("net,cap,negate", list(_cases()))
def test_strip_form_equals_tile_form(env, net, cap, negate):
    """conv_f16 = 1 against conv_f16 = 2, byte for byte on every valid slot; slots >= counts[frame] keep the fill pattern in both.
    Every box of the list lands in a valid slot of the full-count case (the list is rotated through the slots until it has)."""
    w, b, s = env[3][net]
    if negate:                                      # two slopes negative: every pixel is activated before the pool
        s = s.clone()
        s[1] = -s[1]
        s[s.numel() - 2] = -s[s.numel() - 2]
    shape = BATCH_SHAPE if cap % 4 == 0 else 0     # caps 16 / 4: the several-slots-per-block launch; 5 / 3: one slot per block
    for name, cnt in _counts_cases(cap):
        counts = torch.tensor(cnt, dtype=torch.int32, device="cuda")
        valid = (torch.arange(cap, device="cuda")[None, :] < counts[:, None]).reshape(-1)
        rots = range(0, len(BOXES), N * cap - 1) if name == "full" else (0,)
        for rot in rots:
            boxes = _boxes(cap, rot)
            strip = _run(env, net, 1 | shape, boxes, counts, cap, (w, b, s))
            tile = _run(env, net, 2 | shape, boxes, counts, cap, (w, b, s))
            where = (net, cap, name, rot)
            assert bool((strip[~valid] == FILL).all()) and bool((tile[~valid] == FILL).all()), where
            # every valid slot was written by the reference form (an f16 of bytes 7f 7f never fills a whole map: the K padding
            # of the R-Net and the lo halves are not that pattern)
            assert bool((tile[valid] != FILL).flatten(1).any(1).all()), where
            bad = (strip[valid] != tile[valid]).flatten(1).any(1)
            assert not bool(bad.any()), (where, "valid slots that differ:", torch.nonzero(bad).flatten().tolist()[:8])
            assert torch.equal(strip, tile), where


@pytest.mark.parametrize("net", [0, 1])
def test_zero_weights_give_prelu_of_bias_exactly(env, net):
    """All-zero weights, a non-zero bias of both signs: every pixel of every valid slot is PReLU(bias) exactly (both launch
    shapes, both forms) - the pool, the epilogue and the hi / lo stores with the conv taken out."""
    t = NETS[net]
    cout, p = t["cout"], t["p"]
    w = torch.zeros((27, cout), dtype=torch.float32, device="cuda")
    g = torch.Generator().manual_seed(5)
    b = ((torch.rand(cout, generator=g) + 0.25) * torch.where(torch.arange(cout) % 3 == 0, -1.0, 1.0)).cuda()
    s = (torch.rand(cout, generator=g) * 0.5 + 0.1).cuda()
    v = torch.where(b > 0, b, b * s)
    hi = v.half()
    lo = (v - hi.float()).half()
    want = torch.zeros((2, 32), dtype=torch.float16, device="cuda")
    want[0, :cout], want[1, :cout] = hi, lo
    for cap in t["caps"]:
        shape = BATCH_SHAPE if cap % 4 == 0 else 0
        counts = torch.tensor([cap, max(cap - 3, 1), 1], dtype=torch.int32, device="cuda")
        valid = (torch.arange(cap, device="cuda")[None, :] < counts[:, None]).reshape(-1)
        boxes = _boxes(cap, 0)
        for form in (1, 2):
            out = _run(env, net, form | shape, boxes, counts, cap, (w, b, s))
            got = out.view(torch.float16).reshape(N * cap, p * p, 2, 32)[valid]
            assert torch.equal(got.view(torch.int16), want.view(torch.int16).expand_as(got)), (net, cap, form)
            assert bool((out[~valid] == FILL).all()), (net, cap, form)
