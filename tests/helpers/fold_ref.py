"""Float64 references for the ASSEMBLY of the embed net: what the host does between a state dict and the conv kernels
(iresnet.fold_iresnet, _pack_w, _pack_stage, the fused-shortcut weights, embed_route / _issue), shared by
tests/test_fold_ref_host.py (CPU) and tests/test_gpu_embed_assembly.py (GPU).  The single conv, its layouts and `conv_bound`
are embed_ref's; a block as the stage kernels run it is stage_ref's.

Three layers, each tied to the one before it:
  * unfolded_blocks: the IResNet as its definition states it (explicit batch_norm, zero padding AFTER bn1, PReLU, stride-2
    downsample; bn2 -> NCHW flatten -> fc -> features), float64, with every block's input, `mid`, shortcut and output kept.
    Its embedding equals oracle.nets.iresnet_forward on the same float64 state (asserted by the host test).
  * folded_step: ONE conv of fold_iresnet's output dict in float64, fed the unfolded net's own tensors (teacher forcing: a
    fold error shows at the step it was made and nowhere else).  Compared per element within HOST_C (K + 2) 2^-53 mag.
  * engine_operands / step_ref / block_ref: what the device must hold (f16 weights [Cout][kh][kw][cin], f32 biases and
    slopes, the [2 n][10][width] rows of a stage run), derived from the fold dict and the documented layouts only, and one
    step of a real forward from them in float64 with the kernels' rounding bound.

The host bound.  Both sides compute the same real number in float64; `mag` is that number's sum with every term replaced by
its absolute value, taken on the UNFOLDED side, BN terms split ((|x| + |mean|) |s| + |beta|), so that it bounds the running
magnitude of either side whatever cancels.  Roundings along any path from the inputs to an output (u = 2^-53, first order):
  unfolded  bn1 of the input: x - mean, var + eps, sqrt, divide, * gamma, + beta = 6; the product 1 (inside the K of the sum);
            the sum over K products K; the BN after the conv 6; PReLU 1; the residual add 1                     <= K + 14
  folded    a weight: each scale s = gamma / sqrt(var + eps) 3, two scale products 2 = 8; the sum K; the bias add 1; PReLU 1;
            the residual add 1 = K + 11 on the product path.  The bias path: t = beta - mean s is 5, w t 1, the sum over
            cin inputs cin, * s2 (3 + 1), the sum over up to 9 taps 9, + t2 (5 + 1), then the add, PReLU, residual 3:
            cin + 33 <= K + 18 (3x3: cin + 9 <= K for cin >= 2; the 1x1 shortcut, the stem and the FC have no tap sums
            and the FC's bias sums over K terms: K + 18 again)                                                   <= K + 18
Together 2 K + 32 <= 3 (K + 2) for every K >= 26 (the smallest K here is the stem's 27): HOST_C = 3."""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from tests.helpers import embed_ref as er
from tests.helpers import stage_ref as sr

BN_EPS = 1e-5
U64 = 2.0 ** -53
HOST_C = 3
LAYERS = {"r18": [2, 2, 2, 2], "r34": [3, 4, 6, 3], "r50": [3, 4, 14, 3], "r100": [3, 13, 30, 3]}
WIDTHS = [64, 128, 256, 512]
FC_SLICES = 28
INBLOCK_SPLIT = 16        # conv_inblock.hip: K step ks goes to wave ks % 16, the sixteen partials are summed in wave order


def state64(state):
    return {k: torch.as_tensor(v).detach().cpu().double() for k, v in state.items()}


# ---------------------------------------------------------------- the unfolded net
def _bn(x, st, p):
    return F.batch_norm(x, st[p + ".running_mean"], st[p + ".running_var"], st[p + ".weight"], st[p + ".bias"], training=False,
                        eps=BN_EPS)


def _bn_mag(a, st, p):
    """The BN's terms by absolute value: (a + |mean|) |gamma / sqrt(var + eps)| + |beta|, a >= 0 the input's magnitude."""
    shape = (1, -1) + (1,) * (a.dim() - 2)
    s = (st[p + ".weight"] / torch.sqrt(st[p + ".running_var"] + BN_EPS)).abs().reshape(shape)
    return (a + st[p + ".running_mean"].abs().reshape(shape)) * s + st[p + ".bias"].abs().reshape(shape)


def _pad(x):
    return F.pad(x, (1, 1, 1, 1))                      # zeros, AFTER the BN that precedes the conv


def _slope_mag(st, key):
    return st[key].abs().clamp_min(1.0).reshape(1, -1, 1, 1)


def unfolded_block(st, p, x, stride):
    """One block at any map size -> its tensors (NCHW float64) and their magnitudes (module docstring)."""
    w1, w2 = st[p + ".conv1.weight"], st[p + ".conv2.weight"]
    r = SimpleNamespace(x=x, stride=stride, cin=w1.shape[1], cout=w1.shape[0], H=x.shape[2], k=w1.shape[2], sc=None, mag_sc=None)
    r.mid = F.prelu(_bn(F.conv2d(_pad(_bn(x, st, p + ".bn1")), w1), st, p + ".bn2"), st[p + ".prelu.weight"])
    r.mag_mid = _bn_mag(F.conv2d(_pad(_bn_mag(x.abs(), st, p + ".bn1")), w1.abs()), st, p + ".bn2") * _slope_mag(st, p + ".prelu.weight")
    o = _bn(F.conv2d(_pad(r.mid), w2, stride=stride), st, p + ".bn3")
    mo = _bn_mag(F.conv2d(_pad(r.mid.abs()), w2.abs(), stride=stride), st, p + ".bn3")
    if p + ".downsample.0.weight" in st:
        wd = st[p + ".downsample.0.weight"]
        r.sc = _bn(F.conv2d(x, wd, stride=stride), st, p + ".downsample.1")
        r.mag_sc = _bn_mag(F.conv2d(x.abs(), wd.abs(), stride=stride), st, p + ".downsample.1")
    res = x if r.sc is None else r.sc
    r.out, r.mag_out = o + res, mo + res.abs()
    return r


@torch.no_grad()
def unfolded_blocks(state, arch, x):
    """x [B][3][112][112] -> .x, .stem / .mag_stem, .blocks (unfolded_block: x, mid, sc, out and their mags, cin, cout,
    stride, H), .emb / .mag_emb.  Everything float64 NCHW."""
    st = state64(state)
    x = torch.as_tensor(x).double()
    net = SimpleNamespace(x=x, blocks=[])
    w = st["conv1.weight"]
    net.stem = F.prelu(_bn(F.conv2d(_pad(x), w), st, "bn1"), st["prelu.weight"])
    net.mag_stem = _bn_mag(F.conv2d(_pad(x.abs()), w.abs()), st, "bn1") * _slope_mag(st, "prelu.weight")
    h = net.stem
    for li, n in enumerate(LAYERS[arch], start=1):
        for bi in range(n):
            net.blocks.append(unfolded_block(st, f"layer{li}.{bi}", h, 2 if bi == 0 else 1))
            h = net.blocks[-1].out
    net.emb = _bn(F.linear(torch.flatten(_bn(h, st, "bn2"), 1), st["fc.weight"], st["fc.bias"]), st, "features")
    net.mag_emb = _bn_mag(F.linear(torch.flatten(_bn_mag(h.abs(), st, "bn2"), 1), st["fc.weight"].abs(), st["fc.bias"].abs()),
                          st, "features")
    return net


def net_steps(net):
    """[(key, inputs of folded_step, the unfolded tensor it must give, mag, K)] in network order."""
    steps = [("stem", (net.x,), net.stem, net.mag_stem, 27)]
    for i, b in enumerate(net.blocks):
        steps.append(((i, "c1"), (b.x,), b.mid, b.mag_mid, 9 * b.cin))
        if b.sc is not None:
            steps.append(((i, "sc"), (b.x,), b.sc, b.mag_sc, b.cin))
        steps.append(((i, "c2"), (b.mid, b.x if b.sc is None else b.sc), b.out, b.mag_out, 9 * b.cout))
    steps.append(("fc", (net.blocks[-1].out,), net.emb, net.mag_emb, 512 * 49))
    return steps


def host_bound(K, mag):
    return HOST_C * (K + 2) * U64 * mag


# ---------------------------------------------------------------- one conv of the fold dict
def fold_conv(fold, key):
    if key == "stem":
        return fold["stem"]
    return fold["blocks"][key[0]][key[1]]


def class_bias(b9, Ho, Wo):
    """[9 Cout] border-class bias (top / inner / bottom x left / inner / right) over an Ho x Wo map -> [1][Cout][Ho][Wo]"""
    b9 = b9.reshape(3, 3, -1)
    rc, cc = torch.from_numpy(er.border_class(Ho)), torch.from_numpy(er.border_class(Wo))
    return b9[rc][:, cc].permute(2, 0, 1)[None]


@torch.no_grad()
def folded_step(fold, key, inputs):
    """One conv of fold_iresnet's dict in float64 (NCHW): "stem" (from the PACKED [64][16 taps][8] weights), (i, "c1") with the
    border-class bias expanded over the map, (i, "c2") with its residual (inputs = (mid, residual)), (i, "sc"), and "fc", the
    tail GEMM over the last map in NHWC K order."""
    x = inputs[0]
    if key == "fc":
        return x.permute(0, 2, 3, 1).reshape(x.shape[0], -1) @ fold["fc_w"].T + fold["fc_bias"]
    c = fold_conv(fold, key)
    slope = None if c["slope"] is None else torch.as_tensor(c["slope"]).double()
    if key == "stem":
        w = c["w"].reshape(64, 16, 8)[:, :9, :3].reshape(64, 3, 3, 3).permute(0, 3, 1, 2)
        return F.prelu(F.conv2d(x, w, c["bias"], padding=1), slope)
    if key[1] == "c1":
        y = F.conv2d(x, c["w"], padding=1)
        return F.prelu(y + class_bias(c["bias"], y.shape[2], y.shape[3]), slope)
    if key[1] == "sc":
        return F.conv2d(x, c["w"], c["bias"], stride=c["stride"])
    return F.conv2d(x, c["w"], c["bias"], stride=c["stride"], padding=1) + inputs[1]


def folded_forward(fold, x):
    """The folded net running FREE (every step on the step before it) -> the embedding: what the 1 - cos tests see."""
    h = folded_step(fold, "stem", (torch.as_tensor(x).double(),))
    for i, b in enumerate(fold["blocks"]):
        mid = folded_step(fold, (i, "c1"), (h,))
        res = h if b["sc"] is None else folded_step(fold, (i, "sc"), (h,))
        h = folded_step(fold, (i, "c2"), (mid, res))
    return folded_step(fold, "fc", (h,))


def one_minus_cos(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 1.0 - (a * b).sum(1) / np.sqrt((a * a).sum(1) * (b * b).sum(1))


def ratio(got, want, bound):
    return er.worst_ratio(np.abs(_np64(got) - _np64(want)), _np64(bound))


def copy_fold(fold):
    """A copy whose conv dicts and tensors may be changed without touching `fold`."""
    cp = lambda c: None if c is None else {k: (v.clone() if torch.is_tensor(v) else v) for k, v in c.items()}
    return {"stem": cp(fold["stem"]), "blocks": [{k: cp(v) for k, v in b.items()} for b in fold["blocks"]],
            "fc_w": fold["fc_w"].clone(), "fc_bias": fold["fc_bias"].clone()}


# ---------------------------------------------------------------- what the device must hold
def _rows16(w4):
    """f64 [Cout][Cin][kh][kw] -> f16 rows [Cout][kh][kw][cin]"""
    a = np.transpose(np.asarray(w4, np.float64), (0, 2, 3, 1))
    return torch.from_numpy(np.ascontiguousarray(a.reshape(a.shape[0], -1))).to(torch.float16)


def _f32(v):
    return None if v is None else torch.as_tensor(v).detach().cpu().to(torch.float32).contiguous()


def engine_operands(fold, key):
    """The operands of conv `key` as the device must hold them, from the fold dict and the documented layouts alone: .w f16
    [Cout][K], K = [kh][kw][cin] (stem: [16 taps][8]; (i, "fz"): c2's K, then the 1x1 shortcut's Cin; "fc": NHWC order), .bias /
    .slope f32 or None ("fz": the f32 sum of the two f32 biases; "fc": fc_bias), and the geometry .k .stride .pad .bias_mode
    .cin .c2."""
    if key == "fc":
        return SimpleNamespace(w=fold["fc_w"].to(torch.float16).contiguous(), bias=_f32(fold["fc_bias"]), slope=None, k=1, stride=1,
                               pad=0, bias_mode=0, cin=fold["fc_w"].shape[1], c2=0)
    if key == "stem":
        c = fold["stem"]
        return SimpleNamespace(w=c["w"].to(torch.float16).contiguous(), bias=_f32(c["bias"]), slope=_f32(c["slope"]), k=3, stride=1,
                               pad=1, bias_mode=0, cin=8, c2=0)
    i, kind = key
    b = fold["blocks"][i]
    if kind == "fz":
        c2, sc = engine_operands(fold, (i, "c2")), engine_operands(fold, (i, "sc"))
        return SimpleNamespace(w=torch.cat([c2.w, sc.w], 1).contiguous(), bias=c2.bias + sc.bias, slope=None, k=3, stride=c2.stride,
                               pad=1, bias_mode=0, cin=c2.cin, c2=sc.cin)
    c = b[kind]
    k = c["w"].shape[2]
    return SimpleNamespace(w=_rows16(c["w"]), bias=_f32(c["bias"]), slope=_f32(c["slope"]), k=k, stride=c["stride"], pad=k // 2,
                           bias_mode=int(kind == "c1"), cin=c["cin"], c2=0)


def stage_params(fold, first, n):
    """The parameter rows of a stage run, f32 [2 n][10][width]: per conv nine border-class biases (a plain bias nine times),
    then the slope, 1.0 where the conv has none."""
    rows = []
    for i in range(first, first + n):
        for kind in ("c1", "c2"):
            o = engine_operands(fold, (i, kind))
            width = o.w.shape[0]
            bias = o.bias.reshape(9, width) if o.bias_mode == 1 else o.bias.reshape(1, width).repeat(9, 1)
            slope = o.slope if o.slope is not None else torch.ones(width, dtype=torch.float32)
            rows.append(torch.cat([bias, slope.reshape(1, width)], 0))
    return torch.stack(rows).contiguous()


# ---------------------------------------------------------------- one step of a real forward
def _np64(t):
    return None if t is None else (t.detach().cpu().double().numpy() if torch.is_tensor(t) else np.asarray(t, np.float64))


def route_slices(route, slices):
    """`slices` of step_ref's bound: the route's slice count for split-K, the in-workgroup split for the in-block kernel, else 1."""
    return {"splitk": slices, "inblock": INBLOCK_SPLIT}.get(route, 1)


def step_ref(key, ops, inputs, slices=1):
    """(want, mag, bound), float64 NHWC, of conv `key` on `inputs` = (x, residual or None, x2 or None) as the kernels see them
    (f16 maps).  f16 output: (K + 2 + slices) 2^-24 mag + 2^-11 |want| + 2^-25, K the columns of a weight row - K products
    summed in f32 in any order, bias, PReLU, residual, and one more add per slice that is summed on top.  "fc" (inputs = (h,)) ->
    the embedding, f32: its 28 slices of 14 K steps each within (K_slice + 2) 2^-24 mag_slice, summed, plus
    er.fc_tail_bound over |bias| + sum mag_slice."""
    x = _np64(inputs[0])
    w = _np64(ops.w)
    if key == "fc":
        x = x.reshape(x.shape[0], -1)
        assert x.shape[1] == w.shape[1] and (w.shape[1] // er.BK) % FC_SLICES == 0
        per = w.shape[1] // FC_SLICES
        want = np.zeros((x.shape[0], w.shape[0]))
        mag, bound = np.zeros_like(want), np.zeros_like(want)
        for z in range(FC_SLICES):
            xs, ws = x[:, z * per:(z + 1) * per], w[:, z * per:(z + 1) * per]
            m = np.abs(xs) @ np.abs(ws).T
            want += xs @ ws.T
            mag += m
            bound += er.conv_bound(per, m)
        bias = _np64(ops.bias)[None]
        want, mag = want + bias, mag + np.abs(bias)
        return want, mag, bound + er.fc_tail_bound(FC_SLICES, mag)
    residual, x2 = _np64(inputs[1]), _np64(inputs[2])
    K = w.shape[1]
    if key == "stem":
        w = w.reshape(-1, 16, 8)[:, :9].reshape(-1, 72)
    assert (x2 is None) == (ops.c2 == 0)
    want, mag = er.conv_ref(x, w, _np64(ops.bias), ops.bias_mode, _np64(ops.slope), residual, ops.stride, ops.pad, x2=x2, k=ops.k)
    return want, mag, (K + 2 + slices) * er.U32 * mag + er.U16 * np.abs(want) + 2.0 ** -25


def block_ref(x, w1, w2, prm):
    """One stride-1 block as the stage kernels run it (stage_ref.stage_run_ref with one block): x [B][HW][HW][C] f16 values, w1 /
    w2 [C][9 C] f16 values, prm [2][10][C] -> (want_mid, bound_mid, want, bound): the float64 values before the rounding and the
    bounds of the f16 maps `mid` and `out` against them.

    The bound on `out`.  Let v1 be conv1's unrounded float64 value and b1 = (K + 2) 2^-24 mag1 its f32 bound: the kernel's
    unrounded value lies in [v1 - b1, v1 + b1], and rounding to f16 is monotone, so the kernel's `mid` lies in
    [f16(v1 - b1), f16(v1 + b1)] - as does the reference's f16(v1).  dmid = f16(v1 + b1) - f16(v1 - b1) is therefore 0
    wherever conv1's bound cannot carry the value over a rounding boundary, and one f16 ulp of `mid` (the distance between the
    two candidates) where it can.  conv2 is linear in `mid`: on the kernel's `mid` its exact value differs from the reference's
    by at most extra = conv(|dmid|, |w2|), its magnitude is at most mag2 + extra, and its own roundings are conv2's bound on
    those: bound = (K + 2) 2^-24 (mag2 + extra) + extra + 2^-11 (|want| + extra) + 2^-25."""
    x, w1, w2, prm = _np64(x), _np64(w1), _np64(w2), _np64(prm)
    K = w1.shape[1]
    r = sr.stage_run_ref(x, [w1, w2], prm)
    v1, m1 = r.raw[0], r.mag[0]
    b1 = er.conv_bound(K, m1)
    dmid = sr.f16(v1 + b1) - sr.f16(v1 - b1)
    assert (dmid >= 0).all()
    w4 = torch.from_numpy(np.ascontiguousarray(np.abs(w2).reshape(-1, 3, 3, x.shape[3]))).permute(0, 3, 1, 2)
    extra = F.conv2d(er._nchw(dmid), w4, None, 1, 1).permute(0, 2, 3, 1).numpy()
    v2, m2 = r.raw[1], r.mag[1]
    bound = er.conv_bound(K, m2 + extra) + extra + er.U16 * (np.abs(v2) + extra) + 2.0 ** -25
    return v1, er.conv_bound(K, m1, v1), v2, bound


# ---------------------------------------------------------------- planted fold errors (the instrument must notice them)
def bias9(c):
    return c["bias"].reshape(3, 3, -1)


def plant_swap_top_bottom(fold, i):
    c = fold["blocks"][i]["c1"]
    c["bias"] = bias9(c).flip(0).reshape(-1).clone()
    return [(i, "c1")]


def plant_corner_is_edge(fold, blocks=None, corners=((0, 0), (0, 2), (2, 0), (2, 2))):
    """the corner classes take the class of the edge beside them (their row's inner-column class)"""
    hit = []
    for i in (range(len(fold["blocks"])) if blocks is None else blocks):
        b9 = bias9(fold["blocks"][i]["c1"]).clone()
        for rc, cc in corners:
            b9[rc, cc] = b9[rc, 1]
        fold["blocks"][i]["c1"]["bias"] = b9.reshape(-1)
        hit.append((i, "c1"))
    return hit


def plant_plain_bias(fold):
    """no border classes at all: the inner class everywhere"""
    for b in fold["blocks"]:
        b["c1"]["bias"] = bias9(b["c1"])[1, 1].expand(3, 3, -1).reshape(-1).clone()
    return [(i, "c1") for i in range(len(fold["blocks"]))]


def plant_neighbour_slope(fold, i):
    fold["blocks"][i]["c1"]["slope"] = fold["blocks"][i + 1]["c1"]["slope"].clone()
    return [(i, "c1")]


def plant_eps_twice(fold, state, i, prefix):
    """bn3 of block i (`prefix` its name in the state dict) with eps under the root twice"""
    st = state64(state)
    var, mean, gamma, beta = (st[prefix + ".bn3." + n] for n in ("running_var", "running_mean", "weight", "bias"))
    s, s2 = gamma / torch.sqrt(var + BN_EPS), gamma / torch.sqrt(var + 2 * BN_EPS)
    c = fold["blocks"][i]["c2"]
    c["w"] = c["w"] / s[:, None, None, None] * s2[:, None, None, None]
    c["bias"] = beta - mean * s2
    return [(i, "c2")]


def plant_fc_nchw(fold):
    """the FC's columns left in NCHW order"""
    fold["fc_w"] = fold["fc_w"].reshape(512, 49, 512).permute(0, 2, 1).reshape(512, -1).contiguous()
    return ["fc"]


def block_prefix(arch, i):
    for li, n in enumerate(LAYERS[arch], start=1):
        if i < n:
            return f"layer{li}.{i}"
        i -= n
    raise IndexError(i)


# ---------------------------------------------------------------- a real forward, step by step
# The GPU cases: (arch, faces, fuse_shortcut, tapped).  r100: 3 faces launch by launch (a tapped forward replays no plan) reach
# the in-block kernel and the low-batch split-K; 12 the split-K of up to 48; 50 the halo kernels, walk64 with cut walks and the
# fused shortcut on the stride-2 kernel; 50 unfused the shortcut and c2 apart; 128 the 14x14 run as one launch with the 28x28
# stage layer by layer; 160 both runs and walk64 uncut; r50 at 150 the run lengths 13 and 3.
FORWARD_CASES = [("r100", 3, True, True), ("r100", 12, True, False), ("r100", 50, True, False), ("r100", 50, False, False),
                 ("r100", 128, True, False), ("r100", 160, True, False), ("r50", 150, True, False)]
RUN_ROUTES = ("stage28", "stage14")


def picked_faces(B):
    return [0, B // 2, B - 1]


def step_id(s):
    return (s.route, s.slices, s.conv)


def covered(route):
    """{(route, slices, conv key)} a forward over `route` checks: a run stands for the c1 and c2 of each of its blocks."""
    out = set()
    for s in route:
        if s.route in RUN_ROUTES:
            out |= {(s.route, 1, (i, kind)) for i in range(s.conv[0], s.conv[0] + s.conv[1]) for kind in ("c1", "c2")}
        else:
            out.add(step_id(s))
    return out


def check_forward(fold, table, route, x, rec, emb, normed, run_check=None):
    """Every step of a recorded forward against float64.  rec: {conv key of the step: its output rows for the picked faces},
    x / emb / normed: the same faces' rows of the input and of the results.  A step's reference takes its inputs from the
    RECORDED outputs that the network's graph names - stem <- x; (i, c1), (i, sc) <- block i - 1's output; (i, c2) <- mid_i with the
    residual sc_i or block i - 1's output; (i, fz) <- mid_i with block i - 1's output as second input; a run <- the output of the
    block before it; fc <- the last block's output - never from what the engine passed, so a wrong source buffer, residual or
    alias is a miss.  A run is handed to run_check(step, recorded input, recorded output).
    -> {(route, slices, key): worst err / bound} with "emb" and "normed" under the fc's route."""
    ratios, h = {}, {}
    last = table.nblocks - 1
    for s in route:
        key = s.conv
        if s.route in RUN_ROUTES:
            first, n = key
            run_check(s, h[first - 1], rec[key])
            h[first + n - 1] = rec[key]
            ratios[step_id(s)] = 0.0
            continue
        if key == "stem":
            inputs = (x, None, None)
        elif key == "fc":
            inputs = (h[last],)
        else:
            i, kind = key
            entry = (i, "sc") in table.convs
            if kind in ("c1", "sc"):
                inputs = (h[i - 1], None, None)
            elif kind == "c2":
                inputs = (rec[i, "c1"], rec[i, "sc"] if entry else h[i - 1], None)
            else:
                assert kind == "fz" and entry
                inputs = (rec[i, "c1"], None, h[i - 1])
        want, mag, bound = step_ref(key, engine_operands(fold, key), inputs, route_slices(s.route, s.slices))
        if key == "fc":
            got = _np64(emb)
            ratios[s.route, s.slices, "normed"] = ratio(normed, er.normed_ref(got), er.normed_bound(got.shape[1], er.normed_ref(got)))
        else:
            got = _np64(rec[key])
        assert got.shape == want.shape, (key, got.shape, want.shape)
        ratios[step_id(s)] = ratio(got, want, bound)
        if key == "stem":
            h[-1] = rec[key]
        elif key != "fc" and key[1] in ("c2", "fz"):
            h[key[0]] = rec[key]
    return ratios


# ---------------------------------------------------------------- a float32 stand-in for the conv kernels
def standin_step(key, ops, inputs):
    """Step `key` in torch CPU float32 on f16 operands (f32 products and sums, bias, PReLU, residual; f16 store) -> the f16 map
    as float64, NHWC; "fc" -> the f32 embedding."""
    x = torch.from_numpy(np.ascontiguousarray(_np64(inputs[0]))).to(torch.float16).float()
    if key == "fc":
        return (x.reshape(x.shape[0], -1) @ ops.w.float().T + ops.bias).double().numpy()
    w = ops.w.float()
    if key == "stem":
        w = w.reshape(-1, 16, 8)[:, :9].reshape(-1, 72)
    kmain = ops.k * ops.k * ops.cin
    w4 = w[:, :kmain].reshape(-1, ops.k, ops.k, ops.cin).permute(0, 3, 1, 2)
    y = F.conv2d(x.permute(0, 3, 1, 2), w4, None, ops.stride, ops.pad)
    if inputs[2] is not None:
        x2 = torch.from_numpy(np.ascontiguousarray(_np64(inputs[2]))).to(torch.float16).float().permute(0, 3, 1, 2)
        y = y + F.conv2d(x2, w[:, kmain:, None, None], None, ops.stride)[:, :, :y.shape[2], :y.shape[3]]
    y = y + (class_bias(ops.bias, y.shape[2], y.shape[3]) if ops.bias_mode == 1 else ops.bias.reshape(1, -1, 1, 1))
    if ops.slope is not None:
        y = F.prelu(y, ops.slope)
    y = y.permute(0, 2, 3, 1)
    if inputs[1] is not None:
        y = y + torch.from_numpy(np.ascontiguousarray(_np64(inputs[1]))).to(torch.float16).float()
    return y.to(torch.float16).double().numpy()


def standin_forward(fold, table, route, x, fault=None):
    """A forward over `route` (no runs) on the stand-in, the way IResNetHIP._forward_chunk walks it - by the steps' src / dst /
    res names - -> (rec, emb, normed).  Faults: "residual": the c2 of a stride-1 block adds `mid` instead of the block's input;
    "source": a c1 from block 2 on reads the output of block i - 2 instead of block i - 1's (where the shapes agree)."""
    t, rec, older = {"x": x}, {}, {}
    for s in route[:-1]:
        key = s.conv
        ops = engine_operands(fold, key)
        src, res = t[s.src], t.get(s.res)
        if fault == "residual" and key[1:] == ("c2",) and s.res == "h":
            res = t["mid"]
        if fault == "source" and key[1:] == ("c1",) and key[0] >= 2 and older.get(key[0] - 2) is not None \
                and older[key[0] - 2].shape == src.shape:
            src = older[key[0] - 2]
        t[s.dst] = rec[key] = standin_step(key, ops, (src, res, t["h"] if s.x2 else None))
        if s.dst == "h" and key != "stem":
            older[key[0]] = t["h"]
    emb = standin_step("fc", engine_operands(fold, "fc"), (t["h"],))
    e32 = emb.astype(np.float32)
    normed = (e32 / np.sqrt((e32 * e32).sum(1, keepdims=True, dtype=np.float32))).astype(np.float64)
    return rec, emb, normed


