"""Test helper: the three network families the engine imports, as plain nn.Modules written from their published
architectures (ArcFace IResNet, MobileFaceNet, SCRFD) - the input of tests/helpers/torch_export.py.  Nothing here reads
weights.py, onnx_import.py or the protobuf writers of the other helpers."""
import torch
import torch.nn as nn
import torch.nn.functional as F

IRESNET_BLOCKS = {"r18": (2, 2, 2, 2), "r34": (3, 4, 6, 3), "r50": (3, 4, 14, 3), "r100": (3, 13, 30, 3)}


# ------------------------------------------------------------------------------------------------ ArcFace IResNet
class IBasicBlock(nn.Module):
    def __init__(self, inplanes, planes, stride=1, downsample=None, eps=1e-5):
        super().__init__()
        self.bn1 = nn.BatchNorm2d(inplanes, eps=eps)
        self.conv1 = nn.Conv2d(inplanes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes, eps=eps)
        self.prelu = nn.PReLU(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes, eps=eps)
        self.downsample = downsample

    def forward(self, x):
        identity = x
        out = self.bn1(x)
        out = self.conv1(out)
        out = self.bn2(out)
        out = self.prelu(out)
        out = self.conv2(out)
        out = self.bn3(out)
        if self.downsample is not None:
            identity = self.downsample(x)
        return out + identity


def _fully_connected(fc, x, head):
    if head == "linear":
        return fc(x)
    if head == "matmul":
        return torch.matmul(x, fc.weight.t()) + fc.bias
    if head == "addmm":
        return torch.addmm(fc.bias, x, fc.weight.t())
    return torch.addmm(fc.bias, x, fc.weight_t)


def use_transposed_head(module):
    """head 'addmm_t': the weight of ``module.fc`` stored transposed, [in, out], as frameworks other than torch keep it - the
    export is a Gemm with transB = 0.  The copy is a non-persistent buffer (state_dict() does not list it), made here and not
    in forward(), where the tracer would record the transposition; seed the module first."""
    module.fc.register_buffer("weight_t", module.fc.weight.detach().t().contiguous(), persistent=False)
    module.head = "addmm_t"
    return module


class IResNet(nn.Module):
    """``flatten``: 'flatten' (torch.flatten(x, 1)) or 'view' (x.view(x.size(0), -1)); ``head``: 'linear', 'matmul'
    (torch.matmul(x, W.t()) + b), 'addmm' (torch.addmm(b, x, W.t())) or 'addmm_t' (torch.addmm(b, x, Wt), Wt a stored
    transposed copy: use_transposed_head), all on the parameters of ``fc``; ``features``: the
    embedding width (512 in every published net).  ``flatten`` and ``head`` may be changed on a built module."""

    def __init__(self, blocks=(2, 2, 2, 2), flatten="flatten", head="linear", features=512, eps=1e-5, dropout=0.0):
        super().__init__()
        self.flatten, self.head, self.eps = flatten, head, eps
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, 3, 1, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(64, eps=eps)
        self.prelu = nn.PReLU(64)
        self.layer1 = self._make_layer(64, blocks[0])
        self.layer2 = self._make_layer(128, blocks[1])
        self.layer3 = self._make_layer(256, blocks[2])
        self.layer4 = self._make_layer(512, blocks[3])
        self.bn2 = nn.BatchNorm2d(512, eps=eps)
        self.dropout = nn.Dropout(p=dropout, inplace=True)
        self.fc = nn.Linear(512 * 7 * 7, features)
        self.features = nn.BatchNorm1d(features, eps=eps)

    def _make_layer(self, planes, n):
        down = nn.Sequential(nn.Conv2d(self.inplanes, planes, 1, 2, bias=False), nn.BatchNorm2d(planes, eps=self.eps))
        layers = [IBasicBlock(self.inplanes, planes, 2, down, self.eps)]
        self.inplanes = planes
        layers += [IBasicBlock(planes, planes, eps=self.eps) for _ in range(1, n)]
        return nn.Sequential(*layers)

    def forward(self, x):
        x = self.prelu(self.bn1(self.conv1(x)))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        x = self.dropout(self.bn2(x))
        x = torch.flatten(x, 1) if self.flatten == "flatten" else x.view(x.size(0), -1)
        return self.features(_fully_connected(self.fc, x, self.head))


# ------------------------------------------------------------------------------------------------ MobileFaceNet
class ConvBlock(nn.Sequential):
    def __init__(self, cin, cout, k=1, stride=1, pad=0, groups=1):
        super().__init__(nn.Conv2d(cin, cout, k, stride, pad, groups=groups, bias=False), nn.BatchNorm2d(cout), nn.PReLU(cout))


class LinearBlock(nn.Sequential):
    def __init__(self, cin, cout, k=1, stride=1, pad=0, groups=1):
        super().__init__(nn.Conv2d(cin, cout, k, stride, pad, groups=groups, bias=False), nn.BatchNorm2d(cout))


class DepthWise(nn.Module):
    """1x1 expand + PReLU, depthwise 3x3 + PReLU, 1x1 linear project; with ``residual`` the input is added"""

    def __init__(self, cin, cout, expand, stride=1, residual=False, dw_groups=None):
        super().__init__()
        self.residual = residual
        self.layers = nn.Sequential(ConvBlock(cin, expand), ConvBlock(expand, expand, 3, stride, 1, groups=dw_groups or expand),
                                    LinearBlock(expand, cout))

    def forward(self, x):
        return x + self.layers(x) if self.residual else self.layers(x)


MBF_TINY = dict(stem=16, stages=((24, 16, 1, 24), (40, 24, 2, 40), (48, 24, 1, 48)), tail=512)
MBF_WIDE = dict(stem=64, stages=((128, 64, 1, 128), (256, 128, 1, 256), (512, 128, 1, 256)), tail=512)


class MobileFaceNet(nn.Module):
    """``cfg``: stem width; per stage (expand width of its stride-2 block, stage width, residual blocks, their expand width);
    the width of the 1x1 in front of the global depthwise conv.  ``odd_groups``: the first stage's stride-2 block gets a
    grouped 3x3 with that many groups instead of a depthwise one (a defect for the refusal tests).  ``head``: as in IResNet."""

    def __init__(self, cfg=MBF_TINY, features=512, odd_groups=None, head="linear"):
        super().__init__()
        self.head = head
        c = cfg["stem"]
        layers = [ConvBlock(3, c, 3, 2, 1), ConvBlock(c, c, 3, 1, 1, groups=c)]
        for si, (dexp, width, nb, rexp) in enumerate(cfg["stages"]):
            layers.append(DepthWise(c, width, dexp, 2, False, dw_groups=odd_groups if si == 0 else None))
            layers += [DepthWise(width, width, rexp, 1, True) for _ in range(nb)]
            c = width
        t = cfg["tail"]
        layers += [ConvBlock(c, t), LinearBlock(t, t, 7, 1, 0, groups=t)]
        self.layers = nn.Sequential(*layers)
        self.fc = nn.Linear(t, features)
        self.features = nn.BatchNorm1d(features)

    def forward(self, x):
        x = torch.flatten(self.layers(x), 1)
        return self.features(_fully_connected(self.fc, x, self.head))


def layer_list(module):
    """the conv-like layers of a MobileFaceNet in execution order, as an import plan describes them:
    (kind 'conv' | 'dwconv', out channels, in channels per group, kernel, stride, pad, PReLU behind it, residual added)"""
    out = []
    for m in module.layers:
        blocks = list(m.layers) if isinstance(m, DepthWise) else [m]
        for i, b in enumerate(blocks):
            conv = b[0]
            out.append(("dwconv" if conv.groups > 1 else "conv", conv.out_channels, conv.in_channels // conv.groups, conv.kernel_size[0],
                        conv.stride[0], conv.padding[0], isinstance(b, ConvBlock),
                        isinstance(m, DepthWise) and m.residual and i == len(blocks) - 1))
    out.append(("conv", module.fc.out_features, module.fc.in_features, 1, 1, 0, False, False))
    return out


# ------------------------------------------------------------------------------------------------ SCRFD-shaped detector
class ConvBNReLU(nn.Sequential):
    def __init__(self, cin, cout, k=3, stride=1, groups=1):
        super().__init__(nn.Conv2d(cin, cout, k, stride, k // 2, groups=groups, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))


def _unit(cin, cout, stride, depthwise, groups=None):
    if depthwise:
        return nn.Sequential(ConvBNReLU(cin, cin, 3, stride, groups=groups or cin), ConvBNReLU(cin, cout, 1))
    return ConvBNReLU(cin, cout, 3, stride)


class Head(nn.Module):
    def __init__(self, cin, width, anchors, depthwise):
        super().__init__()
        self.tower = nn.Sequential(_unit(cin, width, 1, depthwise), _unit(width, width, 1, depthwise))
        self.cls = nn.Conv2d(width, anchors, 3, 1, 1)
        self.reg = nn.Conv2d(width, 4 * anchors, 3, 1, 1)
        self.kps = nn.Conv2d(width, 10 * anchors, 3, 1, 1)
        self.scale = nn.Parameter(torch.tensor(1.0))

    def forward(self, x):
        t = self.tower(x)
        n = x.shape[0]
        score = self.cls(t).permute(0, 2, 3, 1).reshape(n, -1, 1).sigmoid()
        bbox = (self.reg(t) * self.scale).permute(0, 2, 3, 1).reshape(n, -1, 4)
        kps = self.kps(t).permute(0, 2, 3, 1).reshape(n, -1, 10)
        return score, bbox, kps


class SCRFDNet(nn.Module):
    """conv-bn-relu backbone to strides 8 / 16 / 32, 1x1 laterals, nearest x2 top-down adds, 3x3 output convs, one head per
    stride.  ``upsample``: 'scale' (F.interpolate(scale_factor=2)), 'size' (size= the finer map's) or 'bilinear' (align_corners
    bilinear, which the engine has no kernel for).  Outputs in insightface's order: scores of strides 8, 16, 32, then the
    bboxes, then the keypoints.  ``odd_groups``: a defect for the refusal tests, as in MobileFaceNet."""

    def __init__(self, depthwise=False, upsample="scale", widths=(8, 16, 24, 32, 40), fpn=16, head=24, anchors=2, odd_groups=None):
        super().__init__()
        self.upsample, self.anchors = upsample, anchors
        w = widths
        self.stem = nn.Sequential(ConvBNReLU(3, w[0], 3, 2), _unit(w[0], w[1], 2, depthwise, odd_groups))
        self.c3 = nn.Sequential(_unit(w[1], w[2], 2, depthwise), _unit(w[2], w[2], 1, depthwise))
        self.c4 = _unit(w[2], w[3], 2, depthwise)
        self.c5 = _unit(w[3], w[4], 2, depthwise)
        self.lateral = nn.ModuleList(nn.Conv2d(c, fpn, 1) for c in w[2:])
        self.out = nn.ModuleList(nn.Conv2d(fpn, fpn, 3, 1, 1) for _ in range(3))
        self.heads = nn.ModuleList(Head(fpn, head, anchors, depthwise) for _ in range(3))

    def _up(self, coarse, fine):
        if self.upsample == "scale":
            return F.interpolate(coarse, scale_factor=2, mode="nearest")
        if self.upsample == "size":
            return F.interpolate(coarse, size=fine.shape[-2:], mode="nearest")
        return F.interpolate(coarse, scale_factor=2, mode="bilinear", align_corners=True)

    def forward(self, x):
        c3 = self.c3(self.stem(x))
        c4 = self.c4(c3)
        c5 = self.c5(c4)
        lat = [l(c) for l, c in zip(self.lateral, (c3, c4, c5))]
        lat[1] = lat[1] + self._up(lat[2], lat[1])
        lat[0] = lat[0] + self._up(lat[1], lat[0])
        res = [h(o(t)) for h, o, t in zip(self.heads, self.out, lat)]
        return tuple(r[k] for k in range(3) for r in res)


OUTPUT_ORDER = [(li, kind) for kind in ("score", "bbox", "kps") for li in range(3)]     # of SCRFDNet.forward's tuple


# ------------------------------------------------------------------------------------------------ seeding
def seed_module(module, seed, prelu=True, score_bias=None):
    """Re-initialise from ``seed`` and randomise what torch leaves at a default: every BatchNorm's statistics and affine,
    every PReLU slope (negative, zero, (0, 1) and > 1 mixed; left at 0.25 with ``prelu=False``), every conv / linear bias and
    the heads' scalar scales.  Convs and linears are He-normal.  ``score_bias``: the detector's cls convs' bias.  -> module.eval()"""
    g = torch.Generator().manual_seed(seed)

    def rnd(shape, lo, hi):
        return torch.rand(shape, generator=g) * (hi - lo) + lo

    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                fan = m.weight[0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan) ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.05)
            elif isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
                n = m.num_features
                m.weight.copy_(rnd(n, 0.8, 1.2))
                m.bias.copy_(torch.randn(n, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(n, generator=g) * 0.1)
                m.running_var.copy_(rnd(n, 0.8, 1.2))
            elif isinstance(m, nn.PReLU) and prelu:
                n = m.num_parameters
                kind = torch.randint(0, 4, (n,), generator=g)
                s = rnd(n, 0.05, 0.95)
                s = torch.where(kind == 1, -rnd(n, 0.1, 0.5), s)
                s = torch.where(kind == 2, torch.zeros(n), s)
                s = torch.where(kind == 3, rnd(n, 1.1, 1.6), s)
                m.weight.copy_(s)
            elif isinstance(m, Head):
                m.scale.copy_(rnd((), 0.8, 1.2))
        for m in module.modules():
            if isinstance(m, (IBasicBlock, DepthWise)):              # block-final gamma small, so that deep nets keep their scale
                last = m.bn3 if isinstance(m, IBasicBlock) else m.layers[-1][1]
                last.weight.mul_(0.15)
            elif isinstance(m, Head):
                m.cls.weight.mul_(0.1), m.reg.weight.mul_(0.03), m.kps.weight.mul_(0.05)
                m.reg.bias.fill_(1.5)
                if score_bias is not None:
                    m.cls.bias.fill_(score_bias)
    return module.eval()
