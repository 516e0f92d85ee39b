"""The C calls an ``IResNetHIP.forward`` issues, reduced to what does not change from run to run: the entry point, every
integer argument or struct field by value, each pointer as null (0) or not ("P"), floats as "F"; an fr_conv_sequence call is
expanded into its steps, and a pointer of a step that lies in one of the stream's four plan buffers or its split-K scratch is
written as [buffer index, byte offset] (4 = the scratch), which pins the buffer rotation.  A profiled case also keeps the
(variant, flops) list.  ``python tests/golden/make_embed_calls.py`` writes embed_calls.json; it was run once, on the commit
before the embed host got its route table, and is not run again: the fixture pins that commit's launches in every batch-size
mode.  Lists are run-length encoded: [[count, item], ...]."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ARCH, SEED = "r34", 4321              # the smallest arch with a stage-28 run (3 blocks) and a stage-14 run (5 blocks)
ENTRIES = ("fr_conv_nhwc_f16", "fr_conv_inblock_f16", "fr_conv_splitk_epilogue", "fr_conv_sequence", "fr_conv_walk64_f16",
           "fr_conv_stage14_f16", "fr_conv_stage28_f16", "fr_conv_stage14_f8", "fr_conv_nhwc_f8", "fr_quantize_f16_f8",
           "fr_quantize_f16_f8_centred", "fr_fc_reduce_l2norm")
LAYER = {"use_stage14": False, "use_stage28": False, "use_walk64": False}
# name: (faces, fp8 net, profiled, attributes set for this forward)
CASES = {
    "f16_b1": (1, False, False, {}), "f16_b8": (8, False, False, {}), "f16_b9": (9, False, False, {}),
    "f16_b48": (48, False, False, {}), "f16_b49": (49, False, False, {}), "f16_b100": (100, False, False, {}),
    "f16_b128": (128, False, False, {}), "f16_b130": (130, False, False, {}), "f16_b150": (150, False, False, {}),
    "profiled_b4": (4, False, True, {}), "profiled_b150": (150, False, True, {}),
    "unfused_b4": (4, False, False, {"fuse_shortcut": False}), "unfused_b64": (64, False, False, {"fuse_shortcut": False}),
    "layers_b150": (150, False, False, LAYER),
    "fp8_b16": (16, True, False, {}), "fp8_b150": (150, True, False, {}),
}
R100_CASE = "r100_profiled_b256"      # synthetic r100 (seed 1234), 256 faces, profiled: the (variant, flops) list alone


def crops(B, seed):
    import torch
    x = torch.zeros((B, 112, 112, 8), dtype=torch.float16)
    x[..., :3] = (torch.rand((B, 112, 112, 3), generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(torch.float16)
    return x.cuda()


def build_nets():
    """-> {False: the f16 r34, True: the same after enable_fp8(gptq=False)} (the route does not depend on gptq)"""
    from facerecognition_infrenceengine_amd import weights
    from facerecognition_infrenceengine_amd.iresnet import IResNetHIP
    st = weights.synth_iresnet_state(ARCH, seed=SEED)
    nets = {False: IResNetHIP(st, ARCH, "cuda:0"), True: IResNetHIP(st, ARCH, "cuda:0")}
    assert nets[True].enable_fp8(crops(16, 77), gptq=False) > 0
    return nets


def build_r100():
    from facerecognition_infrenceengine_amd import weights
    from facerecognition_infrenceengine_amd.iresnet import IResNetHIP
    return IResNetHIP(weights.synth_iresnet_state("r100", seed=1234), "r100", "cuda:0")


def fp8_convs(net):
    """[[block, 0 = c1 / 1 = c2]] of the convs that carry an fp8 form"""
    return [[i, j] for i, b in enumerate(net.blocks) for j, c in enumerate(b[:2]) if c.oscale is not None]


def _struct(s, where):
    out = []
    for name, t in s._fields_:
        v = getattr(s, name)
        if t is ctypes.c_void_p:
            out.append(where(v or 0))
        elif t is ctypes.c_float:
            out.append("F")
        elif isinstance(v, ctypes.Structure):
            out.append(_struct(v, where))
        else:
            out.append(int(v))
    return out


def _reduce(name, args, types, bufs):
    def flat(p):
        return "P" if p else 0

    def placed(p):
        for i, b in enumerate(bufs):
            if b.data_ptr() <= p < b.data_ptr() + b.numel() * b.element_size():
                return [i, p - b.data_ptr()]
        return flat(p)

    out = [name]
    for k, (v, t) in enumerate(zip(args, types)):
        if t is ctypes.c_void_p:
            out.append(flat(v.value if isinstance(v, ctypes.c_void_p) else v))
        elif t is ctypes.c_float:
            out.append("F")
        elif name == "fr_conv_sequence" and k == 0:
            out.append([_struct(v[i], placed) for i in range(args[1])])
        elif hasattr(v, "_obj"):                                   # ctypes.byref(struct)
            out.append(_struct(v._obj, flat))
        else:
            out.append(int(v))
    return out


def record(net, x, profiled=False, attrs=None):
    """-> (reduced calls of one forward of ``x``, its (variant, flops) list or None)"""
    import torch
    from facerecognition_infrenceengine_amd import _lib
    calls, saved, was = [], {}, {k: getattr(net, k) for k in (attrs or {})}

    def plan_bufs():
        b = net._plan_bufs.get(torch.cuda.current_stream().cuda_stream)
        return [] if b is None else list(b[0]) + [b[1]]

    for name in ENTRIES:
        saved[name] = net.lib._calls[name]
        net.lib._calls[name] = (lambda *a, _o=saved[name], _n=name:
                                (calls.append(_reduce(_n, a, _lib.SIGNATURES[_n][1], plan_bufs())), _o(*a))[1])
    try:                                                           # the library object is process-wide: always restore
        for k, v in (attrs or {}).items():
            setattr(net, k, v)
        net.profile = [] if profiled else None
        net.forward(x)
        torch.cuda.synchronize()
        prof = [[v, f] for v, f, _, _ in net.profile] if profiled else None
    finally:
        net.lib._calls.update(saved)
        net.profile = None
        for k, v in was.items():
            setattr(net, k, v)
    return calls, prof


def capture(nets, case):
    B, fp8, profiled, attrs = CASES[case]
    return record(nets[fp8], crops(B, 100 + B), profiled, attrs)


def rle(items):
    out = []
    for it in items:
        if out and out[-1][1] == it:
            out[-1][0] += 1
        else:
            out.append([1, it])
    return out


def unrle(runs):
    return [it for n, it in runs for _ in range(n)]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    nets = build_nets()
    out = {"arch": ARCH, "seed": SEED, "fp8_convs": fp8_convs(nets[True]), "stage14_f8": nets[True].stage14_f8 is not None,
           "flops_per_face": {ARCH: nets[False].flops_per_face}, "cases": {}}
    for case in CASES:
        calls, prof = capture(nets, case)
        out["cases"][case] = {"calls": rle(calls)}
        if prof is not None:
            out["cases"][case]["profile"] = rle(prof)
    del nets
    r100 = build_r100()
    out["flops_per_face"]["r100"] = r100.flops_per_face
    out["cases"][R100_CASE] = {"profile": rle(record(r100, crops(256, 356), True)[1])}
    with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "embed_calls.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
