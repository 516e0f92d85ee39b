"""YUV 4:2:0 frame ingest on the MI355X: the device conversion (csrc/yuv_to_bgr.hip) against the NumPy definition of
tests/helpers/yuv_ref.py, byte for byte - every (Y, U, V) triple, every alignment trap of the two layouts, both entry points -
and the host layers above it: ``colour.yuv420_to_bgr``, the YUV rings of ingest.py, ``FaceAnalysis.get_batch_yuv`` and
``FaceRecognitionProcessor.recognize_batch(pixel_format=...)``, which must return exactly what the BGR route returns for the
converted frames (the same bytes into the same kernels)."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from tests.helpers import yuv_ref

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

# wide strips exactly filled (16, 32), wide strips plus a byte tail (18, 34, 1026), tail only (2, 6, 10), a single chroma row
# (H = 2), frame strides H*W*3/2 off 4 bytes (2 x 6 = 18), I420 V planes at odd offsets (2 x 6: 15; 2 x 2: 5)
SHAPES = [(2, 2), (2, 6), (4, 10), (2, 16), (4, 18), (6, 32), (8, 34), (2, 1024 + 2)]
LAYOUTS = ("nv12", "i420")
GUARD, PATTERN = 64, 0xA5


def _consts(matrix):
    from facerecognition_infrenceengine_amd import colour
    return colour.MATRICES[matrix]


def _lid(layout):
    from facerecognition_infrenceengine_amd import colour
    return colour.LAYOUTS[layout]


def _random_yuv(rng, h, w, n=None):
    shape = (h * 3 // 2, w) if n is None else (n, h * 3 // 2, w)
    return rng.integers(0, 256, shape, dtype=np.uint8)


_CASES = {}


def _case(h, w, layout):
    """three seeded frames of one shape and their BGR, computed once and left unchanged"""
    key = (h, w, layout)
    if key not in _CASES:
        rng = np.random.default_rng([h, w, LAYOUTS.index(layout)])
        yuv = _random_yuv(rng, h, w, 3)
        bgr = np.stack([yuv_ref.yuv420_to_bgr(f, layout, "bt601") for f in yuv])
        yuv.setflags(write=False)
        bgr.setflags(write=False)
        _CASES[key] = (yuv, bgr)
    return _CASES[key]


def _guarded(nbytes, lead):
    """device buffer of GUARD + lead + nbytes + GUARD pattern bytes; (buffer, offset of the payload)"""
    buf = torch.full((GUARD + lead + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    return buf, GUARD + lead


# ------------------------------------------------------------------------------------------------------ 1. every value
def test_every_yuv_triple_once_bt601(lib):
    """One 4096 x 4096 NV12 frame holding every (Y, U, V) triple exactly once: block b of the 2048 x 2048 chroma grid carries
    (U, V) = the 16 bits b >> 6, its four pixels Y = 4 (b & 63) + 0..3."""
    from facerecognition_infrenceengine_amd import _lib
    H = W = 4096
    b = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
    u, v = ((b >> 6) >> 8).astype(np.uint8), ((b >> 6) & 255).astype(np.uint8)
    y = np.empty((H, W), np.uint8)
    for dy in range(2):
        for dx in range(2):
            y[dy::2, dx::2] = 4 * (b & 63) + 2 * dy + dx
    up = lambda c: np.repeat(np.repeat(c, 2, axis=0), 2, axis=1).astype(np.int64)
    seen = np.bincount(((y.astype(np.int64) << 16) | (up(u) << 8) | up(v)).reshape(-1), minlength=1 << 24)
    assert seen.shape == (1 << 24,) and (seen == 1).all()
    nv12 = yuv_ref.pack(y, u, v, "nv12")
    want = yuv_ref.yuv420_to_bgr(nv12, "nv12", "bt601")
    src = torch.from_numpy(nv12).cuda()
    dst = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    lib.fr_yuv420_to_bgr_u8(_lib.ptr(src), _lib.ptr(dst), 1, H, W, _lid("nv12"), *_consts("bt601"), _lib.stream_ptr())
    got = dst.cpu().numpy()
    assert np.array_equal(got, want)
    assert got.min() == 0 and got.max() == 255                      # both clamps were reached


@pytest.mark.parametrize("matrix", ["bt709", "jpeg"])
def test_random_frame_other_matrices(lib, matrix):
    from facerecognition_infrenceengine_amd import colour
    rng = np.random.default_rng(709 if matrix == "bt709" else 420)
    for layout in LAYOUTS:
        yuv = _random_yuv(rng, 64, 64)
        got = colour.yuv420_to_bgr(torch.from_numpy(yuv).cuda(), layout, matrix)
        assert got.shape == (64, 64, 3) and got.dtype == torch.uint8
        want = yuv_ref.yuv420_to_bgr(yuv, layout, matrix)
        assert np.array_equal(got.cpu().numpy(), want)
        assert not np.array_equal(want, yuv_ref.yuv420_to_bgr(yuv, layout, "bt601"))      # the matrix does matter


# ------------------------------------------------------------------------------------------------------ 2. shape traps
@pytest.mark.parametrize("layout", LAYOUTS)
def test_uniform_entry_shape_traps_any_byte_alignment_nothing_outside(lib, layout):
    """N = 3 frames of every trap shape; src and dst start 0, 1, 2 and 3 bytes into larger buffers; the destination's
    surroundings keep their pattern."""
    from facerecognition_infrenceengine_amd import _lib
    for h, w in SHAPES:
        yuv, bgr = _case(h, w, layout)
        for off in (0, 1, 2, 3):
            sbuf, so = _guarded(yuv.size, off)
            sbuf[so:so + yuv.size] = torch.from_numpy(yuv.reshape(-1).copy()).cuda()
            dbuf, do = _guarded(bgr.size, off)
            src, dst = sbuf[so:so + yuv.size], dbuf[do:do + bgr.size]
            assert src.data_ptr() % 4 == off and dst.data_ptr() % 4 == off
            lib.fr_yuv420_to_bgr_u8(_lib.ptr(src), _lib.ptr(dst), 3, h, w, _lid(layout), *_consts("bt601"), _lib.stream_ptr())
            want = np.full(dbuf.numel(), PATTERN, np.uint8)
            want[do:do + bgr.size] = bgr.reshape(-1)
            got = dbuf.cpu().numpy()
            assert np.array_equal(got[do:do + bgr.size].reshape(bgr.shape), bgr), (h, w, layout, off)
            assert np.array_equal(got, want), f"{h} x {w} {layout} +{off}: bytes outside the destination were written"
            assert (sbuf[:so] == PATTERN).all() and (sbuf[so + yuv.size:] == PATTERN).all()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("gap", [0, 1])
def test_table_entry_all_shapes_in_one_call_nothing_outside(lib, layout, gap):
    """Every trap shape, plus a frame of several blocks' worth of strips, in ONE launch: sources at 16-byte-aligned offsets of
    one arena; destinations 16-byte aligned (gap 0) or packed behind one pattern byte each (gap 1: odd addresses)."""
    from facerecognition_infrenceengine_amd import _lib
    from facerecognition_infrenceengine_amd.letterbox import frame_table
    shapes = SHAPES + [(64, 176)]                                    # 32 x 11 strips: more than one block's 256 lanes
    cases = [_case(h, w, layout) for h, w in shapes]
    soffs, doffs, so, do = [], [], 0, GUARD
    for h, w in shapes:
        soffs.append(so)
        so += (h * w * 3 // 2 + 15) // 16 * 16
        doffs.append(do)
        do += h * w * 3 + 1 if gap else (h * w * 3 + 15) // 16 * 16
    sarena = torch.full((max(so, 16),), PATTERN, dtype=torch.uint8, device="cuda")
    darena = torch.full((do + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    assert sarena.data_ptr() % 16 == 0 and darena.data_ptr() % 16 == 0
    want = np.full(darena.numel(), PATTERN, np.uint8)
    for (yuv, bgr), s, d in zip(cases, soffs, doffs):
        sarena[s:s + yuv[0].size] = torch.from_numpy(yuv[0].reshape(-1).copy()).cuda()
        want[d:d + bgr[0].size] = bgr[0].reshape(-1)
    tab, _ = frame_table([darena.data_ptr() + d for d in doffs], shapes)
    table = torch.from_numpy(tab).cuda()
    srcs = torch.tensor([sarena.data_ptr() + s for s in soffs], dtype=torch.int64).cuda()
    lib.fr_yuv420_to_bgr_refs_u8(_lib.ptr(table), _lib.ptr(srcs), len(shapes), _lid(layout), *_consts("bt601"), _lib.stream_ptr())
    got = darena.cpu().numpy()
    for (h, w), (_, bgr), d in zip(shapes, cases, doffs):
        assert np.array_equal(got[d:d + bgr[0].size].reshape(h, w, 3), bgr[0]), (h, w, layout)
    assert np.array_equal(got, want), "bytes outside the destination frames were written"
    # the two entry points agree with each other by agreeing with the definition; an entry no conversion exists for is skipped
    bad = np.frombuffer(tab.tobytes(), dtype=np.uint8).copy()
    refs = (_lib.FrameRef * len(shapes)).from_buffer(bad)
    refs[1].H, refs[2].W = 3, 9
    darena.fill_(PATTERN)
    bad_table = torch.from_numpy(bad).cuda()
    lib.fr_yuv420_to_bgr_refs_u8(_lib.ptr(bad_table), _lib.ptr(srcs), len(shapes), _lid(layout), *_consts("bt601"), _lib.stream_ptr())
    got = darena.cpu().numpy()
    for i in (1, 2):
        h, w = shapes[i]
        want[doffs[i]:doffs[i] + h * w * 3] = PATTERN
    assert np.array_equal(got, want)


def test_device_entry_point_tensor_list_and_out_forms(lib):
    from facerecognition_infrenceengine_amd import colour
    shapes = [(4, 10), (2, 6), (8, 34), (6, 32)]
    yuvs = [_case(h, w, "i420")[0][0] for h, w in shapes]
    wants = [_case(h, w, "i420")[1][0] for h, w in shapes]
    outs = colour.yuv420_to_bgr([torch.from_numpy(y.copy()).cuda() for y in yuvs], "i420")
    assert isinstance(outs, list) and [tuple(o.shape) for o in outs] == [(h, w, 3) for h, w in shapes]
    assert all(o.data_ptr() % 16 == 0 and o.is_contiguous() for o in outs)
    for o, w_ in zip(outs, wants):
        assert np.array_equal(o.cpu().numpy(), w_)
    mine = [torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda") for h, w in shapes]
    back = colour.yuv420_to_bgr([torch.from_numpy(y.copy()).cuda() for y in yuvs], "i420", out=mine)
    assert all(a is b for a, b in zip(back, mine)) and all(np.array_equal(o.cpu().numpy(), w_) for o, w_ in zip(mine, wants))
    yuv3, bgr3 = _case(8, 34, "nv12")
    stack = colour.yuv420_to_bgr(torch.from_numpy(yuv3.copy()).cuda(), "nv12")
    assert stack.shape == (3, 8, 34, 3) and np.array_equal(stack.cpu().numpy(), bgr3)
    one = colour.yuv420_to_bgr(torch.from_numpy(yuv3[1].copy()).cuda(), "nv12")
    assert one.shape == (8, 34, 3) and np.array_equal(one.cpu().numpy(), bgr3[1])
    buf = torch.zeros((3, 8, 34, 3), dtype=torch.uint8, device="cuda")
    assert colour.yuv420_to_bgr(torch.from_numpy(yuv3.copy()).cuda(), "nv12", out=buf) is buf
    assert np.array_equal(buf.cpu().numpy(), bgr3)
    with pytest.raises(ValueError):
        colour.yuv420_to_bgr(torch.zeros((9, 5), dtype=torch.uint8, device="cuda"))            # odd W
    with pytest.raises(ValueError):
        colour.yuv420_to_bgr(torch.zeros((4, 4), dtype=torch.uint8, device="cuda"))            # no H with 4 rows
    with pytest.raises(ValueError):
        colour.yuv420_to_bgr(torch.zeros((3, 4), dtype=torch.uint8, device="cuda"), "yuyv")
    with pytest.raises(ValueError):
        colour.yuv420_to_bgr(torch.zeros((3, 4), dtype=torch.uint8, device="cuda"), out=buf)


# ------------------------------------------------------------------------------------------------------------ 3. ingest
def test_frame_ingest_nv12_ring_returns_bgr_and_survives_slot_reuse():
    from facerecognition_infrenceengine_amd.ingest import FrameIngest
    ring = FrameIngest(3, 4, 10, pixel_format="nv12")
    plain = FrameIngest(3, 4, 10)
    assert ring.host_buffer(0).shape == (3, 6, 10) and plain.host_buffer(0).shape == (3, 4, 10, 3)
    assert ring.decode_into(0, 0, b"not an image") is False
    rng = np.random.default_rng(12)
    kept, wants = [], []
    for turn in range(ring.depth + 1):
        yuv = _random_yuv(rng, 4, 10, 3)
        ring.host_buffer(turn)[...] = yuv
        dev, ev = ring.upload(turn)
        assert dev.shape == (3, 4, 10, 3) and dev.dtype == torch.uint8 and dev.is_cuda
        assert dev.shape == plain.upload(turn)[0].shape
        torch.cuda.current_stream().wait_event(ev)
        kept.append(dev.clone())
        ring.release(turn)
        ev.synchronize()                                            # the copy has read the pinned slot: it may be rewritten
        wants.append(np.stack([yuv_ref.yuv420_to_bgr(f, "nv12") for f in yuv]))
    torch.cuda.synchronize()
    assert ring.upload(ring.depth)[0].data_ptr() == ring.upload(0)[0].data_ptr()         # turn depth did reuse slot 0
    for turn, (k, w) in enumerate(zip(kept, wants)):
        assert np.array_equal(k.cpu().numpy(), w), turn
    assert len({w.tobytes() for w in wants}) == len(wants)                               # the contents did change
    with pytest.raises(ValueError):
        FrameIngest(3, 5, 10, pixel_format="nv12")
    with pytest.raises(ValueError):
        FrameIngest(3, 4, 10, pixel_format="rgb")


@pytest.mark.parametrize("det_size", [None, (32, 32)])
def test_ragged_ingest_i420_ring_returns_the_bgr_rings_table(det_size):
    from facerecognition_infrenceengine_amd import _lib
    from facerecognition_infrenceengine_amd.ingest import RaggedIngest
    shapes = [(4, 10), (2, 6), (8, 34)]
    ring = RaggedIngest(shapes, det_size=det_size, pixel_format="i420")
    plain = RaggedIngest(shapes, det_size=det_size)
    assert ring.offsets == plain.offsets and ring.nbytes == plain.nbytes
    assert torch.equal(ring.det_scale, plain.det_scale)
    rng = np.random.default_rng(34)
    kept, wants = [], []
    for turn in range(ring.depth + 1):
        yuvs = [_random_yuv(rng, h, w) for h, w in shapes]
        for i, y in enumerate(yuvs):
            view = ring.host_frame(turn, i)
            assert view.shape == y.shape
            view[...] = y
        arena, table, ev = ring.upload(turn)
        parena, ptable, _ = plain.upload(turn)
        assert arena.shape == parena.shape and table.shape == ptable.shape == (len(shapes) * 32,)
        # the same table as the BGR ring: per entry the frame's offset in the arena, its size and its size on the canvas
        a = (_lib.FrameRef * len(shapes)).from_buffer_copy(table.cpu().numpy().tobytes())
        b = (_lib.FrameRef * len(shapes)).from_buffer_copy(ptable.cpu().numpy().tobytes())
        for i, (h, w) in enumerate(shapes):
            assert a[i].data - arena.data_ptr() == b[i].data - parena.data_ptr() == ring.offsets[i]
            assert (a[i].H, a[i].W, a[i].nh, a[i].nw) == (b[i].H, b[i].W, b[i].nh, b[i].nw) and (a[i].H, a[i].W) == (h, w)
            assert (a[i].nh > 0) == (det_size is not None)
        torch.cuda.current_stream().wait_event(ev)
        kept.append([ring.device_frame(turn, i).clone() for i in range(len(shapes))])
        ring.release(turn)
        ev.synchronize()
        wants.append([yuv_ref.yuv420_to_bgr(y, "i420") for y in yuvs])
    torch.cuda.synchronize()
    for turn, (ks, ws) in enumerate(zip(kept, wants)):
        for k, w in zip(ks, ws):
            assert k.shape == w.shape and np.array_equal(k.cpu().numpy(), w), turn
    with pytest.raises(ValueError):
        RaggedIngest([(4, 10), (3, 6)], pixel_format="i420")


# -------------------------------------------------------------------------------------------------------- 4. end to end
@pytest.fixture(scope="module")
def app():
    from facerecognition_infrenceengine_amd import FaceAnalysis
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = FaceAnalysis(name="buffalo_l").prepare(ctx_id=0)
    assert a.synthetic and a.det_size is None
    return a


def _same_faces(got, want):
    assert [len(g) for g in got] == [len(w) for w in want]
    for gs, ws in zip(got, want):
        for g, w in zip(gs, ws):
            assert np.array_equal(g.bbox.view(np.uint32), w.bbox.view(np.uint32))
            assert np.array_equal(g.kps.view(np.uint32), w.kps.view(np.uint32))
            assert np.float32(g.det_score).view(np.uint32) == np.float32(w.det_score).view(np.uint32)
            assert np.array_equal(g.embedding.view(np.uint32), w.embedding.view(np.uint32))
            assert np.array_equal(g.normed_embedding.view(np.uint32), w.normed_embedding.view(np.uint32))


def test_get_batch_yuv_equals_get_batch_on_the_converted_frame(app):
    from make_golden import synth_frame
    nv12 = yuv_ref.bgr_to_yuv420(synth_frame(480, 640, 0), "nv12")
    bgr = yuv_ref.yuv420_to_bgr(nv12, "nv12")
    want = app.get_batch([bgr])
    assert len(want[0]) >= 1                                        # or the comparison proves nothing
    _same_faces(app.get_batch_yuv([nv12], "nv12"), want)
    _same_faces(app.get_batch_yuv(nv12[None]), want)                                      # array form, default format
    _same_faces(app.get_batch_yuv(torch.from_numpy(nv12[None]).cuda()), want)             # device frames in
    _same_faces([app.get_yuv(nv12)], [app.get(bgr)])
    assert len(app.get_yuv(nv12, max_num=1)) == 1
    i420 = yuv_ref.pack(*yuv_ref.planes(nv12, "nv12"), "i420")
    _same_faces([app.get_yuv(i420, pixel_format="i420")], want)
    with pytest.raises(ValueError):
        app.get_yuv(nv12[:-1])                                      # 719 rows: no H
    mixed = [nv12, yuv_ref.bgr_to_yuv420(synth_frame(240, 320, 4), "nv12")]
    with pytest.raises(ValueError):
        app.get_batch_yuv(mixed)                                    # differing sizes need a detection canvas, as get_batch


def test_get_batch_yuv_mixed_sizes_under_det_size(app):
    from make_golden import synth_frame
    eng = app.clone_with(det_size=(640, 640))
    nv12 = [yuv_ref.bgr_to_yuv420(synth_frame(1080, 1920, 31), "nv12"), yuv_ref.bgr_to_yuv420(synth_frame(480, 640, 0), "nv12")]
    bgr = [yuv_ref.yuv420_to_bgr(f, "nv12") for f in nv12]
    want = eng.get_batch(bgr)
    assert all(len(w) >= 1 for w in want)
    _same_faces(eng.get_batch_yuv(nv12, "nv12"), want)


def _results_equal(got, want):
    assert [len(g) for g in got] == [len(w) for w in want]
    for gs, ws in zip(got, want):
        for g, w in zip(gs, ws):
            assert np.array_equal(g["bbox"], w["bbox"]) and g["person_id"] == w["person_id"]
            assert g["det_score"] == w["det_score"] and g["person_info"] == w["person_info"]
            assert np.float32(g["recognition_score"]).view(np.uint32) == np.float32(w["recognition_score"]).view(np.uint32)


@pytest.mark.parametrize("det_size", [None, (640, 640)])
def test_recognize_batch_nv12_equals_recognize_batch_on_the_converted_frames(app, det_size):
    from facerecognition_infrenceengine_amd.ingest import FrameIngest, RaggedIngest
    from facerecognition_infrenceengine_amd.processor import EmbeddingManager, FaceRecognitionProcessor, InMemoryStore
    from make_golden import synth_frame
    eng = app if det_size is None else app.clone_with(det_size=det_size)
    sizes = [(240, 320, 4), (240, 320, 5)] if det_size is None else [(480, 640, 0), (240, 320, 4)]
    nv12 = [yuv_ref.bgr_to_yuv420(synth_frame(h, w, s), "nv12") for h, w, s in sizes]
    bgr = [yuv_ref.yuv420_to_bgr(f, "nv12") for f in nv12]
    faces = eng.get_batch(bgr)
    assert all(len(f) >= 1 for f in faces)
    rng = np.random.default_rng(9)
    store = InMemoryStore()
    for i in range(30):
        store.add_employee(f"n{i}", "acme", rng.standard_normal(512).astype(np.float32), name=f"N{i}")
    for j, f in enumerate(faces[0]):                                 # frame 0's faces are enrolled
        store.add_employee(f"face0_{j}", "acme", f.embedding, name=f"F0{j}")
    proc = FaceRecognitionProcessor(EmbeddingManager(store=store, device="cuda:0"), face_detector=eng)
    want = proc.recognize_batch(bgr, "acme")
    assert [r["person_id"] for r in want[0]] == [f"face0_{j}" for j in range(len(faces[0]))]
    for _ in range(3):                                               # depth 2: the third turn reuses the first slot
        _results_equal(proc.recognize_batch(nv12, "acme", pixel_format="nv12"), want)
    rings = [v[0] for v in proc._stages.values()]
    assert sorted(r.pixel_format for r in rings) == ["bgr", "nv12"]                       # a ring per format
    assert all(isinstance(r, FrameIngest if det_size is None else RaggedIngest) for r in rings)
    _results_equal(proc.recognize_batch(nv12, ["acme", "acme"], pixel_format="nv12"), proc.recognize_batch(bgr, ["acme", "acme"]))
    got = proc.identify_batch(nv12, "acme", k=3, pixel_format="nv12")
    ref = proc.identify_batch(bgr, "acme", k=3)
    assert [len(g) for g in got] == [len(r) for r in ref]
    for gs, rs in zip(got, ref):
        for g, r in zip(gs, rs):
            assert np.array_equal(g["bbox"], r["bbox"]) and g["det_score"] == r["det_score"]
            assert [(c["person_id"], np.float32(c["score"]).view(np.uint32)) for c in g["candidates"]] == \
                [(c["person_id"], np.float32(c["score"]).view(np.uint32)) for c in r["candidates"]]
    with pytest.raises(ValueError):
        proc.recognize_batch(bgr, "acme", pixel_format="nv12")       # BGR arrays are no [H*3/2, W] frames
    with pytest.raises(ValueError):
        proc.recognize_batch(nv12, "acme", pixel_format="nv12", matrix="bt2020")
