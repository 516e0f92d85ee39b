"""``det_size`` on the MI355X: the device letterbox (csrc/letterbox.hip), the ragged-source alignment warp (csrc/align.hip), the
coordinate mapping and the host layers above them, against the CPU reference of tests/helpers/letterbox_ref.py (composed from
the oracle's own resize, cascade, alignment and nets).  Tolerances are DESIGN.md section 2's, unchanged."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from oracle import align as oalign, match as omatch
from tests.helpers import letterbox_ref as ref

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

RAGGED = [(2160, 3840), (1080, 1920), (480, 640), (1920, 1080), (1000, 1777), (33, 47)]


@pytest.fixture(scope="module")
def app():
    from facerecognition_infrenceengine_amd import FaceAnalysis
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = FaceAnalysis(name="buffalo_l").prepare(ctx_id=0, det_size=(640, 640))
    assert a.synthetic and a.det_size == (640, 640)
    return a


@pytest.fixture(scope="module")
def ragged_frames():
    from make_golden import synth_frame
    return [synth_frame(h, w, 300 + i) for i, (h, w) in enumerate(RAGGED)]


def _dev(frames):
    return [torch.from_numpy(f).cuda() for f in frames]


def _oracle_threads(n=16):
    old = torch.get_num_threads()
    torch.set_num_threads(min(n, os.cpu_count() or n))
    return old


# ---------------------------------------------------------------------------------------------------------------- 1. canvas
@pytest.mark.parametrize("det_size", [(640, 640), (640, 480), (250, 200)])     # square, non-square, a width off the 16-byte path
def test_canvas_of_a_ragged_batch_in_one_launch(app, ragged_frames, det_size):
    eng = app.clone_with(det_size=det_size)
    canvas, scale = eng.letterbox(ragged_frames)
    dw, dh = det_size
    assert canvas.shape == (len(RAGGED), dh, dw, 3) and canvas.dtype == torch.uint8
    got, scale = canvas.cpu().numpy(), scale.cpu().numpy()
    from facerecognition_infrenceengine_amd.letterbox import letterbox_geometry
    total_diff = 0
    for i, f in enumerate(ragged_frames):
        want, s = ref.canvas_ref(f, det_size)
        nh, nw, _ = letterbox_geometry(f.shape[0], f.shape[1], det_size)
        assert scale[i] == s
        assert not got[i, nh:].any() and not got[i, :, nw:].any()                       # every padding byte is 0
        d = np.abs(got[i].astype(np.int16) - want.astype(np.int16))
        npx = int((d.max(axis=2) > 0).sum())
        total_diff += npx
        print(f"canvas {det_size} frame {f.shape[:2]} -> {nh} x {nw}: {npx} pixels differ, max |diff| {int(d.max())}")
        if (nh, nw) == f.shape[:2]:
            assert np.array_equal(got[i, :nh, :nw], f)                                   # equal size: an exact copy
        assert d.max() <= 1 and npx < 1e-3 * nh * nw                                     # <= 1 LSB on < 0.1 % of pixels
    print(f"canvas {det_size}: {total_diff} differing pixels in all (expected 0: the kernel repeats the reference's f32 operations)")


def test_canvas_of_a_uniform_stack_equals_the_list_form(app):
    from make_golden import synth_frame
    frs = np.stack([synth_frame(360, 640, 7), synth_frame(360, 640, 8)])
    a, sa = app.letterbox(torch.from_numpy(frs).cuda())
    b, sb = app.letterbox([frs[0], frs[1]])
    assert torch.equal(a, b) and torch.equal(sa, sb)
    assert np.array_equal(a[:, :360].cpu().numpy(), frs) and not bool(a[:, 360:].any())


# ------------------------------------------------------------------------------------------------------------ 2. detections
def test_unscale_kernel_divides_valid_slots_only(lib):
    from facerecognition_infrenceengine_amd import _lib
    rng = np.random.default_rng(5)
    n, cap = 5, 7
    boxes = (rng.standard_normal((n, cap, 4)) * 700).astype(np.float32)
    kps = (rng.standard_normal((n, cap, 5, 2)) * 700).astype(np.float32)
    boxes[0, 0, 0], kps[1, 0, 0, 0] = np.float32(1e-38), np.float32(-3e38)              # towards subnormal / overflow
    counts = np.array([7, 0, 3, 1, 6], np.int32)
    scale = np.array([1 / 3, 0.36, 1.0, 449 / 33, 0.1337], np.float32)
    invalid = np.arange(cap)[None, :] >= counts[:, None]
    boxes[invalid], kps[invalid] = np.float32(np.nan), np.float32(12345.678)             # must come back bit for bit
    db, dk = torch.from_numpy(boxes).cuda(), torch.from_numpy(kps).cuda()
    dc, ds = torch.from_numpy(counts).cuda(), torch.from_numpy(scale).cuda()
    lib.fr_detections_unscale(_lib.ptr(db), _lib.ptr(dk), _lib.ptr(dc), _lib.ptr(ds), n, cap, _lib.stream_ptr())
    with np.errstate(all="ignore"):
        wb = np.where(invalid[..., None], boxes, boxes / scale[:, None, None])
        wk = np.where(invalid[..., None, None], kps, kps / scale[:, None, None, None])
    assert np.array_equal(db.cpu().numpy().view(np.uint32), wb.view(np.uint32))
    assert np.array_equal(dk.cpu().numpy().view(np.uint32), wk.view(np.uint32))


def test_slot_path_detections_are_the_canvas_detections_divided_by_the_scale(app, ragged_frames):
    dev = _dev(ragged_frames)
    r = app.detect_embed_slots(dev)
    canvas, scale = app.letterbox(dev)
    b, s, k, c = app.det.detect_batch(canvas)
    cnt = c.cpu().numpy()
    assert np.array_equal(r["counts"].cpu().numpy(), cnt) and cnt.sum() >= 4
    sc = scale.cpu().numpy()
    b, s, k = b.cpu().numpy(), s.cpu().numpy(), k.contiguous().cpu().numpy()
    rb, rs, rk = r["bbox"].cpu().numpy(), r["det_score"].cpu().numpy(), r["kps"].cpu().numpy()
    for f, n in enumerate(cnt):
        assert np.array_equal(rs[f, :n], s[f, :n])
        assert np.array_equal(rb[f, :n].view(np.uint32), (b[f, :n] / sc[f]).view(np.uint32))
        assert np.array_equal(rk[f, :n].view(np.uint32), (k[f, :n] / sc[f]).view(np.uint32))
    assert rb.dtype == np.float32 and (b / sc[:, None, None]).dtype == np.float32
    # the compact form (one sync on the counts) returns the same faces
    d = app.detect_embed_device(dev)
    assert d["counts"] == cnt.tolist()
    rows = [(f, j) for f, n in enumerate(cnt) for j in range(n)]
    assert np.array_equal(d["bbox"].cpu().numpy(), np.stack([rb[f, j] for f, j in rows]))
    assert np.array_equal(d["kps"].cpu().numpy(), np.stack([rk[f, j] for f, j in rows]))


# ----------------------------------------------------------------------------------------------------------- 3. ragged warp
def _corner_kps(h, w):
    """three faces per frame: one whose crop is larger than the frame (samples on every border row / column and outside), one
    hanging over the bottom-right corner, one hanging over the top-left one, rotated"""
    dst = oalign.ARCFACE_DST.astype(np.float64)
    big = dst * (1.4 * max(h, w) / 112.0) + np.array([-0.2 * w, -0.2 * h])
    s = max(min(h, w) / 112.0 * 0.6, 0.2)
    br = dst * s + np.array([w - 1 - 56 * s, h - 1 - 56 * s])
    th = 0.4
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    tl = (dst - 56) @ R.T * s + np.array([0.3, 0.2])
    return np.stack([big, br, tl]).astype(np.float32)


def test_ragged_warp_is_bit_identical_to_the_per_frame_warp(lib):
    from facerecognition_infrenceengine_amd import _lib
    from facerecognition_infrenceengine_amd.letterbox import frame_table
    from make_golden import synth_frame
    shapes = [(240, 320), (480, 640), (1080, 1920), (33, 47), (3, 5)]      # the smallest frames LAST: they end the arena
    frames = [synth_frame(h, w, 500 + i) for i, (h, w) in enumerate(shapes)]
    # one arena, frames back to back at odd offsets (a frame's neighbours are other frames' bytes), nothing behind the last
    offs, off = [], 0
    for f in frames:
        offs.append(off)
        off += f.size + 1
    arena = torch.from_numpy(np.concatenate([np.concatenate([f.reshape(-1), np.full(1, 255, np.uint8)]) for f in frames])[:off - 1].copy()).cuda()
    tab, _ = frame_table([arena.data_ptr() + o for o in offs], shapes)
    table = torch.from_numpy(tab).cuda()
    nf, per = len(frames), 3
    kps = np.concatenate([_corner_kps(h, w) for h, w in shapes])           # [nf * 3, 5, 2], frame-major
    fidx = np.repeat(np.arange(nf, dtype=np.int32), per)
    F = nf * per
    dk, di = torch.from_numpy(kps).cuda(), torch.from_numpy(fidx).cuda()
    out = torch.empty((F, 112, 112, 8), dtype=torch.float16, device="cuda")
    out8 = torch.empty((F, 112, 112, 3), dtype=torch.uint8, device="cuda")
    M = torch.empty((F, 2, 3), dtype=torch.float32, device="cuda")
    lib.fr_warp_affine_5pt_refs(_lib.ptr(table), nf, _lib.ptr(dk), _lib.ptr(di), None, F, 112, _lib.ptr(out), _lib.ptr(out8),
                                _lib.ptr(M), _lib.stream_ptr())
    # slots form: cap 4, counts 3 (slot 3 of every frame is empty -> zero-filled)
    cap = 4
    ks = np.zeros((nf, cap, 5, 2), np.float32)
    ks[:, :per] = kps.reshape(nf, per, 5, 2)
    ks[:, per:] = np.nan
    dks, dcn = torch.from_numpy(ks).cuda(), torch.full((nf,), per, dtype=torch.int32, device="cuda")
    outs = torch.empty((nf * cap, 112, 112, 8), dtype=torch.float16, device="cuda")
    lib.fr_warp_affine_5pt_slots_refs(_lib.ptr(table), nf, _lib.ptr(dks), _lib.ptr(dcn), cap, 112, _lib.ptr(outs), _lib.stream_ptr())
    for f, fr in enumerate(frames):
        h, w = shapes[f]
        one = torch.from_numpy(fr[None]).cuda()
        w16 = torch.empty((per, 112, 112, 8), dtype=torch.float16, device="cuda")
        w8 = torch.empty((per, 112, 112, 3), dtype=torch.uint8, device="cuda")
        wM = torch.empty((per, 2, 3), dtype=torch.float32, device="cuda")
        k1 = dk[f * per:(f + 1) * per].contiguous()
        i1 = torch.zeros(per, dtype=torch.int32, device="cuda")
        lib.fr_warp_affine_5pt(_lib.ptr(one), 1, h, w, _lib.ptr(k1), _lib.ptr(i1), None, per, 112, _lib.ptr(w16), _lib.ptr(w8),
                               _lib.ptr(wM), _lib.stream_ptr())
        sl = slice(f * per, (f + 1) * per)
        assert torch.equal(out[sl].view(torch.int16), w16.view(torch.int16)), shapes[f]
        assert torch.equal(out8[sl], w8) and torch.equal(M[sl].view(torch.int32), wM.view(torch.int32)), shapes[f]
        assert bool((w8 != 0).any()), shapes[f]                                  # the faces do sample the frame
        ws = torch.empty((cap, 112, 112, 8), dtype=torch.float16, device="cuda")
        ks1 = dks[f:f + 1].contiguous()
        lib.fr_warp_affine_5pt_slots(_lib.ptr(one), 1, h, w, _lib.ptr(ks1), _lib.ptr(dcn[f:f + 1].contiguous()), cap, 112, _lib.ptr(ws),
                                     _lib.stream_ptr())
        assert torch.equal(outs[f * cap:(f + 1) * cap].view(torch.int16), ws.view(torch.int16)), shapes[f]
        assert torch.equal(ws[:per].view(torch.int16), w16.view(torch.int16)) and not bool(ws[per:].any())


def test_new_entries_check_their_arguments(lib):
    from facerecognition_infrenceengine_amd import _lib
    one = ctypes.c_void_p(16)                                  # never dereferenced: the checks come first
    with pytest.raises(_lib.FrError, match="null pointer"):
        lib.fr_letterbox_u8(None, 1, one, 640, 640, None)
    with pytest.raises(_lib.FrError, match="bad size"):
        lib.fr_letterbox_u8(one, 0, one, 640, 640, None)
    with pytest.raises(_lib.FrError, match="null pointer"):
        lib.fr_detections_unscale(one, one, None, one, 1, 16, None)
    with pytest.raises(_lib.FrError, match="bad size"):
        lib.fr_detections_unscale(one, one, one, one, 1, 0, None)
    with pytest.raises(_lib.FrError, match="null pointer"):
        lib.fr_warp_affine_5pt_refs(None, 1, one, one, None, 1, 112, one, None, None, None)
    assert lib.fr_warp_affine_5pt_refs(None, 1, None, None, None, 0, 112, None, None, None, None) == 0     # no faces: nothing read
    with pytest.raises(_lib.FrError, match="bad argument"):
        lib.fr_warp_affine_5pt_slots_refs(one, 0, one, one, 4, 112, one, None)


# ------------------------------------------------------------------------------------------------- 4. end to end vs the oracle
def _check_frames_vs_oracle(app, r, frames, which, cap_o=16):
    """frames ``which`` of a slot-path result against the reference composition run on the GPU's OWN canvas (test 1 pins the
    canvas; one LSB of one pixel moves a P-Net score by ~1e-3, so the oracle must see the same bytes).  Returns [(slot, oracle
    embedding)]."""
    canvas, scale = app.letterbox(frames)
    canvas, scale = canvas.cpu().numpy(), scale.cpu().numpy()
    counts = r["counts"].cpu().numpy()
    cap = r["bbox"].shape[1]
    emb = r["embedding"].cpu().numpy().reshape(len(counts), cap, 512)
    rb, rs, rk = r["bbox"].cpu().numpy(), r["det_score"].cpu().numpy(), r["kps"].cpu().numpy()
    faces, old = [], _oracle_threads()
    try:
        for i in which:
            _, s, _, ob, ok = ref.detect_ref(canvas[i], scale[i], cap_o=cap_o)
            n = len(s)
            assert counts[i] == n, (i, counts[i], n)
            if n == 0:
                continue
            tol = 5e-3 / float(scale[i])                     # 5e-3 px on the canvas, in frame pixels
            np.testing.assert_allclose(rs[i, :n], s, atol=5e-5)
            np.testing.assert_allclose(rb[i, :n], ob, atol=tol)
            np.testing.assert_allclose(rk[i, :n], ok, atol=tol)
            oemb = ref.embed_ref(frames[i], ok)              # crops of the ORIGINAL frame at the oracle's own landmarks
            e = emb[i, :n]
            cos = (e * oemb).sum(1) / (np.linalg.norm(e, axis=1) * np.linalg.norm(oemb, axis=1))
            print(f"frame {i} {frames[i].shape[:2]}: {n} faces, max 1 - cos {float((1 - cos).max()):.2e}")
            assert (1 - cos).max() < 1e-3, (i, cos)
            faces += [(i * cap + j, oemb[j]) for j in range(n)]
    finally:
        torch.set_num_threads(old)
    return faces


def _planted_ids_equal(r, faces, rows, seed):
    from facerecognition_infrenceengine_amd.gallery import GalleryMatcher
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((rows, 512)).astype(np.float32)
    planted = rng.choice(rows, len(faces), replace=False)
    oemb = np.stack([e for _, e in faces])
    G[planted] = oemb / np.linalg.norm(oemb, axis=1, keepdims=True) + 0.02 * rng.standard_normal(oemb.shape).astype(np.float32)
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    m = GalleryMatcher("cuda:0")
    m.set_rows(list(range(rows)), G, normalise=False)
    Q = r["normed_embedding"][torch.tensor([s for s, _ in faces], device="cuda")].contiguous()
    idx, score = m.match_device(Q)
    oi, _ = omatch.match_rows_fast(np.stack([omatch.renormalise(e / np.linalg.norm(e)) for e in oemb]), G)
    assert np.array_equal(idx.cpu().numpy(), oi) and np.array_equal(oi, planted)
    assert (m.decide_device(idx, score, 0.4).cpu().numpy() == 1).all()


def test_mixed_batch_end_to_end_vs_oracle(app, ragged_frames):
    r = app.detect_embed_slots(_dev(ragged_frames))
    torch.cuda.synchronize()
    assert not app.det._tls.path["batch"]                     # 6 canvases: the all-f32 detector
    faces = _check_frames_vs_oracle(app, r, ragged_frames, range(len(ragged_frames)))
    assert len(faces) >= 6
    _planted_ids_equal(r, faces, 10_000, 21)


# -------------------------------------------------------------------------------------------- 5. mixed call vs separate calls
def test_get_batch_of_three_sizes_equals_three_gets(app):
    from make_golden import synth_frame
    eng = app.clone_with(cap_o=2)                             # at most 6 faces: every embed forward in the same batch-size mode
    frames = [synth_frame(1080, 1920, 31), synth_frame(480, 640, 0), synth_frame(720, 1280, 12)]
    assert all(f.shape[0] * f.shape[1] < eng.det.batch_min_pixels for f in frames)
    mixed = eng.get_batch(frames)
    single = [eng.get(f) for f in frames]
    assert [len(m) for m in mixed] == [len(s) for s in single] and sum(len(m) for m in mixed) >= 3
    for f, (ms, ss) in enumerate(zip(mixed, single)):
        for a, b in zip(ms, ss):
            assert np.array_equal(a.bbox, b.bbox) and np.array_equal(a.kps, b.kps) and a.det_score == b.det_score
            assert np.array_equal(a.embedding, b.embedding) and np.array_equal(a.normed_embedding, b.normed_embedding)
    plain = app.clone_with(det_size=None)
    with pytest.raises(ValueError):
        plain.get_batch(frames)                               # no canvas: differing sizes are refused, as before
    with pytest.raises(ValueError):
        plain.detect_embed_slots(_dev(frames))


# --------------------------------------------------------------------------------------------- 6. the batch path is reached
def test_sixty_four_mixed_frames_take_the_batch_detector(app):
    from facerecognition_infrenceengine_amd.mtcnn import pyramid_scales
    from make_golden import synth_frame
    det = app.det
    shapes = [(2160, 3840), (1080, 1920), (480, 640), (1080, 1920), (1920, 1080), (480, 640), (720, 1280), (1080, 1920)]
    uniq = {}
    frames = []
    for i in range(64):
        h, w = shapes[i % 8]
        key = (h, w, i // 8 if (h, w) != (2160, 3840) else i // 32)          # two distinct 4K frames, distinct seeds elsewhere
        if key not in uniq:
            uniq[key] = synth_frame(h, w, 700 + len(uniq))
        frames.append(uniq[key])
    assert 64 * 640 * 640 >= det.batch_min_pixels
    r = app.detect_embed_slots(_dev(frames))
    torch.cuda.synchronize()
    p = det._tls.path
    nlev = len(pyramid_scales(640, 640, det.minsize, det.factor))
    assert p["frames"] == 64 and p["batch"] and p["unfused_levels"] == 0 and p["split_ro"], p
    assert p["fused_levels"] == p["band_levels"] == nlev * p["chunks"], p          # the band-only exact pass on every level
    geo = [det.p1.out_hw(int(np.ceil(640 * s)), int(np.ceil(640 * s))) for s in pyramid_scales(640, 640, det.minsize, det.factor)]
    big = [hw for hw in geo if hw[0] * hw[1] >= det.split_pconv1_min_px]
    assert len(big) >= 1 and sorted(p["pconv1_mfma_levels"]) == sorted(big * p["chunks"]), (p, geo)
    rec = det.exact_lists()
    assert [e["net"] for e in rec] == ["rnet", "onet"] * p["chunks"], rec
    assert all(0 <= e["count"] <= e["cap"] for e in rec) and det.exact_list_overflow() == [], rec
    which = [0, 1, 2, 4]                                                           # a 4K, a 1080p, a VGA and a portrait frame
    faces = _check_frames_vs_oracle(app, r, frames, which)
    assert len(faces) >= 4
    _planted_ids_equal(r, faces, 10_000, 22)


# ----------------------------------------------------------------------------------------------- 7. processor and camera
def test_processor_and_camera_batcher_take_mixed_sizes(app):
    import queue
    from facerecognition_infrenceengine_amd.camera import CameraManager
    from facerecognition_infrenceengine_amd.ingest import RaggedIngest
    from facerecognition_infrenceengine_amd.processor import EmbeddingManager, FaceRecognitionProcessor, InMemoryStore
    from make_golden import synth_frame
    frames = [synth_frame(1080, 1920, 31), synth_frame(240, 320, 4), synth_frame(480, 640, 0), synth_frame(240, 320, 5)]
    rng = np.random.default_rng(9)
    store = InMemoryStore()
    for i in range(30):
        store.add_employee(f"n{i}", "acme", rng.standard_normal(512).astype(np.float32), name=f"N{i}")
    want_faces = [app.get(f) for f in frames]
    for k in (0, 2):
        for j, f in enumerate(want_faces[k]):
            store.add_employee(f"face{k}_{j}", "acme", f.embedding, name=f"F{k}{j}")
    mgr = EmbeddingManager(store=store, device="cuda:0")
    proc = FaceRecognitionProcessor(mgr, face_detector=app)
    assert proc.accepts_mixed_sizes
    res = proc.recognize_batch(frames, "acme")
    assert [len(x) for x in res] == [len(x) for x in want_faces]
    for k, (got, want) in enumerate(zip(res, want_faces)):
        for j, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g["bbox"], w.bbox.astype(int))                   # original-frame pixels
            if k in (0, 2):
                assert g["person_id"] == f"face{k}_{j}", (k, j, g["person_id"])    # the planted ids
        one = proc.recognize(frames[k], "acme")                                    # and what the per-frame caller gets
        assert [g["person_id"] for g in got] == [g["person_id"] for g in one]
    res2 = proc.recognize_batch(frames, "acme")                                    # the ring's second slot, same results
    assert [[g["person_id"] for g in x] for x in res2] == [[g["person_id"] for g in x] for x in res]
    assert isinstance(next(iter(proc._stages.values()))[0], RaggedIngest)
    # an engine without a detection canvas refuses the same call, as before
    plain = FaceRecognitionProcessor(mgr, face_detector=app.clone_with(det_size=None))
    assert not plain.accepts_mixed_sizes
    with pytest.raises(ValueError):
        plain.recognize_batch(frames, "acme")
    # the camera batcher: ONE engine pass for the mixed batch
    passes = []
    orig = app.det.detect_batch

    def counted(fr, *a, **k):
        passes.append(tuple(fr.shape))
        return orig(fr, *a, **k)
    app.det.detect_batch = counted
    try:
        cm = CameraManager(mgr, processor=proc)
        cm.result_queue = queue.Queue(maxsize=10)
        got = cm.process_batch([(s, f.copy()) for s, f in enumerate(frames)], "acme")
    finally:
        del app.det.detect_batch
    assert passes == [(4, 640, 640, 3)]
    assert [[g["person_id"] for g in x] for x in got] == [[g["person_id"] for g in x] for x in res]
    outs = [cm.result_queue.get_nowait() for _ in range(4)]
    assert [s for s, _ in outs] == [0, 1, 2, 3] and [o.shape for _, o in outs] == [f.shape for f in frames]
