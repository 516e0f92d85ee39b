"""JPEG in, through the layers above the decoder: ``FaceAnalysis.get_batch_jpeg`` and ``Enroller(decoder=...)`` from encoded
bytes equal the same calls on the BGR arrays the definition (tests/helpers/jpeg_decode_ref.py) decodes the files to, field for
field and bit for bit - the pixels are the same pixels."""
import io
import os
import sys
import warnings

import numpy as np
import pytest
from PIL import Image

from tests.helpers import jpeg_decode_cases as cases, jpeg_decode_ref as ref

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))


def _app(**kw):
    from facerecognition_infrenceengine_amd import FaceAnalysis
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return FaceAnalysis(name="buffalo_l").prepare(ctx_id=0, **kw)


@pytest.fixture(scope="module")
def app():
    return _app()


@pytest.fixture(scope="module")
def files():
    """(bytes, the definition's picture) of a few synthetic frames with faces, written three ways"""
    from make_golden import synth_frame
    out = {}
    for name, (h, w, seed, sampling, writer) in {"a": (240, 320, 4, "420", "plain"), "b": (240, 320, 5, "444", "optimize"),
                                                 "c": (240, 320, 6, "422", "dri_row"), "small": (200, 260, 4, "420", "dri_3")}.items():
        data = cases.pil_file(synth_frame(h, w, seed), 95, sampling, writer)
        out[name] = (data, ref.decode(data)[0])
    return out


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g) == len(w)
        for fg, fw in zip(g, w):
            for key in ("bbox", "kps", "embedding", "normed_embedding"):
                assert np.asarray(fg[key]).tobytes() == np.asarray(fw[key]).tobytes(), key
            assert fg["det_score"] == fw["det_score"]


def test_get_batch_jpeg_equals_get_batch_on_the_definitions_pictures(app, files):
    names = ("a", "b", "c")
    want = app.get_batch(np.stack([files[k][1] for k in names]))
    assert sum(len(f) for f in want) >= 1
    _same(app.get_batch_jpeg([files[k][0] for k in names]), want)
    assert app._jpeg_decoder.last_fallbacks == {}
    # one progressive file (the host decodes it) and one that is no picture (a frame without faces) in the batch
    buf = io.BytesIO()
    Image.fromarray(files["b"][1][..., ::-1].copy()).save(buf, "JPEG", quality=90, progressive=True)
    from facerecognition_infrenceengine_amd.ingest import decode_image
    prog = decode_image(buf.getvalue())
    got = app.get_batch_jpeg([files["a"][0], buf.getvalue(), b"\xff\xd8 not a picture", files["c"][0]])
    assert got[2] == []
    _same([got[0], got[1], got[3]], app.get_batch(np.stack([files["a"][1], prog, files["c"][1]])))
    assert set(app._jpeg_decoder.last_fallbacks) == {1, 2} and "progressive" in app._jpeg_decoder.last_fallbacks[1]
    # a scan that breaks off: the device flags it, the host decoder has the last word (Pillow refuses a truncated file too)
    cut = files["a"][0][:len(files["a"][0]) // 2]
    got = app.get_batch_jpeg([cut, files["b"][0]])
    assert "entropy" in app._jpeg_decoder.last_fallbacks[0]
    host = decode_image(cut)
    assert (got[0] == []) if host is None else True
    _same([got[1]], app.get_batch(files["b"][1][None]))
    assert app.get_batch_jpeg([]) == []


def test_get_batch_jpeg_two_sizes_under_det_size(app, files):
    sized = _app(det_size=(320, 320))
    names = ("a", "small", "b")
    _same(sized.get_batch_jpeg([files[k][0] for k in names]), sized.get_batch([files[k][1] for k in names]))
    with pytest.raises(ValueError, match="det_size"):
        app.get_batch_jpeg([files["a"][0], files["small"][0]])


def test_enrol_batch_with_a_decoder_equals_the_host_decoded_run(app, files):
    from facerecognition_infrenceengine_amd.enrol import Enroller
    from facerecognition_infrenceengine_amd.gallery import DeviceGallery
    from facerecognition_infrenceengine_amd.jpeg_decode import JpegDecoder
    buf = io.BytesIO()
    Image.fromarray(files["b"][1][..., ::-1].copy()).save(buf, "JPEG", quality=90, progressive=True)
    jobs = [[files["a"][0], files["a"][0]], [files["b"][0]], [b"not an image", files["c"][0]], [buf.getvalue()], [files["a"][1]]]
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((40, 512)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)

    def run(**kw):
        dg = DeviceGallery("cuda:0", capacity=64)
        dg.upsert(list(range(40)), rows, normalise=False)
        return Enroller(app, **kw).enrol_batch(jobs, dg.view(list(range(40))), ids=[100 + j for j in range(len(jobs))])
    want, got = run(), run(decoder=JpegDecoder("cuda:0"))
    assert [r["status"] for r in want].count("done") >= 1
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert set(g) == set(w) and g["status"] == w["status"]
        for key in w:
            if key == "embedding":
                assert g[key].tobytes() == w[key].tobytes()
            else:
                assert g[key] == w[key], key


# ---------------------------------------------------------------- the rings and what runs on them
@pytest.fixture(scope="module")
def world(app, files):
    """a processor on the module's engine with a gallery that knows two of the faces, and one on a det_size engine"""
    from facerecognition_infrenceengine_amd.processor import EmbeddingManager, FaceRecognitionProcessor, InMemoryStore
    rng = np.random.default_rng(3)
    store = InMemoryStore()
    for i in range(30):
        store.add_employee(f"n{i}", "acme", rng.standard_normal(512).astype(np.float32), name=f"N{i}")
    faces = app.get(files["a"][1]) + app.get(files["b"][1])
    assert len(faces) >= 2
    store.add_employee("e0", "acme", faces[0].embedding, name="Ada Lovelace", employeeId="E-0042")
    store.add_visitor("v0", "acme", faces[-1].embedding, name="A Visitor")
    manager = EmbeddingManager(store=store, device="cuda:0")
    return dict(proc=FaceRecognitionProcessor(manager, face_detector=app),
                sized=FaceRecognitionProcessor(manager, face_detector=_app(det_size=(320, 320))))


def _same_results(a, b):
    """two result lists of a batch, field for field"""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert len(x) == len(y)
        for p, q in zip(x, y):
            assert set(p) == set(q)
            assert np.array_equal(p["bbox"], q["bbox"]) and p["det_score"] == q["det_score"]
            assert p["person_id"] == q["person_id"] and p["person_info"] == q["person_info"]
            assert np.float32(p["recognition_score"]).tobytes() == np.float32(q["recognition_score"]).tobytes()


def _progressive(files, name):
    from facerecognition_infrenceengine_amd.ingest import decode_image
    buf = io.BytesIO()
    Image.fromarray(files[name][1][..., ::-1].copy()).save(buf, "JPEG", quality=90, progressive=True)
    return buf.getvalue(), decode_image(buf.getvalue())


def test_recognize_and_identify_batch_from_a_dense_jpeg_ring(world, files):
    proc = world["proc"]
    names = ("a", "b", "c", "a")
    blobs, arrays = [files[k][0] for k in names], [files[k][1] for k in names]
    want = proc.recognize_batch(arrays, "acme")
    assert sum(len(r) for r in want) >= 2 and any(f["person_id"] == "e0" for r in want for f in r)
    for _ in range(3):                                    # every slot of the ring, and the first of them again
        _same_results(proc.recognize_batch(blobs, "acme", pixel_format="jpeg"), want)
    got, ref_top = proc.identify_batch(blobs, "acme", k=3, pixel_format="jpeg"), proc.identify_batch(arrays, "acme", k=3)
    assert repr(got) == repr(ref_top)
    # one progressive file takes the host's decoder, one blob is no picture: a black frame, no faces
    prog, prog_bgr = _progressive(files, "b")
    got = proc.recognize_batch([blobs[0], prog, b"\xff\xd8 no picture", blobs[2]], "acme", pixel_format="jpeg")
    black = np.zeros_like(arrays[0])
    _same_results(got, proc.recognize_batch([arrays[0], prog_bgr, black, arrays[2]], "acme"))
    assert got[2] == []
    # a good header and a scan that breaks off - the ordinary failure of an MJPEG stream: parse takes it, the device flags it,
    # and the frame is black, not the picture the slot held two turns ago (every slot has held good frames by now)
    cut = blobs[1][:len(blobs[1]) // 2]
    for _ in range(2):
        got = proc.recognize_batch([blobs[0], cut, blobs[2], blobs[3]], "acme", pixel_format="jpeg")
        _same_results(got, proc.recognize_batch([arrays[0], black, arrays[2], arrays[3]], "acme"))
        assert got[1] == []
    ring = next(r for k, (r, _) in proc._stages.items() if k[-1] == "jpeg")
    assert [int(v) for v in ring._jpeg.status[0].cpu()] == [0, 1, 0, 0] == [int(v) for v in ring._jpeg.status[1].cpu()]
    got = proc.recognize_batch([blobs[0], prog, b"\xff\xd8 no picture", blobs[2]], "acme", pixel_format="jpeg")
    assert ring.pixel_format == "jpeg" and ring._jpeg.link_bytes < sum(len(b) for b in (blobs[0], blobs[2])) + 2 * black.nbytes + 4096
    with pytest.raises(ValueError, match="bytes"):
        proc.recognize_batch(arrays, "acme", pixel_format="jpeg")


def test_recognize_batch_two_sizes_on_a_det_size_engine(world, files):
    proc = world["sized"]
    names = ("a", "small", "b")
    blobs, arrays = [files[k][0] for k in names], [files[k][1] for k in names]
    want = proc.recognize_batch(arrays, "acme")
    assert sum(len(r) for r in want) >= 1
    for _ in range(2):
        _same_results(proc.recognize_batch(blobs, "acme", pixel_format="jpeg"), want)
    prog, prog_bgr = _progressive(files, "small")
    got = proc.recognize_batch([blobs[0], prog, blobs[2]], "acme", pixel_format="jpeg")
    _same_results(got, proc.recognize_batch([arrays[0], prog_bgr, arrays[2]], "acme"))
    # a scan that breaks off, in slots that have held good frames: a black frame of its own size
    cut = blobs[1][:len(blobs[1]) // 2]
    for _ in range(2):
        got = proc.recognize_batch([blobs[0], cut, blobs[2]], "acme", pixel_format="jpeg")
        _same_results(got, proc.recognize_batch([arrays[0], np.zeros_like(arrays[1]), arrays[2]], "acme"))
        assert got[1] == []


def test_a_scan_too_long_for_its_slot_is_decoded_by_the_host(files):
    from facerecognition_infrenceengine_amd.ingest import FrameIngest
    ring = FrameIngest(2, 240, 320, "cuda:0", depth=2, pixel_format="jpeg", max_frame_bytes=len(files["c"][0]) // 2)
    assert ring.put(0, 0, files["c"][0]) is False and "room" in ring.fallbacks(0)[0]
    assert ring.put(0, 1, files["small"][0]) is None and "200 x 260" in ring.fallbacks(0)[1]      # not the ring's size: black
    dev, ready = ring.upload(0)
    ready.synchronize()
    ring.release(0)
    assert np.array_equal(dev[0].cpu().numpy(), files["c"][1]) and not dev[1].cpu().numpy().any()
    big = FrameIngest(2, 240, 320, "cuda:0", depth=2, pixel_format="jpeg")
    assert big.put(1, 0, files["a"][0]) is True and big.put(1, 1, files["b"][0]) is True and big.fallbacks(1) == {}
    dev, ready = big.upload(1)
    ready.synchronize()
    assert np.array_equal(dev.cpu().numpy(), np.stack([files["a"][1], files["b"][1]]))
    assert (big._jpeg.status[1].cpu().numpy() == 0).all()
    with pytest.raises(ValueError, match="put"):
        FrameIngest(1, 8, 8, "cuda:0").put(0, 0, files["a"][0])


def test_camera_manager_on_jpeg_captures_serves_a_snapshot(world, files):
    import queue
    from facerecognition_infrenceengine_amd import Hud, JpegEncoder
    from facerecognition_infrenceengine_amd.camera import CameraManager
    from facerecognition_infrenceengine_amd.server import create_app
    proc, hud, enc = world["proc"], Hud(), JpegEncoder(80)
    with pytest.raises(ValueError, match="hud"):
        CameraManager(embedding_manager=None, processor=proc, pixel_format="jpeg")
    cm = CameraManager(embedding_manager=None, processor=proc, hud=hud, encode=enc, pixel_format="jpeg")
    cm.result_queue = queue.Queue(maxsize=64)
    res = cm.process_batch([(0, files["a"][0]), ("lobby", files["b"][0])], "acme")
    want, want_res = proc.recognize_faces_batch([files["a"][1], files["b"][1]], "acme", hud, return_results=True, encode=enc)
    _same_results(res, want_res)
    assert cm.latest_jpeg(0) == want[0] and cm.latest_jpeg("lobby") == want[1] and want[0][:2] == b"\xff\xd8"

    class Embeddings:
        def get_stats(self):
            return {"total_embeddings": 3}

        def force_sync(self):
            pass
    r = create_app(Embeddings(), cm).test_client().get("/api/camera/snapshot?source=0")
    assert r.status_code == 200 and r.mimetype == "image/jpeg" and r.data == want[0]
