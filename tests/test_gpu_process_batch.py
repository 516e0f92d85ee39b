"""GPU end to end: CameraProcessor.process_batch (the counting path in batches) against process_frame run frame by
frame, and its on-device unknown-person clustering against UnknownClusters.assign() fed the same rows one by one."""
import os
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
CAMS = [0, 1, 2, 3]


class Sink:
    """records the manager calls in order"""

    def __init__(self):
        self.calls = []

    def process_detection(self, pid, info, cam, ts, score):
        self.calls.append(("rec", cam, ts, pid, info, score))

    def process_unknown_detection(self, cam, ts, emb, bbox):
        self.calls.append(("unk", cam, ts, np.array(emb), bbox))


class ClusterSink(Sink):
    def process_unknown_cluster(self, cam, ts, cluster, is_new, count, bbox):
        self.calls.append(("clu", cam, ts, (cluster, is_new, count), bbox))


@pytest.fixture(scope="module")
def world():
    """engine, frames and two galleries (30 noise rows each, as test_camera_batcher_equals_per_frame_recognition has them):
    "enrolled" holds the faces of frames 0 and 2 as that test enrols them - the synthetic weights give any two faces a
    cosine around 0.5, so against the WHOLE gallery (the counting path) every face of every frame is then recognised;
    "mixed" holds the same faces with their component in the span of the faces of frames 1 and 3 taken out, so that
    the faces of frames 0 and 2 are recognised (score = the norm of what is left, about 0.7) and those of frames 1 and
    3 score 0 against them and at most a noise row's 0.2 otherwise: unknown."""
    from facerecognition_infrenceengine_amd import FaceAnalysis
    from facerecognition_infrenceengine_amd.processor import EmbeddingManager, InMemoryStore
    from make_golden import synth_frame
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        app = FaceAnalysis(name="buffalo_l", providers=["CUDAExecutionProvider", "CPUExecutionProvider"])
        app.prepare(ctx_id=0)
    frames = [synth_frame(240, 320, s) for s in (4, 5, 6, 21)]
    emb = [[f.normed_embedding.astype(np.float64) for f in app.get(fr)] for fr in frames]
    U = np.stack(emb[1] + emb[3])                                  # rows: the faces that stay unknown
    proj = np.linalg.pinv(U) @ U                                   # projector onto their span
    mgrs = {}
    for name in ("enrolled", "mixed"):
        rng = np.random.default_rng(9)
        store = InMemoryStore()
        for i in range(30):
            store.add_employee(f"n{i}", "acme" if i % 2 else "other", rng.standard_normal(512).astype(np.float32), name=f"N{i}")
        for k in (0, 2):
            for j, e in enumerate(emb[k]):
                row = e if name == "enrolled" else e - proj @ e
                store.add_employee(f"face{k}_{j}", "acme", row.astype(np.float32), name=f"F{k}{j}")
        mgrs[name] = EmbeddingManager(store=store, device="cuda:0")
    return app, frames, mgrs


@pytest.mark.parametrize("gallery", ["enrolled", "mixed"])
def test_process_batch_equals_process_frame(world, gallery):
    from facerecognition_infrenceengine_amd.processor import CameraProcessor
    app, frames, mgrs = world
    mgr = mgrs[gallery]
    a, b = Sink(), Sink()
    want = [CameraProcessor(mgr, a, face_detector=app).process_frame(f, c) for f, c in zip(frames, CAMS)]
    got = CameraProcessor(mgr, b, face_detector=app).process_batch(frames, CAMS)
    assert got == want
    print(gallery, want)
    assert sum(s["recognized"] for s in want) >= 1
    if gallery == "mixed":                                         # some faces are recognised and some are not
        assert sum(s["unknown"] for s in want) >= 2 and want[0]["recognized"] >= 1 and want[1]["unknown"] >= 1
    assert len(a.calls) == len(b.calls) == sum(s["recognized"] + s["unknown"] for s in want)
    assert len({id(c[2]) for c in b.calls}) == 1                   # one timestamp for the whole batch
    for x, y in zip(a.calls, b.calls):
        assert x[0] == y[0] and x[1] == y[1]                       # the same call for the same camera, in order
        if x[0] == "rec":
            assert x[3] == y[3] and x[4] == y[4]                   # pid, metadata
            # the embed net picks its kernels by batch-size mode: per-frame calls and the batch may run in different
            # modes, scores and embeddings then agree to f16-conv rounding (the bound of the camera batcher's test)
            assert isinstance(y[5], float) and abs(x[5] - y[5]) < 5e-4
        else:
            assert x[4] == y[4] and all(isinstance(v, int) for v in y[4])       # the same truncated box
            assert y[3].dtype == np.float32 and np.abs(x[3] - y[3]).max() < 5e-4
    # no gallery: the zero stats for every frame, nothing handed on
    from facerecognition_infrenceengine_amd.processor import EmbeddingManager, InMemoryStore
    c = Sink()
    empty = CameraProcessor(EmbeddingManager(store=InMemoryStore(), device="cuda:0"), c, face_detector=app)
    assert empty.process_batch(frames, CAMS) == [{"faces": 0, "recognized": 0, "unknown": 0}] * 4 and not c.calls
    for proc in (empty, CameraProcessor(mgr, c, face_detector=app)):            # the one error that raises, gallery or not
        with pytest.raises(ValueError, match="4 frames but 3 camera ids"):
            proc.process_batch(frames, CAMS[:3])
    # errors are logged and swallowed, as process_frame's
    assert CameraProcessor(mgr, c, face_detector=app).process_batch([np.zeros((4, 4), np.uint8)], [0]) == \
        [{"faces": 0, "recognized": 0, "unknown": 0}]


def one_by_one(uc, rows):
    """(cluster, is_new, count) of each row through assign(), one at a time"""
    out = []
    for e in rows:
        before = len(uc.hist)
        c = uc.assign(e)
        out.append((c, int(c == before), uc.counts[c]))
    return out


def test_process_batch_clusters_unknown_faces_on_device(world):
    from facerecognition_infrenceengine_amd.enrol import UnknownClusters
    from facerecognition_infrenceengine_amd.processor import CameraProcessor
    app, frames, mgr = world[0], world[1], world[2]["mixed"]
    # a manager without process_unknown_cluster still gets the rows that were clustered: they are the reference
    plain = Sink()
    st0 = CameraProcessor(mgr, plain, face_detector=app, unknown_clusters=UnknownClusters("cuda:0")).process_batch(frames, CAMS)
    rows = [(c[1], c[3]) for c in plain.calls if c[0] == "unk"]
    print("clustered:", [t for s in st0 for t in s["unknown_clusters"]])
    assert len(rows) >= 2 and all(abs(np.linalg.norm(e) - 1) < 1e-5 for _, e in rows)
    ref = UnknownClusters("cuda:0")
    want = one_by_one(ref, [e for _, e in rows])
    assert [t for s in st0 for t in s["unknown_clusters"]] == want
    # with process_unknown_cluster: the same triples, and no embedding handed over
    sink, bank = ClusterSink(), UnknownClusters("cuda:0")
    cp = CameraProcessor(mgr, sink, face_detector=app, unknown_clusters=bank)
    st1 = cp.process_batch(frames, CAMS)
    assert [{k: v for k, v in s.items() if k != "unknown_clusters"} for s in st1] == \
        [{k: v for k, v in s.items() if k != "unknown_clusters"} for s in st0]
    clu = [c for c in sink.calls if c[0] == "clu"]
    assert not [c for c in sink.calls if c[0] == "unk"]
    assert [c[3] for c in clu] == want == [t for s in st1 for t in s["unknown_clusters"]]
    assert [c[1] for c in clu] == [cam for cam, _ in rows]
    assert [c[4] for c in clu] == [c[4] for c in plain.calls if c[0] == "unk"]           # the same boxes
    assert [c for c in sink.calls if c[0] == "rec"] and bank.counts == ref.counts
    # the same frames again: nothing is new, every face's cluster has grown by the faces it was given
    sink.calls.clear()
    st2 = cp.process_batch(frames, CAMS)
    again = one_by_one(ref, [e for _, e in rows])
    got = [t for s in st2 for t in s["unknown_clusters"]]
    assert got == again and all(t[1] == 0 for t in got)
    if len({t[0] for t in want}) == len(want):                     # every face its own cluster: the counts grow by one
        assert [t[2] for t in got] == [t[2] + 1 for t in want]
    assert bank.overflowed == 0
    # two banks: cameras 0, 1 share one, cameras 2, 3 the other; each sees its own cameras' faces only
    x, y = UnknownClusters("cuda:0"), UnknownClusters("cuda:0")
    sink2 = ClusterSink()
    st3 = CameraProcessor(mgr, sink2, face_detector=app,
                          unknown_clusters={0: x, 1: x, 2: y, 3: y}).process_batch(frames, CAMS)
    for bank_, cams in ((x, (0, 1)), (y, (2, 3))):
        alone = UnknownClusters("cuda:0")
        want_b = one_by_one(alone, [e for cam, e in rows if cam in cams])
        assert [t for cam in cams for t in st3[cam]["unknown_clusters"]] == want_b
        assert bank_.counts == alone.counts and len(bank_.hist) == len(alone.hist)
        assert np.abs(bank_.avg.cpu().numpy() - alone.avg.cpu().numpy()).max() < 5e-4      # rows of another engine pass
    assert [c[3] for c in sink2.calls if c[0] == "clu"] == [t for s in st3 for t in s["unknown_clusters"]]
    # a camera without a bank: its unknown faces are not clustered and arrive with their rows, the others as before
    z, sink3 = UnknownClusters("cuda:0"), ClusterSink()
    st4 = CameraProcessor(mgr, sink3, face_detector=app, unknown_clusters={0: z, 1: z}).process_batch(frames, CAMS)
    assert [{k: v for k, v in s.items() if k != "unknown_clusters"} for s in st4] == \
        [{k: v for k, v in s.items() if k != "unknown_clusters"} for s in st0]
    assert [t for cam in (0, 1) for t in st4[cam]["unknown_clusters"]] == [t for cam in (0, 1) for t in st3[cam]["unknown_clusters"]]
    assert st4[2]["unknown_clusters"] == [] and st4[3]["unknown_clusters"] == [] and z.counts == x.counts
    assert [c[1] for c in sink3.calls if c[0] == "clu"] == [cam for cam, _ in rows if cam in (0, 1)]
    loose = [c for c in sink3.calls if c[0] == "unk"]
    assert [c[1] for c in loose] == [cam for cam, _ in rows if cam in (2, 3)] and len(loose) >= 1
    for c, (_, e) in zip(loose, [r for r in rows if r[0] in (2, 3)]):
        assert c[3].dtype == np.float32 and np.abs(c[3] - e).max() < 5e-4 and abs(np.linalg.norm(c[3]) - 1) < 1e-5


def test_process_batch_hands_refused_faces_to_the_manager(world, caplog):
    """a full bank: its faces reach the manager through process_unknown_detection, with their rows"""
    from facerecognition_infrenceengine_amd.enrol import UnknownClusters
    from facerecognition_infrenceengine_amd.processor import CameraProcessor
    app, frames, mgr = world[0], world[1], world[2]["mixed"]
    full = UnknownClusters("cuda:0", capacity=1)
    full.assign(np.eye(1, 512, 3, dtype=np.float32)[0])            # its one cluster: a row no face resembles
    sink = ClusterSink()
    import logging
    with caplog.at_level(logging.WARNING):
        st = CameraProcessor(mgr, sink, face_detector=app, unknown_clusters=full).process_batch(frames, CAMS)
    unk = [c for c in sink.calls if c[0] == "unk"]
    assert len(unk) == sum(s["unknown"] for s in st) >= 2 and not [c for c in sink.calls if c[0] == "clu"]
    assert all(t == (-2, 0, 0) for s in st for t in s["unknown_clusters"])
    assert all(abs(np.linalg.norm(c[3]) - 1) < 1e-5 for c in unk)
    assert full.overflowed == len(unk) and full.counts == [1]
    assert sum("clusters full" in r.message for r in caplog.records) == 1       # logged once per call
