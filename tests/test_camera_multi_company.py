"""CameraManager with cameras of several companies (no GPU: fake captures, fake processor): a second start adds its
sources under its own company, one batching loop serves them all, a turn that mixes companies hands the processor the
per-frame list and a single-company turn the plain id, a repeated start is a no-op, stop clears everything."""
import time

import numpy as np


class FakeCap:
    """An endless camera: frames tagged with the source, a short block per read (as a live camera's read())."""

    def __init__(self, source):
        self.source, self.released = source, False

    def read(self):
        time.sleep(0.001)
        return True, np.full((4, 6, 3), self.source, np.uint8)

    def release(self):
        self.released = True


class FakeProcessor:
    def __init__(self):
        self.calls = []                          # (sources of the frames, company_id as given)

    def recognize_batch(self, frames, company_id):
        self.calls.append(([int(f[0, 0, 0]) for f in frames], company_id))
        return [[{"tag": int(f[0, 0, 0])}] for f in frames]

    def annotate(self, frame, res):
        return frame


def _wait(cond, seconds=10):
    deadline = time.time() + seconds
    while time.time() < deadline and not cond():
        time.sleep(0.005)
    return cond()


def _manager():
    from facerecognition_infrenceengine_amd.camera import CameraManager
    proc, caps, seen = FakeProcessor(), {}, []

    def factory(s):
        assert s not in caps, f"source {s} opened twice"
        caps[s] = FakeCap(s)
        return caps[s]
    cm = CameraManager(embedding_manager=None, processor=proc, capture_factory=factory)
    return cm, proc, caps, seen


def test_second_start_adds_another_companys_cameras_to_the_one_loop():
    cm, proc, caps, seen = _manager()
    cm.start_cameras([0, 1], "acme", display=lambda s, f: seen.append(s))
    try:
        assert _wait(lambda: {0, 1} <= set(seen))
        assert cm.company_of == {0: "acme", 1: "acme"}
        assert all(c == "acme" for _, c in proc.calls)                      # single-company turns: the plain id
        threads = len(cm.threads)
        cm.start_cameras([0, 1], "acme")                                      # a repeated identical start: a no-op
        assert len(cm.threads) == threads and set(caps) == {0, 1}
        cm.start_cameras([1, 2, 3], "globex")                                 # new sources join, source 1 stays acme's
        assert cm.company_of == {0: "acme", 1: "acme", 2: "globex", 3: "globex"}
        assert len(cm.threads) == threads + 2 and set(caps) == {0, 1, 2, 3}
        assert _wait(lambda: {2, 3} <= set(seen))                             # the new sources produce results
        assert _wait(lambda: any(isinstance(c, list) and len(set(c)) == 2 for _, c in proc.calls))
    finally:
        cm.stop_cameras()
    want = {0: "acme", 1: "acme", 2: "globex", 3: "globex"}
    mixed = 0
    for tags, c in proc.calls:
        if isinstance(c, list):                                               # a mixed turn: one id per frame, aligned
            assert len(c) == len(tags) and len(set(c)) > 1 and [want[t] for t in tags] == c
            mixed += 1
        else:                                                                 # one company in the turn: the str, as ever
            assert isinstance(c, str) and all(want[t] == c for t in tags)
    assert mixed >= 1
    assert all(tags == sorted(tags) for tags, _ in proc.calls)                # source order within a turn
    # stop clears everything; every capture was released
    assert cm.company_of == {} and cm.frame_queues == {} and cm.threads == [] and not cm.running
    assert all(c.released for c in caps.values())
    # and the manager starts again from nothing, under whatever company the new start names
    caps.clear()
    cm.start_cameras([3], "initech")
    try:
        assert cm.company_of == {3: "initech"}
        n = len(proc.calls)
        assert _wait(lambda: len(proc.calls) > n)
        assert proc.calls[-1] == ([3], "initech")
    finally:
        cm.stop_cameras()
    assert cm.company_of == {}


def test_process_batch_takes_a_company_list_aligned_with_the_batch():
    import queue
    import pytest
    cm, proc, _, _ = _manager()
    cm.result_queue = queue.Queue(maxsize=10)
    frames = [np.full((4, 6, 3), s, np.uint8) for s in range(4)]
    batch = list(enumerate(frames))
    res = cm.process_batch(batch, ["a", "b", "a", "c"])
    assert proc.calls == [([0, 1, 2, 3], ["a", "b", "a", "c"])] and [r[0]["tag"] for r in res] == [0, 1, 2, 3]
    assert [cm.result_queue.get_nowait()[0] for _ in range(4)] == [0, 1, 2, 3]
    cm.process_batch(batch, ["a"] * 4)                                        # a list that names one company: the str
    cm.process_batch(batch, "a")
    assert proc.calls[1:] == [([0, 1, 2, 3], "a")] * 2
    assert cm.stats["batches"] == 3 and cm.stats["frames"] == 12
    # frames of two sizes (a processor without mixed sizes): one call per size, each with its own frames' ids
    proc.calls.clear()
    odd = [(0, frames[0]), (1, np.full((2, 2, 3), 1, np.uint8)), (2, frames[2]), (3, np.full((2, 2, 3), 3, np.uint8))]
    res = cm.process_batch(odd, ["a", "b", "a", "c"])
    assert proc.calls == [([0, 2], "a"), ([1, 3], ["b", "c"])] and [r[0]["tag"] for r in res] == [0, 1, 2, 3]
    with pytest.raises(ValueError, match="one company id per frame"):
        cm.process_batch(batch, ["a", "b"])
