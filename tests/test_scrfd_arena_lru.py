"""SCRFDHIP keeps the activation arenas of the last MAX_ARENAS (batch size, canvas size, stream) keys of a thread: a gated
camera turn brings any batch size from 1 to the camera count, and one arena per size was kept for ever (no GPU: the arena
and the stream are stand-ins)."""
import threading
import types


def test_arenas_are_bounded_and_the_most_recently_used_stay(monkeypatch):
    import torch
    from facerecognition_infrenceengine_amd import scrfd
    made = []

    def arena(det, plan, N):
        made.append(N)
        return types.SimpleNamespace(N=N)
    monkeypatch.setattr(scrfd, "_Arena", arena)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0))
    det = scrfd.SCRFDHIP.__new__(scrfd.SCRFDHIP)
    det._tls, det.device, det.plan = threading.local(), "cuda:0", lambda hw: None
    hw = (640, 640)
    first = det._arena(1, hw)
    assert det._arena(1, hw) is first and made == [1]                      # a hit builds nothing
    for n in range(2, scrfd.MAX_ARENAS + 1):
        det._arena(n, hw)
    assert det._arena(1, hw) is first and len(det._tls.arenas) == scrfd.MAX_ARENAS      # 1 is the most recently used now
    det._arena(64, hw)                                                     # one more: the oldest (2) goes, 1 stays
    keys = [k[0] for k in det._tls.arenas]
    assert len(keys) == scrfd.MAX_ARENAS and 2 not in keys and keys[-2:] == [1, 64]
    assert det._arena(1, hw) is first
    assert det._arena(2, hw).N == 2 and made.count(2) == 2                 # rebuilt on demand
    for n in range(1, 65):                                                 # every batch size of a 64-camera fleet
        det._arena(n, hw)
    assert len(det._tls.arenas) == scrfd.MAX_ARENAS
