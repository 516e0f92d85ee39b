"""The detector's host plan, pinned as the list of C calls it issues: an eager few-frame ``detect_batch`` records its launches
(function id, argument slots, patched roles) for fr_detect_sequence, and that list - reduced to what does not change from run
to run - equals tests/golden/detect_calls.json, written by the commit before the host plan was split into stages.  Launches,
their order, the side streams' fork / join notes and every small-integer argument (shapes, caps, level counts, layer ids) are
compared by value; pointers, handles and float bit patterns only as "large"."""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("shape", [(1, 96, 128), (3, 96, 128)])
def test_recorded_call_list_equals_the_pinned_one(shape):
    sys.path.insert(0, GOLDEN)
    from make_detect_calls import capture
    with open(os.path.join(GOLDEN, "detect_calls.json")) as f:
        want = json.load(f)["%dx%dx%d" % shape]
    got, replays, second, third = capture(*shape)
    assert replays == 1                                         # the third call replayed the list the second recorded ...
    assert torch.equal(second[3], third[3])                     # ... and returns its tensors bit for bit: the counts
    for f, n in enumerate(second[3].tolist()):                                  # and every slot that holds a face (the rest is not written)
        assert all(torch.equal(a[f, :n], b[f, :n]) for a, b in zip(second[:3], third[:3]))
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "call %d: got %s, pinned %s" % (k, g, w)
