"""The embed net's host, pinned as the list of C calls a forward issues in every batch-size mode: the calls recorded on this
build - reduced to what does not change from run to run (tests/golden/make_embed_calls.py) - equal tests/golden/embed_calls.json,
written by the commit before the host got its route table.  Entry points, their order, every integer argument and struct field,
which pointers are set and, in a replayed sequence, which plan buffer at which offset each step reads and writes; a profiled
forward also its (variant, flops) list, the strings bench.py's roofline block keys on.  Identical calls into an identical
library: the embeddings are that commit's bit for bit."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLDEN)
import make_embed_calls as mec  # noqa: E402


@pytest.fixture(scope="module")
def pinned():
    with open(os.path.join(GOLDEN, "embed_calls.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def nets():
    return mec.build_nets()


def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s %d: got %s, pinned %s" % (what, k, g, w)


@pytest.mark.parametrize("case", list(mec.CASES))
def test_forward_issues_the_pinned_calls(nets, pinned, case):
    assert mec.fp8_convs(nets[True]) == pinned["fp8_convs"] and (nets[True].stage14_f8 is not None) == pinned["stage14_f8"]
    calls, prof = mec.capture(nets, case)
    want = pinned["cases"][case]
    _same(calls, mec.unrle(want["calls"]), "call")
    assert (prof is None) == ("profile" not in want)
    if prof is not None:
        _same(prof, mec.unrle(want["profile"]), "launch")


def test_r100_profiled_forward_names_the_pinned_kernels(pinned):
    """256 faces through the synthetic r100, profiled: the (variant, flops) list of bench.py's instrumented pass"""
    _, prof = mec.record(mec.build_r100(), mec.crops(256, 356), True)
    _same(prof, mec.unrle(pinned["cases"][mec.R100_CASE]["profile"]), "launch")
