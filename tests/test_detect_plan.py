"""The detector's launch plan as a pure function (mtcnn.detect_plan): which arithmetic, which launches, which streams and which
groups of frames a detect_batch call takes, from its frame shape and the settings alone - no library, no device."""
import pytest

from facerecognition_infrenceengine_amd.mtcnn import DetectSettings, detect_plan

# frames (N, H, W) -> levels, batch, few, levels with conv1 on the f16 matrix cores, chunk sizes: default settings, no trace, not
# capturing (computed from the detect_batch that decided all this inline)
TABLE = [((1, 11, 40), 0, False, True, 0, ()),
         ((1, 20, 20), 1, False, True, 0, ()),
         ((1, 480, 640), 10, False, True, 0, ()),
         ((7, 1080, 1920), 12, False, True, 0, ()),
         ((8, 1080, 1920), 12, False, False, 0, ()),
         ((10, 1080, 1920), 12, False, False, 0, ()),
         ((11, 1080, 1920), 12, True, False, 5, ()),
         ((64, 1080, 1920), 12, True, False, 5, ()),
         ((2, 2160, 3840), 14, False, True, 0, ()),
         ((3, 2160, 3840), 14, True, False, 7, ()),
         ((45, 2160, 3840), 14, True, False, 7, ()),
         ((46, 2160, 3840), 14, True, False, 7, (23, 23)),
         ((64, 2160, 3840), 14, True, False, 7, (32, 32)),
         ((128, 2160, 3840), 14, True, False, 7, (43, 43, 42)),
         ((1, 6000, 4000), 16, True, False, 8, ())]


@pytest.mark.parametrize("shape,levels,batch,few,f16,chunks", TABLE)
def test_default_plan(shape, levels, batch, few, f16, chunks):
    p = detect_plan(*shape, DetectSettings())
    assert len(p.scales) == len(p.geo) == len(p.fused) == len(p.f16) == levels
    assert (p.batch, p.few, sum(p.f16)) == (batch, few, f16)
    assert tuple(n1 - n0 for n0, n1 in p.chunks) == chunks
    assert not chunks or (p.chunks[0][0] == 0 and p.chunks[-1][1] == shape[0]
                          and all(a[1] == b[0] for a, b in zip(p.chunks, p.chunks[1:])))
    if levels:
        assert p.pyramid == batch                       # one launch per layer over the whole pyramid: exactly the batches
        assert p.band == batch and p.split == batch
    # few frames, eagerly: one stream, the tensor cache and the recorder; 8 and 10 x 1080p: neither few nor a batch, two side streams
    assert p.solo == (few or p.pyramid) and (p.cache, p.recorder) == (few, few)
    assert p.nside == 2
    assert all(p.fused)                                 # (no level past the 32-bit offsets: such a call is cut)
    assert all(f <= u for f, u in zip(p.f16, p.fused))


def test_pyramid_forces_solo():
    s = DetectSettings()
    for shape in ((11, 1080, 1920), (3, 2160, 3840)):
        for kw in ({}, {"level_streams": 2}, {"capturing": True}):
            p = detect_plan(*shape, s, **kw)
            assert p.pyramid and p.solo
    s.pyramid_launch = False
    p = detect_plan(11, 1080, 1920, s)
    assert not p.pyramid and not p.solo and p.nside == 2 and sum(p.f16) == 5


def test_capturing_single_frame_takes_a_stream_per_level_up_to_four():
    s = DetectSettings()
    p = detect_plan(1, 480, 640, s, capturing=True)
    assert not p.solo and p.nside == 4 and not p.cache and not p.recorder
    assert detect_plan(1, 20, 20, s, capturing=True).nside == 1               # one level: nothing to deal out
    assert detect_plan(1, 96, 128, s, capturing=True).nside == 4              # five levels: one stream for each of 1 .. 4
    s.single_frame_level_streams = 0                                          # 0: as level_streams
    assert detect_plan(1, 480, 640, s, capturing=True).nside == 2
    p = detect_plan(8, 1080, 1920, DetectSettings(), capturing=True)          # not few: the level streams as in an eager call
    assert not p.solo and p.nside == 2


def test_trace_forces_one_stream_and_the_f32_forms():
    s = DetectSettings()
    for shape in ((1, 480, 640), (11, 1080, 1920), (64, 2160, 3840)):
        p = detect_plan(*shape, s, trace=True)
        assert p.solo and not p.pyramid and not p.split and not p.band and not p.chunks and not any(p.f16)
        assert not p.cache and not p.recorder
        assert p.batch == detect_plan(*shape, s).batch


def test_one_stream_forces_solo_and_no_recorder():
    s = DetectSettings()
    s.one_stream = True
    p = detect_plan(1, 480, 640, s)
    assert p.solo and p.cache and not p.recorder
    assert detect_plan(8, 1080, 1920, s).solo and detect_plan(1, 480, 640, s, capturing=True).solo


def test_level_streams_argument():
    s = DetectSettings()
    assert detect_plan(8, 1080, 1920, s, level_streams=1).nside == 1
    assert detect_plan(8, 1080, 1920, s, level_streams=5).nside == 2
    p = detect_plan(1, 480, 640, s, level_streams=1)                          # a few-frame call told its streams: not solo, no cache
    assert p.nside == 1 and not p.solo and not p.cache and not p.recorder
    s.level_streams = 1
    assert detect_plan(8, 1080, 1920, s).nside == 1


def test_unfused_pnet_turns_pyramid_chunks_and_recorder_off():
    s = DetectSettings(fused_pnet=False)
    for shape in ((1, 480, 640), (11, 1080, 1920), (64, 2160, 3840)):
        p = detect_plan(*shape, s)
        assert not p.pyramid and not p.chunks and not p.recorder and not any(p.fused) and not any(p.f16)
    assert detect_plan(1, 480, 640, s).cache


def test_a_chunk_is_planned_for_itself():
    s = DetectSettings()
    whole = detect_plan(64, 2160, 3840, s)
    part = detect_plan(32, 2160, 3840, s, out=True)
    assert whole.chunks == ((0, 32), (32, 64)) and (whole.fused, whole.f16) == (part.fused, part.f16)
    assert not part.chunks and all(part.fused) and part.pyramid and part.batch and sum(part.f16) == 7
    assert not detect_plan(64, 2160, 3840, s, out=True).chunks                # a group of frames is never cut again
    assert not detect_plan(2, 480, 640, s, out=True).cache                    # and never cached or recorded


def test_other_switches_the_plan_reads():
    s = DetectSettings(batch_min_pixels=0)
    p = detect_plan(1, 96, 128, s)
    assert p.batch and not p.few and p.pyramid and p.split and not p.cache and sum(p.f16) == 0
    s.split_pconv1_min_px = 25
    assert sum(detect_plan(1, 96, 128, s).f16) == 5
    s.pnet_band = s.split_ro = False                                          # set_exact()
    p = detect_plan(1, 96, 128, s)
    assert not p.band and not p.split and not any(p.f16) and p.pyramid
    s = DetectSettings()
    s.fused_crop = False
    assert not detect_plan(11, 1080, 1920, s).split and not detect_plan(1, 480, 640, s).recorder
    s = DetectSettings()
    s.use_sequence = False
    p = detect_plan(1, 480, 640, s)
    assert p.cache and not p.recorder
    s = DetectSettings()
    s.phase_marks = []
    assert not detect_plan(1, 480, 640, s).recorder
