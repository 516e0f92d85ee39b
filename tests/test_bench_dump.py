"""bench.py --dump-outputs on the host side: what one step's device outputs become on disk (masking of empty slots,
dtypes, the size cap and its seeded frame sample).  The run through the real timed loop is in test_gpu_bench_contract.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _step(frames=6, cap=4, seed=0, with_embedding=True):
    """a step's outputs as the timed path hands them on: (idx, score, dec, detect_embed_slots dict, normed rows, stream);
    empty slots hold NaN, as undefined device memory may"""
    g = torch.Generator().manual_seed(seed)
    counts = torch.randint(0, cap + 1, (frames,), generator=g, dtype=torch.int32)
    counts[0], counts[1] = 0, cap
    nan = float("nan")
    valid = torch.arange(cap)[None, :] < counts[:, None]
    r = {"counts": counts,
         "bbox": torch.where(valid[:, :, None], torch.rand((frames, cap, 4), generator=g) * 100, nan),
         "kps": torch.where(valid[:, :, None, None], torch.rand((frames, cap, 5, 2), generator=g) * 100, nan),
         "det_score": torch.where(valid, torch.rand((frames, cap), generator=g), nan)}
    rows = valid.reshape(-1)
    if with_embedding:
        r["embedding"] = torch.where(rows[:, None], torch.randn((frames * cap, 512), generator=g), nan)
    normed = torch.where(rows[:, None], torch.randn((frames * cap, 512), generator=g), nan)
    idx = torch.where(rows, torch.randint(0, 10_000_000, (frames * cap,), generator=g), 12345)
    score = torch.where(rows, torch.rand((frames * cap,), generator=g), nan)
    dec = torch.randint(0, 2, (frames * cap,), generator=g, dtype=torch.int32)
    return (idx, score, dec, r, normed, None), valid


def test_step_outputs_mask_empty_slots_and_use_float_types(bench):
    keep, valid = _step()
    out = bench.step_outputs(keep, 4)
    assert set(out) == {"counts", "bbox", "kps", "det_score", "embedding", "normed_embedding", "match_idx", "match_score",
                        "decision"}
    for k, a in out.items():
        assert a.dtype == (np.float64 if k == "match_idx" else np.float32), k
        assert np.isfinite(a).all(), k
    idx, score, dec, r, normed, _ = keep
    rows = valid.reshape(-1).numpy()
    assert out["counts"].tolist() == r["counts"].tolist()
    assert out["bbox"].shape == (6, 4, 4) and out["kps"].shape == (6, 4, 5, 2) and out["det_score"].shape == (6, 4)
    np.testing.assert_array_equal(out["bbox"][valid.numpy()], r["bbox"][valid].numpy())
    assert not out["bbox"][~valid.numpy()].any() and not out["kps"][~valid.numpy()].any()
    np.testing.assert_array_equal(out["normed_embedding"][rows], normed[valid.reshape(-1)].numpy())
    assert not out["embedding"][~rows].any()
    np.testing.assert_array_equal(out["match_idx"][rows], idx[valid.reshape(-1)].numpy().astype(np.float64))
    assert (out["match_idx"][~rows] == -1).all() and not out["decision"][~rows].any()
    # embed groups hand on the normalised rows only
    keep, _ = _step(with_embedding=False)
    assert "embedding" not in bench.step_outputs(keep, 4)


def test_dump_writes_every_array_and_samples_whole_frames_past_the_cap(bench, tmp_path, monkeypatch):
    keep, _ = _step(frames=40)
    full = bench.step_outputs(keep, 4)
    rec = bench.dump_outputs(str(tmp_path / "all"), dict(full))
    assert rec["sampled_frames"] is None and rec["files"] == sorted(k + ".npy" for k in full)
    for k, a in full.items():
        np.testing.assert_array_equal(np.load(tmp_path / "all" / (k + ".npy")), a)

    monkeypatch.setattr(bench, "DUMP_BYTES", (1 << 16) + 100_000)
    rec = bench.dump_outputs(str(tmp_path / "cut"), dict(full))
    files = os.listdir(tmp_path / "cut")
    assert sum(os.path.getsize(tmp_path / "cut" / f) for f in files) <= bench.DUMP_BYTES
    sample = np.load(tmp_path / "cut" / "sample_frames.npy")
    assert sample.dtype == np.float64 and 0 < sample.size < 40 and rec["sampled_frames"] == sample.size
    assert np.all(np.diff(sample) > 0)
    f = sample.astype(np.int64)
    np.testing.assert_array_equal(np.load(tmp_path / "cut" / "bbox.npy"), full["bbox"][f])
    np.testing.assert_array_equal(np.load(tmp_path / "cut" / "normed_embedding.npy"),
                                  full["normed_embedding"].reshape(40, 4, 512)[f].reshape(-1, 512))
    # the sample is fixed: the same frames on every run
    bench.dump_outputs(str(tmp_path / "again"), dict(full))
    np.testing.assert_array_equal(np.load(tmp_path / "again" / "sample_frames.npy"), sample)


def test_bench_rejects_a_step_count_below_one(bench, monkeypatch):
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2
