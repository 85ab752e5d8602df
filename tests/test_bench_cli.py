"""bench.py's command line and its --dump-outputs writer (host only: the writer is fed CPU tensors)."""
import sys

import numpy as np

import bench


def _answer(n):
    import torch
    rng = np.random.default_rng(7)
    face = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    face[0] = 0xFFFFFFFF  # NO_FACE
    part = rng.integers(0, 7, n, dtype=np.uint64).astype(np.uint32)
    point = rng.normal(size=(n, 3))
    return (face, part, point), (torch.from_numpy(face.view(np.int32)), torch.from_numpy(part.view(np.int32)),
                                 torch.from_numpy(point))


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert (a.gpus, a.steps, a.warmup) == (1, 3, 1)
    assert a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_whole_answer(tmp_path):
    (face, part, point), t = _answer(1000)
    bench.dump_outputs(str(tmp_path / "d"), *t)
    got = {n: np.load(str(tmp_path / "d" / (n + ".npy"))) for n in ("face", "part", "point")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["face"][0] == 4294967295.0
    assert np.array_equal(got["face"], face.astype(np.float64))
    assert np.array_equal(got["part"], part.astype(np.float64))
    assert np.array_equal(got["point"], point)


def test_dump_outputs_sample_is_fixed(tmp_path, monkeypatch):
    assert 5 * 8 * bench.DUMP_ROWS <= 64 << 20  # face + part + 3 point columns, float64
    monkeypatch.setattr(bench, "DUMP_ROWS", 500)
    (face, part, point), t = _answer(4000)
    bench.dump_outputs(str(tmp_path / "a"), *t)
    bench.dump_outputs(str(tmp_path / "b"), *t)
    for n in ("face", "part", "point"):
        a, b = np.load(str(tmp_path / "a" / (n + ".npy"))), np.load(str(tmp_path / "b" / (n + ".npy")))
        assert a.shape[0] == 500 and np.array_equal(a, b)
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(4000, 500, replace=False, shuffle=False))
    assert np.unique(idx).size == 500
    assert np.array_equal(np.load(str(tmp_path / "a" / "face.npy")), face[idx].astype(np.float64))
    assert np.array_equal(np.load(str(tmp_path / "a" / "point.npy")), point[idx])
