"""bench.py's host-side pieces on CPU: the output dump (--dump-outputs) and the argument checks."""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def _bench():
    spec = importlib.util.spec_from_file_location("bench_for_test", ROOT / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_outputs_whole_small_and_seeded_sample_of_large(tmp_path):
    torch = pytest.importorskip("torch")
    bench = _bench()
    small = torch.arange(2 * 3 * 4, dtype=torch.uint8).reshape(2, 3, 4)
    large = torch.from_numpy(np.random.default_rng(7).integers(0, 256, bench.DUMP_SAMPLE + 12345, dtype=np.uint8))
    for run in ("a", "b"):
        bench.dump_outputs(tmp_path / run, {"small": small, "large": large})
    got = np.load(tmp_path / "a" / "small.npy")
    assert got.dtype == np.float32 and got.shape == (2, 3, 4) and np.array_equal(got, small.numpy())
    a, b = np.load(tmp_path / "a" / "large.npy"), np.load(tmp_path / "b" / "large.npy")
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_SAMPLE,) and np.array_equal(a, b)   # same positions in every run
    idx = np.sort(np.random.default_rng(0).integers(0, large.numel(), bench.DUMP_SAMPLE, dtype=np.int64))
    assert np.array_equal(a, large.numpy()[idx])
    # the two arrays bench.py dumps, each at most DUMP_SAMPLE float32 elements, stay within 64 MB
    assert 2 * (tmp_path / "a" / "large.npy").stat().st_size <= 64 * 10 ** 6


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_rejects_no_timed_steps(monkeypatch, argv):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1"] + argv)
    with pytest.raises(SystemExit):
        bench.parse()


def test_bench_plain_by_default_full_on_request(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    args = bench.parse()
    assert args.steps == 5 and args.warmup == 2 and not args.full and args.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    args = bench.parse()
    assert args.full and args.dump_outputs == "out"
