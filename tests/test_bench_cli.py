"""bench.py without a GPU: which instance and batch copy computes the last timed step, the coefficient sample and the float64 encoding of
--dump-outputs, and the arguments refused before anything touches a device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dealt(steps, batch, streams):
    """(instance, copy) of every hmult in the order run() in bench.main() enqueues them: full launches of `batch` ops round-robin over the
    instances, then the remainder one op at a time on the one-op instance ("tail")"""
    order = []
    for i in range(steps // batch):
        order += [(i % streams, c) for c in range(batch)]
    order += [("tail", 0)] * (steps % batch)
    return order


@pytest.mark.parametrize("streams", [1, 2, 3])
def test_last_step_is_the_last_op_enqueued(streams):
    ops = list(range(streams))
    for steps in range(1, 61):
        for batch in {bench.pick_batch(steps, streams), 1, 4}:
            order = dealt(steps, batch, streams)
            assert len(order) == steps
            inst, copy = bench.last_step(ops, "tail", steps, batch, streams)
            assert (inst, copy) == order[-1], (steps, batch, streams)


@pytest.mark.parametrize("n_limbs", [34, 35, 50])   # hmult (l - 1 after the rescale), hrotate (l), a wider buffer
def test_dump_columns_fit_the_cap_and_never_change(n_limbs):
    N = 1 << 16
    cols = bench.dump_columns(n_limbs, N)
    assert 2 * n_limbs * len(cols) * 2 * 8 <= bench.DUMP_LIMIT_BYTES < 64_000_000
    assert len(cols) >= N // 4 and np.all(np.diff(cols) > 0) and cols[0] >= 0 and cols[-1] < N
    assert np.array_equal(cols, bench.dump_columns(n_limbs, N))


def test_small_outputs_are_written_whole():
    assert np.array_equal(bench.dump_columns(5, 1 << 10), np.arange(1 << 10))


class _FakeOp:
    """stands in for host.Op: read() returns fixed residues below 2^60"""

    def __init__(self, n_limbs, N):
        rng = np.random.default_rng(7)
        self.bufs = {name: rng.integers(0, 1 << 60, size=(n_limbs, N), dtype=np.uint64) for name in bench.OUTPUT_BUFFERS}

    def read(self, name, copy=0):
        assert copy == 3
        return self.bufs[name].copy()


def test_dump_outputs_writes_exact_float64_halves(tmp_path):
    op = _FakeOp(34, 1 << 16)
    names = bench.dump_outputs(str(tmp_path / "out"), op, 3)
    assert names == ["out_c0_hi", "out_c0_lo", "out_c1_hi", "out_c1_lo"]
    files = sorted((tmp_path / "out").iterdir())
    assert [f.name for f in files] == [n + ".npy" for n in names]
    assert sum(f.stat().st_size for f in files) <= 64_000_000
    cols = bench.dump_columns(34, 1 << 16)
    for name in bench.OUTPUT_BUFFERS:
        base = tmp_path / "out" / name.replace(".", "_")
        hi, lo = np.load(f"{base}_hi.npy"), np.load(f"{base}_lo.npy")
        assert hi.dtype == lo.dtype == np.float64 and hi.shape == lo.shape == (34, len(cols))
        got = (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)
        assert np.array_equal(got, op.bufs[name][:, cols])


def test_bench_refuses_a_step_count_below_one():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr


def test_bench_names_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs DIR" in r.stdout
