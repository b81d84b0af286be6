"""bench.py --dump-outputs: what the timed path computed in its last step, written as .npy files (float32 / float64, at most
64 MB, a fixed seeded sample of a larger view), so that two builds can be compared output for output; --steps sets the
number of timed steps and the line carries ms_per_step."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _StubContext:
    """the call dump_outputs makes, over maps whose values encode the pixel index; the engine-internal buffers (costs: NaN at
    UNKNOWN pixels) are not part of what a caller receives, so reading one fails"""

    def __init__(self, L):
        i = np.arange(L)
        self.maps = ((i * 0.5).astype(np.float32), np.stack([i, -i, 2 * i], 1).astype(np.float32), (i * 7).astype(np.uint32),
                     (i % 3).astype(np.uint8), (i % 11).astype(np.int32))

    def download_maps(self):
        return self.maps

    def get(self, name):
        raise AssertionError("dump_outputs read the engine buffer %r" % name)


def _read(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("L, cap", [(1000, 4096), (50000, 4096)])
def test_dump_outputs_sample(tmp_path, L, cap):
    bench = _bench_module()
    bench.DUMP_MAX_PIXELS = cap
    bench.dump_outputs(_StubContext(L), str(tmp_path / "a"))
    bench.dump_outputs(_StubContext(L), str(tmp_path / "b"))
    a, b = _read(str(tmp_path / "a")), _read(str(tmp_path / "b"))
    assert sorted(a) == ["depth", "normal", "pixel_index", "radius", "selected_views", "states"]
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), k                      # the sample is fixed
    idx = a["pixel_index"].astype(np.int64)
    assert idx.size == min(L, cap) and (np.diff(idx) > 0).all() and idx[-1] < L
    assert np.array_equal(a["depth"], (idx * 0.5).astype(np.float32))
    assert np.array_equal(a["normal"][:, 1], (-idx).astype(np.float32))
    assert np.array_equal(a["selected_views"], (idx * 7).astype(np.float64))
    assert np.array_equal(a["states"], (idx % 3).astype(np.float32)) and np.array_equal(a["radius"], (idx % 11).astype(np.float32))


def test_dump_outputs_size_bound():
    """the default sample stays within 64 MB: 40 bytes a pixel"""
    bench = _bench_module()
    assert bench.DUMP_MAX_PIXELS * (8 + 4 + 12 + 8 + 4 + 4) <= 64 << 20


def _run_bench(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--width", "320", "--height", "224", "--src", "4", "--no-cpu-baseline", "--no-per-iteration", "--dump-outputs", out_dir]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_dump_outputs_repeat(tmp_path):
    """two runs with the same arguments: --steps timed steps, ms_per_step in the line, the same outputs bit for bit"""
    lines = [_run_bench(str(tmp_path / tag), 3) for tag in ("a", "b")]
    for line in lines:
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        assert sum(line["launches_per_step"].values()) > 0
    a, b = _read(str(tmp_path / "a")), _read(str(tmp_path / "b"))
    assert a["pixel_index"].size == 320 * 224                  # a view this small is dumped whole
    assert (a["depth"] != 0).any()
    for k in a:
        assert a[k].dtype in (np.float32, np.float64)
        assert np.isfinite(a[k]).all(), k
        assert a[k].tobytes() == b[k].tobytes(), k
