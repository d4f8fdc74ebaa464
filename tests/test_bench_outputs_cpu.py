"""`bench.py --dump-outputs DIR`: what the files hold and how a large output is cut down (the GPU run itself: tests/test_gpu_bench.py)."""
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT


def _dump(out, n, limit):
    """bench.dump_outputs on n rows of made-up outputs with the size limit set to `limit`, in a process of its own."""
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import bench; bench.DUMP_MAX_BYTES = %d; n = %d; "
            "bench.dump_outputs(%r, {'llk': np.arange(2.0 * n).reshape(n, 2), 'status': np.arange(n, dtype=np.int32), 'candidates': np.arange(n)})"
            % (ROOT, limit, n, str(out)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT, timeout=120)
    return {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}


def test_small_outputs_are_written_whole_in_float64(tmp_path):
    d = _dump(tmp_path, 100, 64 << 20)
    assert sorted(d) == ["candidates", "llk", "status"]
    assert all(v.dtype == np.float64 for v in d.values())
    assert np.array_equal(d["llk"], np.arange(200.0).reshape(100, 2))
    assert np.array_equal(d["status"], np.arange(100.0)) and np.array_equal(d["candidates"], np.arange(100.0))


def test_large_outputs_are_a_fixed_sample_within_the_limit(tmp_path):
    limit = 64 * 1024
    a = _dump(tmp_path / "a", 10000, limit)
    b = _dump(tmp_path / "b", 10000, limit)
    assert sorted(a) == ["candidates", "llk", "rows", "status"]
    assert sum(os.path.getsize(os.path.join(tmp_path / "a", f)) for f in os.listdir(tmp_path / "a")) <= limit
    rows = a["rows"].astype(np.int64)
    assert len(rows) > 1000 and np.all(np.diff(rows) > 0)
    assert np.array_equal(a["llk"], np.arange(20000.0).reshape(10000, 2)[rows])
    assert np.array_equal(a["status"], rows.astype(np.float64)) and np.array_equal(a["candidates"], rows.astype(np.float64))
    assert all(np.array_equal(a[k], b[k]) for k in a)               # the same sample on every run
