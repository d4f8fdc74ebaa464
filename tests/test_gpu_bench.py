"""`bench.py --gpus 1 --steps K --warmup W` as a plain run: exactly K timed steps, the headline fields only, and with --dump-outputs
the outputs of the last timed step - bit for bit what one engine context returns for the same grid."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_times_k_steps_and_dumps_the_last_one(tmp_path):
    steps = 24
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["steps"] == steps and j["warmup"] == 2 and j["n_gpus"] == 1 and j["dtype"] == "f64" and j["higher_is_better"] is True
    assert j["timing"]["repeats"] == 1
    assert j["ms_per_step"] == pytest.approx(1e3 * j["timing"]["timed_region_s_median"] / steps)
    assert j["value"] == pytest.approx(j["config"]["candidates_total"] * j["config"]["replicates"] * 1e3 / j["ms_per_step"])
    assert not {"single_batch", "roofline", "cpu_baseline", "single_call", "host_abi"} & set(j)        # --full only

    got = {k: np.load(str(tmp_path / (k + ".npy"))) for k in ("llk", "jafs", "status", "candidates")}
    assert all(v.dtype == np.float64 for v in got.values())
    from misti_amd import workloads
    from misti_amd.engine import Engine, truth_spectrum
    w = workloads.config2(lambda *a: truth_spectrum(*a))
    assert np.array_equal(got["candidates"], np.arange(w.n_cand))
    with Engine(w.times, w.lh, **w.engine_kwargs()) as e:
        want = e.evaluate(w.split_time, w.params, w.jsfs)
    assert np.array_equal(got["status"], want.status)
    assert np.array_equal(got["llk"], want.llk, equal_nan=True) and np.array_equal(got["jafs"], want.jafs, equal_nan=True)
