"""Lanes dealt over the stream-priority levels (misti_lanes.cpp: lane_plan): where a lane's stream lives changes no bit of its results,
and the levels are what the plan says for the queue limit the process runs under.

The HIP runtime reads GPU_MAX_HW_QUEUES when it initialises, so every case is a fresh child process (this file run as a script), one
at a time.  Shape: six lanes on a numT = 32 grid of 8 splits x 8 rates (8 chains and a trunk), two batches per lane issued round-robin,
against one plain context on the same inputs.  No rate is asserted: a shared test box is not a benchmark box."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

N_LANES = 6


def child():
    import ctypes as C
    import numpy as np
    import torch
    from misti_amd import _lib, synth
    from misti_amd.engine import Engine, Lanes
    inp = synth.psmc_pair(16, 17)
    times, lh, _ = synth.self_consistent(inp, 20, [[1, 4, 20, 0.2, 0]], [])
    kw = dict(bands=[(0, 4, -1, 0.0, 0)], n_param=1, cpfit=True, smooth=True)
    st, rr = np.meshgrid(np.arange(16, 24, dtype=np.float64), np.logspace(-3, np.log10(0.5), 8), indexing="ij")
    split, rates = st.ravel().copy(), rr.ravel()[:, None].copy()
    rows = np.array([[3e7, 9000, 2500, 10000, 6000, 4000, 2600, 4100], [2.9e7, 9100, 2400, 10100, 6100, 3900, 2500, 4000]])
    n, R, K = split.size, rows.shape[0], 2 * N_LANES
    params = [rates * (1.0 + 0.05 * k) for k in range(K)]             # every batch its own grid
    with Engine(times, lh, **kw) as e:
        want = [e.evaluate(split, p, rows) for p in params]
    dev = torch.device("cuda", 0)
    d_split = torch.as_tensor(split, device=dev)
    d_rows = torch.as_tensor(rows, device=dev).contiguous()
    d_par = [torch.as_tensor(p, device=dev).contiguous() for p in params]
    llk = [torch.empty((n, R), dtype=torch.float64, device=dev) for _ in range(K)]
    jafs = [torch.empty((n, 7), dtype=torch.float64, device=dev) for _ in range(K)]
    status = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(K)]
    torch.cuda.synchronize()
    with Lanes(times, lh, lanes=N_LANES, **kw) as pool:
        levels = [pool.level(i) for i in range(pool.n_lanes)]
        for k in range(K):                                             # round-robin, nothing waited for in between
            pool.evaluate_dev(k % N_LANES, n, d_split.data_ptr(), d_par[k].data_ptr(), R, d_rows.data_ptr(), llk[k].data_ptr(), jafs[k].data_ptr(), 0, 0,
                              status[k].data_ptr())
        pool.sync()
        priorities = [torch.cuda.ExternalStream(pool.engine(i).stream_handle(), device=dev).priority for i in range(pool.n_lanes)]
    same = [bool(np.array_equal(llk[k].cpu().numpy(), want[k].llk, equal_nan=True) and np.array_equal(jafs[k].cpu().numpy(), want[k].jafs, equal_nan=True)
                 and np.array_equal(status[k].cpu().numpy(), want[k].status)) for k in range(K)]
    least, greatest = torch.cuda.Stream.priority_range()
    n_levels = least - greatest + 1
    lib = _lib.load()
    plan = (C.c_int * N_LANES)()
    assert lib.misti_lane_plan_(N_LANES, 0, n_levels, 22, plan) == 0
    print(json.dumps(dict(levels=levels, plan=list(plan), n_levels=n_levels, priorities=priorities, same=same,
                          ok=int(sum(int((w.status == 0).sum()) for w in want)), finite=int(sum(int(np.isfinite(w.llk).sum()) for w in want)))))


def run_case(env):
    e = {k: v for k, v in os.environ.items() if k not in ("GPU_MAX_HW_QUEUES", "MISTI_LANE_PRIORITIES", "MISTI_KEEP_HW_QUEUES")}
    e.update(env)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e["PYTHONPATH"] = root + os.pathsep + e.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=300, env=e)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def check_results(out):
    assert len(out["same"]) == 2 * N_LANES and all(out["same"]), out          # bit for bit one plain context's, every batch of every lane
    assert out["finite"] > 0 and out["ok"] > 0                               # ... and that was a computation, not a table of failures
    assert out["levels"] == out["plan"] and all(0 <= l < out["n_levels"] for l in out["levels"])


def test_four_queues_spread_the_lanes_over_the_levels():
    out = run_case({"GPU_MAX_HW_QUEUES": "4"})
    check_results(out)
    assert out["n_levels"] > 1, "this device reports one stream priority"
    assert len(set(out["levels"])) > 1
    assert out["levels"].count(0) == 4                                       # the default level is filled first
    assert len(set(out["priorities"])) == len(set(out["levels"]))            # the streams really are on different priorities
    assert all(p == 0 for p, l in zip(out["priorities"], out["levels"]) if l == 0)


def test_twenty_two_queues_keep_one_level():
    out = run_case({"GPU_MAX_HW_QUEUES": "22"})
    check_results(out)
    assert out["levels"] == [0] * N_LANES and out["priorities"] == [0] * N_LANES


def test_lane_priorities_can_be_switched_off():
    out = run_case({"GPU_MAX_HW_QUEUES": "4", "MISTI_LANE_PRIORITIES": "0"})
    check_results(out)
    assert out["levels"] == [0] * N_LANES and out["priorities"] == [0] * N_LANES


if __name__ == "__main__" and "--child" in sys.argv:
    child()
