#!/usr/bin/env python3
"""What a bootstrap table costs: REPS block-bootstrap replicates of a CHUNKS-chunk JSFS on the device (misti_bootstrap_rows_dev) against
the two host statements - io.bootstrap_table (the reference's resampler: a Python loop under the Mersenne Twister, one interpreter
iteration per drawn chunk) and optimize.block_bootstrap (the device's rule in NumPy).  A timing tool: nothing asserts its numbers.

The device leg writes into one preallocated buffer; every window is one call followed by the library's own stream synchronise, after
a warm-up call of the same size: the median, lowest and highest of --windows windows.  The host legs run --host-reps replicates once
and are SCALED to REPS (their cost per replicate does not depend on how many are drawn).  The device rows are compared with
block_bootstrap's on the replicates both made.  --chunks takes several sizes: tables beyond 1 024 chunks are read from global memory.

    python tools/time_bootstrap_rows.py [--chunks 1000] [--reps 100000] [--host-reps 1000] [--windows 7] [--out profiles/bootstrap_rows_timing.jsonl]"""
import argparse
import ctypes as C
import io
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def chunk_table(n_chunk, seed=1):
    """Chunks of about 10 000 sites with integer class counts, as a JSFS file has them."""
    rng = np.random.default_rng(seed)
    c = np.zeros((n_chunk, 8))
    c[:, 1:] = rng.integers(0, 300, size=(n_chunk, 7))
    c[:, 0] = c[:, 1:].sum(axis=1) + rng.integers(8000, 12000, size=n_chunk)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, nargs="+", default=[1000])
    ap.add_argument("--reps", type=int, default=100000)
    ap.add_argument("--host-reps", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from misti_amd import _lib, io as mio, synth
    from misti_amd.engine import Engine
    from misti_amd.optimize import block_bootstrap
    inp = mio.merge_psmc(mio.read_psmc_file(io.StringIO(synth.psmc_text(16, 1, synth.THETA_1))),
                         mio.read_psmc_file(io.StringIO(synth.psmc_text(17, 2, synth.THETA_2))))
    dev = torch.device("cuda", 0)
    lines = []
    with Engine(inp.times, inp.lambdas) as e:
        for n_chunk in a.chunks:
            c = chunk_table(n_chunk)
            rows = torch.empty((a.reps, 8), dtype=torch.float64, device=dev)
            draws = torch.empty(a.reps, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()

            def call():
                _lib.check(e._lib.misti_bootstrap_rows_dev(e._ctx, n_chunk, c.ctypes.data_as(C.c_void_p), C.c_uint64(0), 0, a.reps, 0,
                                                           C.c_void_p(rows.data_ptr()), C.c_void_p(draws.data_ptr())))
                e.sync()
            call()                                                       # warm-up at the timed size
            ts = []
            for _ in range(a.windows):
                t0 = time.perf_counter()
                call()
                ts.append(time.perf_counter() - t0)
            n_host = min(a.host_reps, a.reps)
            t0 = time.perf_counter()
            want = block_bootstrap(c, n_host, seed=0)
            t_numpy = time.perf_counter() - t0
            same = bool(np.array_equal(rows[:n_host].cpu().numpy(), want))
            as_lists = [list(map(float, r)) for r in c]
            random.seed(0)
            t0 = time.perf_counter()
            mio.bootstrap_table(as_lists, n_host)
            t_loop = time.perf_counter() - t0
            total_draws = int(draws.sum(dtype=torch.int64).item())
            lines.append(dict(what="%d replicates of a %d-chunk table" % (a.reps, n_chunk), build_id=_lib.build_id(), chunks=n_chunk, reps=a.reps,
                              path="LDS" if n_chunk <= 1024 else "global", draws=total_draws,
                              device_seconds=dict(median=round(float(np.median(ts)), 6), lowest=round(min(ts), 6), highest=round(max(ts), 6), windows=a.windows),
                              device_draws_per_second=round(total_draws / float(np.median(ts))),
                              host_reps=n_host, device_rows_equal_block_bootstrap=same,
                              io_bootstrap_table_seconds=dict(measured_at_host_reps=round(t_loop, 4), scaled_to_reps=round(t_loop * a.reps / n_host, 2)),
                              optimize_block_bootstrap_seconds=dict(measured_at_host_reps=round(t_numpy, 4), scaled_to_reps=round(t_numpy * a.reps / n_host, 2))))
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
