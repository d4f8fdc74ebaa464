#!/usr/bin/env python3
"""What parametric-bootstrap replicates cost: REPS replicates of SITES sites drawn from one spectrum on the device
(misti_parametric_rows_dev) against the only alternative that exists, the rule in NumPy on the host (optimize.parametric_rows).
A timing tool: nothing asserts its numbers.

The device leg writes into one preallocated buffer; every window is one call followed by the library's own stream synchronise, after
a warm-up call of the same size: the median, lowest and highest of --windows windows, and draws per second at the median.  The host
leg runs --host-draws draws' worth of whole replicates once (at least one replicate) and is SCALED to the shape (its cost per draw does
not depend on how many replicates are drawn); the device rows are compared with the host's on the replicates both made.  Shapes are
REPS x SITES pairs; the default is the three of DESIGN.md section 6.

    python tools/time_parametric_rows.py [--shapes 1000x1000000 1000x5000000 1x1073741824] [--host-draws 20000000] [--windows 5]
                                         [--out profiles/parametric_rows_timing.jsonl]"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SPECTRUM = [.3, .05, .2, .1, .15, .08, .12]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1000x1000000", "1000x5000000", "1x1073741824"], metavar="REPSxSITES")
    ap.add_argument("--host-draws", type=int, default=20000000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from misti_amd import _lib, io as mio, synth
    from misti_amd.engine import Engine
    from misti_amd.optimize import parametric_rows
    inp = mio.merge_psmc(mio.read_psmc_file(io.StringIO(synth.psmc_text(16, 1, synth.THETA_1))),
                         mio.read_psmc_file(io.StringIO(synth.psmc_text(17, 2, synth.THETA_2))))
    dev = torch.device("cuda", 0)
    lines = []
    with Engine(inp.times, inp.lambdas) as e:
        sp = torch.as_tensor(np.array(SPECTRUM), device=dev)
        for shape in a.shapes:
            reps, sites = (int(v) for v in shape.lower().split("x"))
            rows = torch.empty((reps, 8), dtype=torch.float64, device=dev)
            status = torch.empty(reps, dtype=torch.int32, device=dev)
            bpr = C.c_int32(0)
            _lib.check(e._lib.misti_parametric_geometry(sites, reps, C.byref(bpr)))
            torch.cuda.synchronize()

            def call():
                _lib.check(e._lib.misti_parametric_rows_dev(e._ctx, 1, C.c_void_p(sp.data_ptr()), None, None, 1.0, sites, C.c_uint64(0), 0, reps,
                                                            C.c_void_p(rows.data_ptr()), C.c_void_p(status.data_ptr())))
                e.sync()
            call()                                                       # warm-up at the timed size
            ts = []
            for _ in range(a.windows):
                t0 = time.perf_counter()
                call()
                ts.append(time.perf_counter() - t0)
            n_host = max(1, min(reps, a.host_draws // max(sites, 1)))
            t0 = time.perf_counter()
            want, _ = parametric_rows([SPECTRUM], n_host, sites, 1.0, seed=0)
            t_numpy = time.perf_counter() - t0
            same = bool(np.array_equal(rows[:n_host].cpu().numpy(), want)) and not bool(status.any().item())
            draws, med = reps * sites, float(np.median(ts))
            lines.append(dict(what="%d replicates of %d sites" % (reps, sites), build_id=_lib.build_id(), reps=reps, sites=sites, draws=draws,
                              blocks_per_rep=bpr.value,
                              device_seconds=dict(median=round(med, 6), lowest=round(min(ts), 6), highest=round(max(ts), 6), windows=a.windows),
                              device_draws_per_second=round(draws / med), host_reps=n_host, device_rows_equal_parametric_rows=same,
                              optimize_parametric_rows_seconds=dict(measured_at_host_reps=round(t_numpy, 4), scaled_to_reps=round(t_numpy * reps / n_host, 2)),
                              host_draws_per_second=round(n_host * sites / t_numpy)))
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
