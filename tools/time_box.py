#!/usr/bin/env python3
"""Does a rate cap shorten the straggler tail of config 3's search?  BASELINE config 3's 16 384 random starts, once without a box
(misti_nm_solve_rows) and once inside hi = CAP x the true rates (misti_nm_solve_box with a split per start: the same rows path, the
same starts, split and data row), on one GPU.  A timing tool: nothing asserts its numbers, and the cap is a modelling choice - no
default follows from it.

Each search is warmed up with an untimed call of the same size and then timed once (--repeat for more); a timed call ends in the
library's own stream synchronise.  The JSON lines carry every repetition, the number of starts that end on the iteration cap
(status 2: the stragglers), the iterations issued and the build id.

    python tools/time_box.py [--starts 16384] [--cap 100] [--repeat 1] [--out profiles/box_timing.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TRUE_RATES = (0.2, 0.05)            # workloads.config3's band_truth


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--starts", type=int, default=16384)
    ap.add_argument("--cap", type=float, default=100.0, help="upper bound of every rate, in units of its true value")
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from misti_amd import _lib, workloads
    from misti_amd.engine import Engine, truth_spectrum
    w = workloads.config3(lambda *x: truth_spectrum(*x), n_start=a.starts)
    S = w.n_cand
    rows = np.zeros(S, dtype=np.int32)
    hi = a.cap * np.array(TRUE_RATES)
    box = (np.full(2, -np.inf), hi)
    lines = []
    with Engine(w.times, w.lh, **w.engine_kwargs()) as e:
        calls = (("no box (misti_nm_solve_rows)", None, lambda: e.nm_solve_rows(w.params, w.split_time, rows, w.jsfs, tol=1e-4, maxiter=1000)),
                 ("hi = %g x the true rates (misti_nm_solve_box)" % a.cap, [float(v) for v in hi],
                  lambda: e.nm_solve_box(w.params, rows, w.jsfs, box, split_times=w.split_time, tol=1e-4, maxiter=1000)))
        for what, cap, call in calls:
            call()                                                       # warm-up at the timed size
            ts, r = [], None
            for _ in range(a.repeat):
                t, r = timed(call)
                ts.append(round(t, 4))
            finite = np.isfinite(r["llh"])
            lines.append(dict(what="config 3, %d random starts, %s" % (S, what), build_id=_lib.build_id(), starts=S, upper_bounds=cap,
                              seconds=ts, starts_at_status_2=int((r["status"] == 2).sum()), starts_converged=int((r["status"] == 0).sum()),
                              starts_without_a_value=int((~finite).sum()), iterations_issued=r["iterations_issued"], slots=r["slots"],
                              speculative_iterations=r["speculative_iterations"], best_llh=float(r["llh"][finite].max()) if finite.any() else None,
                              starts_ending_on_the_cap=None if cap is None else int((r["x"] == hi).any(axis=1).sum())))
    for line in lines:
        print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
