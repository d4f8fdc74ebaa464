#!/usr/bin/env python3
"""The split time fitted as a coordinate (ONE misti_nm_solve_split call) against the bootstrap profile over integer splits
(optimize.bootstrap_profile, one misti_nm_solve_rows call), on one GPU.  A timing tool: nothing asserts its numbers.

Two models, ROWS rows of a bootstrap table each (row 0 the data):
  - config 3's model (numT = 128, two optimised bands, --cpfit) with its band ends following the split: the fit runs INIT searches
    per row (initial splits 62, 64, 66 at the -mi initial rates, the best kept), the profile one search per (row, split) pair over
    SPLITS integer splits around 64;
  - config 4's model (no migration, no optimised parameter): the fit is a one-coordinate search from initial splits 48, 50, 52; it has
    no profile to compare with (a fixed-split search has nothing to optimise there), so the scan over the same SPLITS integer splits
    (optimize.bootstrap_scan_dev) stands beside it.
Every shape is warmed up with an untimed call of the same size; each timed call ends in the library's own stream synchronise; REPEAT
timed repetitions alternate between the two routes, and the JSON lines carry every repetition, the median and the build id.

    python tools/time_split_fit.py [--rows 101] [--splits 11] [--repeat 5] [--out profiles/split_fit_timing.jsonl]"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def alternate(repeat, a, b):
    """`repeat` timed calls of a and of b, alternating; (times_a, times_b, last results)."""
    ta, tb, ra, rb = [], [], None, None
    for _ in range(repeat):
        t, ra = timed(a)
        ta.append(t)
        t, rb = timed(b)
        tb.append(t)
    return ta, tb, ra, rb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=101)
    ap.add_argument("--splits", type=int, default=11)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from misti_amd import _lib, io as mio, synth, workloads
    from misti_amd.engine import Engine, truth_spectrum
    from misti_amd.optimize import bootstrap_profile, bootstrap_profile_interval, bootstrap_scan_dev, split_fit, split_fit_interval
    lines = []
    med = lambda t: round(float(np.median(t)), 4)
    r4 = lambda t: [round(float(v), 4) for v in t]

    # config 3's model, band ends following the split
    w = workloads.config3(lambda *x: truth_spectrum(*x), n_start=1)
    kw = w.engine_kwargs()
    kw["bands"] = [(p, s, -1, v, k) for p, s, e, v, k in w.bands]
    start = np.array([[b[3] for b in kw["bands"]]])
    table = np.array(mio.bootstrap_table(synth.chunk_rows(w.jsfs[0], 20), a.rows - 1, random.Random(3)), dtype=np.float64)
    splits = 64.0 + np.arange(a.splits) - a.splits // 2
    init = [62.0, 64.0, 66.0]
    with Engine(w.times, w.lh, **kw) as e:
        fit_call = lambda: split_fit(e, table, start, init)
        prof_call = lambda: bootstrap_profile(e, splits, table, start)
        fit_call(); prof_call()                                                      # warm-up at the timed sizes
        t_fit, t_prof, fit, prof = alternate(a.repeat, fit_call, prof_call)
    iv_fit = split_fit_interval(fit["split"], fit["llh"])
    iv_prof = bootstrap_profile_interval(prof["llh"], splits)
    lines.append(dict(what="config 3 model, band ends following the split", build_id=_lib.build_id(), rows=a.rows, repeat=a.repeat,
                      fit_initial_splits=init, fit_searches=a.rows * len(init), fit_s=r4(t_fit), fit_median_s=med(t_fit),
                      fit_iterations=fit["iterations_issued"], fit_speculative=fit["speculative_iterations"],
                      fit_rows_at_iteration_cap=int((fit["status"] == 2).sum()), fit_data_split=iv_fit["data_split"],
                      fit_interval_95=iv_fit["interval"], fit_rows_excluded=iv_fit["n_excluded"],
                      profile_splits=[float(s) for s in splits], profile_searches=a.rows * a.splits, profile_s=r4(t_prof),
                      profile_median_s=med(t_prof), profile_iterations=prof["iterations_issued"],
                      profile_data_split=iv_prof["data_split"], profile_interval_975=iv_prof["interval"],
                      rows_where_fit_llh_below_profile_best=int((fit["llh"] < prof["llh"].max(axis=1)).sum())))

    # config 4's model: no migration, a one-coordinate search
    w = workloads.config4(lambda *x: truth_spectrum(*x), n_split=4, n_rep=a.rows)
    splits4 = 50.0 + np.arange(a.splits) - a.splits // 2
    init4 = [48.0, 50.0, 52.0]
    with Engine(w.times, w.lh, **w.engine_kwargs()) as e:
        fit_call = lambda: split_fit(e, w.jsfs, None, init4)
        scan_call = lambda: bootstrap_scan_dev(e, splits4, w.jsfs)
        fit_call(); scan_call()
        t_fit, t_scan, fit, scan = alternate(a.repeat, fit_call, scan_call)
    iv_fit = split_fit_interval(fit["split"], fit["llh"])
    lines.append(dict(what="config 4 model, no migration (n_param = 0)", build_id=_lib.build_id(), rows=a.rows, repeat=a.repeat,
                      fit_initial_splits=init4, fit_searches=a.rows * len(init4), fit_s=r4(t_fit), fit_median_s=med(t_fit),
                      fit_iterations=fit["iterations_issued"], fit_speculative=fit["speculative_iterations"],
                      fit_rows_at_iteration_cap=int((fit["status"] == 2).sum()), fit_data_split=iv_fit["data_split"],
                      fit_interval_95=iv_fit["interval"], fit_rows_excluded=iv_fit["n_excluded"],
                      scan_splits=[float(s) for s in splits4], scan_s=r4(t_scan), scan_median_s=med(t_scan),
                      scan_mean_split=float(scan[0]), scan_interval_95=[float(v) for v in scan[1]]))
    for line in lines:
        print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
