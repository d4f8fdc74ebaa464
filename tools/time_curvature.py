#!/usr/bin/env python3
"""What the curvature at a fit costs (Engine.curvature: one stencil of 1 + 2 n^2 evaluations per point) against the cost it
replaces: one search per bootstrap row (Engine.nm_solve_rows over 100 rows), on one GPU.

Config 3's headline model (numT = 128, two optimised bands, --cpfit; D = 2, so 9 candidates per point), the split at 64, a bootstrap
table of 1 + 100 rows.  Timed: `curvature` for 1 point and for 100 points (each at its own row), and `nm_solve_rows` from the -mi
initial values against rows 1 ... 100.  Every figure is the median of REPEATS calls after a warm-up call of the same shape, host clock
around a synchronous call (the calls end in a stream synchronise); the spread (min, max) is kept beside it.  The sandwich standard
errors of the data row are printed beside the standard deviation of the 100 refits: for a reader to compare, not a check.
`--skip-curvature` times only the searches (what a build without misti_curvature can do: the baseline on the parent commit).

    python tools/time_curvature.py [--repeats 7] [--rows 101] [--out FILE] [--skip-curvature]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(call, repeats):
    call()                                                                            # warm-up: allocations, code objects
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = call()
        ts.append(time.perf_counter() - t0)
    return dict(median_s=round(statistics.median(ts), 6), min_s=round(min(ts), 6), max_s=round(max(ts), 6), repeats=repeats), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rows", type=int, default=101)
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-curvature", action="store_true")
    a = ap.parse_args()
    from misti_amd import _lib, io as mio, synth, workloads
    from misti_amd.engine import Engine, truth_spectrum
    w = workloads.config3(lambda *x: truth_spectrum(*x), n_start=1)
    kw = w.engine_kwargs()
    kw["bands"] = [(p, s, -1, v, k) for p, s, e, v, k in w.bands]
    start = np.array([b[3] for b in kw["bands"]])
    table = np.array(mio.bootstrap_table(synth.chunk_rows(w.jsfs[0], 20), a.rows - 1, random.Random(3)), dtype=np.float64)
    B = a.rows - 1
    split = 64.0
    line = dict(what="curvature at a fit against one search per bootstrap row; config 3 model, numT = %d, D = %d" % (len(w.lh), len(start)),
                build=_lib.build_id(), bootstrap_rows=B)
    with Engine(w.times, w.lh, **kw) as e:
        line["nm_solve_rows_%d_rows" % B], fits = timed(lambda: e.nm_solve_rows(np.tile(start, (B, 1)), np.full(B, split), np.arange(1, B + 1), table),
                                                        a.repeats)
        line["nm_solve_rows_iterations"] = fits["iterations_issued"]
        refit_sd = fits["x"][np.isfinite(fits["llh"])].std(axis=0, ddof=1)
        line["refit_sd"] = [float(v) for v in refit_sd]
        if not a.skip_curvature:
            from misti_amd.optimize import observed_covariance, sandwich_covariance, standard_errors
            fit0 = e.nm_solve_rows(start[None, :], [split], [0], table)
            x0 = fit0["x"][0]
            line["curvature_1_point"], one = timed(lambda: e.curvature(x0[None, :], [split], [0], table), a.repeats)
            pts = np.vstack([x0[None, :], fits["x"][:99]])
            line["curvature_100_points"], many = timed(lambda: e.curvature(pts, np.full(100, split), np.arange(100) % a.rows, table), a.repeats)
            line["curvature_points_without_a_value"] = int((many.status != 0).sum())
            obs = observed_covariance(one.hess)
            line["data_fit"] = [float(v) for v in x0]
            line["observed_se"] = [float(v) for v in standard_errors(obs["cov"])[0]]
            line["sandwich_se"] = [float(v) for v in standard_errors(sandwich_covariance(one.hess, one.dlog, table))[0]]
            line["cond"] = float(obs["cond"][0])
            line["searches_over_curvature_1_point"] = round(line["nm_solve_rows_%d_rows" % B]["median_s"] / line["curvature_1_point"]["median_s"], 1)
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
