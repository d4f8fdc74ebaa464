#!/usr/bin/env python3
"""Python API tour on synthetic data (needs an MI355X):

  1. a split-time scan x bootstrap replicates with the likelihood table kept on the device
     (`Engine.evaluate_dev` + `misti_argmax_dev` via `optimize.bootstrap_scan_dev`), i.e. what the bash loops of
     the reference's test.bs/*.sh + bs_conf_int.ipynb do with one MiSTI.py process per (split, replicate);
  2. the same scan WITHOUT the table: the three best splits per replicate, reduced where the values are computed
     (`optimize.scan_best`: `misti_eval_batch_dev` without replicates + `misti_scan_best_dev`);
  3. many independent scans overlapped on a pool of lanes (`lanes.LanePool`);
  4. the uncertainty of a fitted migration rate two ways: one search per bootstrap row (`Engine.nm_solve_rows`, the spread of the
     refits) and ONE fit plus one stencil (`Engine.curvature`, the sandwich standard error of `optimize.sandwich_covariance`).

    python examples/bootstrap_scan.py
"""
import io
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from misti_amd import io as mio, synth                      # noqa: E402
from misti_amd.engine import Engine, truth_spectrum         # noqa: E402
from misti_amd.lanes import LanePool                        # noqa: E402
from misti_amd.optimize import (bootstrap_scan_dev, observed_covariance, sandwich_covariance, scan_best,   # noqa: E402
                                standard_errors)


def main():
    # two synthetic PSMC outputs -> merged grid (numT = 128), a truth with split index 64, data JSFS from its spectrum
    inp = mio.merge_psmc(mio.read_psmc_file(io.StringIO(synth.psmc_text(64, 1, synth.THETA_1))),
                         mio.read_psmc_file(io.StringIO(synth.psmc_text(65, 2, synth.THETA_2))))
    times, lh, _ = synth.self_consistent(inp, 64)
    jafs = truth_spectrum(times, lh, 64, [], [], 0)
    row = synth.counts_from_spectrum(jafs, 10 ** 6)
    table = np.array(mio.bootstrap_table(synth.chunk_rows(row, 20), 200))          # row 0 = the data, 200 resamples
    splits = np.arange(48, 81, dtype=float)

    with Engine(times, lh, cpfit=True, smooth=True) as e:
        t0 = time.perf_counter()
        mean, (lo, hi), best = bootstrap_scan_dev(e, splits, table)
        dt = time.perf_counter() - t0
        top, top_llk, _ = scan_best(e, splits, None, table, k=3)                   # [201][3]: no [33 x 201] table anywhere
    print("split scan %d values x %d replicates: best split %.2f, 95%% interval [%.2f, %.2f]  (%.1f ms, %d llk values)"
          % (len(splits), len(table), mean, lo, hi, 1e3 * dt, len(splits) * len(table)))
    assert (splits[top[:, 0]] == best).all()
    print("the data row's three best splits: %s (llk %s)" % (splits[top[0]], top_llk[0]))

    # the same scan for 40 different resampled tables, overlapped on 8 lanes
    rng = np.random.default_rng(0)
    tables = [table[rng.integers(0, len(table), len(table))] for _ in range(40)]
    with LanePool(times, lh, lanes=8, cpfit=True, smooth=True) as pool:
        pool.map([(splits, None, tables[0])])                                      # contexts warm up
        t0 = time.perf_counter()
        out = pool.map([(splits, None, tb) for tb in tables])
        dt = time.perf_counter() - t0
    best = [splits[np.argmax(llk[:, 0])] for llk, _, _ in out]
    print("40 scans on 8 lanes: %.1f ms in total, best splits %s ..." % (1e3 * dt, best[:5]))

    # a model with one migration band: fit its rate to the data row and to 60 bootstrap rows (one batched search), then take the
    # curvature at the data row's fit alone.  The two figures are printed for a reader to compare; nothing is asserted about them:
    # how close they lie depends on the data (the chunks of this synthetic table are independent draws - real chunks are linked).
    jafs_m = truth_spectrum(times, lh, 64, [(0, 4, 64, 0.3, -1)], [], 0)
    table_m = np.array(mio.bootstrap_table(synth.chunk_rows(synth.counts_from_spectrum(jafs_m, 10 ** 6), 20), 60))
    R = len(table_m)
    with Engine(times, lh, [(0, 4, -1, 0.3, 0)], n_param=1, cpfit=True, smooth=True) as e:
        fits = e.nm_solve_rows(np.full((R, 1), 0.2), np.full(R, 64.0), np.arange(R), table_m)
        cur = e.curvature(fits["x"][:1], [64.0], [0], table_m)                     # 3 evaluations (1 + 2 n^2 with n = 1)
    obs = observed_covariance(cur.hess)
    print("migration rate fitted to the data row: %.5f; sd of %d bootstrap refits %.2g; sandwich se %.2g; observed-information se %.2g "
          "(cond %.3g, stencil status %d)" % (fits["x"][0, 0], R - 1, fits["x"][1:, 0].std(ddof=1),
                                              standard_errors(sandwich_covariance(cur.hess, cur.dlog, table_m))[0, 0],
                                              standard_errors(obs["cov"])[0, 0], obs["cond"][0], cur.status[0]))


if __name__ == "__main__":
    main()
