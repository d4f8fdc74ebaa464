#!/usr/bin/env python3
"""A bootstrap profile in ONE batched search (misti_nm_solve_rows) against the per-pair loop the reference's test.bs scripts run
(one misti_nm_solve per (replicate, split) pair), on one GPU.

Config 3's model (numT = 128, two optimised bands, --cpfit) with its band ends following the split (`-mi 1 4 ${st} ...`), SPLITS split
values around the true split 64 and ROWS rows of a bootstrap table (row 0 the data), one start per pair at the -mi initial values.
The profile is timed in full; the loop is timed on a seeded sample of SAMPLE of the same pairs and extrapolated to all of them (the
JSON line says so).  Both sides check that the sampled pairs agree bit for bit.

    python tools/time_bs_profile.py [--splits 11] [--rows 101] [--sample 12] [--out FILE]"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splits", type=int, default=11)
    ap.add_argument("--rows", type=int, default=101)
    ap.add_argument("--sample", type=int, default=12)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from misti_amd import io as mio, synth, workloads
    from misti_amd.engine import Engine, truth_spectrum
    from misti_amd.optimize import bootstrap_profile, bootstrap_profile_interval
    w = workloads.config3(lambda *x: truth_spectrum(*x), n_start=1)
    kw = w.engine_kwargs()
    kw["bands"] = [(p, s, -1, v, k) for p, s, e, v, k in w.bands]
    start = np.array([[b[3] for b in kw["bands"]]])
    table = np.array(mio.bootstrap_table(synth.chunk_rows(w.jsfs[0], 20), a.rows - 1, random.Random(3)), dtype=np.float64)
    splits = 64.0 + np.arange(a.splits) - a.splits // 2
    with Engine(w.times, w.lh, **kw) as e:
        bootstrap_profile(e, splits[:2], table[:2], start)                           # warm-up: allocations, code objects
        e.nm_solve(start, float(splits[0]), table[0])
        t0 = time.perf_counter()
        prof = bootstrap_profile(e, splits, table, start)
        t_prof = time.perf_counter() - t0
        rng = np.random.default_rng(7)
        pairs = [(int(r), int(p)) for r, p in zip(rng.integers(0, a.rows, a.sample), rng.integers(0, a.splits, a.sample))]
        t0 = time.perf_counter()
        each = [e.nm_solve(start, float(splits[p]), table[r]) for r, p in pairs]
        t_loop = time.perf_counter() - t0
    same = all(np.array_equal(one["x"][0], prof["x"][r, p]) and one["llh"][0] == prof["llh"][r, p] and one["nit"][0] == prof["nit"][r, p]
               for one, (r, p) in zip(each, pairs))
    n_pairs = a.rows * a.splits
    per_pair = t_loop / a.sample
    iv = bootstrap_profile_interval(prof["llh"], splits)
    line = dict(what="bootstrap profile, config 3 model, band ends following the split", splits=a.splits, rows=a.rows, pairs=n_pairs,
                profile_s=round(t_prof, 4), profile_iterations=prof["iterations_issued"], profile_speculative=prof["speculative_iterations"],
                loop_sampled_pairs=a.sample, loop_sample_s=round(t_loop, 4), loop_per_pair_s=round(per_pair, 5),
                loop_all_pairs_s_extrapolated=round(per_pair * n_pairs, 3), loop_is_extrapolated=True,
                speedup_extrapolated=round(per_pair * n_pairs / t_prof, 2), sampled_pairs_bit_identical=bool(same),
                pairs_at_iteration_cap=int((prof["status"] == 2).sum()), data_best_split=iv["data_split"], bootstrap_interval=iv["interval"])
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
