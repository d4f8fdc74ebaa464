#!/usr/bin/env python3
"""Per-candidate pulse times on one GPU: a pulse-date scan in ONE evaluation and a pulse-date profile with an optimised fraction in
ONE batched search (misti_nm_solve_pulses), each against the loop it replaces.

  grid      BASELINE config 5's grid (numT = 128, ancient second genome, 32 splits x 64 band rates x 32 pulse fractions, --cpfit)
            at TIMES pulse times around the true one: one Engine.evaluate with per-candidate pulse times over all of them, against
            one context per pulse time - created, its grid uploaded and evaluated one after another (all of them, nothing
            extrapolated).  The two must agree bit for bit.
  profile   the same model with the band rate and the pulse fraction optimised: ROWS rows of a bootstrap table x SPLITS split
            values x TIMES pulse times with one start each, optimize.sweep_profile = one misti_nm_solve_pulses call.  The loop: one
            Engine per pulse time plus one misti_nm_solve per (row, split, time) tuple, the engines all created and timed, the
            searches timed on a seeded sample of SAMPLE tuples and extrapolated (the JSON says so).  The sampled tuples must agree
            bit for bit.

    python tools/time_pulse_sweep.py [--times 8] [--rows 21] [--splits 5] [--sample 12] [--out FILE]"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pulse_times_of(w, n_times):
    """n_times pulse times around the workload's own, all after the sample date and the band start and below the first split."""
    t0 = w.pulses[0][1]
    return [int(t0 - 2 + 2 * k) for k in range(n_times)]


def grid(n_times):
    from misti_amd import workloads
    from misti_amd.engine import Engine, truth_spectrum
    w = workloads.config5(lambda *a: truth_spectrum(*a))
    kw = w.engine_kwargs()
    ts = pulse_times_of(w, n_times)
    n = w.n_cand
    split, params = np.tile(w.split_time, n_times), np.tile(w.params, (n_times, 1))
    times = np.repeat(np.array(ts, dtype=np.int32), n).reshape(-1, 1)
    with Engine(w.times, w.lh, **kw) as e:
        e.evaluate(split[:64], params[:64], w.jsfs, pulse_times=times[:64])                 # warm-up: allocations, code objects
        e.evaluate(split, params, w.jsfs, pulse_times=times)                                # ... and the batch's own buffers
        t0 = time.perf_counter()
        res = e.evaluate(split, params, w.jsfs, pulse_times=times)
        t_one = time.perf_counter() - t0
    # what there was before: one context per pulse time, the times in its model, one after another
    same = True
    t0 = time.perf_counter()
    for k, t in enumerate(ts):
        k2 = dict(kw)
        k2["pulses"] = [(p, t, v, q) for p, _, v, q in w.pulses]
        with Engine(w.times, w.lh, **k2) as e:
            r = e.evaluate(w.split_time, w.params, w.jsfs)
        same &= r.llk.tobytes() == res.llk[k * n:(k + 1) * n].tobytes() and r.status.tobytes() == res.status[k * n:(k + 1) * n].tobytes()
    t_loop = time.perf_counter() - t0
    best = int(np.argmax(np.where(res.status == 0, res.llk[:, 0], -np.inf)))
    return dict(what="config 5 grid (32 x 64 x 32, numT = 128, --cpfit) at %d pulse times, one evaluation" % n_times, pulse_times=ts,
                candidates=int(n * n_times), one_call_s=round(t_one, 4), evals_per_s=round(n * n_times / t_one, 1),
                loop_contexts=n_times, loop_s=round(t_loop, 4), loop_is_extrapolated=False, speedup=round(t_loop / t_one, 2),
                bit_identical=bool(same), candidates_without_value=int((res.status != 0).sum()), best_pulse_time=int(times[best, 0]),
                true_pulse_time=int(w.pulses[0][1]))


def profile(n_times, n_rows, n_splits, sample):
    from misti_amd import io as mio, synth, workloads
    from misti_amd.engine import Engine, truth_spectrum
    from misti_amd.optimize import sweep_profile
    w = workloads.config5(lambda *a: truth_spectrum(*a), n_split=1, n_rate=1, n_pulse=1)
    kw = w.engine_kwargs()
    ts = pulse_times_of(w, n_times)
    start = np.array([[0.15, 0.1]])
    table = np.array(mio.bootstrap_table(synth.chunk_rows(w.jsfs[0], 20), n_rows - 1, random.Random(3)), dtype=np.float64)
    splits = float(w.truth["split"]) + np.arange(n_splits) - n_splits // 2
    bounds = [[w.bands[0][1], -1]]
    models = [(st, bounds, [t]) for st in splits for t in ts]
    with Engine(w.times, w.lh, **kw) as e:
        sweep_profile(e, models[:2], table[:2], start)                                      # warm-up
        t0 = time.perf_counter()
        prof = sweep_profile(e, models, table, start)
        t_prof = time.perf_counter() - t0
    t0 = time.perf_counter()
    engines = {}
    for t in ts:
        k2 = dict(kw)
        k2["pulses"] = [(p, t, v, q) for p, _, v, q in w.pulses]
        engines[t] = Engine(w.times, w.lh, **k2)
    t_create = time.perf_counter() - t0
    rng = np.random.default_rng(7)
    tuples = [(int(r), int(m)) for r, m in zip(rng.integers(0, n_rows, sample), rng.integers(0, len(models), sample))]
    engines[ts[0]].nm_solve(start, float(splits[0]), table[0])                              # warm-up
    t0 = time.perf_counter()
    each = [engines[models[m][2][0]].nm_solve(start, float(models[m][0]), table[r]) for r, m in tuples]
    t_loop = time.perf_counter() - t0
    for e in engines.values():
        e.close()
    same = all(np.array_equal(one["x"][0], prof["x"][r, m]) and one["llh"][0] == prof["llh"][r, m] and one["nit"][0] == prof["nit"][r, m]
               for one, (r, m) in zip(each, tuples))
    n = n_rows * len(models)
    per = t_loop / sample
    loop_s = t_create + per * n
    data_best = int(np.argmax(np.where(np.isfinite(prof["llh"][0]), prof["llh"][0], -np.inf)))
    return dict(what="pulse-date profile, config 5 model, band rate and pulse fraction optimised, rows x splits x pulse times, one start each, one call",
                rows=n_rows, splits=n_splits, pulse_times=ts, searches=n, profile_s=round(t_prof, 4), profile_iterations=prof["iterations_issued"],
                profile_speculative=prof["speculative_iterations"], loop_engines=n_times, loop_engine_create_s=round(t_create, 4),
                loop_sampled_tuples=sample, loop_per_tuple_s=round(per, 5), loop_all_s_extrapolated=round(loop_s, 2),
                loop_is_extrapolated=True, speedup_extrapolated=round(loop_s / t_prof, 1), sampled_tuples_bit_identical=bool(same),
                searches_at_iteration_cap=int((prof["status"] == 2).sum()), searches_without_value=int((~np.isfinite(prof["llh"])).sum()),
                data_row_best_pulse_time=int(models[data_best][2][0]), data_row_best_split=float(models[data_best][0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--times", type=int, default=8)
    ap.add_argument("--rows", type=int, default=21)
    ap.add_argument("--splits", type=int, default=5)
    ap.add_argument("--sample", type=int, default=12)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = [grid(a.times), profile(a.times, a.rows, a.splits, a.sample)]
    text = "".join(json.dumps(l) + "\n" for l in lines)
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text)
    return 0 if lines[0]["bit_identical"] and lines[1]["sampled_tuples_bit_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
