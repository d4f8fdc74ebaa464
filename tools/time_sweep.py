#!/usr/bin/env python3
"""Named sweeps on one GPU: the reference's GNU-parallel recipe (README.md:110-115 of the reference) in ONE evaluation, and a
boundary profile in ONE batched search (misti_nm_solve_bounds), each against the loop it replaces.

  recipe    `{st} -uf -mi 1 0 {mc} {mi1} 0 -mi 2 0 {mc} {mi2} 0 -mi 1 {mc} {st} {mi3} 0 -mi 2 {mc} {st} {mi4} 0 ::: st 20..25
            ::: mc 8..12 ::: mi1..mi4 (4 values each, the recipe's / 100)`: 6 x 5 x 4^4 = 7 680 models, expanded by the parser
            (misti_amd/sweep.py) and evaluated in one Engine.evaluate with per-candidate band bounds, on a synthetic grid of
            numT = 32 (the test inputs' PSMC files).  The loop: what `parallel` runs, one Engine and one evaluation per model,
            timed on a seeded sample of SAMPLE models and extrapolated (in this process: without the start of a Python process per
            model that `parallel` pays on top).
  profile   config 3's model (numT = 128, --cpfit, two optimised bands starting at 4 and {mc}, ends following the split),
            ROWS rows of a bootstrap table x SPLITS split values around 64 x the MCS boundaries 6, 8, .. with one start each,
            optimize.sweep_profile = one misti_nm_solve_bounds call.  The loop: one Engine per bound set plus one misti_nm_solve
            per (row, split, boundary) tuple (the test.bs scripts with a boundary loop added), the engines all created and timed,
            the searches timed on a seeded sample of SAMPLE tuples and extrapolated (the JSON says so).  The sampled tuples
            must agree bit for bit.

    python tools/time_sweep.py [--rows 101] [--splits 9] [--mcs 5] [--sample 12] [--out FILE]"""
import argparse
import json
import os
import random
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# the recipe's command line; its rates divided by 100 (the scale of golden_sweep.json's reference runs of it): on this grid the
# recipe's own values (up to 20) leave 99 % of the models without a value, a lambda-correction that fails at once
RECIPE = ("{st} -uf -mi 1 0 {mc} {mi1} 0 -mi 2 0 {mc} {mi2} 0 -mi 1 {mc} {st} {mi3} 0 -mi 2 {mc} {st} {mi4} 0 "
          "--sweep st 20 21 22 23 24 25 --sweep mc 8 9 10 11 12 --sweep mi1 0.0 0.005 0.02 0.05 --sweep mi2 0.05 0.1 0.15 0.2 "
          "--sweep mi3 0.0 0.005 0.02 0.05 --sweep mi4 0.01 0.05 0.1 0.15")


def recipe(sample):
    from misti_amd import cli, io as mio, synth
    from misti_amd.engine import Engine, truth_spectrum
    from misti_amd.sweep import expand, structure_error, sweep_error
    with tempfile.TemporaryDirectory() as d:                                    # the PSMC files are only read here
        f1, f2 = os.path.join(d, "g1.psmc"), os.path.join(d, "g2.psmc")
        open(f1, "w").write(synth.psmc_text(16, 1, synth.THETA_1))
        open(f2, "w").write(synth.psmc_text(17, 2, synth.THETA_2))
        inp = mio.read_psmc(f1, f2)
    row = synth.counts_from_spectrum(truth_spectrum(inp.times, inp.lambdas, 22, [(0, 0, 10, 0.02, -1), (1, 10, 22, 0.1, -1)], [], 0), 200000)
    a = cli.build_parser().parse_args([f1, f2, "sim.jafs"] + RECIPE.split())
    assert sweep_error(a) is None
    plan = expand(a)
    ok = [structure_error(plan.split[m], plan.bounds[m], [b[0] for b in plan.bands], 0, len(inp.lambdas)) is None for m in range(plan.n_model)]
    sel = np.where(ok)[0]
    kw = dict(unfolded=True, smooth=True)
    with Engine(inp.times, inp.lambdas, plan.engine_bands(int(sel[0])), [], n_param=plan.n_param, **kw) as e:
        e.evaluate(plan.split[sel[:64]], plan.params[sel[:64]], [row], band_bounds=plan.bounds[sel[:64]])      # warm-up
        t0 = time.perf_counter()
        res = e.evaluate(plan.split[sel], plan.params[sel], [row], band_bounds=plan.bounds[sel])
        t_one = time.perf_counter() - t0
    # the loop `parallel` runs: one model per process - here one Engine (the model's own bands, fixed rates written in) and one evaluation
    pick = np.random.default_rng(7).choice(len(sel), sample, replace=False)
    same = True
    t0 = time.perf_counter()
    for i in pick:
        m = sel[i]
        bands = [(p, int(s), int(e_), float(v), -1) for (p, _, _, _, _), (s, e_), v in zip(plan.bands, plan.bounds[m], plan.params[m])]
        with Engine(inp.times, inp.lambdas, bands, [], n_param=0, **kw) as e:
            r = e.evaluate([plan.split[m]], None, [row])
        same &= bool(r.llk[0, 0] == res.llk[i, 0] or (np.isnan(r.llk[0, 0]) and np.isnan(res.llk[i, 0])))
    t_loop = time.perf_counter() - t0
    per = t_loop / sample
    return dict(what="GNU-parallel recipe, 6 st x 5 mc x 4^4 fixed rates (/ 100), numT = 32, one evaluation", models=int(plan.n_model),
                valid_models=int(len(sel)), one_call_s=round(t_one, 4), models_per_s=round(len(sel) / t_one, 1),
                loop_sampled_models=sample, loop_per_model_s=round(per, 5), loop_all_models_s_extrapolated=round(per * len(sel), 2),
                loop_is_extrapolated=True, speedup_extrapolated=round(per * len(sel) / t_one, 1), sampled_models_bit_identical=bool(same),
                models_without_value=int((res.status != 0).sum()), best_model=plan.assign[int(sel[np.argmax(np.where(res.status == 0, res.llk[:, 0], -np.inf))])])


def profile(n_rows, n_splits, n_mcs, sample):
    from misti_amd import io as mio, synth, workloads
    from misti_amd.engine import Engine, truth_spectrum
    from misti_amd.optimize import sweep_profile
    w = workloads.config3(lambda *x: truth_spectrum(*x), n_start=1)
    kw = w.engine_kwargs()
    bands = [(p, s, -1, v, k) for p, s, e, v, k in w.bands]
    kw["bands"] = bands
    start = np.array([[b[3] for b in bands]])
    table = np.array(mio.bootstrap_table(synth.chunk_rows(w.jsfs[0], 20), n_rows - 1, random.Random(3)), dtype=np.float64)
    splits = 64.0 + np.arange(n_splits) - n_splits // 2
    mcs = 6 + 2 * np.arange(n_mcs)
    models = [(st, [[4, -1], [int(mc), -1]]) for st in splits for mc in mcs]
    with Engine(w.times, w.lh, **kw) as e:
        sweep_profile(e, models[:2], table[:2], start)                                   # warm-up: allocations, code objects
        t0 = time.perf_counter()
        prof = sweep_profile(e, models, table, start)
        t_prof = time.perf_counter() - t0
    # the loop: one Engine per bound set, one misti_nm_solve per (row, split, boundary) tuple
    t0 = time.perf_counter()
    engines = {}
    for mc in mcs:
        k2 = dict(kw)
        k2["bands"] = [bands[0], (bands[1][0], int(mc), -1, bands[1][3], bands[1][4])]
        engines[int(mc)] = Engine(w.times, w.lh, **k2)
    t_create = time.perf_counter() - t0
    rng = np.random.default_rng(7)
    tuples = [(int(r), int(m)) for r, m in zip(rng.integers(0, n_rows, sample), rng.integers(0, len(models), sample))]
    engines[int(mcs[0])].nm_solve(start, float(splits[0]), table[0])                    # warm-up
    t0 = time.perf_counter()
    each = [engines[models[m][1][1][0]].nm_solve(start, float(models[m][0]), table[r]) for r, m in tuples]
    t_loop = time.perf_counter() - t0
    for e in engines.values():
        e.close()
    same = all(np.array_equal(one["x"][0], prof["x"][r, m]) and one["llh"][0] == prof["llh"][r, m] and one["nit"][0] == prof["nit"][r, m]
               for one, (r, m) in zip(each, tuples))
    n = n_rows * len(models)
    per = t_loop / sample
    loop_s = t_create + per * n
    return dict(what="boundary profile, config 3 model, rows x splits x band-1 starts, one start each, one call", rows=n_rows,
                splits=n_splits, boundaries=n_mcs, searches=n, profile_s=round(t_prof, 4), profile_iterations=prof["iterations_issued"],
                profile_speculative=prof["speculative_iterations"], loop_engines=n_mcs, loop_engine_create_s=round(t_create, 4),
                loop_sampled_tuples=sample, loop_per_tuple_s=round(per, 5), loop_all_s_extrapolated=round(loop_s, 2),
                loop_is_extrapolated=True, speedup_extrapolated=round(loop_s / t_prof, 1), sampled_tuples_bit_identical=bool(same),
                searches_at_iteration_cap=int((prof["status"] == 2).sum()), searches_without_value=int((~np.isfinite(prof["llh"])).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=101)
    ap.add_argument("--splits", type=int, default=9)
    ap.add_argument("--mcs", type=int, default=5)
    ap.add_argument("--sample", type=int, default=12)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = [recipe(a.sample), profile(a.rows, a.splits, a.mcs, a.sample)]
    text = "".join(json.dumps(l) + "\n" for l in lines)
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if lines[0]["sampled_models_bit_identical"] and lines[1]["sampled_tuples_bit_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
