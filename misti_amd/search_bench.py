"""`bench.py --workload config3-search | config3-basinhopping`: BASELINE config 3 as a SEARCH - two optimised -mi bands from 16 384
random starts with the simplices resident in HBM - timed end to end: objective evaluations per second INCLUDING the optimiser's own
kernels and the idle slots of finished starts.

  config3-search         SciPy-exact Nelder-Mead per start (misti_nm_solve; reference semantics MigrationInference.Solve,
                         /root/reference/MigrationInference.py:718-733: xatol = fatol = 1e-4, maxiter = 1000), the starts dealt out to
                         `--search-groups` engine contexts whose batches overlap (misti_amd.optimize.solve_grouped_dev)
  config3-basinhopping   the reference's global variant (:723-725: scipy.optimize.basinhopping(T=0.5, Nelder-Mead)) per start
                         (misti_basinhopping), `--bh-niter` hops (SciPy's default of 100 hops is 101 such searches per start)"""
from __future__ import annotations

import json
import os
import statistics
import sys
import time

import numpy as np

GROUPS = 1          # engine contexts the starts are dealt out to (measured on MI355X: 4 groups 1.08 s per search, 1 group 1.00 s - the search
                    # is bound by the latency of its slowest chains, not by throughput; misti_amd.optimize.solve_grouped_dev stays for callers
                    # with several independent searches)
BH_NITER = 100      # SciPy's default niter, which the reference's Solve(globalOpt=True) runs with (/root/reference/MigrationInference.py:723-725)


def _metric():
    metric = "composite-llk evals/sec over (split×mi) grid, 128 merged PSMC intervals"
    try:
        metric = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "BASELINE.json"))).get("metric") or metric
    except Exception:
        pass
    return metric


def run(a, spectrum_fn, dev, local_rank, rank, world, json_fd):
    import torch
    from . import workloads
    from .engine import Engine
    from .optimize import solve_grouped_dev
    w = workloads.config3(spectrum_fn, n_start=int(getattr(a, "bh_starts", 0) or 16384))
    split = float(w.split_time[0])
    S = w.n_cand
    if a.workload == "config3-basinhopping":
        return run_basinhopping(a, w, split, local_rank, rank, world, json_fd)
    if world > 1:
        return run_search_sharded(a, w, split, local_rank, rank, world, json_fd)
    steps = max(1, min(a.steps, 8))                       # a step = one complete search of all starts
    engines = [Engine(w.times, w.lh, device=local_rank, **w.engine_kwargs()) for _ in range(GROUPS)]
    try:
        search = lambda: solve_grouped_dev(engines, split, w.params, w.jsfs[0], tol=1e-4, maxiter=1000)[2]
        for _ in range(min(a.warmup, 1) + 1):             # first call allocates the search state
            r = search()
        dts = []
        while not dts or (sum(dts) < a.min_seconds and len(dts) < 50):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                r = search()
            torch.cuda.synchronize()
            dts.append(time.perf_counter() - t0)
        dt = statistics.median(dts)
        evals = int(r["nfev"].sum())
        # the same search on ONE context (the three batches of an iteration strictly one after another)
        t0 = time.perf_counter()
        r1 = engines[0].nm_solve(w.params, split, w.jsfs[0], tol=1e-4, maxiter=1000)
        t_one = time.perf_counter() - t0
        same = all(np.array_equal(r[k], r1[k], equal_nan=True) for k in ("x", "llh", "nit", "nfev", "status"))
        # the same evaluations as plain batches (no optimiser): what the search costs on top
        t0 = time.perf_counter()
        engines[0].evaluate(np.full(S, split), w.params, w.jsfs)
        t_batch = time.perf_counter() - t0
    finally:
        for e in engines:
            e.close()
    out = {"metric": _metric(), "value": evals * steps / dt, "unit": "llk evals/s", "n_gpus": 1, "steps": steps, "warmup": a.warmup,
           "ms_per_step": 1e3 * dt / steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
           "config": {"workload": "config3-search: numT=128, two optimised bands, Nelder-Mead from %d random starts, simplices resident in HBM" % S,
                      "starts": S, "objective_evaluations_per_search": evals, "iterations_max": int(r["nit"].max()),
                      "iterations_median": float(np.median(r["nit"])), "converged_fraction": float((r["status"] == 0).mean()),
                      "iterations_issued": r["iterations_issued"], "speculative_iterations": r["speculative_iterations"], "batch_slots": r["slots"],
                      "search_groups": GROUPS, "batches_in_flight": GROUPS, "parallelism": "1 GPU"},
           "one_context": {"value": int(r1["nfev"].sum()) / t_one, "s_per_search": t_one, "iterations_issued": r1["iterations_issued"],
                           "speculative_iterations": r1["speculative_iterations"], "equal_to_grouped": bool(same)},
           "timing": {"repeats": len(dts), "timed_region_s_median": dt,
                      "note": "value = objective evaluations SciPy counts (sum of nfev over the starts) per second of the whole search, optimiser kernels, "
                              "speculative points and all-dead slots of finished starts included; one plain host-buffer batch of the %d starts takes %.2f ms"
                              % (S, 1e3 * t_batch)},
           "best": {"llh": float(np.max(r["llh"])), "params": [float(v) for v in r["x"][int(np.argmax(r["llh"]))]], "truth": [0.2, 0.05]}}
    sys.stdout.flush()
    os.write(json_fd, (json.dumps(out) + "\n").encode())


def _fenced(world):
    import torch
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    torch.cuda.synchronize()


def _max_over_ranks(dt, world, local_rank):
    if world == 1:
        return dt
    import torch
    import torch.distributed as dist
    t = torch.tensor([dt], dtype=torch.float64, device=torch.device("cuda", local_rank))
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def run_search_sharded(a, w, split, local_rank, rank, world, json_fd):
    """`--gpus N --workload config3-search`: ONE search of all starts, the starts dealt to the ranks in contiguous blocks
    (optimize.solve_batched_dev inside the process group: dist.search_sharded, one all_gather) - strong scaling."""
    from .engine import Engine
    from .optimize import solve_batched_dev
    S = w.n_cand
    with Engine(w.times, w.lh, device=local_rank, **w.engine_kwargs()) as eng:
        search = lambda: solve_batched_dev(eng, split, w.params, w.jsfs[0], tol=1e-4, maxiter=1000)[2]
        r = search()
        _fenced(world)
        t0 = time.perf_counter()
        r = search()
        _fenced(world)
        dt = _max_over_ranks(time.perf_counter() - t0, world, local_rank)
    if rank != 0:
        return
    evals = int(r["nfev"].sum())
    out = {"metric": _metric(), "value": evals / dt, "unit": "llk evals/s", "n_gpus": world, "steps": 1, "warmup": 1, "ms_per_step": 1e3 * dt,
           "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
           "config": {"workload": "config3-search: numT=128, two optimised bands, Nelder-Mead from %d random starts dealt to %d ranks in contiguous blocks, "
                                  "one all_gather of the results" % (S, world), "starts": S, "starts_per_rank": -(-S // world),
                      "objective_evaluations_per_search": evals, "converged_fraction": float((r["status"] == 0).mean()), "parallelism": "starts sharded over %d GPUs" % world},
           "timing": {"repeats": 1, "timed_region_s_median": dt, "note": "max over ranks, barrier + synchronize on both sides"},
           "best": {"llh": float(np.max(r["llh"])), "params": [float(v) for v in r["x"][int(np.argmax(r["llh"]))]], "truth": [0.2, 0.05]}}
    sys.stdout.flush()
    os.write(json_fd, (json.dumps(out) + "\n").encode())


def run_basinhopping(a, w, split, local_rank, rank, world, json_fd):
    from .engine import Engine
    from .optimize import basinhopping_dev
    S = w.n_cand
    niter = int(getattr(a, "bh_niter", 0) or BH_NITER)
    with Engine(w.times, w.lh, device=local_rank, **w.engine_kwargs()) as eng:
        seeds = list(np.arange(S) + 1000)
        hop = lambda n: basinhopping_dev(eng, split, w.params, w.jsfs[0], seeds, niter=n, T=0.5, stepsize=0.5)
        hop(1)                                            # first call allocates
        _fenced(world)
        t0 = time.perf_counter()
        r = hop(niter)
        _fenced(world)
        dt = _max_over_ranks(time.perf_counter() - t0, world, local_rank)
    if rank != 0:
        return
    evals = int(r["nfev"].sum())
    out = {"metric": _metric(), "value": evals / dt, "unit": "llk evals/s", "n_gpus": world, "steps": 1, "warmup": 1,
           "ms_per_step": 1e3 * dt, "higher_is_better": True, "scaling": "strong" if world > 1 else "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
           "config": {"workload": "config3-basinhopping: numT=128, two optimised bands, scipy-exact basinhopping(T=0.5, Nelder-Mead) from %d random starts, "
                                  "%d hops (SciPy's default, which the reference's Solve(globalOpt=True) runs with: 100), incumbents and simplices resident in HBM" % (S, niter),
                      "starts": S, "hops": niter, "minimisations_per_start": niter + 1, "objective_evaluations": evals, "hops_accepted_mean": float(np.mean(r["accepted"])),
                      "minimization_failures_mean": float(np.mean(r["failures"])), "nfev_per_start_max": int(r["nfev"].max()),
                      "batches_in_flight": 1, "parallelism": "1 GPU" if world == 1 else "starts sharded over %d GPUs" % world},
           "timing": {"repeats": 1, "timed_region_s_median": dt,
                      "note": "value = res.nfev summed over the starts per second of the whole run (host draws of the uniforms included)"},
           "best": {"llh": float(np.max(r["llh"])), "params": [float(v) for v in r["x"][int(np.argmax(r["llh"]))]], "truth": [0.2, 0.05]}}
    sys.stdout.flush()
    os.write(json_fd, (json.dumps(out) + "\n").encode())


def run_de_compare(n_rows=256, pop=16, gens=40, hops=(10, 30), seed=0, device=0, out=None):
    """`python -m misti_amd.search_bench`: config 3's model as a GLOBAL search per bootstrap row, both ways - differential evolution
    (misti_de_search: every generation one dense batch of rows x members points) and basin hopping on the rows path
    (misti_basinhopping_box, hops in lockstep) - on the same rows, from the same start per row, inside the same box (the range config
    3's random starts span).  Reports per leg the wall time of one call, the evaluations (sum of nfev) and the median over rows of the
    best llh reached: what to compare is time and evaluations at equal median llh.  One JSON line per leg."""
    import random
    from . import io as mio, synth, workloads
    from .engine import Engine, truth_spectrum
    w = workloads.config3(lambda *a: truth_spectrum(*a), n_start=max(n_rows, 64))
    split = float(w.split_time[0])
    table = np.array(mio.bootstrap_table(synth.chunk_rows(w.jsfs[0], 20), n_rows - 1, random.Random(3)), dtype=np.float64)
    R = table.shape[0]
    rows = np.arange(R, dtype=np.int32)
    starts = np.ascontiguousarray(w.params[:R])
    box = (w.params.min(axis=0), w.params.max(axis=0))
    splits = np.full(R, split)
    lines = []
    with Engine(w.times, w.lh, device=device, **w.engine_kwargs()) as eng:
        legs = [("de pop=%d gens=%d seed=%d" % (pop, gens, seed),
                 lambda: eng.differential_evolution(starts, rows, table, box, split_times=splits, pop=pop, maxiter=gens, tol=0.0, seed=seed))]
        for n in hops:
            legs.append(("basinhopping hops=%d seed=%d" % (n, seed),
                         lambda n=n: eng.basinhopping_box(starts, rows, table, [seed + 1000 + j for j in range(R)], box, split_times=splits, niter=n)))
        eng.differential_evolution(starts[:4], rows[:4], table, box, split_times=splits[:4], pop=4, maxiter=1)      # first calls allocate
        eng.basinhopping_box(starts[:4], rows[:4], table, [0, 1, 2, 3], box, split_times=splits[:4], niter=1)
        for name, call in legs:
            eng.sync()
            t0 = time.perf_counter()
            r = call()
            dt = time.perf_counter() - t0
            lines.append({"leg": name, "rows": R, "box": [list(map(float, box[0])), list(map(float, box[1]))], "seconds": dt,
                          "nfev": int(r["nfev"].sum()), "median_llh": float(np.median(r["llh"])), "min_llh": float(np.min(r["llh"])),
                          "max_llh": float(np.max(r["llh"])), "evals_per_second": int(r["nfev"].sum()) / dt})
    text = "\n".join(json.dumps(l) for l in lines) + "\n"
    sys.stdout.write(text)
    if out:
        with open(out, "w") as fh:
            fh.write(text)
    return lines


def run_mcmc_compare(n_rows=256, walkers=16, steps=40, pop=16, gens=40, seed=0, device=0, out=None, repeats=5, log_prior=False):
    """`python -m misti_amd.search_bench --mcmc W STEPS`: config 3's model, one ensemble per bootstrap row (misti_ensemble_sample: every
    half-step one dense batch of rows x W / 2 slots) beside the differential-evolution leg of run_de_compare on the same rows and box -
    the two in turns in one process, `repeats` times after a warm-up call each.  A half-step is an engine batch like a DE generation,
    so what to compare is the time per submitted point.  Reports per leg the median and the least seconds of a call, the points handed to
    the engine and, for the sampler, the acceptance fraction.  One JSON line per leg.  `log_prior` (`--mcmc-log-prior`): a third leg, the
    sampler with every rate on the log scale under a normal prior (misti_ensemble_sample_prior) centred on the middle of the box of
    logarithms with a quarter of its width as sd, from the same ensembles mapped with to_sampling."""
    import random
    from . import io as mio, synth, workloads
    from .engine import Engine, truth_spectrum
    from .optimize import ensemble_start
    w = workloads.config3(lambda *a: truth_spectrum(*a), n_start=max(n_rows, 64))
    split = float(w.split_time[0])
    table = np.array(mio.bootstrap_table(synth.chunk_rows(w.jsfs[0], 20), n_rows - 1, random.Random(3)), dtype=np.float64)
    R = table.shape[0]
    rows = np.arange(R, dtype=np.int32)
    starts = np.ascontiguousarray(w.params[:R])
    box = (w.params.min(axis=0), w.params.max(axis=0))
    splits = np.full(R, split)
    with Engine(w.times, w.lh, device=device, **w.engine_kwargs()) as eng:
        de = lambda: eng.differential_evolution(starts, rows, table, box, split_times=splits, pop=pop, maxiter=gens, tol=0.0, seed=seed)
        fit = de()["x"]                                                                     # (also the DE leg's warm-up)
        init = np.stack([ensemble_start(fit[r], box[0], box[1], walkers, 1e-2, seed, 0) for r in range(R)])
        mc = lambda: eng.ensemble_sample(init, rows, table, box, split_times=splits, n_step=steps, seed=seed, ids=np.zeros(R, dtype=np.uint64))
        mc()
        legs = [("de pop=%d gens=%d seed=%d" % (pop, gens, seed), de), ("mcmc walkers=%d steps=%d seed=%d" % (walkers, steps, seed), mc)]
        if log_prior:
            from .optimize import prior_spec, to_sampling
            N = init.shape[2]
            ybox = (np.log(box[0]), np.log(box[1]))
            prior = prior_spec(N, log=range(N), normal={k: (0.5 * (ybox[0][k] + ybox[1][k]), 0.25 * (ybox[1][k] - ybox[0][k])) for k in range(N)})
            yinit = to_sampling(init, prior, ybox)
            mp = lambda: eng.ensemble_sample(yinit, rows, table, ybox, split_times=splits, n_step=steps, seed=seed, ids=np.zeros(R, dtype=np.uint64), prior=prior)
            mp()
            legs.append(("mcmc log scale, normal prior walkers=%d steps=%d seed=%d" % (walkers, steps, seed), mp))
        times = {name: [] for name, _ in legs}
        last = {}
        for _ in range(repeats):
            for name, call in legs:
                eng.sync()
                t0 = time.perf_counter()
                last[name] = call()
                times[name].append(time.perf_counter() - t0)
    lines = []
    for name, _ in legs:
        r, t = last[name], times[name]
        points = int(r["n_points"]) + (R * walkers if "accepted" in r else 0)           # the sampler's n_points leaves the initial ensembles out
        line = {"leg": name, "rows": R, "repeats": repeats, "seconds_median": float(np.median(t)), "seconds_min": float(np.min(t)), "points": points,
                "us_per_point_median": 1e6 * float(np.median(t)) / points}
        if "accepted" in r:
            line.update(acceptance=float(r["accepted"].sum()) / (R * walkers * steps), batches=1 + 2 * steps, slots=R * walkers + 2 * steps * R * (walkers // 2),
                        median_last_llh=float(np.median(r["last_llh"])))
        else:
            line.update(batches=int(r["iterations_issued"]) + 1, median_llh=float(np.median(r["llh"])))
        lines.append(line)
    text = "\n".join(json.dumps(l) for l in lines) + "\n"
    sys.stdout.write(text)
    if out:
        with open(out, "w") as fh:
            fh.write(text)
    return lines


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="differential evolution against basin hopping on config 3's model, per bootstrap row")
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--pop", type=int, default=16)
    ap.add_argument("--gens", type=int, default=40)
    ap.add_argument("--hops", type=int, nargs="+", default=[10, 30])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--mcmc", type=int, nargs=2, default=None, metavar=("W", "STEPS"), help="the sampler's leg beside the DE leg: one ensemble of W walkers per row, STEPS steps")
    ap.add_argument("--mcmc-log-prior", action="store_true", help="with --mcmc: a third leg, the sampler with every rate on the log scale under a normal prior")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if a.mcmc:
        run_mcmc_compare(a.rows, a.mcmc[0], a.mcmc[1], a.pop, a.gens, a.seed, a.device, a.out, a.repeats, a.mcmc_log_prior)
        sys.exit(0)
    run_de_compare(a.rows, a.pop, a.gens, tuple(a.hops), a.seed, a.device, a.out)
