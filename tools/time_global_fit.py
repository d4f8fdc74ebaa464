#!/usr/bin/env python3
"""Time basin hopping with the split as a coordinate against what it replaces (run on the GPU box).

    python tools/time_global_fit.py [--niter 10 100] [--rows 101] [--out FILE]

Config 3's model (band ends following the split), a bootstrap table of `--rows` rows, three (start, initial split) pairs per row -
the model's initial rates at splits 61, 63 and 65 - i.e. rows x 3 searches, and per `niter` three legs in one session on one context:

    global    ONE Engine.basinhopping_split call: niter + 1 minimisations of every search, hops in step
    local     niter + 1 successive Engine.nm_solve_split calls on the same starts: the parent's cost for the same NUMBER of
              minimisations (each with the local search's budget, tol 1e-4 and 1000 iterations - not the same work: basin
              hopping's minimisations stop at SciPy's 200 x coordinates)
    one_row   one Engine.basinhopping call per row at a fixed split (63), the row's three starts in it: what a user does today.
              `--one-row-sample K` times K rows spread over the table and scales to all of them (0: every row)

Every leg is run once after one small warm-up call (the first call of a context allocates); the host clock around a synchronous
call.  One JSON line per (leg, niter) is printed and appended to --out with the library's build id; --text appends the same as a
table."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--niter", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--rows", type=int, default=101)
    ap.add_argument("--one-row-sample", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "global_fit_timing.jsonl"))
    ap.add_argument("--text", default=os.path.join(ROOT, "profiles", "global_fit_timing.txt"))
    ap.add_argument("--tag", default="", help="free text kept in every line (which build this is)")
    a = ap.parse_args()
    import torch
    from misti_amd import _lib, io as mio, synth, workloads
    from misti_amd.engine import Engine, truth_spectrum
    if not torch.cuda.is_available():
        raise SystemExit("time_global_fit: no GPU - a timing taken anywhere else says nothing")
    w = workloads.config3(lambda *s: truth_spectrum(*s), n_start=4)
    bands = [(p, s, -1, v, k) for p, s, e, v, k in w.bands]
    table = np.array(mio.bootstrap_table(synth.chunk_rows(w.jsfs[0], 20), a.rows - 1, random.Random(3)), dtype=np.float64)
    kw = w.engine_kwargs()
    kw["bands"] = bands
    start = [b[3] for b in bands]
    R = table.shape[0]
    pairs = np.array([start + [st] for st in (61.0, 63.0, 65.0)])
    starts = np.vstack([pairs] * R)
    rows = np.repeat(np.arange(R), 3).astype(np.int32)
    sample = list(range(R)) if a.one_row_sample <= 0 else sorted(set(np.linspace(0, R - 1, a.one_row_sample).astype(int).tolist()))
    lines = []
    with Engine(w.times, w.lh, **kw) as e:
        e.basinhopping_split(starts[:3], rows[:3], table, [0, 1, 2], niter=1)           # warm-up: allocations
        for niter in a.niter:
            seeds = [[0, j] for _ in range(R) for j in range(3)]
            t0 = time.perf_counter()
            g = e.basinhopping_split(starts, rows, table, seeds, niter=niter)
            t_global = time.perf_counter() - t0
            t0 = time.perf_counter()
            for _ in range(niter + 1):
                loc = e.nm_solve_split(starts, rows, table)
            t_local = time.perf_counter() - t0
            t0 = time.perf_counter()
            for r in sample:
                e.basinhopping(pairs[:, :2], 63.0, table[r], [[0, j] for j in range(3)], niter=niter)
            t_one = (time.perf_counter() - t0) * R / len(sample)
            base = dict(tag=a.tag, build=_lib.build_id(), rows=R, searches=int(rows.size), niter=niter, device=torch.cuda.get_device_name(0))
            for leg, sec, extra in (("global", t_global, dict(nfev=int(g["nfev"].sum()), failures=int(g["failures"].sum()),
                                                               iterations_issued=g["iterations_issued"],
                                                               speculative_iterations=g["speculative_iterations"])),
                                    ("local", t_local, dict(nfev=int(loc["nfev"].sum()) * (niter + 1), calls=niter + 1)),
                                    ("one_row", t_one, dict(calls=R, rows_timed=len(sample)))):
                rec = dict(base, leg=leg, seconds=sec, **extra)
                print(json.dumps(rec), flush=True)
                lines.append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
    with open(a.text, "a") as f:
        f.write("build %s  %s  %d rows x 3 (start, split) pairs\n" % (lines[0]["build"], lines[0]["device"], R))
        f.write("%8s %10s %12s  %s\n" % ("niter", "leg", "seconds", "notes"))
        for rec in lines:
            notes = ", ".join("%s=%s" % (k, rec[k]) for k in ("nfev", "failures", "calls", "rows_timed", "speculative_iterations") if k in rec)
            f.write("%8d %10s %12.3f  %s\n" % (rec["niter"], rec["leg"], rec["seconds"], notes))


if __name__ == "__main__":
    main()
