#!/usr/bin/env python3
"""Bitwise A/B of two builds of the library (run on the GPU box).

    python -m misti_amd.build --out /tmp/variant.so -DSOMETHING        # a variant build
    MISTI_LIB_AB=1 MISTI_LIB=/tmp/variant.so python tools/ab_compare.py dump a.npz    # 300 random models + configs 2 and 3: llk, status, rates, spectra;
                                                                       # then every batched search and misti_basinhopping on fixed starts, with and without
                                                                       # speculative iterations: results and work counters
    python tools/ab_compare.py dump b.npz                              # the in-tree build
    python tools/ab_compare.py cmp a.npz b.npz                         # arrays that differ in any bit

How the "bit-identical" claims of DESIGN.md section 4 were checked."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def dump(path):
    from random_campaign import random_batch
    from misti_amd import workloads
    from misti_amd.engine import Engine, truth_spectrum
    out = {}
    rng = np.random.default_rng(7)
    for i in range(int(os.environ.get("AB_MODELS", "300"))):
        c = random_batch(rng)
        with Engine(c["times"], c["lh"], c["bands"], c["pulses"], n_param=c["P"], sample_date=c["sd"], **c["flags"]) as e:
            r = e.evaluate(c["split"], c["params"], [c["sfs"]], want_lc=True)
        out["m%d_llk" % i] = r.llk; out["m%d_st" % i] = r.status; out["m%d_lc" % i] = r.lc; out["m%d_j" % i] = r.jafs
    for name in ("config2", "config3"):
        w = getattr(workloads, name)(lambda *a: truth_spectrum(*a))
        n = min(w.n_cand, 4096)
        with Engine(w.times, w.lh, **w.engine_kwargs()) as e:
            r = e.evaluate(w.split_time[:n], w.params[:n], w.jsfs, want_lc=True)
        out[name + "_llk"] = r.llk; out[name + "_st"] = r.status; out[name + "_lc"] = r.lc; out[name + "_j"] = r.jafs
    out.update(searches())
    np.savez(path, **out)
    print("saved", len(out), "arrays")


SEARCH_FIELDS = ("x", "llh", "nit", "nfev", "status", "iterations_issued", "slots", "speculative_iterations")


def searches():
    """Every batched search on fixed starts, once with the default setting and once with MISTI_NM_SPEC=0 (the library reads it per
    call): misti_nm_solve, _rows, _bounds (one bound set SetModel refuses) and _split on config 3's model with its band ends following
    the split and a seeded bootstrap table; misti_nm_solve_pulses on the pulse-sweep golden's model; misti_nm_solve_split on config 4's
    model (n_param == 0); misti_basinhopping.  At most 8 starts and 300 iterations a call (AB_SEARCHES=0 leaves them out)."""
    import json
    import random
    from misti_amd import io as mio, synth, workloads
    from misti_amd.engine import Engine, truth_spectrum
    out = {}
    if os.environ.get("AB_SEARCHES", "1") == "0":
        return out

    def keep(name, r):
        for f in SEARCH_FIELDS:
            out["%s_%s" % (name, f)] = np.atleast_1d(r[f])

    w = workloads.config3(lambda *a: truth_spectrum(*a), n_start=4)
    kw = w.engine_kwargs()
    kw["bands"] = [(p, s, -1, v, k) for p, s, e, v, k in w.bands]
    table = np.array(mio.bootstrap_table(synth.chunk_rows(w.jsfs[0], 20), 4, random.Random(3)), dtype=np.float64)
    start = np.array([b[3] for b in kw["bands"]])
    starts = np.vstack([start, [0.3, 0.02], [0.05, 0.5], start * 2])
    splits = np.array([62.0, 63.5, 64.0, 65.0, 9.0])
    rows = np.array([0, 1, 2, 3, 4], dtype=np.int32)
    bounds = np.array([[[6, -1], [10, -1]], [[12, 8], [10, -1]]] * 2, dtype=np.int32)     # the second set ends before it starts
    w4 = workloads.config4(lambda *a: truth_spectrum(*a), n_split=4, n_rep=12)
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "golden_pulse_sweep.json")))
    grid, sfs = g["grids"][g["cases"][0]["in"]["grid"]], g["cases"][0]["in"]["sfs"]
    ptable = np.array(mio.bootstrap_table(synth.chunk_rows(sfs, 20), 3, random.Random(3)), dtype=np.float64)
    times = np.array([[10, 7], [5, 12]] * 2, dtype=np.int32)
    for tag, spec in (("", None), ("s0_", "0")):
        if spec is None:
            os.environ.pop("MISTI_NM_SPEC", None)
        else:
            os.environ["MISTI_NM_SPEC"] = spec
        with Engine(w.times, w.lh, **kw) as e:
            for i, st in enumerate((64.0, 63.5)):
                keep("%snm%d" % (tag, i), e.nm_solve(starts, st, table[0], maxiter=300))
            keep(tag + "rows", e.nm_solve_rows(np.tile(start, (splits.size, 1)), splits, rows, table, maxiter=300))
            keep(tag + "bounds", e.nm_solve_bounds(np.tile(start, (4, 1)), splits[:4], rows[:4], table, bounds, maxiter=300))
            keep(tag + "split", e.nm_solve_split(np.array([list(start) + [63.0], list(start) + [64.5], [0.3, 0.02, 62.0]]), [0, 2, 4], table, maxiter=200))
            r = e.basinhopping(starts[:2], 64.0, table[0], [11, 12], niter=3, nm_maxiter=100)
            for f, v in r.items():
                out["%sbh_%s" % (tag, f)] = np.atleast_1d(v)
        with Engine(grid["times"], grid["lambdas"], [(0, 4, -1, 0.2, 0)], [(0, 10, 0.05, -1), (1, 3, 0.0, 1)], n_param=2, cpfit=True, smooth=True,
                    unfolded=True) as e:
            keep(tag + "pulses", e.nm_solve_pulses(np.tile([0.2, 0.1], (4, 1)), [20.0, 20.5, 18.0, 20.0], [0, 1, 2, 0], ptable, None, times, maxiter=300))
        with Engine(w4.times, w4.lh, **w4.engine_kwargs()) as e:
            keep(tag + "split0", e.nm_solve_split((44.0 + 1.25 * np.arange(6)).reshape(6, 1), np.arange(6, dtype=np.int32), w4.jsfs, maxiter=300))
    os.environ.pop("MISTI_NM_SPEC", None)
    return out


def cmp(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = 0
    for k in a.files:
        x, y = np.atleast_1d(a[k]), np.atleast_1d(b[k])
        if not (x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))):
            bad += 1
            if bad < 10:
                print("DIFF", k, np.nanmax(np.abs(x.astype(float) - y.astype(float))))
    print("arrays", len(a.files), "different", bad)
    return bad


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) >= 4 and sys.argv[1] == "cmp":
        sys.exit(1 if cmp(sys.argv[2], sys.argv[3]) else 0)
    else:
        print(__doc__)
