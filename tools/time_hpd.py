#!/usr/bin/env python3
"""Time the shortest (HPD) intervals of the ensemble sampler on the device against the path that copies the chain and sorts on the host
(run on the GPU box).

    python tools/time_hpd.py [--rows 256] [--walkers 16] [--steps 2000] [--repeats 5] [--out FILE]

Workload: that of tools/ens_posterior_bench.py - config 3's model at its split, one ensemble per bootstrap row, burn = half the steps,
the quantiles 0.025 0.5 0.975 - with the mass 0.95.  Four legs, in turns in one process, `--repeats` timed calls each after one warm-up
call of each:

    host       Engine.ensemble_posterior(keep_chain=True), then optimize.ensemble_hpd_rule on the copied chain: what the interval cost
               before the device sorted (the two parts are timed separately as well)
    device     Engine.ensemble_posterior(masses=(0.95,)) without the chain: the sampler, the summary kernels, the sort, the window scan
    plain      Engine.ensemble_posterior without masses: it launches nothing new
    kernels    Engine.ensemble_summary_dev alone on the chain of the warm-up call, uploaded once, with the intervals and without: back-to-
               back calls on the context's stream closed by a synchronise

Reported per leg: the median, the least and the greatest seconds of a call.  One JSON line per leg is printed and written to --out."""
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
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--walkers", type=int, default=16)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from misti_amd import _lib, io as mio, synth, workloads
    from misti_amd.engine import Engine, truth_spectrum
    from misti_amd.optimize import ensemble_hpd_rule, ensemble_start
    w = workloads.config3(lambda *args: truth_spectrum(*args), n_start=max(a.rows, 64))
    table = np.array(mio.bootstrap_table(synth.chunk_rows(w.jsfs[0], 20), a.rows - 1, random.Random(3)), dtype=np.float64)
    R, W = table.shape[0], a.walkers
    rows = np.arange(R, dtype=np.int32)
    box = (w.params.min(axis=0), w.params.max(axis=0))
    splits = np.full(R, float(w.split_time[0]))
    init = np.stack([ensemble_start(0.5 * (box[0] + box[1]), box[0], box[1], W, 1e-2, a.seed, 0)] * R)
    burn, probs, masses = a.steps // 2, (0.025, 0.5, 0.975), (0.95,)
    kw = dict(split_times=splits, n_step=a.steps, seed=a.seed, ids=np.zeros(R, dtype=np.uint64), burn=burn, probs=probs)
    legs = ("host", "host: sampler, summaries and copy", "host: ensemble_hpd_rule", "device", "plain", "kernels: with the intervals", "kernels: without")
    times = {k: [] for k in legs}
    with Engine(w.times, w.lh, device=a.device, **w.engine_kwargs()) as eng:
        def host():
            t0 = time.perf_counter()
            r = eng.ensemble_posterior(init, rows, table, box, keep_chain=True, **kw)
            t1 = time.perf_counter()
            h = ensemble_hpd_rule(r["chain"], burn=burn, masses=masses)
            return r, h, t1 - t0, time.perf_counter() - t1

        def timed(f):
            t0 = time.perf_counter()
            out = f()
            return out, time.perf_counter() - t0

        def kernels(**more):
            eng.sync()
            t0 = time.perf_counter()
            out = eng.ensemble_summary_dev(d_chain, d_llh, burn, probs, **more)
            eng.sync()
            return out, time.perf_counter() - t0

        r, h, _, _ = host()                                                      # the warm-up calls
        post, _ = timed(lambda: eng.ensemble_posterior(init, rows, table, box, masses=masses, **kw))
        plain, _ = timed(lambda: eng.ensemble_posterior(init, rows, table, box, **kw))
        d_chain = torch.from_numpy(r["chain"]).to("cuda:%d" % a.device)
        d_llh = torch.from_numpy(r["chain_llh"]).to("cuda:%d" % a.device)
        kernels(masses=masses)
        kernels()
        same = all(post[k].tobytes() == h[k].tobytes() for k in ("hpd", "hpd_at"))
        old = all(post[k].tobytes() == plain[k].tobytes() == r[k].tobytes() for k in ("mean", "cov", "quant", "tau", "window", "best_llh", "best_x", "best_at"))
        for _ in range(a.repeats):
            _, _, ta, tb = host()
            times["host"].append(ta + tb)
            times["host: sampler, summaries and copy"].append(ta)
            times["host: ensemble_hpd_rule"].append(tb)
            times["device"].append(timed(lambda: eng.ensemble_posterior(init, rows, table, box, masses=masses, **kw))[1])
            times["plain"].append(timed(lambda: eng.ensemble_posterior(init, rows, table, box, **kw))[1])
            times["kernels: with the intervals"].append(kernels(masses=masses)[1])
            times["kernels: without"].append(kernels()[1])
        build = _lib.build_id()
    lines = []
    for leg, t in times.items():
        lines.append({"leg": leg, "rows": R, "walkers": W, "steps": a.steps, "burn": burn, "repeats": a.repeats, "build": build,
                      "seconds_median": float(np.median(t)), "seconds_min": float(np.min(t)), "seconds_max": float(np.max(t))})
    q = post["quant"]
    lines.append({"check": "hpd and hpd_at of ensemble_posterior equal ensemble_hpd_rule on the copied chain, bit for bit", "same": bool(same),
                  "the eight older summaries equal with and without masses, bit for bit": bool(old), "sort_tile": _lib.POST_SORT_TILE,
                  "samples_per_marginal": int((a.steps - burn) * W), "chain_bytes": int(r["chain"].nbytes),
                  "sort_workspace_bytes": int(2 * r["chain"][:, burn:].nbytes),
                  "median_width_hpd_over_equal_tailed": float(np.median((post["hpd"][:, :, 0, 1] - post["hpd"][:, :, 0, 0]) / (q[:, :, 2] - q[:, :, 0])))})
    text = "\n".join(json.dumps(l) for l in lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
