#!/usr/bin/env python3
"""Time the posterior summaries of the ensemble sampler on the device against the path that copies the chain (run on the GPU box).

    python tools/ens_posterior_bench.py [--rows 256] [--walkers 16] [--steps 2000] [--repeats 5] [--out FILE]

Workload: config 3's model (numT = 128, two optimised bands, --cpfit) at its split, one ensemble per bootstrap row (the data row and
rows - 1 block-bootstrap rows of its 20 chunks), ensemble_start (spread 1e-2, stream 0) around the centre of the box config 3's random
starts span, T = 1, a = 2, no thinning, burn = half the steps, the quantiles 0.025 0.5 0.975.  Three legs, in turns in one process,
`--repeats` timed calls each after one warm-up call of each:

    host       Engine.ensemble_sample with the chain copied out, then optimize.ensemble_summary fit by fit: what `--mcmc` does (its two
               parts are timed separately as well)
    device     Engine.ensemble_posterior without the chain: the sampler, the summary kernels, the summaries copied
    kernels    Engine.ensemble_summary_dev alone on the chain of the warm-up call, uploaded once: back-to-back calls on the context's
               stream closed by a synchronise

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
    from misti_amd.optimize import ensemble_start, ensemble_summary
    w = workloads.config3(lambda *args: truth_spectrum(*args), n_start=max(a.rows, 64))
    table = np.array(mio.bootstrap_table(synth.chunk_rows(w.jsfs[0], 20), a.rows - 1, random.Random(3)), dtype=np.float64)
    R, W = table.shape[0], a.walkers
    rows = np.arange(R, dtype=np.int32)
    box = (w.params.min(axis=0), w.params.max(axis=0))
    splits = np.full(R, float(w.split_time[0]))
    init = np.stack([ensemble_start(0.5 * (box[0] + box[1]), box[0], box[1], W, 1e-2, a.seed, 0)] * R)
    burn, probs = a.steps // 2, (0.025, 0.5, 0.975)
    kw = dict(split_times=splits, n_step=a.steps, seed=a.seed, ids=np.zeros(R, dtype=np.uint64))
    times = {k: [] for k in ("host", "host: sampler and copy", "host: summary loop", "device", "kernels")}
    with Engine(w.times, w.lh, device=a.device, **w.engine_kwargs()) as eng:
        def host():
            t0 = time.perf_counter()
            r = eng.ensemble_sample(init, rows, table, box, **kw)
            t1 = time.perf_counter()
            s = [ensemble_summary(r["chain"][i], burn, accepted=r["accepted"][i], n_step=a.steps) for i in range(R)]
            return r, s, t1 - t0, time.perf_counter() - t1

        def device():
            return eng.ensemble_posterior(init, rows, table, box, burn=burn, probs=probs, **kw)

        r, s, _, _ = host()                                                      # the warm-up calls
        post = device()
        d_chain = torch.from_numpy(r["chain"]).to("cuda:%d" % a.device)
        d_llh = torch.from_numpy(r["chain_llh"]).to("cuda:%d" % a.device)
        alone = eng.ensemble_summary_dev(d_chain, d_llh, burn, probs)
        eng.sync()
        same = all(np.array_equal(alone[k].cpu().numpy(), post[k], equal_nan=True) for k in ("mean", "cov", "quant", "tau", "window", "best_llh", "best_at"))
        for _ in range(a.repeats):
            _, _, ta, tb = host()
            times["host"].append(ta + tb)
            times["host: sampler and copy"].append(ta)
            times["host: summary loop"].append(tb)
            t0 = time.perf_counter()
            device()
            times["device"].append(time.perf_counter() - t0)
            eng.sync()
            t0 = time.perf_counter()
            eng.ensemble_summary_dev(d_chain, d_llh, burn, probs)
            eng.sync()
            times["kernels"].append(time.perf_counter() - t0)
        build = _lib.build_id()
    med = np.array([v["median"] for v in s])
    lines = []
    for leg, t in times.items():
        lines.append({"leg": leg, "rows": R, "walkers": W, "steps": a.steps, "burn": burn, "repeats": a.repeats, "build": build,
                      "seconds_median": float(np.median(t)), "seconds_min": float(np.min(t)), "seconds_max": float(np.max(t))})
    lines.append({"check": "the summaries of ensemble_posterior equal ensemble_summary_dev on the copied chain", "same": bool(same),
                  "chain_bytes": int(r["chain"].nbytes + r["chain_llh"].nbytes), "median_tau": float(np.median(post["tau"])),
                  "median_window": float(np.median(post["window"])),
                  "largest_difference_of_medians_device_minus_host": float(np.max(np.abs(post["quant"][:, :, 1] - med)))})
    text = "\n".join(json.dumps(l) for l in lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
