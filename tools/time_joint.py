#!/usr/bin/env python3
"""Time the joint regions of coordinate pairs of the ensemble sampler on the device against the path that copies the chain and
histograms it on the host (run on the GPU box).

    python tools/time_joint.py [--rows 256] [--walkers 16] [--steps 2000] [--repeats 3] [--out FILE]

Workload: that of tools/ens_posterior_bench.py - config 3's model at its split, one ensemble per bootstrap row, burn = half the steps,
the quantiles 0.025 0.5 0.975.  The model has two coordinates, so the three pairs are (0, 1), (1, 0) and (0, 1) again.  The legs, in
turns in one process, `--repeats` timed calls each after one warm-up call of each:

    plain      Engine.ensemble_posterior without joint, no chain
    device 1   Engine.ensemble_posterior(joint=...) for one pair at 32 x 32 over the box, no chain
    device 3   the same for three pairs at 64 x 64
    host 1     Engine.ensemble_posterior(keep_chain=True) without joint, then numpy.histogram2d per fit on the copied chain, one pair
               at 32 x 32 (the two parts are timed separately as well)
    host 3     the same for three pairs at 64 x 64
    kernels    Engine.ensemble_joint_dev alone on the chain of the warm-up call, uploaded once: back-to-back calls closed by a synchronise

Reported per leg: the median, the least and the greatest seconds of a call, and the bytes that leave the device for the regions.  One
JSON line per leg is printed and written to --out."""
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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from misti_amd import _lib, io as mio, synth, workloads
    from misti_amd.engine import Engine, truth_spectrum
    from misti_amd.optimize import ensemble_joint_rule, ensemble_start, joint_counts
    w = workloads.config3(lambda *args: truth_spectrum(*args), n_start=max(a.rows, 64))
    table = np.array(mio.bootstrap_table(synth.chunk_rows(w.jsfs[0], 20), a.rows - 1, random.Random(3)), dtype=np.float64)
    R, W = table.shape[0], a.walkers
    rows = np.arange(R, dtype=np.int32)
    box = (w.params.min(axis=0), w.params.max(axis=0))
    splits = np.full(R, float(w.split_time[0]))
    init = np.stack([ensemble_start(0.5 * (box[0] + box[1]), box[0], box[1], W, 1e-2, a.seed, 0)] * R)
    burn = a.steps // 2
    kw = dict(split_times=splits, n_step=a.steps, seed=a.seed, ids=np.zeros(R, dtype=np.uint64), burn=burn, probs=(0.025, 0.5, 0.975))
    shapes = {"1": dict(pairs=[(0, 1)], bins=32), "3": dict(pairs=[(0, 1), (1, 0), (0, 1)], bins=64)}
    joint = {k: dict(v, range="box", masses=(0.95,)) for k, v in shapes.items()}
    window = lambda p: [[box[0][c], box[1][c]] for c in p]
    times, sent = {}, {}
    with Engine(w.times, w.lh, device=a.device, **w.engine_kwargs()) as eng:
        def timed(f):
            t0 = time.perf_counter()
            out = f()
            return out, time.perf_counter() - t0

        def host(k):
            r, ta = timed(lambda: eng.ensemble_posterior(init, rows, table, box, keep_chain=True, **kw))
            t0 = time.perf_counter()
            h = [[np.histogram2d(r["chain"][s, burn:, :, p[0]].reshape(-1), r["chain"][s, burn:, :, p[1]].reshape(-1), bins=shapes[k]["bins"], range=window(p))[0]
                  for p in shapes[k]["pairs"]] for s in range(R)]
            return r, h, ta, time.perf_counter() - t0

        def kernels(k):
            eng.sync()
            out, t = timed(lambda: (eng.ensemble_joint_dev(d_chain, shapes[k]["pairs"], shapes[k]["bins"], burn, d_window[k], (0.95,)), eng.sync())[0])
            return out, t

        legs = {"plain": lambda: timed(lambda: eng.ensemble_posterior(init, rows, table, box, **kw)),
                "device 1": lambda: timed(lambda: eng.ensemble_posterior(init, rows, table, box, joint=joint["1"], **kw)),
                "device 3": lambda: timed(lambda: eng.ensemble_posterior(init, rows, table, box, joint=joint["3"], **kw))}
        first = {k: f()[0] for k, f in legs.items()}                          # the warm-up calls
        r, h, _, _ = host("1")
        host("3")
        d_chain = torch.from_numpy(r["chain"]).to("cuda:%d" % a.device)
        d_window = {k: torch.tensor(np.array([window(p) for p in shapes[k]["pairs"]])).to("cuda:%d" % a.device) for k in shapes}
        for k in shapes:
            kernels(k)
        ref = ensemble_joint_rule(r["chain"], burn=burn, range=np.array([window(p) for p in shapes["3"]["pairs"]]), masses=(0.95,), **shapes["3"])
        same = all(np.ascontiguousarray(first["device 3"]["joint"][k]).tobytes() == ref[k].tobytes() for k in ("counts", "inside", "mode", "level", "cells", "held"))
        near = max(int(np.abs(joint_counts(first["device 1"]["joint"], 0, s) - h[s][0]).sum()) for s in range(R))
        old = all(first[k][n].tobytes() == first["plain"][n].tobytes() for k in ("device 1", "device 3") for n in ("mean", "cov", "quant", "tau", "window", "best_x", "last"))
        for _ in range(a.repeats):
            for k, f in legs.items():
                times.setdefault(k, []).append(f()[1])
            for k in shapes:
                _, _, ta, tb = host(k)
                times.setdefault("host %s" % k, []).append(ta + tb)
                times.setdefault("host %s: sampler, summaries and copy" % k, []).append(ta)
                times.setdefault("host %s: numpy.histogram2d per fit" % k, []).append(tb)
                times.setdefault("kernels %s" % k, []).append(kernels(k)[1])
        for k in shapes:
            j = first["device %s" % k]["joint"]
            sent["device %s" % k] = int(sum(np.asarray(j[n]).nbytes for n in ("counts", "range", "inside", "mode", "level", "cells", "held")))
            sent["host %s" % k] = int(r["chain"].nbytes + r["chain_llh"].nbytes)
        build = _lib.build_id()
    lines = []
    for leg, t in times.items():
        lines.append({"leg": leg, "rows": R, "walkers": W, "steps": a.steps, "burn": burn, "repeats": a.repeats, "build": build,
                      "seconds_median": float(np.median(t)), "seconds_min": float(np.min(t)), "seconds_max": float(np.max(t)),
                      **({"bytes_to_host_for_the_regions": sent[leg]} if leg in sent else {})})
    lines.append({"check": "the joint outputs of ensemble_posterior (3 pairs, 64 x 64) equal ensemble_joint_rule on the copied chain, bit for bit", "same": bool(same),
                  "the older summaries equal with and without joint, bit for bit": bool(old),
                  "largest sum over cells of |device counts - numpy.histogram2d| in a fit (1 pair, 32 x 32; edges may differ by an ulp)": near,
                  "slab": _lib.JOINT_SLAB, "samples_per_fit": int((a.steps - burn) * W), "chain_bytes": int(r["chain"].nbytes)})
    text = "\n".join(json.dumps(l) for l in lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
