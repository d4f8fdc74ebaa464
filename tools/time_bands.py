"""Time misti_traj_bands_dev against the recipe it replaces (copy lc to the host, sort and select there with NumPy) on synthetic rates.

    python tools/time_bands.py [--numT 128] [--m 32000] [--groups 8] [--repeat 5] [--out profiles/bands_reduce.txt]

The device figure is the median over `repeat` calls of the wall time between two stream events around the call (all outputs, three
probabilities), after two warm-up calls.  The gather moves 16 bytes per kept value (8 read, 8 written); the ABI has no call that
launches the gather alone, so the bandwidth printed is that traffic over the WHOLE call's time: a lower bound of the gather's own, which
a kernel trace of this script (rocprofv3 --kernel-trace --stats) refines.  The host figure: the device-to-host copy of lc,
then per group a key transform, numpy.sort along the samples and the order statistics of three probabilities, on as many threads as
--threads says (groups are dealt over a thread pool; NumPy releases the GIL in sort)."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--numT", type=int, default=128)
    ap.add_argument("--m", type=int, default=32000)
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from misti_amd.engine import Engine
    from misti_amd.optimize import post_order_key
    G, m, T = a.groups, a.m, a.numT
    probs = (0.025, 0.5, 0.975)
    eng = Engine(np.arange(1, T) * 0.1, np.ones((T, 2)))
    gen = torch.Generator(device="cuda").manual_seed(1)
    lc = torch.exp(torch.randn((G, m, T + 1, 2), dtype=torch.float64, device="cuda", generator=gen))
    split = torch.rand((G, m), dtype=torch.float64, device="cuda", generator=gen) * (T + 1)
    status = torch.zeros((G, m), dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()                                 # not the null stream: the engine would take that for "its own"
    eng.use_stream(stream.cuda_stream)
    torch.cuda.synchronize()
    times = []
    for it in range(a.repeat + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = eng.trajectory_bands_dev(lc, split, status, probs=probs)
        e1.record(stream)
        e1.synchronize()
        eng.sync()
        if it >= 2:
            times.append(e0.elapsed_time(e1))
    dev_ms = float(np.median(times))
    kept = G * m * 2 * T
    lines = ["trajectory bands: numT = %d, m = %d, G = %d, all outputs, probs %s" % (T, m, G, probs),
             "device  misti_traj_bands_dev  median of %d: %.3f ms  (each: %s)" % (a.repeat, dev_ms, " ".join("%.3f" % t for t in times)),
             "        gather traffic 16 B x %d values = %.1f MB; over the WHOLE call's time: %.3f TB/s (a lower bound of the gather's own)"
             % (kept, 16e-6 * kept, 16.0 * kept / (dev_ms * 1e-3) / 1e12)]
    # the recipe it replaces
    t0 = time.perf_counter()
    h_lc, h_split = lc.cpu().numpy(), split.cpu().numpy()
    t1 = time.perf_counter()
    def one(g):
        below = np.arange(T)[None, :] < h_split[g][:, None]                               # [m][T]
        v = h_lc[g, :, :T, :]
        key = np.where(below[:, :, None] & ~np.isnan(v), post_order_key(v), np.uint64(2 ** 64 - 1))
        key = np.sort(key, axis=0)
        n = (key != np.uint64(2 ** 64 - 1)).sum(axis=0)
        return key[np.clip(((n - 1)[None] * np.asarray(probs)[:, None, None]).astype(np.int64), 0, m - 1), np.arange(T)[None, :, None], np.arange(2)[None, None, :]]
    with ThreadPoolExecutor(a.threads) as pool:
        list(pool.map(one, range(G)))
    t2 = time.perf_counter()
    lines += ["host    device-to-host copy of lc (%.0f MB): %.1f ms; NumPy keys, sort and order statistics on %d threads: %.1f ms; together %.1f ms"
              % (h_lc.nbytes / 1e6, 1e3 * (t1 - t0), a.threads, 1e3 * (t2 - t1), 1e3 * (t2 - t0)),
              "ratio   %.1f x" % (1e3 * (t2 - t0) / dev_ms)]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    eng.close()


if __name__ == "__main__":
    main()
