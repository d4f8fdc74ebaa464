#!/usr/bin/env python3
"""Time the per-replicate reduction of a bootstrap scan with and without the likelihood table (run on the GPU box).

    python tools/time_scan_best.py --leg table [--out FILE]     # misti_llk_dev + misti_argmax_dev: the [n_cand][n_rep] table, then its arg-max
    python tools/time_scan_best.py --leg fused [--out FILE]     # misti_scan_best_dev at k = 1 and k = 8: no table

Both legs run on hand-made spectra (random, normalised) and random counts at 256 x 1 000 (config 4's shape) and 65 536 x 1 000.  The
table leg uses only entry points an older build has as well, so with MISTI_LIB=<older build> MISTI_LIB_AB=1 it times that build: the
yardstick.  Per shape: warm-up calls, then `--reps` windows of back-to-back calls on the context's stream, each closed by a device
synchronise and timed by the host clock; the window is sized so that it lasts about `--window-ms`.  Reported: the median, the lowest
and the highest per-call time of the windows, and how much device memory the leg took (free memory before the buffers were
allocated minus after the first call: the caller's outputs plus what the context allocated; the allocator's granularity included).
One JSON line per (leg, shape, k) is printed and appended to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((256, 1000), (65536, 1000))


def grid():
    import io
    from misti_amd import synth, io as mio
    return mio.merge_psmc(mio.read_psmc_file(io.StringIO(synth.psmc_text(16, 1, synth.THETA_1))),
                          mio.read_psmc_file(io.StringIO(synth.psmc_text(17, 2, synth.THETA_2))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", choices=("table", "fused"), required=True)
    ap.add_argument("--reps", type=int, default=7, help="timed windows per shape (the median is reported; at least 5)")
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_best_timing.jsonl"))
    ap.add_argument("--tag", default="", help="free text kept in every line (which build this is)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    import torch
    from misti_amd import _lib
    from misti_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit("time_scan_best: no GPU - a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    inp = grid()
    lines = []
    for n, R in SHAPES:
        rng = np.random.default_rng(n)
        j = rng.random((n, 7)) + 0.05
        rows = np.zeros((R, 8))
        rows[:, 1:] = rng.integers(0, 50000, size=(R, 7))
        rows[:, 0] = rows[:, 1:].sum(axis=1)
        d_j = torch.as_tensor(j / j.sum(axis=1, keepdims=True), device=dev)
        d_r = torch.as_tensor(rows, device=dev)
        for k in ((1,) if a.leg == "table" else (1, 8)):
            with Engine(inp.times, inp.lambdas) as e:               # a fresh context: its buffers are this leg's alone
                torch.cuda.synchronize()
                free0 = torch.cuda.mem_get_info(dev)[0]
                best = torch.empty((R, k), dtype=torch.int32, device=dev)
                val = torch.empty((R, k), dtype=torch.float64, device=dev)
                if a.leg == "table":
                    table = torch.empty((n, R), dtype=torch.float64, device=dev)

                    def call():
                        e.llk_dev(n, d_j.data_ptr(), 0, R, d_r.data_ptr(), table.data_ptr())
                        e.argmax_dev(n, R, table.data_ptr(), best.data_ptr(), val.data_ptr())
                else:
                    def call():
                        e.scan_best_dev(n, d_j.data_ptr(), 0, R, d_r.data_ptr(), k, best.data_ptr(), val.data_ptr())
                torch.cuda.synchronize()
                call()
                e.sync()
                taken = free0 - torch.cuda.mem_get_info(dev)[0]
                for _ in range(a.warmup):
                    call()
                e.sync()
                t0 = time.perf_counter()
                call()
                e.sync()
                one = time.perf_counter() - t0
                calls = max(4, min(20000, int(a.window_ms * 1e-3 / max(one, 1e-6))))
                per_call = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        call()
                    e.sync()
                    per_call.append((time.perf_counter() - t0) / calls)
                check = int(best[:, 0].to(torch.int64).sum().item())
            rec = dict(leg=a.leg, tag=a.tag, build=_lib.build_id(), n_cand=n, n_rep=R, k=k, calls_per_window=calls, windows=a.reps,
                       ms_per_call_median=1e3 * statistics.median(per_call), ms_per_call_min=1e3 * min(per_call), ms_per_call_max=1e3 * max(per_call),
                       device_bytes_taken=int(taken), sum_of_first_places=check, device=torch.cuda.get_device_name(dev))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
