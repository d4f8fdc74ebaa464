#!/usr/bin/env python3
"""Time the profile likelihood per group and replicate against the two ways of getting at it that existed before (run on the GPU box).

    python tools/time_scan_profile.py [--out FILE]

On hand-made spectra (random, normalised) and random counts at the headline bootstrap shape, 65 536 candidates x 1 000 rows, with 64
groups and with 4 096 groups (labels: candidate index modulo the group count - a grid's innermost axis), three legs on the SAME
buffers in one session, each on a fresh context:

    profile   misti_scan_profile_dev alone: no table
    table     misti_llk_dev into the [n_cand][n_rep] table, then torch.amax over the grouped view of it (values only, no indices)
    scan_k1   misti_scan_best_dev with k = 1: the same n_cand x n_rep fma chains with one group - what the profile should cost

Per leg: warm-up calls, then `--reps` windows of back-to-back calls, each closed by a device synchronise and timed by the host clock;
the window is sized so that it lasts about `--window-ms`; the legs' windows ALTERNATE, so that a drift of the machine reaches all of
them.  A cold call (the first one of the context, its buffers not yet allocated) is reported beside the warm ones.  Reported: the
median, the lowest and the highest per-call time of the windows and the device memory the leg took.  The profile is checked against
the table's reduction (values bit for bit) before anything is timed.  One JSON line per (leg, shape) is printed and appended to
--out."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((65536, 1000, 64), (65536, 1000, 4096))


def grid():
    import io
    from misti_amd import synth, io as mio
    return mio.merge_psmc(mio.read_psmc_file(io.StringIO(synth.psmc_text(16, 1, synth.THETA_1))),
                          mio.read_psmc_file(io.StringIO(synth.psmc_text(17, 2, synth.THETA_2))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7, help="timed windows per leg and shape (the median is reported; at least 5)")
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_profile_timing.jsonl"))
    ap.add_argument("--tag", default="", help="free text kept in every line (which build this is)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    import torch
    from misti_amd import _lib
    from misti_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit("time_scan_profile: no GPU - a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    inp = grid()
    lines = []
    for n, R, G in SHAPES:
        rng = np.random.default_rng(n + G)
        j = rng.random((n, 7)) + 0.05
        rows = np.zeros((R, 8))
        rows[:, 1:] = rng.integers(0, 50000, size=(R, 7))
        rows[:, 0] = rows[:, 1:].sum(axis=1)
        d_j = torch.as_tensor(j / j.sum(axis=1, keepdims=True), device=dev)
        d_r = torch.as_tensor(rows, device=dev)
        d_g = torch.as_tensor((np.arange(n) % G).astype(np.int32), device=dev)
        legs = {}
        for leg in ("profile", "table", "scan_k1"):
            e = Engine(inp.times, inp.lambdas)                       # a fresh context: its buffers are this leg's alone
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info(dev)[0]
            if leg == "profile":
                val = torch.empty((R, G), dtype=torch.float64, device=dev)
                best = torch.empty((R, G), dtype=torch.int32, device=dev)
                call = lambda e=e, val=val, best=best: e.scan_profile_dev(n, d_j.data_ptr(), 0, d_g.data_ptr(), G, R, d_r.data_ptr(), val.data_ptr(),
                                                                          best.data_ptr())
                done = e.sync
            elif leg == "table":
                table = torch.empty((n, R), dtype=torch.float64, device=dev)
                val = torch.empty((G, R), dtype=torch.float64, device=dev)
                stream = torch.cuda.ExternalStream(e.stream_handle(), device=dev)      # the reduction follows the table on the engine's stream

                def call(e=e, table=table, val=val, stream=stream):
                    e.llk_dev(n, d_j.data_ptr(), 0, R, d_r.data_ptr(), table.data_ptr())
                    with torch.cuda.stream(stream):
                        torch.amax(table.view(n // G, G, R), dim=0, out=val)
                done = e.sync
            else:
                val = torch.empty((R, 1), dtype=torch.float64, device=dev)
                best = torch.empty((R, 1), dtype=torch.int32, device=dev)
                call = lambda e=e, val=val, best=best: e.scan_best_dev(n, d_j.data_ptr(), 0, R, d_r.data_ptr(), 1, best.data_ptr(), val.data_ptr())
                done = e.sync
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            done()
            cold = time.perf_counter() - t0
            taken = free0 - torch.cuda.mem_get_info(dev)[0]
            for _ in range(a.warmup):
                call()
            done()
            t0 = time.perf_counter()
            call()
            done()
            one = time.perf_counter() - t0
            legs[leg] = dict(e=e, call=call, done=done, val=val, cold=cold, taken=taken, per_call=[],
                             calls=max(4, min(20000, int(a.window_ms * 1e-3 / max(one, 1e-6)))))
        # the profile's values are the table's, reduced: bit for bit (amax never picks a NaN here: every candidate has a value)
        if not torch.equal(legs["profile"]["val"], legs["table"]["val"].T.contiguous()):
            raise SystemExit("time_scan_profile: the profile differs from the reduced table at %d x %d, %d groups" % (n, R, G))
        for _ in range(a.reps):                                      # alternate the legs' windows
            for leg, L in legs.items():
                t0 = time.perf_counter()
                for _ in range(L["calls"]):
                    L["call"]()
                L["done"]()
                L["per_call"].append((time.perf_counter() - t0) / L["calls"])
        for leg, L in legs.items():
            p = L["per_call"]
            rec = dict(leg=leg, tag=a.tag, build=_lib.build_id(), n_cand=n, n_rep=R, n_group=G, calls_per_window=L["calls"], windows=a.reps,
                       ms_per_call_median=1e3 * statistics.median(p), ms_per_call_min=1e3 * min(p), ms_per_call_max=1e3 * max(p),
                       ms_cold_call=1e3 * L["cold"], device_bytes_taken=int(L["taken"]), device=torch.cuda.get_device_name(dev))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            L["e"].close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
