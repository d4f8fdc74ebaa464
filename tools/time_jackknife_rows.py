#!/usr/bin/env python3
"""What the leave-out rows of a delete-m block jackknife cost: all G = ceil(CHUNKS / M) rows of a table of CHUNKS chunks made on the
device (misti_jackknife_rows_dev) against the only alternative that exists, the rule in NumPy on the host (optimize.jackknife_rows).
A timing tool: nothing asserts its numbers.

The device leg writes into one preallocated buffer; every window is one call - the copy of the chunk table included - followed by the
library's own stream synchronise, after a warm-up call of the same size: the median, lowest and highest of --windows windows.  The
host leg makes the first --host-rows rows once and is SCALED to G (a row costs the same whichever group it leaves out, to within the
part of the table in front of the group); the device rows are compared with the host's on the rows both made.  Shapes are CHUNKSxM
pairs; the default is the largest table the ABI takes and a 1 000-chunk one.

    python tools/time_jackknife_rows.py [--shapes 65535x1 1000x1] [--host-rows 256] [--windows 5] [--out profiles/jackknife_rows.txt]"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def table(n_chunk):
    """Counts in multiples of 0.1: the order of the additions shows in the last bits."""
    rng = np.random.default_rng(n_chunk)
    c = np.zeros((n_chunk, 8))
    c[:, 1:] = rng.integers(0, 400, size=(n_chunk, 7)) * 0.1
    c[:, 0] = rng.integers(1, 50, size=n_chunk) * 0.1 + c[:, 1:].sum(axis=1)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["65535x1", "1000x1"], metavar="CHUNKSxM")
    ap.add_argument("--host-rows", type=int, default=256)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from misti_amd import _lib, io as mio, synth
    from misti_amd.engine import Engine
    from misti_amd.optimize import jackknife_rows
    inp = mio.merge_psmc(mio.read_psmc_file(io.StringIO(synth.psmc_text(16, 1, synth.THETA_1))),
                         mio.read_psmc_file(io.StringIO(synth.psmc_text(17, 2, synth.THETA_2))))
    dev = torch.device("cuda", 0)
    lines = []
    with Engine(inp.times, inp.lambdas) as e:
        for shape in a.shapes:
            n_chunk, m = (int(v) for v in shape.lower().split("x"))
            c = table(n_chunk)
            G = C.c_int64(0)
            _lib.check(e._lib.misti_jackknife_geometry(n_chunk, m, C.byref(G)))
            G = G.value
            rows = torch.empty((G, 8), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()

            def call():
                _lib.check(e._lib.misti_jackknife_rows_dev(e._ctx, n_chunk, c.ctypes.data_as(C.c_void_p), m, 0, G, 0, C.c_void_p(rows.data_ptr())))
                e.sync()
            call()                                                       # warm-up at the timed size
            ts = []
            for _ in range(a.windows):
                t0 = time.perf_counter()
                call()
                ts.append(time.perf_counter() - t0)
            n_host = max(1, min(G, a.host_rows))
            t0 = time.perf_counter()
            want = jackknife_rows(c, m, first=0, n=n_host)
            t_numpy = time.perf_counter() - t0
            same = bool(np.array_equal(rows[:n_host].cpu().numpy(), want))
            med = float(np.median(ts))
            lines.append(dict(what="%d leave-out rows of %d chunks in groups of %d" % (G, n_chunk, m), build_id=_lib.build_id(), chunks=n_chunk, m=m, groups=G,
                              additions=8 * G * (n_chunk - m),
                              device_seconds=dict(median=round(med, 6), lowest=round(min(ts), 6), highest=round(max(ts), 6), windows=a.windows),
                              host_rows=n_host, device_rows_equal_jackknife_rows=same,
                              optimize_jackknife_rows_seconds=dict(measured_at_host_rows=round(t_numpy, 4), scaled_to_groups=round(t_numpy * G / n_host, 2))))
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
