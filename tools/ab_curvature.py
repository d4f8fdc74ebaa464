#!/usr/bin/env python3
"""A/B of misti_curvature between two builds of the library (run on the GPU box), at the points of
tests/golden/golden_curvature_exact.json.gz - what tools/ab_compare.py does not cover.

    MISTI_LIB_AB=1 MISTI_LIB=/tmp/variant.so python tools/ab_curvature.py dump a.npz     # a variant build (python -m misti_amd.build --out ...)
    python tools/ab_curvature.py dump b.npz                                              # the in-tree build
    python tools/ab_curvature.py cmp a.npz b.npz        # per array: the same bits or not, and the largest relative difference of an entry

Smooth model, rel_step 1e-1, 1e-2 and 1e-4, the points with a purely relative step.  The `ab_curvature` lines of
profiles/curvature_exact.txt were made with it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def dump(path):
    import curvature_exact as cx
    from misti_amd.engine import Engine
    out = {}
    for m in cx.load()["models"]:
        ps = [p for p in m["points"] if not p["boundary"] and p["abs_step"] == 0]
        with Engine(m["times"], m["lh"], [tuple(b) for b in m["bands"]], [tuple(p) for p in m["pulses"]], n_param=m["n_param"], cpfit=True,
                    true_eps=True, unfolded=m["unfolded"], sample_date=m["sample_date"]) as e:
            for rel in (1e-1, 1e-2, 1e-4):
                r = e.curvature(np.array([p["x"] for p in ps]), np.array([p["split"] for p in ps]), np.zeros(len(ps), dtype=np.int32),
                                np.array(ps[0]["table"], dtype=np.float64), rel_step=rel)
                for k in ("llh0", "grad", "hess", "dlog", "status"):
                    out["%s_rel%g_%s" % (m["name"], rel, k)] = getattr(r, k)
    np.savez(path, **out)
    print("saved", len(out), "arrays")


def cmp(pa, pb):
    a, b = np.load(pa), np.load(pb)
    for k in sorted(a.files):
        x, y = a[k], b[k]
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.nanmax(np.abs(x - y) / np.abs(x)) if x.dtype.kind == "f" and x.size else 0.0
        print("ab_curvature %-55s %s max rel diff %.2e" % (k, "same bits" if x.tobytes() == y.tobytes() else "DIFFERS  ", rel))


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) >= 4 and sys.argv[1] == "cmp":
        cmp(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
