"""The fixture of misti_lsq_probe without a GPU (tests/golden/make_lsq_probe.py): its conditions and coverage, the float64
restatement (tests/lsq_rule.py) run again - same rows, same side of every comparison as the 80-digit run - and against NumPy's and
SciPy's own functions, the argument checks of the entry, which all come before the context is looked at, and its declaration."""
import ctypes as C
import gzip
import json
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import lsq_rule as R
import make_lsq_probe as G


@pytest.fixture(scope="module")
def fx():
    with gzip.open(os.path.join(HERE, "golden", "golden_lsq_probe.json.gz"), "rt") as f:
        return json.load(f)


def test_fixture_conditions_and_coverage(fx):
    assert G.check(fx)
    assert os.path.getsize(G.OUT) < (1 << 20)
    assert fx["header"]["device_factor"] == R.DEVICE_FACTOR == 4.0 and fx["header"]["scalar_ulps"] == R.SCALAR_ULPS
    assert sorted(fx["kinds"]) == sorted(R.KINDS)


def _same(a, b):
    return all(x == y or (x != x and y != y) for x, y in zip(a, b))


@pytest.mark.parametrize("kind", sorted(R.KINDS))
def test_restatement_takes_the_exact_side_of_every_comparison(fx, kind):
    """The restatement run again: the stored rows bit for bit, and the outcome of every live comparison that of the 80-digit run."""
    for p in fx["kinds"][kind]:
        K = R.F64()
        row, _ = R.run(K, kind, p["in"])
        assert _same(row[:len(p["rule"])], p["rule"]), (kind, p["t"], row, p["rule"])
        assert "".join("1" if o else "0" for (_, _, o) in R.live(K.trace)) == p["seq"], (kind, p["t"])
        assert R.discrete(kind, p, row) == p["disc"]
    w = R.worst(kind, fx["kinds"][kind], [p["rule"] for p in fx["kinds"][kind]])
    assert w == {c: v["rule"] for c, v in fx["header"]["worst"][kind].items()}


# classes in which SciPy's answer is not comparable: a zero singular value leaves LAPACK's vectors arbitrary, a step outside the
# region is refused, and at |det| <~ eps F nothing has a correct digit
NOT_UNIQUE = {"zero_col", "both_zero", "n1_zero", "det_below", "singular"}


@pytest.mark.parametrize("kind", ["SVD2", "SVD4", "STEP", "STEPN", "SELECT", "UPDATE", "SOLVE3"])
def test_restatement_against_scipy(fx, kind):
    """NumPy's / SciPy's own functions, run here: the same discrete outcome as the restatement on every problem SciPy answers, and
    values inside the device's bound around the exact answers (which checks the exact answers against LAPACK as well)."""
    head, n = fx["header"]["worst"][kind], 0
    for p in fx["kinds"][kind]:
        if set(p["t"]) & NOT_UNIQUE or "nan" in p["t"]:
            continue
        sp, info = R.scipy_row(kind, p["in"])
        if sp is None:
            assert "shrunk_radius" in p["t"]
            continue
        n += 1
        if "rank1" in p["t"]:
            # SciPy iterates on alpha there and rescales to the radius; the device writes the step down: the same step, alpha = 0
            assert abs(sp[0] - p["rule"][0]) <= 4 * R.EPS * p["in"][6] and abs(sp[1] - p["rule"][1]) <= 4 * R.EPS * p["in"][6], (sp, p["rule"])
            continue
        if kind in ("STEP", "STEPN"):
            assert info["iters"] == p["ex"]["iters"] and (sp[2] == 0.0) == p["disc"]["alpha0"], (p["t"], info, p["ex"]["iters"])
        elif kind in ("SELECT", "UPDATE"):
            assert R.discrete(kind, p, sp) == p["disc"], (p["t"], sp, p["rule"])
        for c, v in R.figures(kind, p, sp).items():
            bound = 0.01 if c.endswith(":phi") else R.DEVICE_FACTOR * max(head[c]["rule"], head[c]["scipy"] or 0.0, 0.5)
            assert v <= bound or ("iters10" in p["t"] and c.endswith(":phi")), (kind, c, v, bound, p["t"])
    refused = sum("shrunk_radius" in p["t"] for p in fx["kinds"][kind])
    assert n >= len([p for p in fx["kinds"][kind] if not (set(p["t"]) & NOT_UNIQUE or "nan" in p["t"] or "rank1" in p["t"])]) - refused


def _call(L, ctx, kind, n, probs, out=True):
    a = None if probs is None else np.ascontiguousarray(probs, dtype=np.float64)
    o = np.zeros((max(n, 1), R.LSQ_OUT)) if out else None
    ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    return L.misti_lsq_probe(ctx, kind, n, ptr(a), ptr(o))


def test_probe_checks_its_arguments_before_the_context():
    """misti_lsq_probe WITHOUT a context (there is no device here): a bad argument is reported as such, a good one gets as far as
    'ctx is NULL'."""
    from misti_amd import _lib
    L = _lib.load()
    E_ARG = -1
    E_LIMIT = L.misti_lsq_probe(None, 0, (1 << 20) + 1, None, None)
    assert E_LIMIT not in (E_ARG, 0) and b"MISTI_LSQ_MAX_PROBLEMS" in L.misti_last_error()
    good = [0.0] * R.LSQ_IN
    for kind in range(8):
        row = list(good)
        row[12], row[19] = 1.0, 2.0
        assert _call(L, None, kind, 1, [row]) == E_ARG and b"ctx is NULL" in L.misti_last_error()
    assert _call(L, None, 0, 0, None, out=False) == E_ARG and b"ctx is NULL" in L.misti_last_error()
    for kind in (-1, 8, 100):
        assert _call(L, None, kind, 1, [good]) == E_ARG and b"kind" in L.misti_last_error()
    assert _call(L, None, 0, -1, [good]) == E_ARG and b"negative" in L.misti_last_error()
    assert _call(L, None, 0, 1, None) == E_ARG and b"NULL" in L.misti_last_error() and b"ctx" not in L.misti_last_error()
    assert _call(L, None, 0, 1, [good], out=False) == E_ARG and b"ctx" not in L.misti_last_error()
    for kind, at in ((2, 12), (4, 12), (5, 19)):
        for bad in (0.0, 3.0, 1.5, math.nan):
            row = list(good)
            row[12], row[19] = 1.0, 1.0
            row[at] = bad
            assert _call(L, None, kind, 2, [[0.0] * 12 + [1.0] + [0.0] * 6 + [1.0], row]) == E_ARG
            assert b"N " in L.misti_last_error() and b"problems[1]" in L.misti_last_error()
    assert _call(L, None, 6, 1, [[0.5] + good[1:]]) == E_ARG and b"finite" in L.misti_last_error()
    # the values of a problem may be anything
    assert _call(L, None, 0, 1, [[math.nan] + good[1:]]) == E_ARG and b"ctx is NULL" in L.misti_last_error()
    assert _call(L, None, 7, 1, [[math.inf] * R.LSQ_IN]) == E_ARG and b"ctx is NULL" in L.misti_last_error()


def test_probe_is_declared_and_bound():
    import re
    from misti_amd import _lib
    from misti_amd.engine import Engine
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "misti_hip.h")).read()
    assert re.search(r"^int misti_lsq_probe\(misti_ctx\* ctx, int kind, int64_t n, const double\* problems", hdr, flags=re.M)
    assert "#define MISTI_ABI_VERSION 6" in hdr and hdr.index("introspection (tests)") < hdr.index("int misti_pair_residuals(") < hdr.index("int misti_lsq_probe(")
    assert "#define MISTI_LSQ_IN %d\n" % R.LSQ_IN in hdr and "#define MISTI_LSQ_OUT %d\n" % R.LSQ_OUT in hdr
    for name, k in R.KINDS.items():
        assert "MISTI_LSQ_%s = %d" % (name, k) in hdr
    assert Engine.LSQ_KINDS == R.KINDS and (Engine.LSQ_IN, Engine.LSQ_OUT) == (R.LSQ_IN, R.LSQ_OUT)
    assert "misti_lsq_probe" in _lib.SYMBOLS
