"""The pair-chain fixtures without a GPU (tests/golden/make_pair_branches.py): the coverage they promise, the float64 restatements of
the cascade, Taylor, uniformisation and reduced forms (tests/pair_branches.py) inside the bounds the device is held to, and the
argument checks of misti_pair_residuals, which all come before the context is looked at."""
import ctypes as C
import gzip
import json
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

import pair_branches as pb


def load(name):
    with gzip.open(os.path.join(HERE, "golden", name), "rt") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def fwd():
    return load("golden_pair_branches.json.gz")


@pytest.fixture(scope="module")
def res():
    return load("golden_pair_residuals.json.gz")


def test_fixture_coverage(fwd, res):
    assert pb.coverage_forward(fwd) >= 1000
    assert 150 <= pb.coverage_residuals(res) <= 400
    assert fwd["bound"] == res["bound"] == pb.W_BOUND == 2e-13


def test_labels_are_the_restated_branches(fwd, res):
    for m in fwd["models"]:
        for c in m["candidates"]:
            for t, iv in enumerate(c["intervals"]):
                a0, a1, b0, b1, q = pb.forward_interval(m["lh"][t][0], m["lh"][t][1], c["params"][0], c["params"][1], m["times"][t])
                assert iv["branch"] == pb.branch(b0, b1, q) and iv["nbmax"] == q
    for p in res["problems"]:
        l0, l1, q, neg, ok = pb.eval_point(p["mu0"], p["mu1"], p["x0"], p["x1"], p["role"])
        assert (l0, l1, q + neg) == (p["l0"], p["l1"], p["nbmax"]) and ok
        if p["role"] >= 2:                                   # the stepped rate: x + sqrt(eps) sign(x) max(1, |x|)
            x = p["x0"] if p["role"] < 4 else p["x1"]
            assert (l0 if p["role"] < 4 else l1) == x + 1.4901161193847656e-08 * math.copysign(1.0, x) * max(1.0, abs(x))


def test_float64_restatements_of_the_forward_map(fwd):
    """The chain of every candidate in float64 Python, interval by interval in the device's branch (pair_eigen is not restated: a
    two-way stiff interval continues from the exact state).  Same bound as the device."""
    worst = {}
    for m in fwd["models"]:
        for c in m["candidates"]:
            v = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
            for t, iv in enumerate(c["intervals"]):
                a0, a1, b0, b1, q = pb.forward_interval(m["lh"][t][0], m["lh"][t][1], c["params"][0], c["params"][1], m["times"][t])
                want = [[c["exact"][t][2 * i + k] for i in range(3)] for k in range(2)]
                for k in range(2):
                    got = pb.expv64(a0, a1, b0, b1, v[k], q, 0.0)
                    scale = max(abs(x) for x in c["exact"][t])
                    if got is None or scale < pb.NORM_FLOOR:
                        v[k] = want[k]
                        continue
                    err = max(abs(got[i] - want[k][i]) for i in range(3)) / scale
                    worst[iv["branch"]] = max(worst.get(iv["branch"], 0.0), err)
                    assert err <= pb.W_BOUND, (m["name"], c["params"], t, k, iv, err)
                    v[k] = got
    assert set(worst) == set(pb.BRANCHES) - {"eigen"}


def test_float64_restatements_of_the_residual(res):
    from parity import FLOOR_ULPS
    assert FLOOR_ULPS == 16
    n_red = n_int = 0
    for p in res["problems"]:
        ex = p["exact"]
        scale = max(abs(x) for x in ex["w"])
        P = p["P"]
        s = (P[0] + P[1]) + P[2]
        if p["red"]:
            w = pb.reduced64(p["red"], p["l0"], p["l1"], p["mu0"], p["mu1"], P)
            n_red += 1
        else:
            w = pb.expv64(p["l0"], p["l1"], p["mu0"], p["mu1"], P, p["q"], p["neg"])
        if w is None:
            continue
        assert max(abs(w[i] - ex["w"][i]) for i in range(3)) <= pb.W_BOUND * scale, p
        if p["cpfit"]:
            assert abs(((w[0] + w[1]) + w[2]) - p["tgt"] - ex["res"]) <= pb.W_BOUND * scale + pb.W_BOUND * abs(p["tgt"]), p
        elif p["regime"] == "ect_series":
            pn = [x / s for x in P]
            wn, vint = pb.taylor64(pb.TAYLOR_DEGREES[int(p["branch"][-1])], p["l0"], p["l1"], p["mu0"], p["mu1"], pn)
            ect = (p["l0"] * vint[0] + p["l1"] * vint[1]) / (1.0 - ((wn[0] + wn[1]) + wn[2]))
            assert abs(ect - ex["ect"]) <= pb.ect_floor(ex["ect"], ex["pnc"]), (p, ect)
            n_int += 1
    assert n_red >= 16 and n_int >= 42


def _call(L, ctx, cpfit, n, probs, out=True):
    a = None if probs is None else np.ascontiguousarray(probs, dtype=np.float64)
    o = np.zeros((max(n, 1), 4)) if out else None
    ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    return L.misti_pair_residuals(ctx, cpfit, n, ptr(a), ptr(o))


def test_probe_checks_its_arguments_before_the_context():
    """misti_pair_residuals WITHOUT a context (there is no device here): a bad argument is reported as such, a good one gets as far as
    'ctx is NULL'."""
    from misti_amd import _lib
    L = _lib.load()
    E_ARG = -1
    E_LIMIT = L.misti_pair_residuals(None, 1, (1 << 20) + 1, None, None)
    assert E_LIMIT not in (E_ARG, 0) and b"MISTI_PAIR_MAX_PROBLEMS" in L.misti_last_error()
    good = [0.3, 0.0, 0.0, 0.4, 0.1, 0.5, 1.0, 2.0, 3.0, 1.0]
    assert _call(L, None, 1, 1, [good]) == E_ARG and b"ctx is NULL" in L.misti_last_error()
    assert _call(L, None, 1, 0, None, out=False) == E_ARG and b"ctx is NULL" in L.misti_last_error()
    assert _call(L, None, 2, 1, [good]) == E_ARG and b"cpfit" in L.misti_last_error()
    assert _call(L, None, 1, -1, [good]) == E_ARG and b"negative" in L.misti_last_error()
    assert _call(L, None, 1, 1, None) == E_ARG and b"NULL" in L.misti_last_error() and b"ctx" not in L.misti_last_error()
    assert _call(L, None, 1, 1, [good], out=False) == E_ARG and b"ctx" not in L.misti_last_error()

    def bad(cpfit, what, **kw):
        p = list(good)
        for k, v in kw.items():
            p[int(k[1:])] = v
        assert _call(L, None, cpfit, 2, [good if cpfit else good[:9] + [0.0], p]) == E_ARG, (kw, L.misti_last_error())
        assert what in L.misti_last_error() and b"problems[1]" in L.misti_last_error(), (kw, L.misti_last_error())

    for role in (-1.0, 6.0, 2.5, math.nan):
        bad(1, b"role", _8=role)
    for red in (-1.0, 3.0, 0.5, math.inf):
        bad(1, b"red", _9=red)
    bad(0, b"without cpfit", _9=1.0)
    bad(1, b"mu1 == 0 and P[0] == 0", _1=1e-300)                       # red = 1 with migration into state 0
    bad(1, b"mu1 == 0 and P[0] == 0", _2=1e-300)                       # ... with state 0 not empty
    bad(1, b"mu0 == 0 and P[1] == 0", _9=2.0)                          # red = 2 on a problem made for red = 1
    bad(1, b"not finite", _0=math.nan)
    bad(1, b"not finite", _4=math.inf)
    bad(1, b"not finite", _5=math.nan)
    bad(1, b"negative", _0=-0.1)
    # the point may be anything
    assert _call(L, None, 1, 1, [good[:6] + [math.inf, math.nan] + good[8:]]) == E_ARG and b"ctx is NULL" in L.misti_last_error()
    assert _call(L, None, 1, 1, [good[:8] + [5.0, 0.0]]) == E_ARG and b"ctx is NULL" in L.misti_last_error()
    assert _call(L, None, 1, 1, [[0.0, 0.3, 0.2, 0.0, 0.1, 0.5, 1.0, 2.0, 0.0, 2.0]]) == E_ARG and b"ctx is NULL" in L.misti_last_error()


def test_probe_is_declared_and_bound():
    import re
    from misti_amd import _lib
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "misti_hip.h")).read()
    assert re.search(r"^int misti_pair_residuals\(misti_ctx\* ctx, int cpfit, int64_t n, const double\* problems", hdr, flags=re.M)
    assert "#define MISTI_ABI_VERSION 6" in hdr and hdr.index("introspection (tests)") < hdr.index("int misti_pair_residuals(")
    assert "misti_pair_residuals" in _lib.SYMBOLS
