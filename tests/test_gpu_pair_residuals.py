"""The pair-chain residual as the chain kernels evaluate it (pair_eval, through the probe misti_pair_residuals) against 50-digit
arithmetic: every branch of the exponential again under all six roles, the --cpfit rank-one regime (pair_reduced), a negative trial
rate, non-finite and overflowing points, and the default fit's expected coalescence time in both of its forms - the integral series
against its own floor, the formula branch against the error of the reference's formula at the same points.  The exact values and
the reference formula's figures are tests/golden/golden_pair_residuals.json.gz (tests/golden/make_pair_branches.py)."""
import gzip
import json
import math
import os

import numpy as np
import pytest

import pair_branches as pb

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx():
    with gzip.open(os.path.join(HERE, "golden", "golden_pair_residuals.json.gz"), "rt") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def engine():
    from misti_amd.engine import Engine
    with Engine([1.0] * 5, [[1.0, 1.0]] * 6, [], [], n_param=0, cpfit=True) as e:      # the probe reads no model: any context will do
        yield e


def _row(p):
    return [p["mu0"], p["mu1"]] + list(p["P"]) + [p["tgt"], float(p["x0"]), float(p["x1"]), p["role"], p["red"]]


def _ratio(err, bound):
    """err / bound; an exact result of an exact zero (e^-3e5 underflows) is inside any bound."""
    return 0.0 if err == 0.0 else err / bound if bound > 0.0 else math.inf


def test_fixture_covers_what_it_promises(fx):
    assert 150 <= pb.coverage_residuals(fx) <= 400
    assert fx["bound"] == 2e-13


def test_cpfit_residuals_against_50_digits(fx, engine):
    from parity import record
    ps = [p for p in fx["problems"] if p["cpfit"]]
    out = engine.pair_residuals([_row(p) for p in ps], cpfit=True)
    worst, over = {}, []
    for p, o in zip(ps, out):
        ex = p["exact"]
        scale = max(abs(x) for x in ex["w"])
        ew = _ratio(max(abs(o[1 + i] - ex["w"][i]) for i in range(3)), pb.W_BOUND * scale)
        er = _ratio(abs(o[0] - ex["res"]), pb.W_BOUND * scale + pb.W_BOUND * abs(p["tgt"]))
        key = p["branch"] if p["regime"] == "cpfit_branch" else p["regime"]
        worst[key] = max(worst.get(key, 0.0), ew, er)
        if not (ew <= 1 and er <= 1):
            over.append((p, o.tolist(), ew, er))
        if p["red"]:
            assert o[p["red"]] == 0.0                      # the empty state stays exactly empty
    for k in sorted(worst):
        print("pair_residuals cpfit %-16s worst error / bound = %.3e" % (k, worst[k]))
    record("pair_residuals_cpfit", worst_over_bound=worst)
    assert set(pb.BRANCHES) | {"reduced", "negative_rate"} <= set(worst)
    assert not over, over[:4]


def test_points_without_a_value_come_back_nan(fx, engine):
    for cpfit in (1, 0):
        ps = [p for p in fx["nan_points"] if p["cpfit"] == cpfit]
        assert ps
        out = engine.pair_residuals([_row(p) for p in ps], cpfit=bool(cpfit))
        assert np.isnan(out).all(), (cpfit, out)


def test_default_fit_expected_coalescence_time(fx, engine):
    """tgt is 0 in these problems, so the residual IS the expected coalescence time."""
    from parity import record, SELF_FACTOR
    ps = [p for p in fx["problems"] if not p["cpfit"]]
    assert all(p["tgt"] == 0.0 for p in ps)
    out = engine.pair_residuals([_row(p) for p in ps], cpfit=False)
    worst, rel, over = {}, {}, []
    for p, o in zip(ps, out):
        ex = p["exact"]
        scale = max(abs(x) for x in ex["w"])
        ew = _ratio(max(abs(o[1 + i] - ex["w"][i]) for i in range(3)), pb.W_BOUND * scale)
        floor = pb.ect_floor(ex["ect"], ex["pnc"])
        if p["regime"] == "ect_series":
            assert p["branch"].startswith("taylor")
            key, bound = "ect_series_" + p["branch"], floor
        else:
            key = p["regime"]
            bound = max(SELF_FACTOR * fx["reference_formula"][key]["worst_relative_error"] * abs(ex["ect"]), floor)
        ee = _ratio(abs(o[0] - ex["ect"]), bound)
        worst[key] = max(worst.get(key, 0.0), ee)
        worst["w_" + key] = max(worst.get("w_" + key, 0.0), ew)
        rel[key] = max(rel.get(key, 0.0), abs(o[0] - ex["ect"]) / abs(ex["ect"]))
        if not (ee <= 1 and ew <= 1):
            over.append((p, o.tolist(), ee, ew))
    for k in sorted(rel):
        print("pair_residuals default fit %-28s worst ect error / bound = %.3e (relative %.3e), w / bound = %.3e" % (k, worst[k], rel[k], worst["w_" + k]))
    record("pair_residuals_default_fit", worst_over_bound=worst, worst_relative=rel, reference_formula=fx["reference_formula"])
    assert not over, over[:4]


def test_lanes_do_not_depend_on_their_company(fx, engine):
    """The same problems forward, reversed, and padded so that each sits alone in its wave (63 copies of an ordinary Taylor problem
    after it): bit-identical."""
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    for cpfit in (1, 0):
        rows = np.array([_row(p) for p in fx["problems"] if p["cpfit"] == cpfit])
        n = len(rows)
        assert n >= 64
        a = engine.pair_residuals(rows, cpfit=bool(cpfit))
        r = engine.pair_residuals(rows[::-1].copy(), cpfit=bool(cpfit))[::-1]
        alone = np.stack([engine.pair_residuals(rows[i:i + 1], cpfit=bool(cpfit))[0] for i in range(n)])
        filler = np.array([0.01, 0.02, 0.2, 0.3, 0.1, 0.0, 0.003, 0.002, 0.0, 0.0])
        padded = np.tile(filler, (64 * n, 1))
        padded[::64] = rows
        p = engine.pair_residuals(padded, cpfit=bool(cpfit))[::64]
        for name, b in (("reversed", r), ("one per call", alone), ("one per wave", p)):
            diff = np.argwhere(bits(a) != bits(b))
            assert diff.size == 0, (cpfit, name, len(diff), diff[:4].tolist())
