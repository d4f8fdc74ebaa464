"""The solver's linear algebra as the chain kernels run it (rcp64 / sqrt64, svd_mx2 / svd_aug, solve_tr / solve_tr_n, next_step,
select_step, tr_update, solve3 / solve3_ge / mat3_solve, through the probe misti_lsq_probe) against exact arithmetic.  The problems,
their exact answers (80-digit runs, stored as doubles), SciPy's answers and those of the float64 restatement (tests/lsq_rule.py) are
tests/golden/golden_lsq_probe.json.gz (tests/golden/make_lsq_probe.py); nothing here needs mpmath or SciPy.

THE BOUND OF rcp64 / sqrt64, derived from their source and the accuracy of the seeds, not from their comment:
  rcp64: r0 = v_rcp_f64(x) has a relative error e0 (the ISA gives the f64 seeds about 2^-23: "precision 2^29 ulp"; anything below
  2^-18 serves).  A Newton step r' = r + r (1 - x r), each factor one fma, squares it: e1 = e0^2 <= 2^-36, e2 = e0^4 <= 2^-72, plus
  the rounding of the residual 1 - x r (relative 2^-53 of a quantity that is itself <= 2^-36: nothing).  The last fma rounds ONCE
  a value that is 1/x (1 - e2): the result is within 0.5 + e2 / 2^-53 <= 0.5 + 2^-19 ulp of 1/x.
  sqrt64: y0 = v_rsq_f64(x), g = x y0, h = y0 / 2, and two coupled steps r = 1/2 - h g, g += g r, h += h r, which take the error
  of g from e0 to 1.5 e0^2 to ~2^-90, but leave g and h with the few 2^-53 of their own roundings (d, n: g = sqrt(x) (1 + d),
  h = (1 + n) / (2 g)).  The closing half step s = g + (x - g g) h has an exact residual up to one rounding (fma) and
  equals sqrt(x) (1 + d^2 / 2 - d n + ...) before ITS one rounding: within 0.5 + 2^-45 ulp of sqrt(x).
  Both are therefore held to lsq_rule.SCALAR_ULPS = 0.5 + 2^-20 ulp of the correctly rounded result on [2^-510, 2^510], where no
  intermediate leaves the normal range - i.e. they may differ from it only where the exact value is within 2^-20 ulp of a rounding
  boundary.  Outside that range (the comment of the functions excludes it) the values are recorded, not asserted.

THE BOUND OF THE OTHER KINDS is per class DEVICE_FACTOR = 4 x the worst figure of the restatement, in units of eps kappa
(lsq_rule.figures): the restatement is the same algorithm with correctly rounded operations; by the derivation above rcp64 and sqrt64
ARE correctly rounded up to 2^-20 ulp, so what the device adds is a * rcp(b) in place of a / b (two roundings for one) and fma
contraction, over the few dozen operations of a step - the factor 4 of the issue stands.  The exact answers are stored rounded to
double, so every figure carries up to half a unit of its own: a class whose restatement happens to be exact is held to 4 x 0.5 units,
except the classes that are exact BY STRUCTURE (EXACT below: zero columns, rank-one steps, the 3-4-5 step on the region), held to 0."""
import gzip
import json
import math
import os

import numpy as np
import pytest

import lsq_rule as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ["SVD2", "SVD4", "STEP", "STEPN", "SELECT", "UPDATE", "SOLVE3"]
EXACT = {"zero_col", "both_zero", "n1_zero", "rank1", "gn_on_region", "inside"}


@pytest.fixture(scope="module")
def fx():
    with gzip.open(os.path.join(HERE, "golden", "golden_lsq_probe.json.gz"), "rt") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def engine():
    from misti_amd.engine import Engine
    with Engine([1.0] * 5, [[1.0, 1.0]] * 6, [], [], n_param=0, cpfit=True) as e:      # the probe reads no model: any context will do
        yield e


@pytest.fixture(scope="module")
def outs(fx, engine):
    """One launch per kind, shared by the tests."""
    return {k: engine.lsq_probe(k, [p["in"] for p in ps]) for k, ps in fx["kinds"].items()}


def test_scalar_reciprocal_and_square_root(fx, outs):
    from parity import record
    ps, out = fx["kinds"]["SCALAR"], outs["SCALAR"]
    worst, where, outside, over = {"rcp": 0.0, "sqrt": 0.0}, {}, {"rcp": 0.0, "sqrt": 0.0}, []
    for p, o in zip(ps, out):
        x, fig = p["in"][0], R.figures("SCALAR", p, o)
        if "in_range" in p["t"]:
            for name in ("rcp", "sqrt"):
                if fig[name] > worst[name]:
                    worst[name], where[name] = fig[name], x.hex()
                if not fig[name] <= R.SCALAR_ULPS:
                    over.append((name, x.hex(), fig[name]))
        elif "recorded" in p["t"]:
            for name in ("rcp", "sqrt"):
                outside[name] = max(outside[name], fig[name])
    for name in ("rcp", "sqrt"):
        print("lsq_probe SCALAR %-4s worst on [2^-510, 2^510] = %.9f ulp at %s (bound %.9f); outside the range %.3g ulp (recorded)"
              % (name, worst[name], where.get(name), R.SCALAR_ULPS, outside[name]))
    record("lsq_probe_scalar", worst_ulps=worst, worst_at=where, bound_ulps=R.SCALAR_ULPS, outside_range_ulps=outside)
    assert not over, over[:8]
    sq = lambda x: float(outs_of(fx, outs, x)[1])
    assert sq(0.0) == 0.0 and sq(math.inf) == math.inf
    assert math.isnan(sq(-1.0)) and math.isnan(sq(math.nan)) and math.isnan(sq(-math.inf))


def outs_of(fx, outs, x):
    for p, o in zip(fx["kinds"]["SCALAR"], outs["SCALAR"]):
        if "special" in p["t"] and (p["in"][0] == x or (x != x and p["in"][0] != p["in"][0])) and math.copysign(1, p["in"][0]) == math.copysign(1, x):
            return o
    raise KeyError(x)


@pytest.mark.parametrize("kind", ["STEP", "STEPN", "SELECT", "UPDATE"])
def test_discrete_outcomes_are_the_fixtures(fx, outs, kind):
    """Branch, alpha == 0, the regularised-step count, axis, the path of select_step, term, accept and the case of the new radius:
    the fixture's on every problem."""
    wrong = []
    for i, (p, o) in enumerate(zip(fx["kinds"][kind], outs[kind])):
        d = R.discrete(kind, p, o.tolist())
        if d != p["disc"]:
            wrong.append((i, p["t"], d, p["disc"]))
    assert not wrong, (len(wrong), wrong[:6])


@pytest.mark.parametrize("kind", KINDS)
def test_values_against_exact_arithmetic(fx, outs, kind):
    from parity import record
    ps, head = fx["kinds"][kind], fx["header"]["worst"][kind]
    worst, over = {}, []
    for i, (p, o) in enumerate(zip(ps, outs[kind])):
        for c, v in R.figures(kind, p, o.tolist()).items():
            worst[c] = max(worst.get(c, 0.0), v)
            if c.endswith(":phi"):
                # the step the device returns is the exact p(alpha_device) rescaled: alpha itself satisfies SciPy's stopping test -
                # not asserted in ONE class, det_below: beyond kappa = 1 / eps the small singular value is rounding noise in LAPACK's
                # decomposition as in ours, SciPy's own alpha misses the test there (0.99999...: stored in the header), and neither
                # alpha means anything for the exact matrix
                ok = v < 0.01 or "iters10" in p["t"] or c == "det_below:phi"
            else:
                ok = v <= (0.0 if c in EXACT else R.DEVICE_FACTOR * max(head[c]["rule"], 0.5))
            if not ok:
                over.append((i, c, v, head[c]["rule"], p["t"]))
    for c in sorted(worst):
        print("lsq_probe %-6s %-24s device %-10.4g restatement %-10.4g scipy %s" % (kind, c, worst[c], head[c]["rule"], head[c]["scipy"]))
    record("lsq_probe_" + kind.lower(), device_worst=worst, restatement_worst={c: head[c]["rule"] for c in worst},
           scipy_worst={c: head[c]["scipy"] for c in worst}, factor=R.DEVICE_FACTOR)
    assert set(worst) == set(head)
    assert not over, (len(over), over[:6])


def test_rank_one_steps_are_exact(fx, outs):
    n = 0
    for p, o in zip(fx["kinds"]["STEP"], outs["STEP"]):
        if "rank1" in p["t"]:
            Delta, ax = p["in"][6], int(o[5])
            assert ax == p["disc"]["axis"] and o[1 - ax] == 0.0 and abs(o[ax]) == Delta and o[2] == 0.0 and o[4] == 0.0, (p, o)
            assert (o[ax] < 0) == ("g_pos" in p["t"])
            n += 1
    assert n == 4


def test_structural_zeros_of_the_elimination(fx, outs):
    """solve3_ge and mat3_solve: a component that does not depend on an entry of the matrix has the same bits whatever that entry."""
    ps, out, n = fx["kinds"]["SOLVE3"], outs["SOLVE3"], 0
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    for i, p in enumerate(ps):
        if "pair" in p and p["pair"] > i:
            a, b = out[i], out[p["pair"]]
            assert (bits(a[p["same"]]) == bits(b[p["same"]])).all(), (p, a, b)
            assert (bits(a[3:15]) != bits(b[3:15])).any()
            n += 1
    assert n == 40


def test_lanes_do_not_depend_on_their_company(fx, outs, engine):
    """Every kind in order (the shared launch), reversed, one problem per call (every problem of a kind, or 400 of them evenly
    spread) and padded to one problem per wave: the same bits."""
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    for kind, ps in fx["kinds"].items():
        rows = np.zeros((len(ps), R.LSQ_IN))
        for i, p in enumerate(ps):
            rows[i, :len(p["in"])] = p["in"]
        a, n = outs[kind], len(ps)
        r = engine.lsq_probe(kind, rows[::-1].copy())[::-1]
        pick = np.unique(np.linspace(0, n - 1, min(n, 400)).astype(int))
        alone = np.stack([engine.lsq_probe(kind, rows[i:i + 1])[0] for i in pick])
        padded = np.tile(rows[0], (64 * n, 1))
        padded[::64] = rows
        w = engine.lsq_probe(kind, padded)[::64]
        for name, x, y in (("reversed", a, r), ("one per call", a[pick], alone), ("one per wave", a, w)):
            diff = np.argwhere(bits(x) != bits(y))
            assert diff.size == 0, (kind, name, len(diff), diff[:4].tolist())
