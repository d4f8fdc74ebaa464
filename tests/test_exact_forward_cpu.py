"""tests/golden/golden_exact_forward.json.gz (the forward map in 50 digits, tests/exact_forward.py) on the CPU: the regimes it promises,
the restatement's ties to the oracle's structure, the no-migration identity on the exact side, and the NumPy oracle's own
coalescent_rates against the exact values in units of the bound the device is held to (tests/test_gpu_exact_forward.py)."""
import gzip
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import pair_branches as pb

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "golden_exact_forward.json.gz")
SOFT = tuple("taylor%d" % i for i in range(7)) + ("series",)


@pytest.fixture(scope="module")
def fx():
    with gzip.open(PATH, "rt") as f:
        return json.load(f)


def _candidates(fx):
    for r in fx["regimes"]:
        for m in r["models"]:
            for c in m["candidates"]:
                for h in m["hold"]:
                    yield r["name"], m, c, h, c["exact"][str(h)]


def test_fixture_covers_what_it_promises(fx):
    per_branch = pb.coverage_exact_forward(fx)
    assert set(per_branch) == set(pb.BRANCHES)
    assert fx["dps"] == 50 and fx["w_bound"] == pb.W_BOUND == 2e-13
    assert os.path.getsize(PATH) <= 400 * 1024


def test_restatement_takes_the_oracle_structure():
    """The integer tables of exact_forward are the oracle's generator and pulse operator: equal at rates where float64 is exact."""
    import mpmath as mp
    import exact_forward as xf
    from oracle.misti_oracle import _PairChain, _pulse_pairs
    ch = _PairChain()
    for l0, l1, mu0, mu1 in ((3.0, 5.0, 7.0, 11.0), (1.0, 0.0, 0.0, 2.0), (0.5, 0.25, 0.125, 0.0)):
        ch.set_mu(mu0, mu1)
        want = ch._matrix([l0, l1])
        got = xf.generator(l0, l1, mu0, mu1)
        assert all(float(got[i, j]) == want[i][j] for i in range(3) for j in range(3))
    p0 = [[0.5, 0.25, 0.125], [0.0625, 0.75, 0.03125]]
    for pu in ([0.25, 0.0], [0.0, 0.375], [0.0, 0.0], [1.0, 0.0]):
        want = _pulse_pairs(p0, pu)
        for k in (0, 1):
            got = xf.pulse([mp.mpf(v) for v in p0[k]], pu[0], pu[1])
            assert [float(v) for v in got] == [float(v) for v in want[k]], pu


def test_fixture_is_what_the_restatement_gives(fx):
    """A sample of every regime again from tests/exact_forward.py, and three stiff or decaying candidates at 80 digits."""
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import exact_forward as xf
    import make_exact_forward as gen
    job = lambda m, c, h: (m["times"], m["lh"], m["bands"], m["pulses"], c["split"], c["params"], h)
    for r in fx["regimes"]:
        m = r["models"][-1]
        for c in m["candidates"][::7]:
            for h in m["hold"]:
                assert gen.exact_record(job(m, c, h)) == c["exact"][str(h)], (m["name"], c["split"], c["params"])
    models = {m["name"]: m for r in fx["regimes"] for m in r["models"]}
    old = xf.DPS
    try:
        xf.DPS = 80
        for name, i in (("stiff_0", 0), ("decay_700", 3), ("decay_skew", 0)):
            c = models[name]["candidates"][i]
            again, have = gen.exact_record(job(models[name], c, 0)), c["exact"]["0"]
            assert again["branch"] == have["branch"]
            np.testing.assert_allclose(again["x"], have["x"], rtol=4 * pb.EPS)
            np.testing.assert_allclose(again["pr"], have["pr"], rtol=4 * pb.EPS, atol=1e-320)
    finally:
        xf.DPS = old


def test_no_migration_identity_on_the_exact_side(fx):
    """Without migration and without a pulse the seen rate of genome k is the model's own rate of population k: x = l_k T, checked
    against the exact product of the two doubles."""
    n = 0
    for regime, m, c, h, e in _candidates(fx):
        if e["status"] not in (0, 3) or m["pulses"]:
            continue
        if m["bands"] and not ("no_migration" in c["tags"] and not any(c["params"])):
            continue
        for t in range(e["n_eval"]):
            src = t if c["split"] == int(c["split"]) or t <= int(c["split"]) else t - 1
            for k in (0, 1):
                want = float(Fraction(m["lh"][src][k]) * Fraction(e["T"][t]))
                assert abs(e["x"][t][k] - want) <= pb.EPS * want, (m["name"], c["split"], t, k)
                n += 1
    assert n >= 300


def test_rows_from_the_split_on_are_the_models(fx):
    """What the fixture states for the rows the kernel does not evaluate: the model's own rates; row numT is zero unless a fractional
    split has inserted an interval, which moves every later row down by one (row s + 1 repeats row s)."""
    for regime, m, c, h, e in _candidates(fx):
        if e["status"] not in (0, 3):
            assert set(e) == {"status"}
            continue
        s = int(c["split"])
        want = m["lh"][e["n_eval"]:] + [[0.0, 0.0]] if c["split"] == s else m["lh"][s:]
        assert e["model_rows"] == want and len(e["pr"]) == e["n_eval"] + 1, (m["name"], c["split"])


def _oracle_x(m, c, h, e):
    from oracle.misti_oracle import OracleModel
    val = lambda v, p: c["params"][p] if p >= 0 else v
    split = int(math.ceil(c["split"]))
    mi = [[pop + 1, s, split if end < 0 else end, val(v, p), 0] for pop, s, end, v, p in m["bands"]]
    pu = [[pop + 1, t, val(v, p), 0] for pop, t, v, p in m["pulses"]]
    o = OracleModel(list(m["times"]), [list(r) for r in m["lh"]], [1] * 8, c["split"], mi, pu, trueEPS=True)
    assert o.times[:e["n_eval"]] == e["T"]
    rates = o.coalescent_rates(hold_mu=bool(h))
    return [[rates[t][k] * e["T"][t] for k in (0, 1)] for t in range(e["n_eval"])]


def test_oracle_against_50_digits(fx):
    """The NumPy oracle (SciPy's Pade exponential) in units of the device's bound: asserted where every interval up to this one is in
    a Taylor class or the series range, and on the tiny intervals; recorded elsewhere (stiff generators: DESIGN section 3 puts the dense
    exponential at ~1e-11 there)."""
    from parity import record
    worst, fails = {}, {}
    for regime, m, c, h, e in _candidates(fx):
        if e["status"] != 0 or not e["n_eval"]:
            continue
        try:
            with np.errstate(all="ignore"):
                got = _oracle_x(m, c, h, e)
        except (ValueError, ZeroDivisionError, OverflowError):          # log of an underflowed mass
            fails[regime] = fails.get(regime, 0) + 1
            continue
        for t in range(e["n_eval"]):
            soft = all(b in SOFT for b in e["branch"][:t + 1])
            for k in (0, 1):
                units = abs(got[t][k] - e["x"][t][k]) / pb.forward_bound(t, e["ratio"][t][k], e["x"][t][k])
                key = regime + ("" if soft or regime == "tiny" else "_stiff")
                worst[key] = max(worst.get(key, 0.0), units if math.isfinite(units) else float("inf"))
                if soft or regime == "tiny":
                    assert units <= 1.0, (m["name"], c["split"], c["params"], h, t, k, got[t][k], e["x"][t][k], units)
    for k in sorted(worst):
        print("oracle forward map %-22s worst %.3e of the bound" % (k, worst[k]))
    print("oracle forward map: no value for", fails)
    record("exact_forward_oracle", worst=worst, no_value=fails)
    assert {"branches", "tiny", "no_migration", "pulses", "hold_mu", "fractional"} <= set(worst)
