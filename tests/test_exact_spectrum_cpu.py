"""tests/exact_spectrum.py - the 50-digit expected spectrum behind tests/golden/golden_exact_spectrum.json - against the pinned
oracle's float64 jaf_spectrum (which follows the reference's arithmetic: dense Pade expm, inv, deletion and restoration of the
stationary states without migration), and a few fixture entries recomputed.

  (a) where the oracle is accurate (every two-population interval in the series regime, q <= 96) the two agree to 1e-12: the
      restatement computes the reference's mathematics, including mu = 0, pulses, the ancient sample, fractional splits and
      the closed form after the split;
  (b) cheap fixture entries recomputed agree with the stored 40-digit strings to 1e-30;
  (c) on the stiff cases (q > 96) the oracle's distance from the exact value is recorded, not asserted.
"""
import json
import os

import mpmath as mp
import pytest

import exact_spectrum as ex
from parity import record

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_exact_spectrum.json")
with open(FIXTURE) as _f:
    FX = json.load(_f)
RTOL, ATOL = 1e-12, 1e-14


def _cases(stiff):
    for m in FX["models"]:
        for c in m["candidates"]:
            if c["status"] == "ok" and (c["q"] > FX["q_switch"]) == stiff:
                yield m, c


def _oracle_error(m, c):
    om = ex.oracle_model(m, c["split"], c["params"])
    assert [list(r) for r in om.lc] == c["lc"]
    om.jaf_spectrum()
    s = sum(om.JAFS)
    exact = [float(v) for v in c["jafs"]]
    return max(abs(o / s - e) / (RTOL * e + ATOL) for o, e in zip(om.JAFS, exact))


def test_fixture_covers_the_regimes():
    regimes = {m["regime"] for m in FX["models"]}
    assert regimes >= {"switch", "strong_migration", "tiny_q", "pulse", "ancient_sample", "split", "post_split", "replicates"}
    qs = {c["q"] for m in FX["models"] if m["regime"] == "switch" for c in m["candidates"]}
    assert {95.99, 96.0, 96.00000000000001, 97.0, 1e6} <= qs
    assert any(c["status"] == "inf_coal" for m in FX["models"] for c in m["candidates"])
    assert os.path.getsize(FIXTURE) < 1 << 20


def test_exact_matches_oracle_where_oracle_is_accurate():
    worst, n = 0.0, 0
    for m, c in _cases(stiff=False):
        err = _oracle_error(m, c)
        assert err <= 1.0, (m["name"], c["split"], c["params"], err)
        worst, n = max(worst, err), n + 1
    assert n >= 40
    record("exact_spectrum_vs_oracle_nonstiff", candidates=n, worst_err_over_bound=worst)


def test_oracle_drift_on_stiff_cases_recorded():
    drift = {}
    for m, c in _cases(stiff=True):
        drift[m["name"]] = max(drift.get(m["name"], 0.0), _oracle_error(m, c) * RTOL)
    assert drift
    record("exact_spectrum_oracle_drift_stiff", worst=max(drift.values()), per_model=drift)


CHEAP = [("tiny_q1e-06", 0), ("tiny_q0.001", 1), ("post_n70", 1), ("pulse_pop1_at0", 2), ("rows_unfolded", 1)]


@pytest.mark.parametrize("name,ci", CHEAP)
def test_fixture_entries_recompute(name, ci):
    m = next(m for m in FX["models"] if m["name"] == name)
    c = m["candidates"][ci]
    J = ex.spectrum(ex.oracle_model(m, c["split"], c["params"]))
    with mp.workdps(ex.DPS):
        for got, want in zip(J, c["jafs"]):
            assert abs(got - mp.mpf(want)) <= mp.mpf("1e-30") * abs(mp.mpf(want))
        for r, want in zip(m["rows"], c["llk"]):
            got = ex.llk(J, r, m["unfolded"])
            assert abs(got - mp.mpf(want)) <= mp.mpf("1e-30") * abs(mp.mpf(want))
