"""The expected spectrum of the HIP path against 50-digit arithmetic (tests/golden/golden_exact_spectrum.json, made by
tests/golden/make_exact_spectrum.py from tests/exact_spectrum.py): the 44-state propagation on both sides of the switch
between the uniformisation series and the Talbot contour (q = 96), strong two-way migration, tiny intervals, pulses, the
ancient sample, integer and fractional splits, the closed form after the split over many intervals and past e^-745, and
the replicate epilogue (8 rows inline, 9 rows in llk_kernel).

Every model runs two ways - one candidate per batch, and all candidates eight times over in one batch, where the duplicated
parameter vectors share a chain and its trunk - and both must meet the same bound:

    |got_c - exact_c| <= 1e-12 exact_c + 1e-14 sum(exact)           (each of the 7 normalised classes)
    |llk - exact|     <= 1e-12 |llk| + FLOOR_ULPS EPS llk_summand_scale

The bound is fixed for every case (the llk bound also carries the class floor of a row that counts sites in a class
below TINY, see _check).  A model with the split at numT (two populations in the infinite interval) is MISTI_INF_COAL
on the device whatever its migration (include/misti_hip.h); the fixture says so per candidate.
"""
import json
import os

import numpy as np
import pytest

from parity import EPS, FLOOR_ULPS, llk_summand_scale, record

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_exact_spectrum.json")
with open(FIXTURE) as _f:
    FX = json.load(_f)
MODELS = FX["models"]
RTOL, ATOL = 1e-12, 1e-14
DBL_MIN = 2.2250738585072014e-308
TINY = 1e-6
STATUS = {"ok": 0, "inf_coal": 3}


def _engine(m):
    from misti_amd.engine import Engine
    return Engine(m["times"], m["lh"], [tuple(b) for b in m["bands"]], [tuple(p) for p in m["pulses"]], n_param=m["n_param"],
                  cpfit=True, true_eps=True, unfolded=m["unfolded"], sample_date=m["sample_date"])


def _check(m, cand, lc, status, jafs, llk, rows):
    """Errors of one candidate's device output, relative to the bound (<= 1 passes); asserts the status and the rates."""
    name = (m["name"], cand["split"], cand["params"])
    assert status == STATUS[cand["device_status"]], (name, status)
    if cand["device_status"] != "ok":
        return 0.0, 0.0
    want_lc = np.array(cand["lc"])
    split = int(cand["split"]) + (1 if cand["split"] % 1 else 0)
    # with trueEPS the rates of the two-population intervals are the inputs: bit for bit, or the fixture does not apply
    assert np.array_equal(lc[:split], want_lc[:split]), (name, lc[:split], want_lc[:split])
    # After the split the rates come from the closed form of the single-population correction (exp / log on both sides, and
    # the last interval's mean in a different but equivalent arrangement): a few ulps apart at most.  What the spectrum sees is
    # tau_t = lc_t T_t (and 1/lc of the last interval): 4 ulps of max(tau, 1) per interval moves S by < 2e-15 over the
    # intervals where mass is left (S < 40), and the classes by 6x that relative - two orders inside RTOL.
    times = np.array(m["times"] if split == int(cand["split"]) else _split_times(m["times"], cand["split"]))
    for t in range(split, len(want_lc)):
        if t < len(want_lc) - 1:
            tau_d, tau_w = lc[t][0] * times[t], want_lc[t][0] * times[t]
            assert abs(tau_d - tau_w) <= 4 * EPS * max(1.0, abs(tau_w)), (name, t, lc[t], want_lc[t])
        else:
            assert abs(lc[t][0] - want_lc[t][0]) <= 8 * EPS * want_lc[t][0], (name, t, lc[t], want_lc[t])
    exact = np.array([float(v) for v in cand["jafs"]])
    bound = RTOL * exact + ATOL * exact.sum()
    err_j = float(np.max(np.abs(jafs - exact) / bound))
    err_l = 0.0
    # a class below the smallest normal double (mu = 0 with q = 1e5: e^-7239) is 0 or subnormal in any float64 spectrum; a row
    # that counts sites in it has no float64 log-likelihood to compare (the classes themselves are still checked above)
    cls = (lambda v: list(v)) if m["unfolded"] else (lambda v: [v[0] + v[6], v[1] + v[5], v[2] + v[4], v[3]])
    # A class below TINY is held to the absolute floor ATOL sum(exact) only (the contour quadrature is accurate relative to
    # the norm of the state vector, not to each of its components: with mu = 0 and q ~ 1e2 - 1e3 class 3 is 1e-17 - 1e-11);
    # a row counting n sites there carries that class error into its llk as n ATOL sum(exact) / exact_c, which is added.
    for r, row in enumerate(rows):
        counted = [(n, j) for n, j in zip(cls(row[1:]), cls(exact)) if n > 0]
        if any(j < DBL_MIN for n, j in counted):
            continue
        want = float(cand["llk"][r])
        tol = RTOL * abs(want) + FLOOR_ULPS * EPS * llk_summand_scale(row, np.maximum(exact, DBL_MIN), m["unfolded"])
        tol += sum(n * ATOL * exact.sum() / j for n, j in counted if j < TINY)
        err_l = max(err_l, abs(llk[r] - want) / tol)
    return err_j, err_l


def _split_times(times, split):
    s = int(split)
    t = list(times)
    t1 = (split % 1) * t[s]
    t[s:s + 1] = [t1, t[s] - t1]
    return t


def _run(m, rows, batched):
    cands = m["candidates"]
    P = m["n_param"]
    out = []
    with _engine(m) as e:
        if batched:
            reps = 8                                    # >= TRUNK_MIN_SHARE candidates per parameter vector: the trunk runs
            split = [c["split"] for c in cands] * reps
            par = np.array([c["params"] for c in cands] * reps).reshape(-1, P)
            r = e.evaluate(split, par, jsfs=rows, want_lc=True)
            for k in range(len(split)):
                out.append((cands[k % len(cands)], r.lc[k], int(r.status[k]), r.jafs[k], r.llk[k]))
        else:
            for c in cands:
                r = e.evaluate([c["split"]], np.array([c["params"]]).reshape(1, P), jsfs=rows, want_lc=True)
                out.append((c, r.lc[0], int(r.status[0]), r.jafs[0], r.llk[0]))
    return out


def _regimes():
    return sorted({m["regime"] for m in MODELS})


@pytest.mark.parametrize("batched", [False, True], ids=["one_per_batch", "one_batch_trunk"])
@pytest.mark.parametrize("regime", _regimes())
def test_spectrum_against_50_digits(regime, batched):
    worst_j, worst_l, where, n = 0.0, 0.0, None, 0
    failures = []
    for m in (m for m in MODELS if m["regime"] == regime):
        row_sets = [m["rows"]]
        if len(m["rows"]) > 8:
            row_sets.append(m["rows"][:8])              # 8 rows: the candidate kernel's inline epilogue
        for rows in row_sets:
            for cand, lc, status, jafs, llk in _run(m, np.array(rows), batched):
                n += 1
                try:
                    ej, el = _check(m, cand, lc, status, jafs, llk, rows)
                except AssertionError as exc:
                    failures.append(("assert", str(exc)[:300]))
                    continue
                if max(ej, el) > max(worst_j, worst_l):
                    where = (m["name"], cand["split"], cand["params"])
                worst_j, worst_l = max(worst_j, ej), max(worst_l, el)
                if ej > 1 or el > 1:
                    failures.append((m["name"], cand["split"], cand["params"], ej, el, list(jafs), cand["jafs"]))
    record("exact_spectrum_%s_%s" % (regime, "batched" if batched else "single"), candidates=n,
           worst_class_err_over_bound=worst_j, worst_llk_err_over_bound=worst_l, worst_case=str(where))
    assert not failures, failures[:4]
