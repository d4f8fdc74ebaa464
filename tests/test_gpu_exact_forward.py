"""forward_kernel (misti_kernels.hip, behind misti_forward_rates / misti_forward_rates_dev / Engine.forward_rates) against the forward map
in 50-digit arithmetic: tests/golden/golden_exact_forward.json.gz (tests/exact_forward.py, tests/golden/make_exact_forward.py; no
mpmath needed here).

What is held is x_t = seen rate x length of every interval and genome, to a bound that follows from what the suite already asserts
(pair_branches.forward_bound): pair_expv is within W_BOUND = 2e-13 of the largest component of its result, the state entering interval t
carries the errors of the t intervals before it, so

    |x_dev - x_exact| <= (t + 1) W_BOUND max|v_exact| / nc_exact + 8 EPS max(1, x_exact).

The bound is the project's own branch bound, not a fit to what the device gives.  On an interval of tiny rate x length it permits a
large RELATIVE error of the rate (x = -log(nc / before) cancels); that figure is recorded per decade, not asserted.

Measured on the MI355X (worst error in units of the bound): see DESIGN.md section 3, "The forward map against 50 digits"."""
import ctypes as C
import gzip
import json
import math
import os

import numpy as np
import pytest

import pair_branches as pb

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REGIMES = ("branches", "tiny", "no_migration", "decay", "pulses", "hold_mu", "fractional", "statuses")
DBL_MIN = 2.2250738585072014e-308
GUARD = 64


@pytest.fixture(scope="module")
def fx():
    with gzip.open(os.path.join(HERE, "golden", "golden_exact_forward.json.gz"), "rt") as f:
        return json.load(f)


def _engine(m):
    from misti_amd.engine import Engine
    return Engine(m["times"], m["lh"], [tuple(b) for b in m["bands"]], [tuple(p) for p in m["pulses"]], n_param=m["n_param"], true_eps=True)


def _inputs(m, cands=None):
    cands = m["candidates"] if cands is None else cands
    split = np.array([c["split"] for c in cands], dtype=np.float64)
    params = np.array([c["params"] for c in cands], dtype=np.float64).reshape(len(cands), m["n_param"]) if m["n_param"] else None
    return split, params


@pytest.fixture(scope="module")
def runs(fx):
    """Every model of the fixture through Engine.forward_rates once, per setting of hold_mu: {(model, hold): (lh, pr, status)}."""
    out = {}
    for r in fx["regimes"]:
        for m in r["models"]:
            split, params = _inputs(m)
            with _engine(m) as e:
                for h in m["hold"]:
                    out[m["name"], h] = e.forward_rates(split, params, want_pr=True, hold_mu=bool(h))
    return out


def _forward_dev(e, split, params, hold, want_pr=True, want_status=True):
    """misti_forward_rates_dev on device buffers with a guard band of GUARD elements right behind each output, which must come back
    untouched.  Returns (lh, pr or None, status or None) as NumPy arrays."""
    import torch
    from misti_amd import _lib
    dev = torch.device("cuda", e.device)
    n, rows = len(split), e.numT + 1
    d_split = torch.as_tensor(np.ascontiguousarray(split, dtype=np.float64), device=dev)
    d_par = torch.as_tensor(np.ascontiguousarray(params, dtype=np.float64), device=dev) if e.n_param else None
    n_lh, n_pr = n * rows * 2, n * (e.numT + 2) * 6
    lh = torch.full((n_lh + GUARD,), 7.0, dtype=torch.float64, device=dev)
    pr = torch.full((n_pr + GUARD,), 7.0, dtype=torch.float64, device=dev) if want_pr else None
    st = torch.full((n + GUARD,), 7, dtype=torch.int32, device=dev) if want_status else None
    torch.cuda.synchronize(dev)
    v = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    _lib.check(e._lib.misti_forward_rates_dev(e._ctx, n, v(d_split), v(d_par), int(hold), v(lh), v(pr), v(st)))
    e.sync()
    for buf, size in ((lh, n_lh), (pr, n_pr), (st, n)):
        if buf is not None:
            assert bool((buf[size:] == 7).all()), "guard band written"
    return (lh[:n_lh].cpu().numpy().reshape(n, rows, 2), pr[:n_pr].cpu().numpy().reshape(n, e.numT + 2, 6) if want_pr else None,
            st[:n].cpu().numpy() if want_status else None)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_bits(what, a, b):
    diff = np.argwhere(_bits(a) != _bits(b))
    assert diff.size == 0, (what, len(diff), diff[:4].tolist())


def _each(fx, runs, regime):
    for r in fx["regimes"]:
        if r["name"] != regime:
            continue
        for m in r["models"]:
            for h in m["hold"]:
                lh, pr, status = runs[m["name"], h]
                for ci, c in enumerate(m["candidates"]):
                    yield m, h, c, c["exact"][str(h)], lh[ci], pr[ci], int(status[ci])


@pytest.mark.parametrize("regime", REGIMES)
def test_rates_against_50_digits(fx, runs, regime):
    """x = seen rate x length of every interval within the bound, per regime and per branch.  Past e^-745 (model decay_past_745) a rate is
    within the bound or not finite: a finite wrong rate fails."""
    from parity import record
    worst, count, over, past = {}, {}, [], []
    for m, h, c, e, lh, pr, status in _each(fx, runs, regime):
        assert status == e["status"], (m["name"], c["split"], c["params"], h, status)
        if status not in (0, 3):
            assert np.isnan(lh).all()
            continue
        for t in range(e["n_eval"]):
            for k in (0, 1):
                x_dev, x = float(lh[t][k]) * e["T"][t], e["x"][t][k]
                bound = pb.forward_bound(t, e["ratio"][t][k], x)
                units = abs(x_dev - x) / bound
                if m["name"] == "decay_past_745":
                    past.append(dict(params=c["params"], t=t, genome=k, ln_nc=e["ln_nc"][t][k], x_exact=x, x_device=repr(x_dev),
                                     units=units if math.isfinite(x_dev) else None))
                    if not math.isfinite(x_dev):
                        continue
                for key in (regime, "branch_" + e["branch"][t]):
                    worst[key] = max(worst.get(key, 0.0), units)
                    count[key] = count.get(key, 0) + 1
                if not units <= 1.0:
                    over.append((m["name"], c["split"], c["params"], h, t, k, e["branch"][t], x_dev, x, units))
    for key in sorted(worst):
        print("exact_forward %-14s %-18s n=%5d worst=%.3e of the bound" % (regime, key, count[key], worst[key]))
    for p in past:
        print("exact_forward past e^-745:", json.dumps(p))
    record("exact_forward_rates_" + regime, worst=worst, intervals=count, past_745=past)
    assert regime in worst or regime == "statuses"
    assert not over, over[:8]


def test_every_branch_is_met_through_the_kernel(fx, runs):
    labels = {b for r in fx["regimes"] for m in r["models"] for c in m["candidates"] for e in c["exact"].values() for b in e.get("branch", ())}
    assert labels == set(pb.BRANCHES)


def test_tiny_intervals_relative_error_of_the_rate(fx, runs):
    """Recorded, not asserted (the bound permits it): the relative error of the RATE on intervals of rate x length 1e-2 ... 1e-12 -
    what a user of generated data sees.  The bound itself is held by test_rates_against_50_digits[tiny]."""
    from parity import record
    rel = {}
    for m, h, c, e, lh, pr, status in _each(fx, runs, "tiny"):
        for t in (0, 2, 3):
            for k in (0, 1):
                want = e["x"][t][k] / e["T"][t]
                key = "1e-%02d" % m["decade"]
                rel[key] = max(rel.get(key, 0.0), abs(float(lh[t][k]) - want) / want)
    for key in sorted(rel):
        print("exact_forward tiny rate x length %s: worst relative error of the rate %.3e" % (key, rel[key]))
    record("exact_forward_tiny_relative", worst_relative_error=rel)
    assert len(rel) == 11


def test_pair_state_trace(fx, runs):
    """`pr`: every component within (t + 1) W_BOUND of the largest exact component of its genome's state; row 0 after a pulse in the first
    interval within 4 ulps per component; rows past the split exactly 0.  A state whose largest exact component is no normal double
    (past e^-708) is not held: the bound would lie below the spacing of the doubles there."""
    from parity import record
    worst, over, n_pulse0 = 0.0, [], 0
    for regime in REGIMES:
        for m, h, c, e, lh, pr, status in _each(fx, runs, regime):
            if status not in (0, 3):
                assert (pr == 0).all()
                continue
            n = e["n_eval"]
            assert (pr[n + 1:] == 0).all() and (n > 0 or (pr == 0).all()), (m["name"], c["split"])
            if n == 0:
                continue
            for j in range(6):
                want = e["pr"][0][j]
                assert abs(pr[0][j] - want) <= 4 * pb.EPS * abs(want), (m["name"], c["params"], j, pr[0][j], want)
            n_pulse0 += e["pr"][0] != [1.0, 0.0, 0.0, 1.0, 0.0, 0.0]
            for t in range(n):
                for k in (0, 1):
                    want = [e["pr"][t + 1][j] for j in (k, 2 + k, 4 + k)]
                    scale = max(abs(w) for w in want)
                    if scale < DBL_MIN:
                        continue
                    err = max(abs(pr[t + 1][j] - w) for j, w in zip((k, 2 + k, 4 + k), want)) / (scale * (t + 1) * pb.W_BOUND)
                    worst = max(worst, err)
                    if not err <= 1.0:
                        over.append((m["name"], c["split"], c["params"], h, t, k, e["branch"][t], err))
    print("exact_forward pr trace: worst %.3e of (t + 1) W_BOUND; %d first rows after a pulse" % (worst, n_pulse0))
    record("exact_forward_pr", worst=worst, first_rows_after_a_pulse=n_pulse0)
    assert n_pulse0 >= 12
    assert not over, over[:8]


def test_hold_mu_is_the_own_rates_where_migration_is_constant(fx, runs):
    """The header's promise: hold_mu = 1 is hold_mu = 0 bit for bit on a model whose migration is constant up to the split - at every
    split, the one at numT included.  (Both settings against the exact restatement: test_rates_against_50_digits[hold_mu].)"""
    for what, a, b in zip(("lh", "pr", "status"), runs["constant", 0], runs["constant", 1]):
        _same_bits(what, a, b)
    lh0, lh1 = runs["fixed_ends", 0][0], runs["fixed_ends", 1][0]
    assert (_bits(lh0) != _bits(lh1)).any()                 # and it is not the same thing where the rates change


def test_rows_the_kernel_does_not_evaluate(fx, runs):
    """Bit for bit: rows at and past the split are the model's rates, row numT as the fixture states it (zero, or the model's last
    row below an inserted interval).  Without migration and pulses the evaluated rows are the model's rates too, within the bound
    (test_rates_against_50_digits); how many come back bit-equal is recorded."""
    from parity import record
    equal = total = 0
    for regime in REGIMES:
        for m, h, c, e, lh, pr, status in _each(fx, runs, regime):
            if status not in (0, 3):
                continue
            n = e["n_eval"]
            _same_bits((m["name"], c["split"], h), lh[n:], np.array(e["model_rows"], dtype=np.float64).reshape(-1, 2))
            if not m["bands"] and not m["pulses"]:
                rows = np.array(m["lh"] if c["split"] == int(c["split"]) else m["lh"][:int(c["split"]) + 1] + m["lh"][int(c["split"]):])[:n]
                equal += int((lh[:n] == rows).sum())
                total += 2 * n
    print("exact_forward no migration: %d of %d evaluated rates bit-equal to the model's" % (equal, total))
    record("exact_forward_no_migration", bit_equal=equal, rates=total)
    assert total >= 80


def test_shapes(fx):
    """One thread per candidate, 64 per block: the 65 candidates of the walk in one call, reversed, one per call, and the first 1, 63, 64
    and 65 of them - the same bits in rows, trace and status; then 64 * 3 + 1 candidates (the last block holds one thread).  Device
    buffers with a guard band behind each output."""
    m = fx["regimes"][0]["models"][0]
    assert m["name"] == "walk" and len(m["candidates"]) == 65
    split, params = _inputs(m)
    with _engine(m) as e:
        base = _forward_dev(e, split, params, 0)
        host = e.forward_rates(split, params, want_pr=True)
        rev = _forward_dev(e, split[::-1].copy(), params[::-1].copy(), 0)
        singles = [_forward_dev(e, split[i:i + 1], params[i:i + 1], 0) for i in range(65)]
        prefixes = {n: _forward_dev(e, split[:n], params[:n], 0) for n in (1, 63, 64, 65)}
        idx = np.arange(64 * 3 + 1) % 65
        cyc = _forward_dev(e, split[idx], params[idx], 0)
    assert (base[2] == 0).all()
    for i, what in enumerate(("lh", "pr", "status")):
        _same_bits("host " + what, base[i], host[i])
        _same_bits("reversed " + what, base[i], rev[i][::-1])
        _same_bits("alone " + what, base[i], np.concatenate([s[i] for s in singles]))
        for n, got in prefixes.items():
            _same_bits("first %d %s" % (n, what), base[i][:n], got[i])
        _same_bits("cycled " + what, base[i][idx], cyc[i])


def test_host_form_is_the_device_form(fx):
    """misti_forward_rates and misti_forward_rates_dev on the same inputs: the same bits in lh, pr and status, for hold_mu 0 and 1, with
    refused candidates in the batch; with pr and status NULL the lh rows are the same bits again."""
    models = {m["name"]: m for r in fx["regimes"] for m in r["models"]}
    for name in ("statuses", "fractional", "pulses_mixed", "end_at_split"):
        m = models[name]
        split, params = _inputs(m)
        with _engine(m) as e:
            for h in m["hold"]:
                host = e.forward_rates(split, params, want_pr=True, hold_mu=bool(h))
                devf = _forward_dev(e, split, params, h)
                bare = _forward_dev(e, split, params, h, want_pr=False, want_status=False)
                host_bare = e.forward_rates(split, params, want_pr=False, hold_mu=bool(h))
                for i, what in enumerate(("lh", "pr", "status")):
                    _same_bits((name, h, what), host[i], devf[i])
                _same_bits((name, h, "lh without pr and status"), host[0], bare[0])
                _same_bits((name, h, "host lh without pr"), host[0], host_bare[0])


def test_statuses(fx, runs):
    """The header's codes per candidate, NaN rows and an all-zero trace for a refused candidate; a split at 0 returns the model."""
    seen = set()
    for m, h, c, e, lh, pr, status in _each(fx, runs, "statuses"):
        assert status == e["status"], (c["tags"], status)
        seen.add(status)
        if status in (1, 4):
            assert np.isnan(lh).all() and (pr == 0).all(), c["tags"]
        else:
            assert np.isfinite(lh).all()
        if "split_0" in c["tags"]:
            _same_bits("split 0", lh, np.array(m["lh"] + [[0.0, 0.0]]))
            assert (pr == 0).all()
    assert seen == {0, 1, 3, 4}
