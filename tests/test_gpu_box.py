"""Box constraints on the batched searches - misti_nm_solve_box / misti_basinhopping_box, Engine.nm_solve_box / basinhopping_box and
`--box`.  The target is SciPy's own bounded Nelder-Mead (scipy.optimize.minimize(method='Nelder-Mead', bounds=Bounds(lo, hi)), and
scipy.optimize.basinhopping around it) on this engine's objective, bit for bit, on config 3's model with its band ends following the
split, on config 4's no-migration model (a 1-D search) and on the pulse-sweep golden's model.  Eight starts per test; SciPy's side of
a comparison is computed once and shared between the speculative and the three-batch path."""
import ctypes as C
import random
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

FIELDS = ("x", "llh", "nit", "nfev", "status")
COUNTERS = ("iterations_issued", "slots", "speculative_iterations")
MAXITER = 200
INF = np.inf
SPLITS = np.array([61.0, 62.5, 63.0, 64.25, 64.0, 65.5, 62.0, 63.75])
ROWS = np.array([0, 1, 2, 3, 4, 2, 0, 1], dtype=np.int32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def model():
    """Config 3's model as tests/test_gpu_split_fit.py builds it: band ends -1, a 5-row bootstrap table."""
    from misti_amd import io as mio, synth, workloads
    from misti_amd.engine import Engine, truth_spectrum
    w = workloads.config3(lambda *a: truth_spectrum(*a), n_start=4)
    bands = [(p, s, -1, v, k) for p, s, e, v, k in w.bands]
    table = np.array(mio.bootstrap_table(synth.chunk_rows(w.jsfs[0], 20), 4, random.Random(3)), dtype=np.float64)
    kw = w.engine_kwargs()
    kw["bands"] = bands
    eng = Engine(w.times, w.lh, **kw)
    start = np.array([b[3] for b in bands])
    yield eng, table, start
    eng.close()


@pytest.fixture(scope="module")
def nomig():
    """Config 4's model: no migration, no optimised parameter; 12 rows of its bootstrap table."""
    from misti_amd import workloads
    from misti_amd.engine import Engine, truth_spectrum
    w = workloads.config4(lambda *a: truth_spectrum(*a), n_split=4, n_rep=12)
    eng = Engine(w.times, w.lh, **w.engine_kwargs())
    assert eng.n_param == 0 and w.jsfs.shape == (12, 8)
    yield eng, w.jsfs
    eng.close()


@pytest.fixture(scope="module")
def boxed(model):
    """The eight starts over (rate, rate, split) and a box per start that binds: the upper bound of the first rate is half the smallest
    first rate the UNBOXED search fits from these starts, the split stays within 1.5 of each initial split.  Start 1 lies outside its
    box (its split), start 2 exactly on an upper bound (its first rate), start 3 has its second rate held fixed (lo == hi)."""
    eng, table, start = model
    starts = np.array([list(start) + [st] for st in SPLITS])
    starts[5, :2] = [0.3, 0.02]
    starts[6, :2] = [0.05, 0.5]
    free = eng.nm_solve_split(starts, ROWS, table, maxiter=MAXITER)
    assert np.isfinite(free["llh"]).all()
    R = 0.5 * float(free["x"][:, 0].min())
    assert R > 0
    lo = np.array([[0.0, 0.0, st - 1.5] for st in SPLITS])
    hi = np.array([[R, INF, st + 1.5] for st in SPLITS])
    starts[1, 2] = SPLITS[1] + 4.0
    starts[2, 0] = R
    lo[3, 1] = hi[3, 1] = 0.75 * start[1]
    return starts, lo, hi, R


def objective(eng, table, row, split=None):
    """-engine.evaluate against one row over (parameters, split), or over the parameters at a fixed split; no value scores +inf."""
    P = eng.n_param

    def obj(x):
        st, par = (x[-1], x[:-1]) if split is None else (split, x)
        v = float(eng.evaluate([st], [list(par)] if P else None, table[row:row + 1]).llk[0, 0])
        return -v if np.isfinite(v) else np.inf
    return obj


def scipy_box_search(obj, x0, lo, hi, maxiter=MAXITER):
    from scipy import optimize
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                  # "Initial guess is not within the specified bounds"
        return optimize.minimize(obj, np.asarray(x0, dtype=float), method="Nelder-Mead", bounds=optimize.Bounds(lo, hi),
                                 options=dict(xatol=1e-4, fatol=1e-4, maxiter=maxiter))


def assert_equals_scipy(got, refs):
    for s, ref in enumerate(refs):
        print(s, "scipy", ref.x, -ref.fun, ref.nit, ref.nfev, ref.status,
              "device", got["x"][s], got["llh"][s], got["nit"][s], got["nfev"][s], got["status"][s])
    for s, ref in enumerate(refs):
        assert same_bits(np.asarray(ref.x, dtype=np.float64), got["x"][s]), (s, ref.x, got["x"][s])
        assert same_bits(np.float64(-ref.fun), got["llh"][s]), (s, -ref.fun, got["llh"][s])
        assert ref.nit == got["nit"][s] and ref.nfev == got["nfev"][s] and ref.status == got["status"][s], (s, ref.nit, ref.nfev, ref.status)


def on_a_bound(x, lo, hi):
    return bool(((x == lo) | (x == hi)).any())


_SCIPY = {}


def scipy_refs(key, make):
    """SciPy's side of a comparison, computed once per module run."""
    if key not in _SCIPY:
        _SCIPY[key] = make()
    return _SCIPY[key]


# ---- 1. equals SciPy with bounds=, bit for bit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ["default", "0"])
@pytest.mark.parametrize("N", [3, 2])
def test_box_search_equals_scipy_with_bounds_bit_for_bit(model, boxed, monkeypatch, N, spec):
    eng, table, start = model
    starts, lo, hi, R = boxed
    if spec == "0":
        monkeypatch.setenv("MISTI_NM_SPEC", "0")
    if N == 3:                                           # the split as a coordinate
        x0, blo, bhi, split_times = starts, lo, hi, None
    else:                                                # a split per start
        x0, blo, bhi, split_times = starts[:, :2].copy(), lo[:, :2].copy(), hi[:, :2].copy(), SPLITS
    refs = scipy_refs(("nm", N), lambda: [scipy_box_search(objective(eng, table, int(ROWS[s]), None if N == 3 else float(SPLITS[s])),
                                                           x0[s], blo[s], bhi[s]) for s in range(8)])
    # the box is not idle - on SciPy's own results
    xs = np.array([r.x for r in refs])
    n_bound = sum(on_a_bound(xs[s], blo[s], bhi[s]) for s in range(8))
    print("upper rate bound", R, "starts ending on a bound", n_bound)
    assert n_bound >= 3
    assert same_bits(xs[3, 1], blo[3, 1]) and blo[3, 1] == bhi[3, 1]
    assert (xs >= blo).all() and (xs <= bhi).all()
    assert ((x0 < blo) | (x0 > bhi)).any(axis=1).sum() >= 1 and x0[2, 0] == bhi[2, 0]
    got = eng.nm_solve_box(x0, ROWS, table, (blo, bhi), split_times=split_times, maxiter=MAXITER)
    assert got["x"].shape == (8, N) and np.isfinite(got["llh"]).all()
    assert_equals_scipy(got, refs)
    assert same_bits(got["split"], got["x"][:, -1] if N == 3 else SPLITS)
    assert (got["speculative_iterations"] > 0) == (spec == "default")


# ---- 2. the no-migration model: one coordinate, params = NULL ----------------------------------------------------------------------
def test_no_migration_model_with_a_split_box_equals_scipy(nomig):
    eng, table = nomig
    rows = np.arange(8, dtype=np.int32)
    starts = (44.0 + 1.25 * np.arange(8)).reshape(8, 1)
    lo, hi = starts - 1.5, starts + 1.5
    starts[2, 0] += 3.0                                  # outside its box
    starts[4, 0] = hi[4, 0]                              # on the upper bound
    lo[6, 0] = hi[6, 0] = 50.25                          # held fixed: a search with nothing to move
    refs = [scipy_box_search(objective(eng, table, int(rows[s])), starts[s], lo[s], hi[s]) for s in range(8)]
    xs = np.array([r.x for r in refs])
    assert sum(on_a_bound(xs[s], lo[s], hi[s]) for s in range(8)) >= 2 and (xs >= lo).all() and (xs <= hi).all()
    got = eng.nm_solve_box(starts, rows, table, (lo, hi), maxiter=MAXITER)
    assert got["x"].shape == (8, 1) and np.isfinite(got["llh"]).all()
    assert_equals_scipy(got, refs)
    assert same_bits(got["x"][6, 0], np.float64(50.25))


# ---- 3. an infinite box is no box --------------------------------------------------------------------------------------------------
def test_an_infinite_box_returns_the_bytes_of_the_search_without_one(model, boxed):
    eng, table, start = model
    starts = boxed[0]
    none3 = (np.full(3, -INF), np.full(3, INF))
    none2 = (np.full((8, 2), -INF), np.full((8, 2), INF))
    a = eng.nm_solve_split(starts, ROWS, table, maxiter=MAXITER)
    b = eng.nm_solve_box(starts, ROWS, table, none3, maxiter=MAXITER)
    for f in FIELDS + ("split",):
        assert same_bits(a[f], b[f]), f
    assert [a[f] for f in COUNTERS] == [b[f] for f in COUNTERS]
    a = eng.nm_solve_pulses(starts[:, :2], SPLITS, ROWS, table, None, None, maxiter=MAXITER)
    b = eng.nm_solve_box(starts[:, :2], ROWS, table, none2, split_times=SPLITS, maxiter=MAXITER)
    for f in FIELDS:
        assert same_bits(a[f], b[f]), f
    assert [a[f] for f in COUNTERS] == [b[f] for f in COUNTERS]
    hops = dict(niter=2, T=0.5, stepsize=0.05, interval=2, nm_maxfev=60)
    seeds = [900 + s for s in range(8)]
    a = eng.basinhopping_split(starts, ROWS, table, seeds, **hops)
    b = eng.basinhopping_box(starts, ROWS, table, seeds, none3, **hops)
    for f in ("x", "llh", "nfev", "failures", "accepted", "split"):
        assert same_bits(a[f], b[f]), f
    assert [a[f] for f in COUNTERS] == [b[f] for f in COUNTERS]


# ---- 4. basin hopping around the boxed search ----------------------------------------------------------------------------------------
def test_basin_hopping_equals_scipy_with_bounds_bit_for_bit(model, boxed, monkeypatch):
    from scipy import optimize
    from scipy.optimize import _basinhopping as bh
    eng, table, start = model
    starts, lo, hi, R = boxed
    seeds = [300 + s for s in range(8)]
    stepsize = 2.0                                       # rates of order 0.1 inside [0, R]: nearly every displacement leaves the box
    trials = []
    displace = bh.RandomDisplacement.__call__

    def recorded(self, x):                               # SciPy's own trial points, as its RandomDisplacement returns them
        y = displace(self, x)
        trials[-1].append(np.array(y, dtype=np.float64))
        return y
    monkeypatch.setattr(bh.RandomDisplacement, "__call__", recorded)
    refs = []
    for s in range(8):
        trials.append([])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            refs.append(optimize.basinhopping(objective(eng, table, int(ROWS[s])), starts[s], niter=3, T=0.5, stepsize=stepsize, interval=2,
                                              minimizer_kwargs=dict(method="Nelder-Mead", bounds=optimize.Bounds(lo[s], hi[s]),
                                                                    options=dict(xatol=1e-4, fatol=1e-4, maxfev=60, maxiter=600)),
                                              rng=np.random.default_rng(seeds[s])))
    monkeypatch.undo()
    assert all(len(t) == 3 for t in trials)
    left = sum(bool(((y < lo[s]) | (y > hi[s])).any()) for s in range(8) for y in trials[s])
    print("trial points outside their box:", left, "of", 24)
    assert left >= 1
    got = eng.basinhopping_box(starts, ROWS, table, seeds, (lo, hi), niter=3, T=0.5, stepsize=stepsize, interval=2, nm_maxfev=60)
    for s, ref in enumerate(refs):
        print(s, "scipy", ref.x, -ref.fun, ref.nfev, ref.minimization_failures,
              "device", got["x"][s], got["llh"][s], got["nfev"][s], got["failures"][s], got["accepted"][s])
    for s, ref in enumerate(refs):
        assert same_bits(np.asarray(ref.x, dtype=np.float64), got["x"][s]), (s, ref.x, got["x"][s])
        assert same_bits(np.float64(-ref.fun), got["llh"][s]), (s, -ref.fun, got["llh"][s])
        assert ref.nfev == got["nfev"][s] and ref.minimization_failures == got["failures"][s], (s, ref.nfev, ref.minimization_failures)
    assert (got["x"] >= lo).all() and (got["x"] <= hi).all() and same_bits(got["split"], got["x"][:, -1])
    # no hop at all: the initial minimisation is the boxed search itself
    alone = eng.nm_solve_box(starts, ROWS, table, (lo, hi), maxiter=25)
    zero = eng.basinhopping_box(starts, ROWS, table, seeds, (lo, hi), niter=0, nm_maxiter=25, nm_maxfev=100000)
    assert same_bits(zero["x"], alone["x"]) and same_bits(zero["llh"], alone["llh"]) and same_bits(zero["nfev"], alone["nfev"])
    assert np.array_equal(zero["failures"], (alone["status"] != 0).astype(np.int32))


# ---- 5. per-start bounds and pulse times together with a box -----------------------------------------------------------------------
def test_per_start_bounds_and_pulse_times_with_a_box_equal_fresh_engines():
    from misti_amd.engine import Engine
    grid = load_golden("golden_pulse_sweep")[0]["in"]
    flags = dict(n_param=2, cpfit=True, smooth=True, unfolded=True)

    def engine(band_start, pulse_time):
        return Engine(grid["times"], grid["lambdas"], [(0, band_start, -1, 0.2, 0)], [(0, 10, 0.05, -1), (1, pulse_time, 0.0, 1)], **flags)
    table = np.array([grid["sfs"], [v * 2 for v in grid["sfs"]]], dtype=np.float64)
    band_start = [4, 6, 2, 4, 8, 6, 2, 4]
    pulse_time = [5, 5, 12, 15, 3, 12, 5, 3]
    splits = [20.0, 19.5, 21.0, 18.25, 20.0, 19.0, 20.5, 21.25]
    rows = np.array([0, 1, 0, 1, 1, 0, 1, 0], dtype=np.int32)
    starts = np.array([[0.2, 0.1, st] for st in splits])
    bounds = np.array([[[b, -1]] for b in band_start], dtype=np.int32)
    times = np.array([[10, t] for t in pulse_time], dtype=np.int32)
    lo = np.array([[0.0, 0.0, st - 1.0] for st in splits])
    hi = np.array([[0.15, 0.5, st + 1.0] for st in splits])
    lo[5, 1] = hi[5, 1] = 0.08
    with engine(4, 5) as e:
        got = e.nm_solve_box(starts, rows, table, (lo, hi), band_bounds=bounds, pulse_times=times, maxiter=MAXITER)
        per = e.nm_solve_box(starts[:, :2], rows, table, (lo[:, :2], hi[:, :2]), split_times=splits, band_bounds=bounds, pulse_times=times,
                             maxiter=MAXITER)
    assert np.isfinite(got["llh"]).all() and (got["x"] >= lo).all() and (got["x"] <= hi).all()
    assert sum(on_a_bound(got["x"][s], lo[s], hi[s]) for s in range(8)) >= 1
    for s in range(8):
        with engine(band_start[s], pulse_time[s]) as e:
            one = e.nm_solve_box(starts[s:s + 1], rows[s:s + 1], table, (lo[s], hi[s]), maxiter=MAXITER)
            one_per = e.nm_solve_box(starts[s:s + 1, :2], rows[s:s + 1], table, (lo[s, :2], hi[s, :2]), split_times=splits[s:s + 1], maxiter=MAXITER)
        for f in FIELDS + ("split",):
            assert same_bits(got[f][s:s + 1], one[f]), (s, f, got[f][s], one[f])
            assert same_bits(per[f][s:s + 1], one_per[f]), (s, f, per[f][s], one_per[f])


# ---- 6. argument errors ------------------------------------------------------------------------------------------------------------
def test_argument_errors_before_any_device_work(model, boxed):
    from misti_amd._lib import MistiError
    eng, table, start = model
    starts, lo, hi, R = boxed
    eng.nm_solve_box(starts, ROWS, table, (lo, hi), maxiter=5)
    stats = (C.c_int64 * 2)()
    eng._lib.misti_nm_last_stats(eng._ctx, stats)
    before = (stats[0], stats[1])
    assert before[0] > 0
    swapped_lo, nan_hi = lo.copy(), hi.copy()
    swapped_lo[4, 2] = hi[4, 2] + 1.0
    nan_hi[7, 0] = np.nan
    for box, text in (((lo[:2], hi[:2]), "n_box must be 1 or n_start"), ((swapped_lo, hi), "box 4, coordinate 2"), ((lo, nan_hi), "box 7, coordinate 0")):
        with pytest.raises(MistiError) as err:
            eng.nm_solve_box(starts, ROWS, table, box, maxiter=5)
        assert err.value.code == -1 and text in str(err.value), (text, str(err.value))
        with pytest.raises(MistiError) as err:
            eng.basinhopping_box(starts, ROWS, table, list(range(8)), box, niter=1, nm_maxfev=10)
        assert err.value.code == -1 and text in str(err.value), (text, str(err.value))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    x, llh = np.empty((8, 3)), np.empty(8)
    full = [ptr(starts), None, ptr(ROWS), 5, ptr(table), None, None, 8, ptr(lo), ptr(hi), 1e-4, 1e-4, 10, ptr(x), ptr(llh), None, None, None]
    for k in (0, 2, 4, 8, 9, 13, 14):                    # starts, rows, jsfs, box_lo, box_hi, x, llh
        args = list(full)
        args[k] = None
        assert eng._lib.misti_nm_solve_box(eng._ctx, 8, *args) == -1, k
    uni = np.zeros((8, 1, 4))
    hops = [1, 0.5, 0.5, 50, 0.5, 0.9, 1e-4, 1e-4, 10, 10, ptr(uni), ptr(x), ptr(llh), None, None, None]
    for k in (8, 9):
        args = list(full[:10])
        args[k] = None
        assert eng._lib.misti_basinhopping_box(eng._ctx, 8, *args, *hops) == -1, k
    assert eng._lib.misti_nm_solve_box(None, 8, *full) == -1
    eng._lib.misti_nm_last_stats(eng._ctx, stats)
    assert (stats[0], stats[1]) == before                # nothing ran
    again = eng.nm_solve_box(starts, ROWS, table, (lo, hi), maxiter=5)             # the context is as usable as before
    assert np.isfinite(again["llh"]).all()


# ---- 7. the old paths are untouched ------------------------------------------------------------------------------------------------
def test_old_searches_are_byte_equal_around_a_box_search(model, boxed):
    eng, table, start = model
    bstarts, lo, hi, R = boxed
    starts = np.vstack([start, [0.3, 0.02], [0.05, 0.5]])
    splits = np.array([62.0, 63.5, 64.0])
    rows = np.array([0, 3, 1], dtype=np.int32)

    def old():
        return [eng.nm_solve(starts, 63.5, table[0], maxiter=200),
                eng.nm_solve_rows(starts, splits, rows, table, maxiter=200),
                eng.nm_solve_pulses(starts, splits, rows, table, np.array([[[4, -1], [10, -1]]] * 3, dtype=np.int32), None, maxiter=200),
                eng.nm_solve_split(np.hstack([starts, splits[:, None]]), rows, table, maxiter=200),
                eng.basinhopping(starts[:2], 64.0, table[0], [11, 12], niter=2, nm_maxiter=60)]
    a = old()
    eng.nm_solve_box(bstarts, ROWS, table, (lo, hi), maxiter=200)
    eng.basinhopping_box(bstarts, ROWS, table, list(range(8)), (lo, hi), niter=1, nm_maxfev=30)
    b = old()
    for ra, rb in zip(a, b):
        for f, v in ra.items():
            if isinstance(v, np.ndarray):
                assert same_bits(v, rb[f]), f
            else:
                assert v == rb[f], f


# ---- 8. the command line -------------------------------------------------------------------------------------------------------------
def _inputs(tmp_path):
    from misti_amd import synth, io as mio
    from oracle.batch import oracle_truth_spectrum
    f1, f2, fj = (str(tmp_path / n) for n in ("g1.psmc", "g2.psmc", "bs.sfs"))
    open(f1, "w").write(synth.psmc_text(16, 1, synth.THETA_1))
    open(f2, "w").write(synth.psmc_text(17, 2, synth.THETA_2))
    inp = mio.read_psmc(f1, f2)
    jafs = oracle_truth_spectrum(inp.times, inp.lambdas, 20, [(0, 2, 20, 0.1, -1)], [], 0)
    row = synth.counts_from_spectrum(jafs, 200000)
    table = mio.bootstrap_table(synth.chunk_rows(row, 20), 3, random.Random(5))
    open(fj, "w").write(mio.format_jsfs(table))
    return f1, f2, fj, inp


def test_cli_fit_st_with_a_box_prints_the_boxed_fits(tmp_path):
    from conftest import ROOT
    from misti_amd import io as mio
    from misti_amd.engine import Engine
    f1, f2, fj, inp = _inputs(tmp_path)
    units = str(tmp_path / "nounits.txt")
    R, A, B = 0.05, 19.25, 20.25                         # the data were made with a rate of 0.1 at split 20: the cap binds
    cmd = [sys.executable, "-m", "misti_amd.cli", f1, f2, fj, "20", "-mi", "1", "2", "20", "0.1", "1", "--cpfit", "--funits", units,
           "--grid-st", "19", "20", "0.5", "--all-bs", "--fit-st", "--box", "0", "0", str(R), "--box", "st", str(A), str(B)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("bs_id =")]
    pat = re.compile(r"^bs_id = (\S+) \tsplitT = (\S+) \ttime = \S+ \tmigration rates optim = \[(\S+)\] \tllh = (\S+)$")
    parsed = [pat.match(l) for l in lines]
    assert len(lines) == 4 and all(parsed), lines
    assert "fit-st: box: 0 in [0, 0.05], st in [19.25, 20.25]" in r.stdout
    rows, _, _ = mio.read_jsfs(fj)
    table = np.array(rows, dtype=float)
    with Engine(inp.times, inp.lambdas, [(0, 2, -1, 0.1, 0)], [], n_param=1, cpfit=True, smooth=True, unfolded=False,
                sample_date=inp.sampleDateDiscr) as e:
        starts = np.array([[0.1, st] for _ in range(4) for st in (19.0, 19.5, 20.0)])
        res = e.nm_solve_box(starts, np.repeat(np.arange(4), 3).astype(np.int32), table, ([0.0, A], [R, B]))
    best = np.argmax(res["llh"].reshape(4, 3), axis=1)
    for r_, m in enumerate(parsed):
        s = 3 * r_ + best[r_]
        assert int(m.group(1)) == r_ and m.group(2) == str(float(res["split"][s])), (r_, m.group(2), res["split"][s])
        assert m.group(3) == str(res["x"][s, 0]) and m.group(4) == str(res["llh"][s])
        assert 0.0 <= float(m.group(3)) <= R and A <= float(m.group(2)) <= B
    assert any(float(m.group(3)) == R for m in parsed)
