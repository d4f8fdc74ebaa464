"""The split time as a coordinate of the batched Nelder-Mead - misti_nm_solve_split, Engine.nm_solve_split, optimize.split_fit and
`--fit-st`.  The reference has no such search: the target is SciPy's Nelder-Mead on this engine's own objective over (parameters,
split), bit for bit, on config 3's model with its band ends following the split and on config 4's no-migration model (a 1-D search)."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

FIELDS = ("x", "llh", "nit", "nfev", "status")
OPTIONS = {"xatol": 1e-4, "fatol": 1e-4, "maxiter": 1000}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def model():
    """Config 3's model as tests/test_gpu_bs_profile.py builds it: band ends -1, a 5-row bootstrap table."""
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


def scipy_search(eng, table, row, x0):
    """scipy.optimize.minimize(method='Nelder-Mead') on -engine.evaluate over (parameters, split); no value scores +inf."""
    from scipy import optimize
    P = eng.n_param

    def obj(x):
        v = float(eng.evaluate([x[-1]], [list(x[:-1])] if P else None, table[row:row + 1]).llk[0, 0])
        return -v if np.isfinite(v) else np.inf
    return optimize.minimize(obj, np.asarray(x0, dtype=float), method="Nelder-Mead", options=OPTIONS)


def assert_equals_scipy(eng, table, got, starts, rows):
    for s in range(len(rows)):
        ref = scipy_search(eng, table, int(rows[s]), starts[s])
        print(s, starts[s], rows[s], "scipy", ref.x, -ref.fun, ref.nit, ref.nfev, ref.status,
              "device", got["x"][s], got["llh"][s], got["nit"][s], got["nfev"][s], got["status"][s])
        assert same_bits(np.asarray(ref.x, dtype=np.float64), got["x"][s]), (s, ref.x, got["x"][s])
        assert same_bits(np.float64(-ref.fun), got["llh"][s]), (s, -ref.fun, got["llh"][s])
        assert ref.nit == got["nit"][s] and ref.nfev == got["nfev"][s] and ref.status == got["status"][s], (s, ref.nit, ref.nfev, ref.status)
        assert got["split"][s] == got["x"][s, -1]


# ---- 1. equals SciPy, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ["default", "0"])
def test_split_as_coordinate_equals_scipy_bit_for_bit(model, monkeypatch, spec):
    eng, table, start = model
    if spec == "0":
        monkeypatch.setenv("MISTI_NM_SPEC", "0")
    splits = [61.0, 62.5, 63.0, 64.25, 64.0, 65.5, 62.0, 63.75]
    rows = np.array([0, 1, 2, 3, 4, 2, 0, 1], dtype=np.int32)
    starts = np.array([list(start) + [st] for st in splits])
    starts[5, :2] = [0.3, 0.02]
    starts[6, :2] = [0.05, 0.5]
    got = eng.nm_solve_split(starts, rows, table, tol=1e-4, maxiter=1000)
    assert got["x"].shape == (8, 3) and np.isfinite(got["llh"]).all()
    assert_equals_scipy(eng, table, got, starts, rows)
    assert (got["speculative_iterations"] > 0) == (spec == "default")


# ---- 2. the no-migration model: a 1-D search ---------------------------------------------------------------------------------------
def test_no_migration_model_is_a_one_coordinate_search(nomig):
    from misti_amd._lib import MistiError
    eng, table = nomig
    rows = np.arange(12, dtype=np.int32)
    starts = (44.0 + 1.25 * np.arange(12)).reshape(12, 1)              # 44, 45.25, ... 57.75: integer and fractional initial splits
    got = eng.nm_solve_split(starts, rows, table, tol=1e-4, maxiter=1000)
    assert got["x"].shape == (12, 1) and np.isfinite(got["llh"]).all()
    assert_equals_scipy(eng, table, got, starts, rows)
    # the searches with a fixed split still have nothing to optimise on this model
    with pytest.raises((MistiError, ValueError)):
        eng.nm_solve(np.empty((1, 0)), 50.0, table[0])
    with pytest.raises((MistiError, ValueError)):
        eng.nm_solve_rows(np.empty((1, 0)), [50.0], [0], table)
    # ... and the library itself refuses them (MISTI_E_ARG), whatever the binding does with a zero-width array
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    x0, split, row = np.zeros(1), np.array([50.0]), np.zeros(1, dtype=np.int32)
    x, llh = np.empty(1), np.empty(1)
    assert eng._lib.misti_nm_solve(eng._ctx, 1, ptr(x0), 50.0, ptr(table), 1e-4, 1e-4, 10, ptr(x), ptr(llh), None, None, None) == -1
    assert eng._lib.misti_nm_solve_rows(eng._ctx, 1, ptr(x0), ptr(split), ptr(row), 12, ptr(table), 1e-4, 1e-4, 10,
                                        ptr(x), ptr(llh), None, None, None) == -1


# ---- 3. never worse than the scan ------------------------------------------------------------------------------------------------
def test_fit_from_the_scan_winner_is_never_worse(model):
    from misti_amd.optimize import bootstrap_profile
    eng, table, start = model
    grid = [61.0, 62.0, 63.0, 64.0, 65.0, 66.0]
    prof = bootstrap_profile(eng, grid, table, [start])
    best = np.argmax(prof["llh"], axis=1)
    R = table.shape[0]
    x0 = np.array([list(prof["x"][r, best[r]]) + [grid[best[r]]] for r in range(R)])
    llh_scan = prof["llh"][np.arange(R), best]
    fit = eng.nm_solve_split(x0, np.arange(R, dtype=np.int32), table)
    print("scan", llh_scan, "fit", fit["llh"], "split", fit["split"])
    assert (fit["llh"] >= llh_scan).all()                              # the start is a vertex and the best vertex is returned
    assert np.isfinite(fit["split"]).all() and (fit["split"] >= 0).all() and (fit["split"] < eng.numT).all()


def test_no_migration_fit_from_the_scan_winner_is_never_worse(nomig):
    """The same on the 1-D model, the start taken from bootstrap_scan_dev's per-row winner."""
    from misti_amd.optimize import bootstrap_scan_dev
    eng, table = nomig
    grid = np.arange(45.0, 56.0)
    _, _, best = bootstrap_scan_dev(eng, grid, table)
    llh_scan = eng.evaluate(grid, None, table).llk.max(axis=0)
    fit = eng.nm_solve_split(best.reshape(-1, 1), np.arange(12, dtype=np.int32), table)
    assert (fit["llh"] >= llh_scan).all()
    assert np.isfinite(fit["split"]).all() and (fit["split"] >= 0).all() and (fit["split"] < eng.numT).all()


# ---- 4. per-start bounds and pulse times -----------------------------------------------------------------------------------------
def test_per_start_bounds_and_pulse_times_equal_fresh_engines():
    from misti_amd.engine import Engine
    grid = load_golden("golden_pulse_sweep")[0]["in"]
    flags = dict(n_param=2, cpfit=True, smooth=True, unfolded=True)

    def engine(band_start, pulse_time):
        return Engine(grid["times"], grid["lambdas"], [(0, band_start, -1, 0.2, 0)], [(0, 10, 0.05, -1), (1, pulse_time, 0.0, 1)], **flags)
    table = np.array([grid["sfs"], [v * 2 for v in grid["sfs"]]], dtype=np.float64)
    band_start = [4, 6, 2, 4, 8]
    pulse_time = [5, 5, 12, 15, 3]
    splits = [20.0, 19.5, 21.0, 18.25, 20.0]
    rows = np.array([0, 1, 0, 1, 1], dtype=np.int32)
    starts = np.array([[0.2, 0.1, st] for st in splits])
    bounds = np.array([[[b, -1]] for b in band_start], dtype=np.int32)
    times = np.array([[10, t] for t in pulse_time], dtype=np.int32)
    with engine(4, 5) as e:
        got = e.nm_solve_split(starts, rows, table, band_bounds=bounds, pulse_times=times)
    assert np.isfinite(got["llh"]).all()
    for s in range(5):
        with engine(band_start[s], pulse_time[s]) as e:
            one = e.nm_solve_split(starts[s:s + 1], rows[s:s + 1], table)
        for f in FIELDS + ("split",):
            assert same_bits(got[f][s:s + 1], one[f]), (s, f, got[f][s], one[f])


# ---- 5. refusals and limits ------------------------------------------------------------------------------------------------------
def test_refused_initial_splits_score_minus_inf_and_leave_neighbours_alone(model):
    """Initial splits -3, numT + 7.5 and numT + 20: every point SciPy's iteration forms from such a simplex (reflections,
    contractions and shrinks of vertices st and 1.05 st) is refused as well, so the start ends with llh = -inf.  An initial split
    of exactly numT is different and is checked against SciPy instead: its simplex (numT, 1.05 numT) is all +inf, the stable sort
    leaves the vertex at 1.05 numT last, and the first reflection 2 numT - 1.05 numT = 0.95 numT lies inside the grid and has a
    value - SciPy's search walks back into the grid, and so does this one."""
    eng, table, start = model
    good = np.array([list(start) + [63.0], list(start) + [64.5], [0.3, 0.02, 62.0]])
    rows = np.array([0, 2, 4], dtype=np.int32)
    alone = eng.nm_solve_split(good, rows, table, maxiter=200)
    bad = np.array([list(start) + [-3.0], list(start) + [eng.numT + 20.0], list(start) + [eng.numT + 7.5]])
    mixed = np.vstack([bad[0], good[0], bad[1], good[1], good[2], bad[2]])
    got = eng.nm_solve_split(mixed, np.array([1, 0, 3, 2, 4, 0], dtype=np.int32), table, maxiter=200)
    assert (got["llh"][[0, 2, 5]] == -np.inf).all()
    for f in FIELDS:
        assert same_bits(got[f][[1, 3, 4]], alone[f]), (f, got[f], alone[f])
    edge = np.array([list(start) + [float(eng.numT)]])
    at_edge = eng.nm_solve_split(edge, [1], table)
    assert_equals_scipy(eng, table, at_edge, edge, [1])


def test_sixteen_parameters_are_beyond_the_limit():
    from misti_amd._lib import MistiError
    from misti_amd.engine import Engine
    grid = load_golden("golden_pulse_sweep")[0]["in"]
    bands = [(p, 2 + 5 * i, 6 + 5 * i, 0.1, 4 * p + i) for p in (0, 1) for i in range(4)]
    pulses = [(k & 1, 3 + k, 0.01, 8 + k) for k in range(8)]
    with Engine(grid["times"], grid["lambdas"], bands, pulses, n_param=16, cpfit=True, smooth=True, unfolded=True) as e:
        with pytest.raises(MistiError) as err:
            e.nm_solve_split(np.full((1, 17), 0.1), [0], [grid["sfs"]])
        assert err.value.code == -4                                    # MISTI_E_LIMIT
        stats = (C.c_int64 * 2)()
        e._lib.misti_nm_last_stats(e._ctx, stats)
        assert (stats[0], stats[1]) == (0, 0)                          # nothing ran


def test_argument_errors_before_any_device_work(model):
    from misti_amd._lib import MistiError
    eng, table, start = model
    ok = np.array([list(start) + [63.0]])
    eng.nm_solve_split(ok, [0], table, maxiter=5)
    stats = (C.c_int64 * 2)()
    eng._lib.misti_nm_last_stats(eng._ctx, stats)
    before = (stats[0], stats[1])
    assert before[0] > 0
    for starts, rows, kw in ((ok, [5], {}), (ok, [-1], {}), (np.array([[0.1, np.nan, 63.0]]), [0], {}), (np.array([[0.1, 0.1, np.inf]]), [0], {}),
                             (ok, [0], dict(maxiter=0))):
        with pytest.raises(MistiError) as err:
            eng.nm_solve_split(starts, rows, table, **kw)
        assert err.value.code == -1, (starts, rows, kw)                # MISTI_E_ARG
    x, llh = np.empty((1, 3)), np.empty(1)
    row = np.zeros(1, dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    full = [ptr(ok), ptr(row), None, None, 5, ptr(table), 1e-4, 1e-4, 10, ptr(x), ptr(llh), None, None, None]
    for k in (0, 1, 5, 9, 10):                                         # starts, rows, jsfs, x, llh
        args = list(full)
        args[k] = None
        assert eng._lib.misti_nm_solve_split(eng._ctx, 1, *args) == -1, k
    args = list(full)
    args[4] = 0                                                        # n_rep < 1
    assert eng._lib.misti_nm_solve_split(eng._ctx, 1, *args) == -1
    assert eng._lib.misti_nm_solve_split(None, 1, *full) == -1
    eng._lib.misti_nm_last_stats(eng._ctx, stats)
    assert (stats[0], stats[1]) == before                              # nothing ran


# ---- 6. the old paths are untouched ----------------------------------------------------------------------------------------------
def test_old_searches_are_byte_equal_around_a_split_search(model):
    eng, table, start = model
    starts = np.vstack([start, [0.3, 0.02], [0.05, 0.5]])
    splits = np.array([62.0, 63.5, 64.0])
    rows = np.array([0, 3, 1], dtype=np.int32)

    def old():
        return [eng.nm_solve(starts, 63.5, table[0], maxiter=200),
                eng.nm_solve_rows(starts, splits, rows, table, maxiter=200),
                eng.nm_solve_pulses(starts, splits, rows, table, np.array([[[4, -1], [10, -1]]] * 3, dtype=np.int32), None, maxiter=200),
                eng.basinhopping(starts[:2], 64.0, table[0], [11, 12], niter=2, nm_maxiter=60)]
    a = old()
    eng.nm_solve_split(np.hstack([starts, splits[:, None]]), rows, table, maxiter=200)
    b = old()
    for ra, rb in zip(a, b):
        for f, v in ra.items():
            if isinstance(v, np.ndarray):
                assert same_bits(v, rb[f]), f
            else:
                assert v == rb[f], f


# ---- 7. the command line ---------------------------------------------------------------------------------------------------------
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


def test_cli_fit_st_prints_the_fitted_split_per_row_and_the_interval(tmp_path):
    from conftest import ROOT
    from misti_amd import io as mio
    from misti_amd.engine import Engine
    from misti_amd.optimize import split_fit, split_fit_interval
    f1, f2, fj, inp = _inputs(tmp_path)
    units = str(tmp_path / "nounits.txt")
    cmd = [sys.executable, "-m", "misti_amd.cli", f1, f2, fj, "20", "-mi", "1", "2", "20", "0.1", "1", "--cpfit", "--funits", units,
           "--grid-st", "19", "20", "0.5", "--all-bs", "--fit-st"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("bs_id =")]
    pat = re.compile(r"^bs_id = (\S+) \tsplitT = (\S+) \ttime = \S+ \tmigration rates optim = \[(\S+)\] \tllh = (\S+)$")
    parsed = [pat.match(l) for l in lines]
    assert len(lines) == 4 and all(parsed), lines
    assert [int(m.group(1)) for m in parsed] == [0, 1, 2, 3]
    rows, _, _ = mio.read_jsfs(fj)
    table = np.array(rows, dtype=float)
    with Engine(inp.times, inp.lambdas, [(0, 2, -1, 0.1, 0)], [], n_param=1, cpfit=True, smooth=True, unfolded=False,
                sample_date=inp.sampleDateDiscr) as e:
        starts = np.array([[0.1, st] for _ in range(4) for st in (19.0, 19.5, 20.0)])
        res = e.nm_solve_split(starts, np.repeat(np.arange(4), 3).astype(np.int32), table)
        fit = split_fit(e, table, [[0.1]], [19.0, 19.5, 20.0])
    best = np.argmax(res["llh"].reshape(4, 3), axis=1)
    for r_, m in enumerate(parsed):
        s = 3 * r_ + best[r_]
        assert m.group(2) == str(float(res["split"][s])), (r_, m.group(2), res["split"][s])
        assert m.group(3) == str(res["x"][s, 0]) and m.group(4) == str(res["llh"][s])
        assert fit["split"][r_] == res["split"][s] and fit["start"][r_] == best[r_]
    iv = split_fit_interval(fit["split"], fit["llh"])
    m = re.search(r"fit-st: bootstrap fitted splitT mean = (\S+) 95% t-interval = \[(\S+), (\S+)\] over (\d+) replicates", r.stdout)
    assert m, r.stdout[-800:]
    assert float(m.group(1)) == iv["mean"] and int(m.group(4)) == iv["n_boot"] == 3
    assert np.array_equal([float(m.group(2)), float(m.group(3))], iv["interval"], equal_nan=True)
