"""Basin hopping per bootstrap row - misti_basinhopping_rows (a split time, a row, band bounds and pulse times per start) and
misti_basinhopping_split (the split as the last coordinate), Engine.basinhopping_rows / basinhopping_split,
optimize.split_fit_global and `--hops`.  The rows form is held to the one-row form (misti_basinhopping) bit for bit; the split form
has no reference run: its target is scipy.optimize.basinhopping on this engine's own objective over (parameters, split), bit for
bit, on config 3's model with its band ends following the split and on config 4's no-migration model (a 1-D search).
Sizes: at most 8 starts, niter <= 3, stepsize 0.05 and interval 2 (the step adjustment fires); nm_maxfev = 60 wherever SciPy runs
beside the device, so SciPy's side is at most (niter + 1) x 60 evaluations per start and the budget cut is exercised too."""
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

FIELDS = ("x", "llh", "nfev", "failures", "accepted")
HOPS = dict(niter=3, T=0.5, stepsize=0.05, interval=2)
SPLITS = [61.0, 62.5, 63.0, 64.25, 64.0, 65.5, 62.0, 63.75]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def config3():
    """Config 3's workload, band ends -1, and a 5-row bootstrap table (as tests/test_gpu_split_fit.py builds them)."""
    from misti_amd import io as mio, synth, workloads
    from misti_amd.engine import truth_spectrum
    w = workloads.config3(lambda *a: truth_spectrum(*a), n_start=4)
    bands = [(p, s, -1, v, k) for p, s, e, v, k in w.bands]
    table = np.array(mio.bootstrap_table(synth.chunk_rows(w.jsfs[0], 20), 4, random.Random(3)), dtype=np.float64)
    return w, bands, table


def engine_a(config3, band_starts=None):
    from misti_amd.engine import Engine
    w, bands, _ = config3
    if band_starts is not None:
        bands = [(p, b, e, v, k) for (p, s, e, v, k), b in zip(bands, band_starts)]
    kw = w.engine_kwargs()
    kw["bands"] = bands
    return Engine(w.times, w.lh, **kw)


@pytest.fixture(scope="module")
def model(config3):
    """Model A."""
    eng = engine_a(config3)
    yield eng, config3[2], np.array([b[3] for b in config3[1]])
    eng.close()


@pytest.fixture(scope="module")
def nomig():
    """Model B - config 4's: no migration, no optimised parameter; 12 rows of its bootstrap table."""
    from misti_amd import workloads
    from misti_amd.engine import Engine, truth_spectrum
    w = workloads.config4(lambda *a: truth_spectrum(*a), n_split=4, n_rep=12)
    eng = Engine(w.times, w.lh, **w.engine_kwargs())
    assert eng.n_param == 0 and w.jsfs.shape == (12, 8)
    yield eng, w.jsfs
    eng.close()


def scipy_hops(obj, x0, seed, n_coord, niter=3, stepsize=0.05):
    from scipy import optimize
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return optimize.basinhopping(obj, np.asarray(x0, dtype=float), niter=niter, T=0.5, stepsize=stepsize, interval=2,
                                     minimizer_kwargs=dict(method="Nelder-Mead", options=dict(maxfev=60, maxiter=200 * n_coord)),
                                     rng=np.random.default_rng(seed))


def split_objective(eng, table, row):
    """-engine.evaluate over (parameters, split) against one row; no value scores +inf."""
    P = eng.n_param

    def obj(x):
        v = float(eng.evaluate([x[-1]], [list(x[:-1])] if P else None, table[row:row + 1]).llk[0, 0])
        return -v if np.isfinite(v) else np.inf
    return obj


def assert_equals_scipy(got, s, ref):
    print(s, "scipy", ref.x, -ref.fun, ref.nfev, ref.minimization_failures,
          "device", got["x"][s], got["llh"][s], got["nfev"][s], got["failures"][s], got["accepted"][s])
    assert same_bits(np.asarray(ref.x, dtype=np.float64), got["x"][s]), (s, ref.x, got["x"][s])
    assert same_bits(np.float64(-ref.fun), got["llh"][s]), (s, -ref.fun, got["llh"][s])
    assert ref.nfev == got["nfev"][s] and ref.minimization_failures == got["failures"][s], (s, ref.nfev, ref.minimization_failures)


# ---- 1. the rows form equals the one-row form, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ["default", "0"])
def test_rows_form_equals_the_one_row_form_bit_for_bit(model, monkeypatch, spec):
    eng, table, start = model
    if spec == "0":
        monkeypatch.setenv("MISTI_NM_SPEC", "0")
    rows = np.array([0, 1, 2, 3, 4, 2, 0, 1], dtype=np.int32)
    starts = np.tile(start, (8, 1))
    starts[5] = [0.3, 0.02]
    starts[6] = [0.05, 0.5]
    seeds = [700 + s for s in range(8)]
    got = eng.basinhopping_rows(starts, SPLITS, rows, table, seeds, nm_maxfev=120, **HOPS)
    assert got["x"].shape == (8, 2) and np.isfinite(got["llh"]).all()
    assert (got["speculative_iterations"] > 0) == (spec == "default") and got["iterations_issued"] > 0
    for s in range(8):
        one = eng.basinhopping(starts[s:s + 1], SPLITS[s], table[rows[s]], [seeds[s]], nm_maxfev=120, **HOPS)
        print(s, [(f, got[f][s], one[f][0]) for f in FIELDS])
        for f in FIELDS:
            assert same_bits(got[f][s:s + 1], one[f]), (s, f, got[f][s], one[f])
    assert got["accepted"].sum() > 0 and (got["nfev"] <= 4 * 120).all()


# ---- 2. bounds and pulse times per start ---------------------------------------------------------------------------------------------
def test_band_bounds_per_start_equal_engines_built_with_them_and_broken_bounds_equal_scipy_on_inf(model, config3):
    eng, table, start = model
    sets = {0: [4, 10], 1: [6, 12]}                                          # the bands' starts; ends -1
    which = [0, 1, 1, 0, 1, 0, 0]
    bounds = np.array([[[sets[b][0], -1], [sets[b][1], -1]] for b in which], dtype=np.int32)
    bounds[3] = [[70, 8], [10, -1]]                                          # start >= end: breaks SetModel's checks
    rows = np.array([0, 1, 2, 3, 4, 2, 1], dtype=np.int32)
    splits = SPLITS[:7]
    starts = np.tile(start, (7, 1))
    starts[4] = [0.3, 0.02]
    seeds = [810 + s for s in range(7)]
    got = eng.basinhopping_rows(starts, splits, rows, table, seeds, band_bounds=bounds, nm_maxfev=60, **HOPS)
    good = [s for s in range(7) if s != 3]
    assert np.isfinite(got["llh"][good]).all()
    for b, band_starts in sets.items():
        sel = [s for s in good if which[s] == b]
        with engine_a(config3, band_starts) as e:                            # the reference is the OLD entry point, one row at a time
            for s in sel:
                one = e.basinhopping(starts[s:s + 1], splits[s], table[rows[s]], [seeds[s]], nm_maxfev=60, **HOPS)
                for f in FIELDS:
                    assert same_bits(got[f][s:s + 1], one[f]), (b, s, f, got[f][s], one[f])
    assert not same_bits(got["llh"][1:2], eng.basinhopping_rows(starts[1:2], splits[1:2], rows[1:2], table, seeds[1:2], nm_maxfev=60, **HOPS)["llh"])
    # the broken start: no point of it ever has a value - SciPy on an objective that returns inf
    ref = scipy_hops(lambda x: np.inf, starts[3], seeds[3], 2)
    assert got["llh"][3] == -np.inf and ref.fun == np.inf
    assert_equals_scipy(got, 3, ref)
    assert got["failures"][3] == HOPS["niter"] + 1 and got["nfev"][3] == 4 * 60


def test_pulse_times_per_start_equal_engines_built_with_them():
    """On the pulse model of tests/test_gpu_split_fit.py (two pulses, the second one's fraction optimised)."""
    from misti_amd.engine import Engine
    grid = load_golden("golden_pulse_sweep")[0]["in"]
    flags = dict(n_param=2, cpfit=True, smooth=True, unfolded=True)

    def engine(band_start, pulse_time):
        return Engine(grid["times"], grid["lambdas"], [(0, band_start, -1, 0.2, 0)], [(0, 10, 0.05, -1), (1, pulse_time, 0.0, 1)], **flags)
    table = np.array([grid["sfs"], [v * 2 for v in grid["sfs"]]], dtype=np.float64)
    band_start, pulse_time = [4, 6, 2], [5, 12, 15]
    splits = [20.0, 19.5, 21.0]
    rows = np.array([0, 1, 1], dtype=np.int32)
    starts = np.array([[0.2, 0.1]] * 3)
    bounds = np.array([[[b, -1]] for b in band_start], dtype=np.int32)
    times = np.array([[10, t] for t in pulse_time], dtype=np.int32)
    opts = dict(niter=2, T=0.5, stepsize=0.05, interval=2, nm_maxfev=60)
    with engine(4, 5) as e:
        rw = e.basinhopping_rows(starts, splits, rows, table, [31, 32, 33], band_bounds=bounds, pulse_times=times, **opts)
        sp = e.basinhopping_split(np.hstack([starts, np.array(splits)[:, None]]), rows, table, [31, 32, 33], band_bounds=bounds, pulse_times=times, **opts)
    assert np.isfinite(rw["llh"]).all() and np.isfinite(sp["llh"]).all()
    for s in range(3):
        with engine(band_start[s], pulse_time[s]) as e:
            one = e.basinhopping(starts[s:s + 1], splits[s], table[rows[s]], [31 + s], **opts)
            one_sp = e.basinhopping_split(np.array([list(starts[s]) + [splits[s]]]), rows[s:s + 1], table, [31 + s], **opts)
        for f in FIELDS:
            assert same_bits(rw[f][s:s + 1], one[f]), (s, f, rw[f][s], one[f])
            assert same_bits(sp[f][s:s + 1], one_sp[f]), (s, f, sp[f][s], one_sp[f])


# ---- 3. the fitted split equals SciPy, bit for bit -----------------------------------------------------------------------------------
def test_fitted_split_equals_scipy_bit_for_bit(model, nomig):
    accepted = 0
    eng, table, start = model
    starts = np.array([list(start) + [st] for st in (62.5, 63.0, 64.25, 65.5)])
    starts[3, :2] = [0.3, 0.02]
    rows = np.array([0, 2, 4, 1], dtype=np.int32)
    got = eng.basinhopping_split(starts, rows, table, [900 + s for s in range(4)], nm_maxfev=60, **HOPS)
    assert got["x"].shape == (4, 3) and same_bits(got["split"], got["x"][:, -1].copy()) and got["speculative_iterations"] > 0
    for s in range(4):
        assert_equals_scipy(got, s, scipy_hops(split_objective(eng, table, int(rows[s])), starts[s], 900 + s, 3))
    accepted += got["accepted"].sum()
    eng, table = nomig
    starts = np.array([[44.0], [47.25], [52.5], [57.75]])
    rows = np.array([0, 3, 7, 11], dtype=np.int32)
    got = eng.basinhopping_split(starts, rows, table, [950 + s for s in range(4)], nm_maxfev=60, **HOPS)
    assert got["x"].shape == (4, 1)
    for s in range(4):
        assert_equals_scipy(got, s, scipy_hops(split_objective(eng, table, int(rows[s])), starts[s], 950 + s, 1))
    accepted += got["accepted"].sum()
    assert accepted > 0                                                      # the Metropolis branch ran


# ---- 4. a hop that leaves the grid ---------------------------------------------------------------------------------------------------
def test_a_hop_that_leaves_the_grid_scores_inf_as_scipy_sees_it(nomig):
    from misti_amd.engine import draw_uniforms
    eng, table = nomig
    step = 3.0 * eng.numT                                                    # larger than the grid: most trial splits lie off it
    starts = np.array([[50.0], [52.5]])
    rows = np.array([1, 5], dtype=np.int32)
    got = eng.basinhopping_split(starts, rows, table, [61, 62], niter=3, T=0.5, stepsize=step, interval=2, nm_maxfev=60)    # returns: no error
    uni = draw_uniforms([61, 62], 2, 3, 1)
    first = starts[:, 0] + (-step + 2 * step * uni[:, 0, 0])                 # (about) where the first hop lands: the initial minimum moved little
    print("first trial splits about", first)
    assert ((first < 0) | (first > eng.numT)).any()                          # a hop did leave the grid
    for s in range(2):
        assert_equals_scipy(got, s, scipy_hops(split_objective(eng, table, int(rows[s])), starts[s], 61 + s, 1, stepsize=step))
    assert np.isfinite(got["llh"]).all()


# ---- 5. niter = 0 is the local search ------------------------------------------------------------------------------------------------
def test_no_hops_is_the_local_search_and_hops_never_lose(model):
    eng, table, start = model
    starts = np.array([list(start) + [st] for st in SPLITS[:6]])
    starts[5, :2] = [0.3, 0.02]
    rows = np.array([0, 1, 2, 3, 4, 2], dtype=np.int32)
    local = eng.nm_solve_split(starts, rows, table, tol=1e-4, maxiter=1000)
    budget = dict(nm_maxiter=1000, nm_maxfev=10 ** 9, xatol=1e-4, fatol=1e-4)
    none = eng.basinhopping_split(starts, rows, table, [1] * 6, niter=0, **budget)
    for f in ("x", "llh", "nfev"):
        assert same_bits(none[f], local[f]), (f, none[f], local[f])
    assert np.array_equal(none["failures"], (local["status"] != 0).astype(np.int32)) and (none["accepted"] == 0).all()
    hops = eng.basinhopping_split(starts, rows, table, [70 + s for s in range(6)], niter=3, T=0.5, stepsize=0.05, interval=2, **budget)
    ok = local["status"] == 0
    print("local", local["llh"], local["status"], "hops", hops["llh"], hops["accepted"])
    assert ok.any() and (hops["llh"][ok] >= none["llh"][ok]).all()


# ---- 6. optimize and the command line ------------------------------------------------------------------------------------------------
def test_split_fit_global_picks_per_row_from_the_documented_generators(model):
    from misti_amd.optimize import split_fit_global
    eng, table, start = model
    opts = dict(niter=2, T=0.5, stepsize=0.05, interval=2, nm_maxfev=60)
    fit = split_fit_global(eng, table[:3], [start], [62.0, 64.5], seed=5, **opts)
    pairs = np.array([list(start) + [62.0], list(start) + [64.5]])
    direct = eng.basinhopping_split(np.vstack([pairs] * 3), np.repeat(np.arange(3), 2).astype(np.int32), table[:3],
                                    [np.random.default_rng([5, j]) for _ in range(3) for j in range(2)], **opts)
    best = np.argmax(direct["llh"].reshape(3, 2), axis=1)
    for r in range(3):
        s = 2 * r + best[r]
        assert fit["start"][r] == best[r] and same_bits(fit["x"][r], direct["x"][s]) and fit["split"][r] == direct["split"][s]
        for f in ("llh", "nfev", "failures", "accepted"):
            assert fit[f][r] == direct[f][s], (r, f)
    alone = split_fit_global(eng, table[1:2], [start], [62.0, 64.5], seed=5, **opts)
    for f in ("x", "split", "llh", "nfev", "failures", "accepted", "start"):
        assert same_bits(alone[f][0], fit[f][1]), f


def _inputs(tmp_path):
    """The small files of tests/test_gpu_split_fit.py's command-line test."""
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


LINE = re.compile(r"^bs_id = (\S+) \tsplitT = (\S+) \ttime = \S+ \tmigration rates optim = \[(\S+)\] \tllh = (\S+) "
                  r"\thops accepted = (\d+) \tfailed minimisations = (\d+)$")


def test_cli_hops_with_fit_st_and_with_grid_solve(tmp_path):
    from conftest import ROOT
    from misti_amd import io as mio
    from misti_amd.engine import Engine
    from misti_amd.optimize import split_fit_global
    f1, f2, fj, inp = _inputs(tmp_path)
    base = [sys.executable, "-m", "misti_amd.cli", f1, f2, fj, "20", "-mi", "1", "2", "20", "0.1", "1", "--cpfit", "--funits",
            str(tmp_path / "nounits.txt"), "--grid-st", "19", "20", "--all-bs", "--hops", "2"]
    r = subprocess.run(base + ["--fit-st", "--hop-seed", "3"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    parsed = [LINE.match(l) for l in r.stdout.splitlines() if l.startswith("bs_id =")]
    assert len(parsed) == 4 and all(parsed), r.stdout[-1500:]
    assert "fit-st: basin hopping with 2 hops, step 0.5, seed 3" in r.stdout
    assert re.search(r"fit-st: bootstrap fitted splitT mean = \S+ 95% t-interval = ", r.stdout) or "fit-st: no bootstrap interval" in r.stdout
    rows, _, _ = mio.read_jsfs(fj)
    with Engine(inp.times, inp.lambdas, [(0, 2, -1, 0.1, 0)], [], n_param=1, cpfit=True, smooth=True, unfolded=False,
                sample_date=inp.sampleDateDiscr) as e:
        fit = split_fit_global(e, np.array(rows, dtype=float), [[0.1]], [19.0, 20.0], seed=3, niter=2, T=0.5, stepsize=0.5)
    for r_, m in enumerate(parsed):
        assert int(m.group(1)) == r_ and m.group(2) == str(float(fit["split"][r_])), (r_, m.group(2), fit["split"][r_])
        assert m.group(3) == str(fit["x"][r_, 0]) and m.group(4) == str(fit["llh"][r_])
        assert (int(m.group(5)), int(m.group(6))) == (fit["accepted"][r_], fit["failures"][r_])
    r = subprocess.run(base + ["--grid-solve"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    parsed = [LINE.match(l) for l in r.stdout.splitlines() if l.startswith("bs_id =")]
    assert len(parsed) == 8 and all(parsed), r.stdout[-1500:]                  # 4 rows x 2 splits, row outermost
    assert [(int(m.group(1)), m.group(2)) for m in parsed] == [(b, s) for b in range(4) for s in ("19.0", "20.0")]
    assert "grid-solve: basin hopping with 2 hops, step 0.5, seed 0" in r.stdout
    assert re.search(r"grid-solve: bs_id = 0 best splitT = \S+ optim = \[\S+\] llh = ", r.stdout)


# ---- 7. argument errors --------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_their_codes_and_leave_the_context_usable(model):
    from misti_amd._lib import MistiError
    eng, table, start = model
    ok_rows = dict(starts=[start], split_times=[63.0], rows=[0], table=table, rngs=[1], niter=1, nm_maxfev=20)
    ok_split = dict(starts=[list(start) + [63.0]], rows=[0], table=table, rngs=[1], niter=1, nm_maxfev=20)
    stats = (C.c_int64 * 2)()

    def refused(fn, ok, code=-1, **change):
        before = fn(**ok)                                                     # a valid call ...
        with pytest.raises(MistiError) as err:
            fn(**dict(ok, **change))
        assert err.value.code == code, change
        eng._lib.misti_nm_last_stats(eng._ctx, stats)
        assert stats[0] == before["iterations_issued"]                        # ... nothing ran in the refused one ...
        after = fn(**ok)                                                      # ... and the context is as usable as before
        for f in FIELDS:
            assert same_bits(before[f], after[f]), (change, f)
    for fn, ok in ((eng.basinhopping_rows, ok_rows), (eng.basinhopping_split, ok_split)):
        for change in (dict(rows=[5]), dict(rows=[-1]), dict(niter=-1), dict(nm_maxiter=0), dict(nm_maxfev=0), dict(interval=0),
                       dict(table=np.empty((0, 8)))):
            refused(fn, ok, **change)
    refused(eng.basinhopping_rows, ok_rows, split_times=[np.nan])
    refused(eng.basinhopping_rows, ok_rows, split_times=[np.inf])
    refused(eng.basinhopping_split, ok_split, starts=[[0.1, np.nan, 63.0]])
    refused(eng.basinhopping_split, ok_split, starts=[[0.1, 0.1, -np.inf]])
    # NULL pointers, straight at the library
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    st2, st3 = np.array([start]), np.array([list(start) + [63.0]])
    split, row = np.array([63.0]), np.zeros(1, dtype=np.int32)
    uni, x, llh = np.full(4, 0.5), np.empty(3), np.empty(1)
    tail = [1, 0.5, 0.05, 2, 0.5, 0.9, 1e-4, 1e-4, 400, 20, ptr(uni), ptr(x), ptr(llh), None, None, None]
    rows_args = [ptr(st2), ptr(split), ptr(row), None, None, 5, ptr(table)] + tail
    split_args = [ptr(st3), ptr(row), None, None, 5, ptr(table)] + tail
    for fn, args, nulls in ((eng._lib.misti_basinhopping_rows, rows_args, (0, 1, 2, 6, 17, 18, 19)),
                            (eng._lib.misti_basinhopping_split, split_args, (0, 1, 5, 16, 17, 18))):
        for k in nulls:                                                       # starts, (split_times,) rows, jsfs, uniforms, x, llh
            a = list(args)
            a[k] = None
            assert fn(eng._ctx, 1, *a) == -1, k
        assert fn(None, 1, *args) == -1 and fn(eng._ctx, -1, *args) == -1
        assert fn(eng._ctx, 0, *args) == 0                                    # no start: nothing to do
        assert fn(eng._ctx, 1, *args) == 0 and np.isfinite(llh[0])            # the counters may be NULL
    eng.basinhopping_rows(**ok_rows)


def test_too_many_starts_are_beyond_the_limit_for_both_forms():
    """MISTI_E_LIMIT for n_start > INT32_MAX / (8 (N + 1)), N the number of coordinates - on a 15-parameter model, where the limit is
    lowest: 16 777 215 starts for the rows form (N = 15), 15 790 320 for the split form (N = 16).  Straight at the library, every array
    at its full size but never written: zero pages, of which the checks read the rows and the split times (some 200 MB) and - the
    limits come before the scan of the starts - nothing else.  Nothing runs, and a valid call afterwards succeeds."""
    from misti_amd.engine import Engine
    grid = load_golden("golden_pulse_sweep")[0]["in"]
    bands = [(p, 2 + 5 * i, 6 + 5 * i, 0.1, 4 * p + i) for p in (0, 1) for i in range(4)]
    pulses = [(k & 1, 3 + k, 0.01, 8 + k) for k in range(7)]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    table = np.array([grid["sfs"]], dtype=np.float64)
    hop = [0, 0.5, 0.05, 2, 0.5, 0.9, 1e-4, 1e-4, 20, 20, None]                 # niter = 0: no uniforms
    stats = (C.c_int64 * 2)()
    with Engine(grid["times"], grid["lambdas"], bands, pulses, n_param=15, cpfit=True, smooth=True, unfolded=True) as e:
        lib, ctx = e._lib, e._ctx
        for form, N in (("rows", 15), ("split", 16)):
            fn = getattr(lib, "misti_basinhopping_" + form)
            limit = (2 ** 31 - 1) // (8 * (N + 1))

            def call(S):
                starts = np.zeros((S, N)) if S > 1 else np.full((1, N), 0.1)
                if form == "split":
                    starts[:1, -1] = 25.0
                rows, x, llh = np.zeros(S, dtype=np.int32), np.zeros((S, N)), np.zeros(S)
                per_start = [ptr(np.full(S, 25.0) if S == 1 else np.zeros(S))] if form == "rows" else []
                return fn(ctx, S, ptr(starts), *per_start, ptr(rows), None, None, 1, ptr(table), *hop, ptr(x), ptr(llh), None, None, None), llh
            assert call(1)[0] == 0                                            # a valid call ...
            lib.misti_nm_last_stats(ctx, stats)
            before = (stats[0], stats[1])
            assert before[0] > 0
            rc, _ = call(limit + 1)
            assert rc == -4 and b"too many starts" in lib.misti_last_error()  # MISTI_E_LIMIT
            lib.misti_nm_last_stats(ctx, stats)
            assert (stats[0], stats[1]) == before                             # ... nothing ran in the refused one ...
            assert call(1)[0] == 0                                            # ... and the context is as usable as before


def test_sixteen_parameters_and_the_split_are_beyond_the_limit():
    from misti_amd._lib import MistiError
    from misti_amd.engine import Engine
    grid = load_golden("golden_pulse_sweep")[0]["in"]
    bands = [(p, 2 + 5 * i, 6 + 5 * i, 0.1, 4 * p + i) for p in (0, 1) for i in range(4)]
    pulses = [(k & 1, 3 + k, 0.01, 8 + k) for k in range(8)]
    with Engine(grid["times"], grid["lambdas"], bands, pulses, n_param=16, cpfit=True, smooth=True, unfolded=True) as e:
        with pytest.raises(MistiError) as err:
            e.basinhopping_split(np.full((1, 17), 0.1), [0], [grid["sfs"]], [1], niter=1)
        assert err.value.code == -4                                           # MISTI_E_LIMIT
        stats = (C.c_int64 * 2)()
        e._lib.misti_nm_last_stats(e._ctx, stats)
        assert (stats[0], stats[1]) == (0, 0)                                 # nothing ran
