"""Differential evolution per search on the device - misti_de_search, Engine.differential_evolution, optimize.split_fit_de /
bootstrap_profile_de and `--de` - against optimize.differential_evolution_rule driven by Engine.evaluate as its objective, bit for
bit: x, llh, nit, nfev, status, the final population and its values, and the number of points handed to the engine.

The shapes are the smallest at which the rule's branches can still go wrong, all inside one workgroup: a synthetic model on a
16-interval grid (the pulse case: the 32-interval grid of the pulse golden), populations of 4 and 7 (7 does not divide the selection
kernel's workgroup), at most 6 generations, 3 - 4 searches over 3 rows: a generation is at most 28 points.  The widths - searches over
several workgroups, up to 256 members, 16 coordinates - are held by tests/test_gpu_population_widths.py.  The rule's side of a case is
computed once."""
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

FIELDS = ("x", "llh", "nit", "nfev", "status", "population", "population_llh")
TABLE = np.array([[3e7, 9000, 2500, 10000, 6000, 4000, 2600, 4100], [2.9e7, 9100, 2400, 10100, 6100, 3900, 2500, 4000],
                  [3.1e7, 8900, 2600, 9900, 5900, 4100, 2700, 4200]])
ROWS = np.array([0, 1, 2, 1], dtype=np.int32)
SPLITS = np.array([11.0, 12.5, 12.0, 11.25])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def grid():
    from misti_amd import synth
    inp = synth.psmc_pair(8, 9)
    times, lh, _ = synth.self_consistent(inp, 11, [[1, 2, 11, 0.2, 0]], [])
    assert len(lh) == 16
    return times, lh


def engine(grid, bands, pulses=(), n_param=0):
    from misti_amd.engine import Engine
    return Engine(grid[0], grid[1], bands=bands, pulses=pulses, n_param=n_param, cpfit=True, smooth=True)


@pytest.fixture(scope="module")
def two_rates(grid):
    """Both populations' migration from interval 2 to the split, the two rates optimised."""
    e = engine(grid, [(0, 2, -1, 0.2, 0), (1, 2, -1, 0.1, 1)], n_param=2)
    yield e
    e.close()


def rule(eng, starts, rows, box, split_times=None, band_bounds=None, pulse_times=None, table=TABLE, **kw):
    """optimize.differential_evolution_rule on -Engine.evaluate: point m of a batch against its own search's row, split, band bounds
    and pulse times; no value scores +inf, as objective() of the kernels has it."""
    from misti_amd.optimize import differential_evolution_rule
    P = eng.n_param
    rows = np.asarray(rows)

    def fun(X, s):
        split = X[:, -1] if split_times is None else np.asarray(split_times)[s]
        r = eng.evaluate(split, X[:, :P] if P else None, table, band_bounds=None if band_bounds is None else np.asarray(band_bounds)[s],
                         pulse_times=None if pulse_times is None else np.asarray(pulse_times)[s])
        v = r.llk[np.arange(len(s)), rows[s]]
        return np.where(np.isnan(v) | (v == -np.inf), np.inf, -v)
    return differential_evolution_rule(fun, starts, box[0], box[1], **kw)


def device(eng, starts, rows, box, split_times=None, **kw):
    return eng.differential_evolution(starts, rows, TABLE, box, split_times=split_times, fit_split=split_times is None, return_population=True, **kw)


def assert_same(dev, ref, searches=None):
    for s in range(len(ref["llh"])) if searches is None else searches:
        print(s, "rule", ref["x"][s], ref["llh"][s], ref["nit"][s], ref["status"][s], "device", dev["x"][s], dev["llh"][s], dev["nit"][s], dev["status"][s])
    for k in FIELDS:
        a, b = (dev[k], ref[k]) if searches is None else (dev[k][searches], ref[k][searches])
        assert same_bits(np.asarray(a, dtype=b.dtype), b), k
    if searches is None:
        assert dev["n_points"] == ref["n_points"]


# ---- 1. N = 2 at a split per search: a fixed coordinate, a refused box, a search that stops early ---------------------------------------
MIXED = dict(pop=7, maxiter=6, tol=1e-6, atol=0.0, F=(0.5, 1.0), CR=0.7, seed=3)


@pytest.fixture(scope="module")
def mixed(two_rates):
    """Search 0: an ordinary box.  Search 1: a box a hair wide - its values agree to far less than tol x |mean| (a relative width of 5e-9
    against tol = 1e-6), so it stops after the initial population while the others run on.  Search 2: its second rate held fixed
    (lo == hi).  Search 3: negative rates throughout, which the engine refuses: no point ever has a value."""
    lo = np.array([[0.01, 0.01], [0.2, 0.1], [0.01, 0.15], [-0.5, -0.5]])
    hi = np.array([[1.0, 1.0], [0.2 + 1e-9, 0.1 + 1e-9], [1.0, 0.15], [-0.1, -0.1]])
    starts = np.array([[0.2, 0.1], [0.2, 0.1], [5.0, 0.3], [-0.2, -0.2]])               # search 2 starts outside its box: clipped
    ref = rule(two_rates, starts, ROWS, (lo, hi), split_times=SPLITS, **MIXED)
    dev = device(two_rates, starts, ROWS, (lo, hi), split_times=SPLITS, **MIXED)
    return starts, lo, hi, ref, dev


def test_a_mixed_call_equals_the_rule(mixed):
    starts, lo, hi, ref, dev = mixed
    assert_same(dev, ref)
    assert ref["status"].tolist() == [2, 0, 2, 2] and ref["nit"].tolist() == [6, 0, 6, 6]
    assert ref["n_points"] == 7 * (7 + 1 + 7 + 7) == int(dev["nfev"].sum())                   # no points for the stopped search
    assert np.isfinite(dev["llh"][:3]).all() and dev["llh"][3] == -np.inf and (dev["population_llh"][3] == -np.inf).all()
    assert (dev["population"][2][:, 1] == 0.15).all() and dev["x"][2, 1] == 0.15
    assert (dev["population"] >= lo[:, None, :]).all() and (dev["population"] <= hi[:, None, :]).all()
    assert same_bits(dev["split"], SPLITS)
    assert len({float(v) for v in dev["population_llh"][0]}) > 3                              # the search moved


def test_a_search_alone_equals_the_search_among_others(two_rates, mixed):
    starts, lo, hi, ref, dev = mixed
    for s in (0, 2):
        alone = device(two_rates, starts[s:s + 1], ROWS[s:s + 1], (lo[s:s + 1], hi[s:s + 1]), split_times=SPLITS[s:s + 1], ids=[s], **MIXED)
        for k in FIELDS:
            assert same_bits(alone[k][0], dev[k][s]), (s, k)
    perm = np.array([3, 1, 0, 2])
    shuffled = device(two_rates, starts[perm], ROWS[perm], (lo[perm], hi[perm]), split_times=SPLITS[perm], ids=perm, **MIXED)
    for k in FIELDS:
        assert same_bits(shuffled[k], dev[k][perm]), k


# ---- 2. the other coordinate counts ----------------------------------------------------------------------------------------------------
SMALL = dict(pop=4, maxiter=5, tol=1e-9, atol=0.0, F=(0.5, 1.0), CR=0.7, seed=1)


def test_one_coordinate(grid):
    with engine(grid, [(0, 2, -1, 0.2, 0)], n_param=1) as e:
        starts = np.array([[0.2], [0.05], [0.9]])
        box = (np.array([0.01]), np.array([1.0]))
        ref = rule(e, starts, ROWS[:3], box, split_times=SPLITS[:3], **SMALL)
        dev = device(e, starts, ROWS[:3], box, split_times=SPLITS[:3], **SMALL)
    assert_same(dev, ref)
    assert np.isfinite(dev["llh"]).all()


def test_two_rates_and_a_fitted_split(two_rates):
    starts = np.array([[0.2, 0.1, 11.0], [0.3, 0.05, 12.5], [0.1, 0.2, 10.0]])
    box = (np.array([0.01, 0.01, 9.0]), np.array([1.0, 1.0, 13.5]))
    ref = rule(two_rates, starts, ROWS[:3], box, **SMALL)
    dev = device(two_rates, starts, ROWS[:3], box, **SMALL)
    assert_same(dev, ref)
    assert np.isfinite(dev["llh"]).all() and same_bits(dev["split"], dev["x"][:, 2])
    assert (dev["split"] != np.floor(dev["split"])).any()                                     # fractional splits went through


def test_a_model_without_parameters_searches_the_split_alone(grid):
    with engine(grid, [(0, 2, -1, 0.2, -1)]) as e:
        assert e.n_param == 0
        starts = np.array([[11.0], [12.0], [10.5], [9.0]])
        box = (np.array([8.0]), np.array([14.0]))
        ref = rule(e, starts, ROWS, box, **SMALL)
        dev = device(e, starts, ROWS, box, **SMALL)
    assert_same(dev, ref)
    assert np.isfinite(dev["llh"]).all()


def test_band_bounds_and_pulse_times_per_search():
    """The pulse model of tests/golden/golden_pulse_sweep.json (its own 32-interval grid: the small grid above has no pulse its
    lambda correction accepts): a band's rate and the second pulse's fraction searched, every search with its own band interval and
    pulse times.  Search 3's pulse lies beyond the grid: the engine refuses every point of it."""
    from misti_amd import io as mio, synth
    from misti_amd.engine import Engine
    g = load_golden("golden_pulse_sweep")[0]["in"]
    table = np.array(mio.bootstrap_table(synth.chunk_rows(g["sfs"], 20), 3, random.Random(3)), dtype=np.float64)
    bb = np.array([[[4, -1]], [[5, -1]], [[4, 16]], [[4, -1]]], dtype=np.int32)
    pt = np.array([[10, 3], [10, 5], [10, 7], [10, 99]], dtype=np.int32)
    splits = np.array([20.0, 20.5, 18.0, 20.0])
    starts = np.tile([0.2, 0.1], (4, 1))
    box = (np.array([0.01, 0.0]), np.array([0.5, 0.3]))
    with Engine(g["times"], g["lambdas"], [(0, 4, -1, 0.2, 0)], [(0, 10, 0.05, -1), (1, 3, 0.0, 1)], n_param=2, cpfit=True, smooth=True,
                unfolded=True) as e:
        ref = rule(e, starts, ROWS, box, split_times=splits, band_bounds=bb, pulse_times=pt, table=table, **SMALL)
        dev = e.differential_evolution(starts, ROWS, table, box, split_times=splits, band_bounds=bb, pulse_times=pt, return_population=True, **SMALL)
    assert_same(dev, ref)
    assert np.isfinite(dev["llh"][:3]).any() and dev["llh"][3] == -np.inf


# ---- 3. the edges of the call ------------------------------------------------------------------------------------------------------------
def test_no_search_writes_nothing(two_rates):
    r = two_rates.differential_evolution(np.empty((0, 2)), np.empty(0, dtype=np.int32), TABLE, ([0.01, 0.01], [1.0, 1.0]),
                                         split_times=np.empty(0), return_population=True, **SMALL)
    assert r["x"].shape == (0, 2) and r["llh"].shape == (0,) and r["n_points"] == 0 and r["population"].shape == (0, 4, 2)


def test_polish_never_loses_to_the_search_it_follows(two_rates):
    from misti_amd.optimize import bootstrap_profile_de, split_fit_de
    box = (np.array([0.01, 0.01]), np.array([1.0, 1.0]))
    kw = dict(pop=4, maxiter=3, seed=2)
    plain = bootstrap_profile_de(two_rates, [11.0, 12.0], TABLE, [0.2, 0.1], box, **kw)
    pol = bootstrap_profile_de(two_rates, [11.0, 12.0], TABLE, [0.2, 0.1], box, polish=True, polish_maxiter=60, **kw)
    assert pol["llh"].shape == (3, 2) and same_bits(pol["de_llh"], plain["llh"]) and same_bits(plain["llh"], plain["de_llh"])
    assert (pol["llh"] >= pol["de_llh"]).all() and (pol["llh"] > pol["de_llh"]).any()
    assert (pol["x"] >= box[0]).all() and (pol["x"] <= box[1]).all()
    # a row's searches draw from streams 0, 1: the same whichever rows the call holds
    one = bootstrap_profile_de(two_rates, [11.0, 12.0], TABLE[1:2], [0.2, 0.1], box, **kw)
    assert same_bits(one["llh"][0], plain["llh"][1]) and same_bits(one["x"][0], plain["x"][1])
    box3 = (np.array([0.01, 0.01, 9.0]), np.array([1.0, 1.0, 13.5]))
    fit = split_fit_de(two_rates, TABLE, [0.2, 0.1, 11.0], box3, polish=True, polish_maxiter=60, **kw)
    assert fit["llh"].shape == (3,) and (fit["llh"] >= fit["de_llh"]).all() and same_bits(fit["split"], fit["x"][:, 2])


# ---- 4. the command line -----------------------------------------------------------------------------------------------------------------
def test_cli_de_prints_what_the_api_returns(tmp_path):
    """`--grid-solve --de` on the JSFS row of tests/golden/golden_pulse_sweep.json (three bootstrap rows behind it), on the synthetic PSMC
    pair that golden was made on: every result line carries the rate and the llh bootstrap_profile_de returns, digit for digit."""
    from misti_amd import io as mio, synth
    from misti_amd.engine import Engine
    from misti_amd.optimize import bootstrap_profile_de
    g = load_golden("golden_pulse_sweep")[0]["in"]
    f1, f2, fj = (str(tmp_path / n) for n in ("g1.psmc", "g2.psmc", "bs.sfs"))
    open(f1, "w").write(synth.psmc_text(16, 1, synth.THETA_1))
    open(f2, "w").write(synth.psmc_text(17, 2, synth.THETA_2))
    open(fj, "w").write(mio.format_jsfs(mio.bootstrap_table(synth.chunk_rows(g["sfs"], 20), 3, random.Random(5))))
    inp = mio.read_psmc(f1, f2)
    cmd = [sys.executable, "-m", "misti_amd.cli", f1, f2, fj, "20", "-mi", "1", "2", "20", "0.1", "1", "--cpfit", "--funits", str(tmp_path / "nounits.txt"),
           "--grid-st", "19", "20", "--all-bs", "--grid-solve", "--box", "0", "0.01", "1", "--de", "5", "4", "--de-seed", "7", "--de-CR", "0.9"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    pat = re.compile(r"^bs_id = (\S+) \tsplitT = (\S+) \ttime = \S+ \tmigration rates optim = \[(\S+)\] \tllh = (\S+)$")
    parsed = [pat.match(l) for l in r.stdout.splitlines() if l.startswith("bs_id =")]
    assert len(parsed) == 8 and all(parsed), r.stdout[-1500:]
    rows, _, _ = mio.read_jsfs(fj)
    with Engine(inp.times, inp.lambdas, [(0, 2, -1, 0.1, 0)], [], n_param=1, cpfit=True, smooth=True, unfolded=False, sample_date=inp.sampleDateDiscr) as e:
        prof = bootstrap_profile_de(e, [19, 20], np.array(rows, dtype=float), [0.1], (np.array([0.01]), np.array([1.0])), pop=5, maxiter=4, seed=7, CR=0.9)
    for j, m in enumerate(parsed):
        assert int(m.group(1)) == j // 2 and m.group(3) == str(prof["x"][j // 2, j % 2, 0]) and m.group(4) == str(prof["llh"][j // 2, j % 2]), (j, m.groups())
    assert "differential evolution with 5 members, at most 4 generations, F in [0.5, 1], CR 0.9, seed 7" in r.stdout
    assert "8 pairs in one population search" in r.stdout and "%d points" % prof["n_points"] in r.stdout
