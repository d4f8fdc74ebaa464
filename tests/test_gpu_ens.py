"""Ensemble MCMC per search on the device - misti_ensemble_sample, Engine.ensemble_sample and `--mcmc` - against optimize.ensemble_rule
driven by Engine.evaluate as its objective, bit for bit: the chain, its values, the per-walker acceptance counters, the final ensemble
and the number of points handed to the engine.

The shapes are those of tests/test_gpu_de.py: its synthetic model on a 16-interval grid (the pulse case: the 32-interval grid of the
pulse golden), the three-row table, at most 4 searches, ensembles of 4 - 8 walkers, at most 6 steps: a half-step is at most 12
points, all inside one workgroup.  The widths - searches over several workgroups, 256 walkers, 16 coordinates - are held by
tests/test_gpu_population_widths.py.  The rule's side of a case is computed once."""
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

FIELDS = ("chain", "chain_llh", "accepted", "last", "last_llh")
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


def rule(eng, init, rows, box, split_times=None, band_bounds=None, pulse_times=None, table=TABLE, **kw):
    """optimize.ensemble_rule on -Engine.evaluate: point m of a batch against its own search's row, split, band bounds and pulse times; no
    value scores +inf."""
    from misti_amd.optimize import ensemble_rule
    P = eng.n_param
    rows = np.asarray(rows)

    def fun(X, s):
        split = X[:, -1] if split_times is None else np.asarray(split_times)[s]
        r = eng.evaluate(split, X[:, :P] if P else None, table, band_bounds=None if band_bounds is None else np.asarray(band_bounds)[s],
                         pulse_times=None if pulse_times is None else np.asarray(pulse_times)[s])
        v = r.llk[np.arange(len(s)), rows[s]]
        return np.where(np.isnan(v) | (v == -np.inf), np.inf, -v)
    return ensemble_rule(fun, init, box[0], box[1], **kw)


def device(eng, init, rows, box, split_times=None, table=TABLE, **kw):
    return eng.ensemble_sample(init, rows, table, box, split_times=split_times, fit_split=split_times is None, **kw)


def start(points, lo, hi, W, spread=0.2, seed=1):
    """init[S][W][N]: an ensemble around every point, inside its box."""
    from misti_amd.optimize import ensemble_start
    points = np.atleast_2d(points)
    lo, hi = (np.broadcast_to(np.asarray(v, dtype=float), points.shape) for v in (lo, hi))
    spread = np.broadcast_to(spread, (len(points),))
    return np.stack([ensemble_start(p, lo[s], hi[s], W, spread[s], seed, s) for s, p in enumerate(points)])


def assert_same(dev, ref, searches=None):
    for s in range(len(ref["last"])) if searches is None else searches:
        print(s, "rule", ref["last_llh"][s], ref["accepted"][s], "device", dev["last_llh"][s], dev["accepted"][s])
    for k in FIELDS:
        a, b = (dev[k], ref[k]) if searches is None else (dev[k][searches], ref[k][searches])
        assert same_bits(np.asarray(a, dtype=b.dtype), b), k
    if searches is None:
        assert dev["n_points"] == ref["n_points"]


# ---- 1. N = 2 at a split per search: boxes, temperatures and a fixed coordinate per search ---------------------------------------------
MIXED = dict(n_step=5, thin=2, a=2.0, seed=3)


@pytest.fixture(scope="module")
def mixed(two_rates):
    """Search 0: an ordinary box.  Search 1: a tight box around its ensemble - stretches beyond it are rejected in advance.  Search 2:
    its second rate held fixed (lo == hi; d = 0).  Search 3: a hot ensemble (T = 50) in a wide box."""
    lo = np.array([[0.01, 0.01], [0.15, 0.06], [0.01, 0.15], [0.001, 0.001]])
    hi = np.array([[1.0, 1.0], [0.25, 0.14], [1.0, 0.15], [3.0, 3.0]])
    T = np.array([1.0, 2.0, 0.5, 50.0])
    init = start([[0.2, 0.1], [0.2, 0.1], [0.3, 0.15], [0.5, 0.4]], lo, hi, 6, spread=[0.05, 0.3, 0.05, 0.05])
    ref = rule(two_rates, init, ROWS, (lo, hi), split_times=SPLITS, temperature=T, **MIXED)
    dev = device(two_rates, init, ROWS, (lo, hi), split_times=SPLITS, temperature=T, **MIXED)
    return init, lo, hi, T, ref, dev


def test_a_mixed_call_equals_the_rule(mixed):
    init, lo, hi, T, ref, dev = mixed
    assert_same(dev, ref)
    assert dev["chain"].shape == (4, 2, 6, 2) and dev["chain_llh"].shape == (4, 2, 6) and dev["accepted"].dtype == np.int32
    assert np.isfinite(dev["last_llh"]).any(axis=1).all() and (dev["chain"][2][:, :, 1] == 0.15).all()
    assert (dev["chain"] >= lo[:, None, None, :]).all() and (dev["chain"] <= hi[:, None, None, :]).all()
    assert (dev["accepted"] <= 5).all() and dev["accepted"].sum() > 0 and not same_bits(dev["last"], init)      # the ensembles moved
    assert 0 < ref["n_points"] < 5 * 4 * 6                                            # the rule rejected proposals in advance


def test_a_search_alone_equals_the_search_among_others(two_rates, mixed):
    init, lo, hi, T, ref, dev = mixed
    n = 0
    for s in range(4):
        alone = device(two_rates, init[s:s + 1], ROWS[s:s + 1], (lo[s:s + 1], hi[s:s + 1]), split_times=SPLITS[s:s + 1], temperature=T[s:s + 1], ids=[s], **MIXED)
        n += alone["n_points"]
        for k in FIELDS:
            assert same_bits(alone[k][0], dev[k][s]), (s, k)
    assert n == dev["n_points"] == ref["n_points"]                  # per search too: out-of-box proposals are not submitted
    perm = np.array([3, 1, 0, 2])
    shuffled = device(two_rates, init[perm], ROWS[perm], (lo[perm], hi[perm]), split_times=SPLITS[perm], temperature=T[perm], ids=perm, **MIXED)
    for k in FIELDS:
        assert same_bits(shuffled[k], dev[k][perm]), k


# ---- 2. the other models ---------------------------------------------------------------------------------------------------------------
SMALL = dict(n_step=6, thin=1, seed=1)


def test_one_coordinate(grid):
    with engine(grid, [(0, 2, -1, 0.2, 0)], n_param=1) as e:
        box = (np.array([0.01]), np.array([1.0]))
        init = start([[0.2], [0.05], [0.9]], *box, 4)
        ref = rule(e, init, ROWS[:3], box, split_times=SPLITS[:3], **SMALL)
        dev = device(e, init, ROWS[:3], box, split_times=SPLITS[:3], **SMALL)
    assert_same(dev, ref)
    assert np.isfinite(dev["last_llh"]).any(axis=1).all() and dev["accepted"].sum() > 0


def test_two_rates_and_a_fitted_split(two_rates):
    box = (np.array([0.01, 0.01, 9.0]), np.array([1.0, 1.0, 13.5]))
    init = start([[0.2, 0.1, 11.0], [0.3, 0.1, 12.0], [0.1, 0.2, 10.0]], *box, 8, spread=0.05)
    ref = rule(two_rates, init, ROWS[:3], box, temperature=3.0, **SMALL)
    dev = device(two_rates, init, ROWS[:3], box, temperature=3.0, **SMALL)
    assert_same(dev, ref)
    print("walkers with a value per search:", np.isfinite(dev["last_llh"]).sum(axis=1), "accepted:", dev["accepted"].sum(axis=1))
    assert np.isfinite(dev["last_llh"]).any() and dev["accepted"].sum() > 0
    assert (dev["last"][:, :, 2] != np.floor(dev["last"][:, :, 2])).any()                                          # fractional splits went through


def test_a_model_without_parameters_samples_the_split_alone(grid):
    with engine(grid, [(0, 2, -1, 0.2, -1)]) as e:
        assert e.n_param == 0
        box = (np.array([8.0]), np.array([14.0]))
        init = start([[11.0], [12.0], [10.5], [9.0]], *box, 4, spread=0.1)
        ref = rule(e, init, ROWS, box, **SMALL)
        dev = device(e, init, ROWS, box, **SMALL)
    assert_same(dev, ref)
    assert np.isfinite(dev["last_llh"]).all()


def test_band_bounds_and_pulse_times_per_search():
    """The pulse model of tests/golden/golden_pulse_sweep.json on its own 32-interval grid (tests/test_gpu_de.py): every search with its
    own band interval and pulse times.  Search 3's pulse lies beyond the grid: the engine refuses every point of it, nothing moves."""
    from misti_amd import io as mio, synth
    from misti_amd.engine import Engine
    g = load_golden("golden_pulse_sweep")[0]["in"]
    table = np.array(mio.bootstrap_table(synth.chunk_rows(g["sfs"], 20), 3, random.Random(3)), dtype=np.float64)
    bb = np.array([[[4, -1]], [[5, -1]], [[4, 16]], [[4, -1]]], dtype=np.int32)
    pt = np.array([[10, 3], [10, 5], [10, 7], [10, 99]], dtype=np.int32)
    splits = np.array([20.0, 20.5, 18.0, 20.0])
    box = (np.array([0.01, 0.0]), np.array([0.5, 0.3]))
    init = start(np.tile([0.2, 0.1], (4, 1)), *box, 4, spread=0.1)
    with Engine(g["times"], g["lambdas"], [(0, 4, -1, 0.2, 0)], [(0, 10, 0.05, -1), (1, 3, 0.0, 1)], n_param=2, cpfit=True, smooth=True,
                unfolded=True) as e:
        ref = rule(e, init, ROWS, box, split_times=splits, band_bounds=bb, pulse_times=pt, table=table, **SMALL)
        dev = e.ensemble_sample(init, ROWS, table, box, split_times=splits, band_bounds=bb, pulse_times=pt, **SMALL)
    assert_same(dev, ref)
    assert np.isfinite(dev["last_llh"][:3]).any() and (dev["last_llh"][3] == -np.inf).all() and not dev["accepted"][3].any()
    assert same_bits(dev["last"][3], init[3])


def test_a_walker_the_engine_refuses(two_rates):
    """A negative rate inside a box that allows it: the walker has no value, accepts the first proposal that has one, and a proposal
    into the negative region is evaluated, refused and rejected."""
    box = (np.array([-0.3, 0.01]), np.array([1.0, 1.0]))
    init = start([[0.2, 0.1], [0.1, 0.2]], *box, 6, spread=0.1)
    init[0, 1] = [-0.1, 0.1]
    init[1, 4] = [-0.2, 0.3]
    ref = rule(two_rates, init, ROWS[:2], box, split_times=SPLITS[:2], **SMALL)
    dev = device(two_rates, init, ROWS[:2], box, split_times=SPLITS[:2], **SMALL)
    assert_same(dev, ref)
    zero = device(two_rates, init, ROWS[:2], box, split_times=SPLITS[:2], n_step=0)
    assert zero["last_llh"][0, 1] == -np.inf and zero["last_llh"][1, 4] == -np.inf and np.isfinite(zero["last_llh"]).any(axis=1).all()
    assert same_bits(zero["last"], init) and zero["n_points"] == 0


# ---- 3. the edges of the call ------------------------------------------------------------------------------------------------------------
def raw_call(eng, init, rows, lo, hi, split_times, n_step=4, thin=1, temperature=(1.0,), a=2.0, want_chain=True, n_rep=3):
    """misti_ensemble_sample through the raw descriptor on a live context, every output pre-filled with a mark.  Returns (code,
    message, outputs): what the call wrote is what no longer carries the mark."""
    import ctypes as C
    from misti_amd import _lib
    init = np.ascontiguousarray(init, dtype=np.float64)
    S, W, N = init.shape
    K = max(n_step // max(thin, 1), 0) if 0 <= n_step < 10 ** 6 else 1
    MARK = -777.0
    out = dict(chain=np.full((max(S, 1), max(K, 1), W, N), MARK), chain_llh=np.full((max(S, 1), max(K, 1), W), MARK), accepted=np.full((max(S, 1), W), -777, dtype=np.int32),
               last=np.full((max(S, 1), W, N), MARK), last_llh=np.full((max(S, 1), W), MARK), n_points=np.full(1, -777, dtype=np.int64))
    keep = [np.ascontiguousarray(v, dtype=t) for v, t in ((rows, np.int32), (TABLE, np.float64), (lo, np.float64), (hi, np.float64), (split_times, np.float64),
                                                          (temperature, np.float64))]
    r_of, tab, lo_, hi_, sp, T = keep
    lo_, hi_ = (v.reshape(-1, N) if N else v.reshape(1, 0) for v in (lo_, hi_))
    q = _lib.EnsSample(size=C.sizeof(_lib.EnsSample), split=_lib.SPLIT_PER_START, split_times=sp.ctypes.data, n_start=S, init=init.ctypes.data, rows=r_of.ctypes.data,
                       n_rep=n_rep, jsfs=tab.ctypes.data, n_box=lo_.shape[0], box_lo=lo_.ctypes.data, box_hi=hi_.ctypes.data, walkers=W, n_step=n_step, thin=thin,
                       n_temp=T.size, temperature=T.ctypes.data, a=a, seed=0, chain=out["chain"].ctypes.data if want_chain else None,
                       chain_llh=out["chain_llh"].ctypes.data if want_chain else None, accepted=out["accepted"].ctypes.data, last=out["last"].ctypes.data,
                       last_llh=out["last_llh"].ctypes.data, n_points=out["n_points"].ctypes.data)
    rc = eng._lib.misti_ensemble_sample(eng._ctx, C.byref(q))
    return rc, eng._lib.misti_last_error().decode(), out


def untouched(out):
    return all((v == -777).all() for v in out.values())


def test_no_search_writes_nothing(two_rates):
    rc, why, out = raw_call(two_rates, np.empty((0, 4, 2)), np.empty(0, dtype=np.int32), [0.01, 0.01], [1.0, 1.0], np.empty(0))
    assert rc == 0 and untouched(out)
    r = two_rates.ensemble_sample(np.empty((0, 4, 2)), np.empty(0, dtype=np.int32), TABLE, ([0.01, 0.01], [1.0, 1.0]), split_times=np.empty(0), **SMALL)
    assert r["chain"].shape == (0, 6, 4, 2) and r["last"].shape == (0, 4, 2) and r["n_points"] == 0


# The checks behind the context, in the header's order, on a live context; nothing is written.  INIT is inside LO / HI below.
LO, HI = np.array([[0.01, 0.01], [0.1, 0.1]]), np.array([[1.0, 1.0], [0.5, 0.5]])
INIT = np.array([[[0.2, 0.1], [0.3, 0.2], [0.9, 0.05], [0.02, 1.0]], [[0.2, 0.1], [0.3, 0.2], [0.5, 0.5], [0.1, 0.4]]])


def bad(what, **kw):
    init, lo, hi = INIT.copy(), LO.copy(), HI.copy()
    for k, v in what.items():
        {"init": init, "lo": lo, "hi": hi}[k[0]][k[1:]] = v
    return dict(init=init, lo=lo, hi=hi, **kw)


FINITE = " (the sampler's prior is uniform on a finite box)"
TOO_LONG = "the chain of 2 searches x 1000000000 kept steps x 4 walkers x 2 coordinates exceeds INT32_MAX / 8 elements (raise thin)"


# (arguments, code, the word the case is named by, the whole text)
BEHIND = [
    (bad({}, n_step=10 ** 9, thin=1), -4, "exceeds INT32_MAX / 8 elements", TOO_LONG),
    (bad({("hi", 1, 0): np.inf}), -1, "box 1, coordinate 0: a bound is not finite", "box 1, coordinate 0: a bound is not finite" + FINITE),
    (bad({("lo", 0, 1): np.nan}), -1, "box 0, coordinate 1: a bound is not finite", "box 0, coordinate 1: a bound is not finite" + FINITE),
    (bad({("lo", 1, 1): 0.6}), -1, "box 1, coordinate 1: the lower bound 0.6 is greater than the upper bound 0.5", None),
    (bad({("lo", 1, 0): 0.5, ("lo", 1, 1): 0.5}), -1, "box 1: every coordinate is fixed", None),
    (bad({("init", 1, 2, 1): np.nan}), -1, "init[1][2][1] is not finite", None),
    (bad({("init", 0, 3, 0): np.inf}), -1, "init[0][3][0] is not finite", None),
    (bad({("init", 1, 0, 0): 0.05}), -1, "init[1][0][0] = 0.05 is outside its box [0.1, 0.5]", None),       # inside box 0, outside its own
    (bad({("init", 0, 1, 1): 1.5}), -1, "init[0][1][1] = 1.5 is outside its box [0.01, 1]", None),
    # the order: the chain limit before the box, the box before init, a lower box index and walker first
    (bad({("hi", 1, 0): np.inf, ("init", 0, 0, 0): np.nan}, n_step=10 ** 9), -4, "exceeds INT32_MAX / 8", TOO_LONG),
    (bad({("lo", 1, 1): 0.6, ("init", 0, 0, 0): np.nan}), -1, "lower bound", "box 1, coordinate 1: the lower bound 0.6 is greater than the upper bound 0.5"),
    (bad({("lo", 0, 0): 2.0, ("hi", 1, 0): np.inf}), -1, "box 0, coordinate 0: the lower bound", "box 0, coordinate 0: the lower bound 2 is greater than the upper bound 1"),
    (bad({("init", 0, 3, 1): 7.0, ("init", 1, 0, 0): np.nan}), -1, "init[0][3][1]", "init[0][3][1] = 7 is outside its box [0.01, 1]"),
]


@pytest.mark.parametrize("case, code, word, text", BEHIND, ids=["case%d-%d-%s" % (i, c[1], c[2]) for i, c in enumerate(BEHIND)])
def test_errors_behind_the_context_come_in_the_headers_order_and_write_nothing(two_rates, case, code, word, text):
    kw = dict(case)
    rc, why, out = raw_call(two_rates, kw.pop("init"), ROWS[:2], kw.pop("lo"), kw.pop("hi"), SPLITS[:2], **kw)
    assert (rc, why) == (code, text or word)             # None: the word is the whole text already
    assert untouched(out)


def test_the_limits_of_the_model_and_the_accepted_descriptor(grid, two_rates):
    # without a chain asked for, the same number of steps is no chain too large (n_step = 0 keeps the call short)
    rc, why, out = raw_call(two_rates, INIT, ROWS[:2], LO, HI, SPLITS[:2], n_step=0)
    assert rc == 0 and same_bits(out["last"], INIT) and out["n_points"][0] == 0 and np.isfinite(out["last_llh"]).any() and not out["accepted"].any()
    assert (out["chain"] == -777).all()
    # a model without an optimised parameter has no coordinate at a split per search
    with engine(grid, [(0, 2, -1, 0.2, -1)]) as e:
        rc, why, out = raw_call(e, np.zeros((1, 4, 0)), ROWS[:1], np.zeros((1, 0)), np.zeros((1, 0)), SPLITS[:1])
        assert (rc, why) == (-1, "the model has no optimised parameter") and untouched(out)


def test_no_step_returns_the_initial_ensemble_with_its_values(two_rates):
    box = (np.array([0.01, 0.01]), np.array([1.0, 1.0]))
    init = start([[0.2, 0.1], [0.4, 0.3], [0.1, 0.6]], *box, 4)
    r = device(two_rates, init, ROWS[:3], box, split_times=SPLITS[:3], n_step=0, seed=5)
    assert same_bits(r["last"], init) and r["chain"].shape == (3, 0, 4, 2) and r["n_points"] == 0 and not r["accepted"].any()
    llk = two_rates.evaluate(np.repeat(SPLITS[:3], 4), init.reshape(-1, 2), TABLE).llk[np.arange(12), np.repeat(ROWS[:3], 4)]
    assert same_bits(r["last_llh"], llk.reshape(3, 4))
    # continuing from `last` in a second call, with ids the first did not use
    more = device(two_rates, r["last"], ROWS[:3], box, split_times=SPLITS[:3], n_step=2, seed=5, ids=[10, 11, 12])
    assert same_bits(more["chain"][:, -1], more["last"]) and not same_bits(more["last"], init)


# ---- 4. the command line -----------------------------------------------------------------------------------------------------------------
def test_cli_mcmc_prints_the_summary_of_what_the_api_returns(tmp_path):
    """`--grid-solve --mcmc` on the fixture of tests/test_gpu_de.py's command-line test: behind every fit line one `mcmc:` line per
    coordinate whose numbers are ensemble_summary of what Engine.ensemble_sample returns from ensemble_start around that fit, and
    --mcmc-out holds that chain."""
    from misti_amd import io as mio, synth
    from misti_amd.engine import Engine
    from misti_amd.optimize import ensemble_start, ensemble_summary
    g = load_golden("golden_pulse_sweep")[0]["in"]
    f1, f2, fj, fo = (str(tmp_path / n) for n in ("g1.psmc", "g2.psmc", "bs.sfs", "chain.npz"))
    open(f1, "w").write(synth.psmc_text(16, 1, synth.THETA_1))
    open(f2, "w").write(synth.psmc_text(17, 2, synth.THETA_2))
    open(fj, "w").write(mio.format_jsfs(mio.bootstrap_table(synth.chunk_rows(g["sfs"], 20), 3, random.Random(5))))
    inp = mio.read_psmc(f1, f2)
    cmd = [sys.executable, "-m", "misti_amd.cli", f1, f2, fj, "20", "-mi", "1", "2", "20", "0.1", "1", "--cpfit", "--funits", str(tmp_path / "nounits.txt"),
           "--grid-st", "19", "20", "--all-bs", "--grid-solve", "--box", "0", "0.01", "1", "--mcmc", "4", "6", "--mcmc-burn", "2", "--mcmc-seed", "7",
           "--mcmc-spread", "0.05", "--mcmc-temp", "2.5", "--mcmc-out", fo]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    lines = r.stdout.splitlines()
    fit = re.compile(r"^bs_id = (\S+) \tsplitT = (\S+) \ttime = \S+ \tmigration rates optim = \[(\S+)\] \tllh = (\S+)$")
    pat = re.compile(r"^mcmc: bs_id = (\d+) \tsplitT = (\S+) \tcoordinate (\d+) \tmean = (\S+) \tmedian = (\S+) \t2\.5% = (\S+) \t97\.5% = (\S+) \ttau = (\S+) \taccepted = (\S+)( \t\(short\))?$")
    at = [i for i, l in enumerate(lines) if fit.match(l)]
    assert len(at) == 8, r.stdout[-1500:]
    rows, _, _ = mio.read_jsfs(fj)
    rows = np.array(rows, dtype=float)
    lo, hi = np.array([0.01]), np.array([1.0])
    x = np.array([float(fit.match(lines[i]).group(3)) for i in at]).reshape(4, 2, 1)
    init = np.stack([[ensemble_start(x[b, j], lo, hi, 4, 0.05, 7, j) for j in range(2)] for b in range(4)]).reshape(8, 4, 1)
    with Engine(inp.times, inp.lambdas, [(0, 2, -1, 0.1, 0)], [], n_param=1, cpfit=True, smooth=True, unfolded=False, sample_date=inp.sampleDateDiscr) as e:
        want = e.ensemble_sample(init, np.repeat(np.arange(4), 2), rows, (lo, hi), split_times=np.tile([19.0, 20.0], 4), n_step=6, temperature=2.5, seed=7,
                                 ids=np.tile([0, 1], 4))
    for n, i in enumerate(at):
        m = pat.match(lines[i + 1])
        assert m, lines[i + 1]
        s = ensemble_summary(want["chain"][n], 2, accepted=want["accepted"][n], n_step=6)
        assert int(m.group(1)) == n // 2 and int(m.group(3)) == 0
        assert [m.group(k) for k in range(4, 10)] == [str(v) for v in (s["mean"][0], s["median"][0], s["q025"][0], s["q975"][0], s["tau"][0], s["acceptance"])], (n, m.groups())
        assert bool(m.group(10)) == bool(s["short"][0])
    out = np.load(fo)
    assert same_bits(out["chain"].reshape(want["chain"].shape), want["chain"]) and same_bits(out["chain_llh"].reshape(want["chain_llh"].shape), want["chain_llh"])
    assert "ensemble MCMC with 4 walkers, 6 steps" in r.stdout and "from spread 0.05 around the fit" in r.stdout and "%d proposals evaluated" % want["n_points"] in r.stdout


def test_cli_mcmc_after_de_with_the_same_w_starts_from_des_final_population(tmp_path):
    """`--de 4 3 --mcmc 4 5`: the sampler's W is DE's population, so the initial ensembles are DE's final populations - the `mcmc:` lines
    are ensemble_summary of Engine.ensemble_sample from bootstrap_profile_de(..., return_population=True)["population"]; with another W the
    ensembles are drawn around the fits as without --de."""
    from misti_amd import io as mio, synth
    from misti_amd.engine import Engine
    from misti_amd.optimize import bootstrap_profile_de, ensemble_summary
    g = load_golden("golden_pulse_sweep")[0]["in"]
    f1, f2, fj, fo = (str(tmp_path / n) for n in ("g1.psmc", "g2.psmc", "bs.sfs", "chain.npz"))
    open(f1, "w").write(synth.psmc_text(16, 1, synth.THETA_1))
    open(f2, "w").write(synth.psmc_text(17, 2, synth.THETA_2))
    open(fj, "w").write(mio.format_jsfs(mio.bootstrap_table(synth.chunk_rows(g["sfs"], 20), 1, random.Random(5))))
    inp = mio.read_psmc(f1, f2)
    cmd = [sys.executable, "-m", "misti_amd.cli", f1, f2, fj, "20", "-mi", "1", "2", "20", "0.1", "1", "--cpfit", "--funits", str(tmp_path / "nounits.txt"),
           "--grid-st", "19", "20", "--all-bs", "--grid-solve", "--box", "0", "0.01", "1", "--de", "4", "3", "--de-seed", "7", "--mcmc", "4", "5",
           "--mcmc-burn", "1", "--mcmc-seed", "9", "--mcmc-out", fo]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    rows, _, _ = mio.read_jsfs(fj)
    rows = np.array(rows, dtype=float)
    R = rows.shape[0]
    lo, hi = np.array([0.01]), np.array([1.0])
    with Engine(inp.times, inp.lambdas, [(0, 2, -1, 0.1, 0)], [], n_param=1, cpfit=True, smooth=True, unfolded=False, sample_date=inp.sampleDateDiscr) as e:
        prof = bootstrap_profile_de(e, [19, 20], rows, [0.1], (lo, hi), pop=4, maxiter=3, seed=7, return_population=True)
        assert prof["population"].shape == (R, 2, 4, 1) and prof["population_llh"].shape == (R, 2, 4)
        want = e.ensemble_sample(prof["population"].reshape(R * 2, 4, 1), np.repeat(np.arange(R), 2), rows, (lo, hi), split_times=np.tile([19.0, 20.0], R),
                                 n_step=5, seed=9, ids=np.tile([0, 1], R))
    out = np.load(fo)
    assert same_bits(out["chain"], want["chain"]) and same_bits(out["last"], want["last"]) and same_bits(out["accepted"], want["accepted"])
    got = [l for l in r.stdout.splitlines() if l.startswith("mcmc:")]
    assert len(got) == R * 2
    for n, l in enumerate(got):
        s = ensemble_summary(want["chain"][n], 1, accepted=want["accepted"][n], n_step=5)
        assert "\tmean = %s " % s["mean"][0] in l and "\taccepted = %s" % s["acceptance"] in l, l
    assert "from DE's final population" in r.stdout and "%d proposals evaluated" % want["n_points"] in r.stdout
