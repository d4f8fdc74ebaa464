"""Tempered ensemble MCMC on the device - misti_tempered_sample, Engine.tempered_sample and `--mcmc-ladder` - against
optimize.tempered_rule driven by Engine.evaluate as its objective, bit for bit: the cold chain, the values of every rung, the
acceptance and swap counters, the final rungs, the per-rung means, logz and the number of points handed to the engine.

The shapes are those of tests/test_gpu_ens.py: its synthetic model on a 16-interval grid and its three-row table, at most 3 fits, at
most 3 rungs, 4 - 6 walkers, at most 6 steps: a half-step is at most 27 points.  The rule's side of a case is computed once."""
import ctypes as C
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

FIELDS = ("chain", "chain_llh", "accepted", "swap_proposed", "swap_accepted", "last", "last_llh", "rung_llh", "logz")
TABLE = np.array([[3e7, 9000, 2500, 10000, 6000, 4000, 2600, 4100], [2.9e7, 9100, 2400, 10100, 6100, 3900, 2500, 4000],
                  [3.1e7, 8900, 2600, 9900, 5900, 4100, 2700, 4200]])
ROWS = np.array([0, 1, 2], dtype=np.int32)
SPLITS = np.array([11.0, 12.5, 12.0])


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


def engine(grid, bands, n_param=0):
    from misti_amd.engine import Engine
    return Engine(grid[0], grid[1], bands=bands, pulses=(), n_param=n_param, cpfit=True, smooth=True)


@pytest.fixture(scope="module")
def two_rates(grid):
    e = engine(grid, [(0, 2, -1, 0.2, 0), (1, 2, -1, 0.1, 1)], n_param=2)
    yield e
    e.close()


def objective(eng, rows, split_times, table=TABLE):
    """-Engine.evaluate: point m of a batch against its own fit's row and split; no value scores +inf."""
    P = eng.n_param
    rows = np.asarray(rows)

    def fun(X, s):
        split = X[:, -1] if split_times is None else np.asarray(split_times)[s]
        v = eng.evaluate(split, X[:, :P] if P else None, table).llk[np.arange(len(s)), rows[s]]
        return np.where(np.isnan(v) | (v == -np.inf), np.inf, -v)
    return fun


def rule(eng, init, rows, box, ladder, split_times=None, **kw):
    from misti_amd.optimize import tempered_rule
    return tempered_rule(objective(eng, rows, split_times), init, box[0], box[1], ladder, **kw)


def device(eng, init, rows, box, ladder, split_times=None, **kw):
    return eng.tempered_sample(init, rows, TABLE, box, ladder, split_times=split_times, fit_split=split_times is None, **kw)


def start(points, lo, hi, L, W, spread=0.2, seed=1):
    """init[S][L][W][N]: per rung an ensemble of its own around every point, inside the fit's box."""
    from misti_amd.optimize import ensemble_start
    points = np.atleast_2d(points)
    lo, hi = (np.broadcast_to(np.asarray(v, dtype=float), points.shape) for v in (lo, hi))
    return np.stack([[ensemble_start(p, lo[s], hi[s], W, spread, seed, 100 * s + l) for l in range(L)] for s, p in enumerate(points)])


def assert_same(dev, ref, fits=None):
    print("rule   swaps", ref["swap_accepted"].tolist(), "of", ref["swap_proposed"].tolist(), "rung llh", ref["rung_llh"].tolist(), "logz", ref["logz"].tolist())
    print("device swaps", dev["swap_accepted"].tolist(), "of", dev["swap_proposed"].tolist(), "rung llh", dev["rung_llh"].tolist(), "logz", dev["logz"].tolist())
    for k in FIELDS:
        a, b = (dev[k], ref[k]) if fits is None else (dev[k][fits], ref[k][fits])
        assert same_bits(np.asarray(a, dtype=b.dtype), b), k
    if fits is None:
        assert dev["n_points"] == ref["n_points"]


# ---- 1. three fits at a split per fit: a ladder per fit, a fixed coordinate -------------------------------------------------------------
MIXED = dict(n_step=5, thin=2, swap_every=1, burn=1, a=2.0, seed=3)
LO = np.array([[0.01, 0.01], [0.05, 0.02], [0.01, 0.15]])
HI = np.array([[1.0, 1.0], [0.6, 0.5], [1.0, 0.15]])             # fit 2 holds its second rate fixed
LADDER = np.array([[1.0, 3.0, 9.0], [0.5, 4.0, 40.0], [2.0, 2.5, 100.0]])


@pytest.fixture(scope="module")
def mixed(two_rates):
    init = start([[0.2, 0.1], [0.2, 0.1], [0.3, 0.15]], LO, HI, 3, 6, spread=0.1)
    ref = rule(two_rates, init, ROWS, (LO, HI), LADDER, split_times=SPLITS, **MIXED)
    dev = device(two_rates, init, ROWS, (LO, HI), LADDER, split_times=SPLITS, **MIXED)
    return init, ref, dev


def test_a_mixed_call_equals_the_rule(mixed):
    init, ref, dev = mixed
    assert_same(dev, ref)
    assert dev["chain"].shape == (3, 2, 6, 2) and dev["chain_llh"].shape == (3, 3, 2, 6) and dev["accepted"].shape == (3, 3, 6)
    assert dev["swap_proposed"].dtype == np.int32 and dev["swap_proposed"].shape == (3, 2)
    # both branches of the swap ran, on the rule's side and so on the device's
    assert ref["swap_accepted"].sum() > 0 and (ref["swap_proposed"] - ref["swap_accepted"]).sum() > 0
    # (a rung with a walker the engine has no value for has the mean -inf, and so has the fit's logz: IEEE arithmetic, as the rule says)
    assert (dev["chain"][2][:, :, 1] == 0.15).all() and dev["accepted"].sum() > 0 and np.isfinite(dev["logz"]).any()


def test_kept_steps_and_the_reduction(two_rates, mixed):
    from misti_amd.optimize import tempered_reduction
    init, ref, dev = mixed
    rung, logz = tempered_reduction(dev["chain_llh"], LADDER, burn=1)
    assert same_bits(dev["rung_llh"], rung) and same_bits(dev["logz"], logz)
    # step 4 is kept (thin 2) and has a swap round (round 4: the pair (1, 2)); step 5 moves on.  Stopping at 4: the last kept row is
    # the state after the swap, for the coordinates of the cold rung and the values of every rung
    four = device(two_rates, init, ROWS, (LO, HI), LADDER, split_times=SPLITS, **dict(MIXED, n_step=4))
    assert same_bits(four["chain"], dev["chain"]) and same_bits(four["chain_llh"], dev["chain_llh"])
    assert same_bits(four["chain"][:, -1], four["last"][:, 0]) and same_bits(four["chain_llh"][:, :, -1], four["last_llh"])
    two = device(two_rates, init, ROWS, (LO, HI), LADDER, split_times=SPLITS, **dict(MIXED, n_step=2, burn=0))      # round 2: the pair (1, 2) too
    assert same_bits(two["chain"][:, -1], two["last"][:, 0]) and same_bits(two["chain_llh"][:, :, -1], two["last_llh"])
    one = device(two_rates, init, ROWS, (LO, HI), LADDER, split_times=SPLITS, **dict(MIXED, n_step=1, thin=1, burn=0))   # round 1: the pair (0, 1)
    assert same_bits(one["chain"][:, -1], one["last"][:, 0]) and same_bits(one["chain_llh"][:, :, -1], one["last_llh"])
    assert one["swap_proposed"][:, 1].sum() == 0 and one["swap_proposed"][:, 0].sum() > 0


def test_one_rung_equals_ensemble_sample(two_rates, mixed):
    init = mixed[0]
    T = LADDER[:, 0]
    kw = dict(n_step=5, thin=2, a=2.0, seed=3)
    ens = two_rates.ensemble_sample(init[:, 0], ROWS, TABLE, (LO, HI), split_times=SPLITS, temperature=T, **kw)
    for swap_every in (0, 1):
        pt = device(two_rates, init[:, :1], ROWS, (LO, HI), T[:, None], split_times=SPLITS, swap_every=swap_every, burn=1, **kw)
        for k in ("chain", "chain_llh", "accepted", "last", "last_llh"):
            assert same_bits(pt[k].reshape(ens[k].shape), ens[k]), k
        assert pt["n_points"] == ens["n_points"] and same_bits(pt["logz"], np.zeros(3)) and pt["swap_proposed"].shape == (3, 0)


def test_a_fit_alone_equals_the_fit_among_others(two_rates, mixed):
    init, ref, dev = mixed
    n = 0
    for s in range(3):
        alone = device(two_rates, init[s:s + 1], ROWS[s:s + 1], (LO[s:s + 1], HI[s:s + 1]), LADDER[s], split_times=SPLITS[s:s + 1], ids=[s], **MIXED)
        n += alone["n_points"]
        for k in FIELDS:
            assert same_bits(alone[k][0], dev[k][s]), (s, k)
    assert n == dev["n_points"]
    perm = np.array([2, 0, 1])
    shuffled = device(two_rates, init[perm], ROWS[perm], (LO[perm], HI[perm]), LADDER[perm], split_times=SPLITS[perm], ids=perm, **MIXED)
    for k in FIELDS:
        assert same_bits(shuffled[k], dev[k][perm]), k


# ---- 2. the other models ---------------------------------------------------------------------------------------------------------------
def test_two_rates_and_a_fitted_split(two_rates):
    box = (np.array([0.01, 0.01, 9.0]), np.array([1.0, 1.0, 13.5]))
    init = start([[0.2, 0.1, 11.0], [0.3, 0.1, 12.0]], *box, 2, 6, spread=0.05)
    kw = dict(n_step=6, thin=1, swap_every=1, burn=2, seed=1)
    ref = rule(two_rates, init, ROWS[:2], box, [3.0, 30.0], **kw)
    dev = device(two_rates, init, ROWS[:2], box, [3.0, 30.0], **kw)
    assert_same(dev, ref)
    assert np.isfinite(dev["last_llh"]).any() and dev["accepted"].sum() > 0 and dev["swap_proposed"].sum() > 0
    assert (dev["last"][..., 2] != np.floor(dev["last"][..., 2])).any()                                          # fractional splits went through


def test_a_model_without_parameters_samples_the_split_alone(grid):
    with engine(grid, [(0, 2, -1, 0.2, -1)]) as e:
        assert e.n_param == 0
        box = (np.array([8.0]), np.array([14.0]))
        init = start([[11.0], [12.0], [10.5]], *box, 2, 4, spread=0.1)
        kw = dict(n_step=6, thin=1, swap_every=2, burn=0, seed=1)
        ref = rule(e, init, ROWS, box, [1.0, 20.0], **kw)
        dev = device(e, init, ROWS, box, [1.0, 20.0], **kw)
    assert_same(dev, ref)
    assert np.isfinite(dev["last_llh"]).all() and (dev["swap_proposed"] == 4 * 2).all()      # rounds 1 and 3 (t = 2, 6): every walker has a value


# ---- 3. the summaries ---------------------------------------------------------------------------------------------------------------------
def test_with_post_the_summaries_are_the_rules_on_the_cold_chain(two_rates, mixed):
    from misti_amd.optimize import ensemble_posterior_rule
    init, ref, dev = mixed
    kw = dict(MIXED, n_step=6, thin=1, burn=2)
    post = dict(probs=(0.1, 0.5, 0.9), max_lag=None, c=5.0)
    kept = device(two_rates, init, ROWS, (LO, HI), LADDER, split_times=SPLITS, post=dict(post, keep_chain=True), **kw)
    want = ensemble_posterior_rule(kept["chain"], kept["chain_llh"][:, 0], burn=2, probs=post["probs"])
    for k in ("mean", "cov", "quant", "tau", "window", "best_llh", "best_x", "best_at"):
        assert same_bits(kept[k], want[k]), k
    plain = device(two_rates, init, ROWS, (LO, HI), LADDER, split_times=SPLITS, **kw)
    for k in FIELDS:
        assert same_bits(kept[k], plain[k]), k
    gone = device(two_rates, init, ROWS, (LO, HI), LADDER, split_times=SPLITS, post=post, **kw)                 # chain=NULL: the summaries still come
    assert "chain" not in gone
    for k in ("mean", "cov", "quant", "tau", "window", "best_llh", "best_x", "best_at", "chain_llh", "rung_llh", "logz", "last"):
        assert same_bits(gone[k], kept[k]), k


# ---- 4. the edges of the call ------------------------------------------------------------------------------------------------------------
def raw_call(eng, init, rows, lo, hi, split_times, ladder, n_step=4, thin=1, swap_every=1, burn=0):
    """misti_tempered_sample through the raw descriptor on a live context, every output pre-filled with a mark."""
    from misti_amd import _lib
    init = np.ascontiguousarray(init, dtype=np.float64)
    S, L, W, N = init.shape
    K = max(n_step // max(thin, 1), 0) if 0 <= n_step < 10 ** 6 else 1
    s, k = max(S, 1), max(K, 1)
    f64 = lambda *shape: np.full(shape, -777.0)
    i32 = lambda *shape: np.full(shape, -777, dtype=np.int32)
    out = dict(chain=f64(s, k, W, N), chain_llh=f64(s, L, k, W), accepted=i32(s, L, W), swap_proposed=i32(s, L), swap_accepted=i32(s, L), last=f64(s, L, W, N),
               last_llh=f64(s, L, W), rung_llh=f64(s, L), logz=f64(s), n_points=np.full(1, -777, dtype=np.int64))
    r_of, tab, lo_, hi_, sp, T = [np.ascontiguousarray(v, dtype=t) for v, t in ((rows, np.int32), (TABLE, np.float64), (lo, np.float64), (hi, np.float64),
                                                                                  (split_times, np.float64), (ladder, np.float64))]
    lo_, hi_ = (v.reshape(-1, N) if N else v.reshape(1, 0) for v in (lo_, hi_))
    q = _lib.PtSample(size=C.sizeof(_lib.PtSample), split=_lib.SPLIT_PER_START, split_times=sp.ctypes.data, n_start=S, init=init.ctypes.data, rows=r_of.ctypes.data,
                      n_rep=3, jsfs=tab.ctypes.data, n_box=lo_.shape[0], box_lo=lo_.ctypes.data, box_hi=hi_.ctypes.data, walkers=W, n_rung=L,
                      n_ladder=1 if T.ndim == 1 else T.shape[0], n_step=n_step, ladder=T.ctypes.data, thin=thin, swap_every=swap_every, burn=burn, a=2.0, seed=0,
                      **{k_: v.ctypes.data for k_, v in out.items()})
    rc = eng._lib.misti_tempered_sample(eng._ctx, C.byref(q), None)
    return rc, eng._lib.misti_last_error().decode(), out


def untouched(out):
    return all((v == -777).all() for v in out.values())


def test_refusals_behind_the_context_write_nothing(grid, two_rates, mixed):
    init = mixed[0][:2, :2, :4].copy()
    lo, hi = LO[:2], HI[:2]
    ok = dict(rows=ROWS[:2], lo=lo, hi=hi, split_times=SPLITS[:2], ladder=[1.0, 4.0])
    rc, why, out = raw_call(two_rates, init, n_step=10 ** 9, **ok)
    assert (rc, why) == (-4, "the chain of 2 fits x 2 rungs x 1000000000 kept steps x 4 walkers x 2 coordinates exceeds INT32_MAX / 8 elements (raise thin)")
    assert untouched(out)
    rc, why, out = raw_call(two_rates, init, **dict(ok, hi=np.array([[1.0, np.inf], [0.6, 0.5]])))
    assert (rc, why) == (-1, "box 0, coordinate 1: a bound is not finite (the sampler's prior is uniform on a finite box)") and untouched(out)
    worse = init.copy()
    worse[1, 1, 2, 0] = 0.01
    rc, why, out = raw_call(two_rates, worse, **ok)
    assert (rc, why) == (-1, "init[1][1][2][0] = 0.01 is outside its box [0.05, 0.6]") and untouched(out)
    worse[0, 1, 3, 1] = np.nan
    rc, why, out = raw_call(two_rates, worse, **ok)
    assert (rc, why) == (-1, "init[0][1][3][1] is not finite") and untouched(out)
    with engine(grid, [(0, 2, -1, 0.2, -1)]) as e:
        rc, why, out = raw_call(e, np.zeros((1, 2, 4, 0)), ROWS[:1], np.zeros((1, 0)), np.zeros((1, 0)), SPLITS[:1], [1.0, 2.0])
        assert (rc, why) == (-1, "the model has no optimised parameter") and untouched(out)
    # no fit: accepted, nothing written
    rc, why, out = raw_call(two_rates, np.empty((0, 2, 4, 2)), np.empty(0, dtype=np.int32), lo[:1], hi[:1], np.empty(0), [1.0, 4.0])
    assert rc == 0 and untouched(out)


def test_no_step_returns_the_initial_rungs_with_their_values(two_rates, mixed):
    init = mixed[0]
    r = device(two_rates, init, ROWS, (LO, HI), LADDER, split_times=SPLITS, n_step=0, burn=4)
    assert same_bits(r["last"], init) and r["chain"].shape == (3, 0, 6, 2) and r["chain_llh"].shape == (3, 3, 0, 6) and r["n_points"] == 0
    assert not r["accepted"].any() and not r["swap_proposed"].any() and np.isnan(r["rung_llh"]).all() and np.isnan(r["logz"]).all()
    llk = two_rates.evaluate(np.repeat(SPLITS, 18), init.reshape(-1, 2), TABLE).llk[np.arange(54), np.repeat(ROWS, 18)]
    assert same_bits(r["last_llh"], llk.reshape(3, 3, 6))
    empty = two_rates.tempered_sample(np.empty((0, 2, 4, 2)), np.empty(0, dtype=np.int32), TABLE, (LO[0], HI[0]), [1.0, 2.0], split_times=np.empty(0), n_step=4)
    assert empty["chain"].shape == (0, 4, 4, 2) and empty["logz"].shape == (0,) and empty["n_points"] == 0


# ---- 5. the command line -----------------------------------------------------------------------------------------------------------------
def test_cli_ladder_prints_what_the_api_returns(tmp_path):
    """`--grid-solve --mcmc 4 6 --mcmc-ladder 3 16` on the fixture of tests/test_gpu_ens.py's command-line test: behind every fit line the
    `mcmc:` line of the cold rung (ensemble_summary of the cold chain) and the fit's `ladder:` line, both from what Engine.tempered_sample
    returns on temperature_ladder(T, 16, 3) with every rung started from ensemble_start around that fit; --mcmc-out holds it."""
    from misti_amd import io as mio, synth
    from misti_amd.engine import Engine
    from misti_amd.optimize import ensemble_start, ensemble_summary, temperature_ladder
    g = load_golden("golden_pulse_sweep")[0]["in"]
    f1, f2, fj, fo = (str(tmp_path / n) for n in ("g1.psmc", "g2.psmc", "bs.sfs", "chain.npz"))
    open(f1, "w").write(synth.psmc_text(16, 1, synth.THETA_1))
    open(f2, "w").write(synth.psmc_text(17, 2, synth.THETA_2))
    open(fj, "w").write(mio.format_jsfs(mio.bootstrap_table(synth.chunk_rows(g["sfs"], 20), 3, random.Random(5))))
    inp = mio.read_psmc(f1, f2)
    cmd = [sys.executable, "-m", "misti_amd.cli", f1, f2, fj, "20", "-mi", "1", "2", "20", "0.1", "1", "--cpfit", "--funits", str(tmp_path / "nounits.txt"),
           "--grid-st", "19", "20", "--all-bs", "--grid-solve", "--box", "0", "0.01", "1", "--mcmc", "4", "6", "--mcmc-burn", "2", "--mcmc-seed", "7",
           "--mcmc-spread", "0.05", "--mcmc-temp", "2.5", "--mcmc-ladder", "3", "16", "--mcmc-out", fo]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    lines = r.stdout.splitlines()
    fit = re.compile(r"^bs_id = (\S+) \tsplitT = (\S+) \ttime = \S+ \tmigration rates optim = \[(\S+)\] \tllh = (\S+)$")
    pat = re.compile(r"^mcmc: bs_id = (\d+) \tsplitT = (\S+) \tcoordinate (\d+) \tmean = (\S+) \tmedian = (\S+) \t2\.5% = (\S+) \t97\.5% = (\S+) \ttau = (\S+) \taccepted = (\S+)( \t\(short\))?$")
    lad = re.compile(r"^ladder: bs_id = (\d+) \tsplitT = (\S+) \tT = \[(.*?)\] \tswaps accepted = \[(.*?)\] \trung llh = \[(.*?)\] \tlogz = (\S+)$")
    at = [i for i, l in enumerate(lines) if fit.match(l)]
    assert len(at) == 8, r.stdout[-1500:]
    rows, _, _ = mio.read_jsfs(fj)
    rows = np.array(rows, dtype=float)
    lo, hi = np.array([0.01]), np.array([1.0])
    x = np.array([float(fit.match(lines[i]).group(3)) for i in at]).reshape(4, 2, 1)
    init = np.stack([[ensemble_start(x[b, j], lo, hi, 4, 0.05, 7, j) for j in range(2)] for b in range(4)]).reshape(8, 1, 4, 1)
    ladder = temperature_ladder(2.5, 16.0, 3)
    assert same_bits(ladder, 2.5 * 16.0 ** (np.arange(3) / 2.0))
    with Engine(inp.times, inp.lambdas, [(0, 2, -1, 0.1, 0)], [], n_param=1, cpfit=True, smooth=True, unfolded=False, sample_date=inp.sampleDateDiscr) as e:
        want = e.tempered_sample(np.ascontiguousarray(np.repeat(init, 3, axis=1)), np.repeat(np.arange(4), 2), rows, (lo, hi), ladder, split_times=np.tile([19.0, 20.0], 4),
                                 n_step=6, swap_every=1, burn=2, seed=7, ids=np.tile([0, 1], 4))
    nums = lambda text: [float(v) for v in text.split(", ")]
    for n, i in enumerate(at):
        m = pat.match(lines[i + 1])
        assert m, lines[i + 1]
        s = ensemble_summary(want["chain"][n], 2, accepted=want["accepted"][n, 0], n_step=6)
        assert int(m.group(1)) == n // 2 and int(m.group(3)) == 0
        assert [m.group(k) for k in range(4, 10)] == [str(v) for v in (s["mean"][0], s["median"][0], s["q025"][0], s["q975"][0], s["tau"][0], s["acceptance"])], (n, m.groups())
        m = lad.match(lines[i + 2])
        assert m, lines[i + 2]
        with np.errstate(all="ignore"):
            rate = want["swap_accepted"][n] / want["swap_proposed"][n].astype(float)
        assert same_bits(np.array(nums(m.group(3))), ladder) and same_bits(np.array(nums(m.group(5))), want["rung_llh"][n])
        assert np.array_equal(np.array(nums(m.group(4))), rate, equal_nan=True) and same_bits(np.float64(m.group(6)), want["logz"][n])
    out = np.load(fo)
    for k in ("chain", "chain_llh", "accepted", "swap_proposed", "swap_accepted", "last", "last_llh", "rung_llh", "logz"):
        assert same_bits(out[k], want[k]), k
    assert same_bits(out["ladder"], ladder)
    assert "tempered ensemble MCMC with 3 rungs" in r.stdout and "%d proposals evaluated" % want["n_points"] in r.stdout
