"""Priors and log-scale coordinates on the device - misti_ensemble_sample_prior, misti_tempered_sample_prior, the `prior` keyword of
Engine.ensemble_sample / ensemble_posterior / tempered_sample and `--mcmc-log` / `--mcmc-prior` - against optimize.ensemble_prior_rule
and optimize.tempered_prior_rule driven by Engine.evaluate as their objective, bit for bit: chain, chain_llh, accepted, last, last_llh,
n_points, and for the ladder the swap counters, rung_llh and logz.

The shapes are those of tests/test_gpu_pt.py: its synthetic model on a 16-interval grid and its three-row table, at most 3 fits, at
most 3 rungs, 6 walkers, at most 6 steps: a half-step is at most 27 points.  The rule's side of a case is computed once."""
import ctypes as C
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

ENS = ("chain", "chain_llh", "accepted", "last", "last_llh")
PT = ENS + ("swap_proposed", "swap_accepted", "rung_llh", "logz")
POST = ("mean", "cov", "quant", "tau", "window", "best_llh", "best_x", "best_at")
TABLE = np.array([[3e7, 9000, 2500, 10000, 6000, 4000, 2600, 4100], [2.9e7, 9100, 2400, 10100, 6100, 3900, 2500, 4000],
                  [3.1e7, 8900, 2600, 9900, 5900, 4100, 2700, 4200]])
ROWS = np.array([0, 1, 2], dtype=np.int32)
SPLITS = np.array([11.0, 12.5, 12.0])
LINEAR, LOG, FLAT, NORMAL, EXPONENTIAL = 0, 1, 0, 1, 2


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


@pytest.fixture(scope="module")
def two_rates(grid):
    from misti_amd.engine import Engine
    e = Engine(grid[0], grid[1], bands=[(0, 2, -1, 0.2, 0), (1, 2, -1, 0.1, 1)], pulses=(), n_param=2, cpfit=True, smooth=True)
    yield e
    e.close()


def objective(eng, rows, split_times, seen=None):
    """-Engine.evaluate: point m of a batch (NATURAL coordinates - the rule has mapped it) against its own search's row and split."""
    P = eng.n_param
    rows = np.asarray(rows)

    def fun(X, s):
        if seen is not None:
            seen.append((np.array(X), np.array(s)))
        split = X[:, -1] if split_times is None else np.asarray(split_times)[s]
        v = eng.evaluate(split, X[:, :P], TABLE).llk[np.arange(len(s)), rows[s]]
        return np.where(np.isnan(v) | (v == -np.inf), np.inf, -v)
    return fun


def start(points, lo, hi, W, spread=0.1, seed=1, L=None):
    """init[S][W][N] (or [S][L][W][N]) around every point, inside the search's box (sampling coordinates)."""
    from misti_amd.optimize import ensemble_start
    points = np.atleast_2d(points)
    lo, hi = (np.broadcast_to(np.asarray(v, dtype=float), points.shape) for v in (lo, hi))
    if L is None:
        return np.stack([ensemble_start(p, lo[s], hi[s], W, spread, seed, 50 + s) for s, p in enumerate(points)])
    return np.stack([[ensemble_start(p, lo[s], hi[s], W, spread, seed, 100 * s + l) for l in range(L)] for s, p in enumerate(points)])


def assert_same(dev, ref, fields):
    for k in fields:
        assert same_bits(np.asarray(dev[k], dtype=np.asarray(ref[k]).dtype), ref[k]), k
    assert dev["n_points"] == ref["n_points"]


# ---- 1. three searches at a split per search, a prior per search ---------------------------------------------------------------------------
# search 0: rate 0 LOG + FLAT (log-uniform), rate 1 LINEAR + NORMAL, at a temperature at which likelihood and prior are of one size (the
# llh of its walkers spans thousands).  Search 1: rate 0 LINEAR + EXPONENTIAL, rate 1 a FIXED LOG coordinate, at a temperature that
# flattens the likelihood: there the prior alone decides, so its decisions differ from the prior-less rule's.  Search 2: EXPONENTIAL
# again, at a split and row where most walkers have no value (both one-sided branches of the decision).
LN = lambda v: float(np.log(v))
PRIOR = dict(scale=np.array([[LOG, LINEAR], [LINEAR, LOG], [LINEAR, LINEAR]], dtype=np.int32),
             kind=np.array([[FLAT, NORMAL], [EXPONENTIAL, FLAT], [EXPONENTIAL, FLAT]], dtype=np.int32),
             p0=np.array([[0.0, 0.12], [0.05, 0.0], [0.005, 0.0]]), p1=np.array([[0.0, 0.03], [0.0, 0.0], [0.0, 0.0]]))
LO = np.array([[LN(0.01), 0.01], [0.05, LN(0.15)], [0.01, 0.02]])
HI = np.array([[LN(1.0), 1.0], [0.6, LN(0.15)], [1.0, 0.5]])
TEMP = np.array([1e3, 1e8, 1e10])
MIXED = dict(n_step=5, thin=2, a=2.0, seed=3)


@pytest.fixture(scope="module")
def mixed(two_rates):
    from misti_amd.optimize import ens_natural, ensemble_prior_rule, ensemble_rule
    init = start([[LN(0.2), 0.1], [0.2, LN(0.15)], [0.3, 0.1]], LO, HI, 6)
    seen = []
    ref = ensemble_prior_rule(objective(two_rates, ROWS, SPLITS, seen), init, LO, HI, prior=PRIOR, temperature=TEMP, **MIXED)
    f = objective(two_rates, ROWS, SPLITS)
    plain = ensemble_rule(lambda X, s: f(ens_natural(PRIOR["scale"][s], X), s), init, LO, HI, temperature=TEMP, **MIXED)      # the same draws, no prior
    dev = two_rates.ensemble_sample(init, ROWS, TABLE, (LO, HI), split_times=SPLITS, temperature=TEMP, prior=PRIOR, **MIXED)
    return init, ref, dev, plain, seen


def test_a_mixed_call_equals_the_prior_rule(mixed):
    from misti_amd.optimize import ens_exp
    init, ref, dev, plain, seen = mixed
    print("llh spread per search", [float(np.ptp(v[np.isfinite(v)])) if np.isfinite(v).any() else None for v in ref["chain_llh"]])
    print("rule accepted", ref["accepted"].tolist(), "points", ref["n_points"], "without the prior", plain["accepted"].tolist(), plain["n_points"])
    assert_same(dev, ref, ENS)
    assert dev["chain"].shape == (3, 2, 6, 2) and dev["accepted"].dtype == np.int32
    assert (dev["chain"] >= LO[:, None, None, :]).all() and (dev["chain"] <= HI[:, None, None, :]).all()
    # the prior term is exercised, on the rule's side and so on the device's: both outcomes of the decision, a rejection in advance, and
    # a decision the prior-less rule takes otherwise on the same draws (everything before the first such decision is identical)
    assert 0 < ref["accepted"].sum() < ref["n_points"] < 5 * 3 * 6
    assert not same_bits(ref["accepted"], plain["accepted"])
    # the fixed LOG coordinate: lo exactly in the chain, ens_exp(lo) at the engine
    assert same_bits(dev["chain"][1][:, :, 1], np.full((2, 6), LO[1, 1]))
    at1 = [X[s == 1, 1] for X, s in seen]
    assert all(same_bits(v, np.full(len(v), ens_exp(LO[1, 1]))) for v in at1) and sum(len(v) for v in at1) > 6
    assert (np.concatenate([X[s == 0, 0] for X, s in seen]) <= 1.0).all()


def test_a_search_alone_equals_the_search_among_others_and_one_prior_for_all_equals_it_repeated(two_rates, mixed):
    init, ref, dev, plain, seen = mixed
    n = 0
    for s in range(3):
        alone = two_rates.ensemble_sample(init[s:s + 1], ROWS[s:s + 1], TABLE, (LO[s:s + 1], HI[s:s + 1]), split_times=SPLITS[s:s + 1], temperature=TEMP[s:s + 1],
                                          ids=[s], prior={k: v[s] for k, v in PRIOR.items()}, **MIXED)
        n += alone["n_points"]
        for k in ENS:
            assert same_bits(alone[k][0], dev[k][s]), (s, k)
    assert n == dev["n_points"]
    one = {k: v[0] for k, v in PRIOR.items()}
    box = (np.tile(LO[0], (3, 1)), np.tile(HI[0], (3, 1)))
    x0 = np.stack([init[0]] * 3)
    kw = dict(split_times=SPLITS, temperature=[1.0, 3.0, 9.0], **MIXED)
    a = two_rates.ensemble_sample(x0, ROWS, TABLE, box, prior=one, **kw)
    b = two_rates.ensemble_sample(x0, ROWS, TABLE, box, prior={k: np.tile(v, (3, 1)) for k, v in one.items()}, **kw)
    for k in ENS:
        assert same_bits(a[k], b[k]), k
    assert a["n_points"] == b["n_points"] and not same_bits(a["chain"][0], a["chain"][1])


# ---- 2. a fitted split: the split LINEAR + NORMAL, a rate LOG ---------------------------------------------------------------------------------
def test_a_fitted_split_with_a_normal_prior_and_a_log_rate(two_rates):
    from misti_amd.optimize import ensemble_prior_rule, prior_spec
    prior = prior_spec(3, log=(0,), normal={2: (11.5, 0.5)})
    box = (np.array([LN(0.01), 0.01, 9.0]), np.array([LN(1.0), 1.0, 13.5]))
    init = start([[LN(0.2), 0.1, 11.0], [LN(0.3), 0.1, 12.0]], *box, 6, spread=0.05)
    kw = dict(n_step=6, thin=1, temperature=3.0, seed=1)
    ref = ensemble_prior_rule(objective(two_rates, ROWS[:2], None), init, *box, prior=prior, **kw)
    dev = two_rates.ensemble_sample(init, ROWS[:2], TABLE, box, fit_split=True, prior=prior, **kw)
    assert_same(dev, ref, ENS)
    assert np.isfinite(dev["last_llh"]).any() and dev["accepted"].sum() > 0
    assert (dev["last"][..., 2] != np.floor(dev["last"][..., 2])).any() and (dev["last"][..., 0] <= 0.0).all()


# ---- 3. the ladder -------------------------------------------------------------------------------------------------------------------------------
LADDER = np.array([[1.0, 3.0, 9.0], [0.5, 4.0, 40.0], [2.0, 2.5, 100.0]])
TEMPERED = dict(n_step=5, thin=2, swap_every=1, burn=1, a=2.0, seed=3)


@pytest.fixture(scope="module")
def tempered(two_rates):
    from misti_amd.optimize import tempered_prior_rule
    init = start([[LN(0.2), 0.1], [0.2, LN(0.15)], [0.3, 0.1]], LO, HI, 6, L=3)
    ref = tempered_prior_rule(objective(two_rates, ROWS, SPLITS), init, LO, HI, LADDER, prior=PRIOR, **TEMPERED)
    dev = two_rates.tempered_sample(init, ROWS, TABLE, (LO, HI), LADDER, split_times=SPLITS, prior=PRIOR, **TEMPERED)
    return init, ref, dev


def test_three_rungs_equal_the_tempered_prior_rule(tempered):
    init, ref, dev = tempered
    print("rule swaps", ref["swap_accepted"].tolist(), "of", ref["swap_proposed"].tolist(), "logz", ref["logz"].tolist())
    assert_same(dev, ref, PT)
    assert ref["swap_accepted"].sum() > 0 and (ref["swap_proposed"] - ref["swap_accepted"]).sum() > 0      # swaps accepted and refused
    assert same_bits(dev["chain"][1][:, :, 1], np.full((2, 6), LO[1, 1])) and dev["accepted"].sum() > 0


def test_one_rung_equals_the_ensemble_sampler_with_the_prior(two_rates, tempered):
    init = tempered[0]
    kw = dict(n_step=5, thin=2, a=2.0, seed=3)
    ens = two_rates.ensemble_sample(init[:, 0], ROWS, TABLE, (LO, HI), split_times=SPLITS, temperature=LADDER[:, 0], prior=PRIOR, **kw)
    pt = two_rates.tempered_sample(init[:, :1], ROWS, TABLE, (LO, HI), LADDER[:, :1], split_times=SPLITS, swap_every=1, burn=1, prior=PRIOR, **kw)
    for k in ENS:
        assert same_bits(pt[k].reshape(ens[k].shape), ens[k]), k
    assert pt["n_points"] == ens["n_points"] and same_bits(pt["logz"], np.zeros(3))


# ---- 4. a prior that says nothing --------------------------------------------------------------------------------------------------------------
def test_no_prior_and_the_all_flat_all_linear_prior_are_the_samplers_without_one(two_rates, tempered):
    from misti_amd.optimize import prior_spec
    lo, hi = np.array([0.01, 0.01]), np.array([1.0, 1.0])
    init = start([[0.2, 0.1], [0.25, 0.1], [0.3, 0.12]], lo, hi, 6, L=3)
    kw = dict(split_times=SPLITS, n_step=4, seed=5)
    want = two_rates.ensemble_sample(init[:, 0], ROWS, TABLE, (lo, hi), temperature=2.0, **kw)
    for prior in (None, prior_spec(2), {k: np.tile(v, (3, 1)) for k, v in prior_spec(2).items()}):
        got = two_rates.ensemble_sample(init[:, 0], ROWS, TABLE, (lo, hi), temperature=2.0, prior=prior, **kw)
        assert_same(got, want, ENS)
    want = two_rates.tempered_sample(init, ROWS, TABLE, (lo, hi), [1.0, 4.0, 16.0], burn=1, **kw)
    for prior in (None, prior_spec(2)):
        got = two_rates.tempered_sample(init, ROWS, TABLE, (lo, hi), [1.0, 4.0, 16.0], burn=1, prior=prior, **kw)
        assert_same(got, want, PT)


# ---- 6. the summaries -----------------------------------------------------------------------------------------------------------------------------
def test_with_post_the_summaries_are_the_rules_on_the_chain_in_sampling_coordinates(two_rates, mixed, tempered):
    from misti_amd.optimize import ensemble_posterior_rule
    init, ref, dev, _, _ = mixed
    kw = dict(split_times=SPLITS, temperature=TEMP, prior=PRIOR, n_step=6, thin=1, a=2.0, seed=3)
    post = dict(burn=2, probs=(0.1, 0.5, 0.9))
    kept = two_rates.ensemble_posterior(init, ROWS, TABLE, (LO, HI), keep_chain=True, **post, **kw)
    plain = two_rates.ensemble_sample(init, ROWS, TABLE, (LO, HI), **kw)
    assert_same(kept, plain, ENS)
    want = ensemble_posterior_rule(kept["chain"], kept["chain_llh"], **post)
    for k in POST:
        assert same_bits(kept[k], want[k]), k
    gone = two_rates.ensemble_posterior(init, ROWS, TABLE, (LO, HI), **post, **kw)
    assert "chain" not in gone and all(same_bits(gone[k], kept[k]) for k in POST + ("last", "last_llh", "accepted"))
    assert (kept["quant"][0, 0] <= 0.0).all() and (kept["quant"][0, 0] >= LO[0, 0]).all()                       # a log coordinate: its logarithm is summarised
    # the ladder's cold chain
    tinit = tempered[0]
    pt = two_rates.tempered_sample(tinit, ROWS, TABLE, (LO, HI), LADDER, split_times=SPLITS, prior=PRIOR, post=dict(post, keep_chain=True), **dict(TEMPERED, n_step=6, thin=1, burn=2))
    want = ensemble_posterior_rule(pt["chain"], pt["chain_llh"][:, 0], **post)
    for k in POST:
        assert same_bits(pt[k], want[k]), k


# ---- 7. the edges of the call ------------------------------------------------------------------------------------------------------------------
def raw_call(eng, entry, init, prior, n_prior, lo=LO, hi=HI):
    """The raw descriptors on a live context, every output pre-filled with a mark."""
    from misti_amd import _lib
    init = np.ascontiguousarray(init, dtype=np.float64)
    S, W, N = init.shape[0], init.shape[-2], init.shape[-1]
    f64 = lambda *shape: np.full(shape, -777.0)
    out = dict(chain=f64(S, 4, W, N), chain_llh=f64(S, 4, W), accepted=np.full((S, W), -777, dtype=np.int32), last=f64(S, W, N), last_llh=f64(S, W),
               n_points=np.full(1, -777, dtype=np.int64))
    tab, lo_, hi_, T = (np.ascontiguousarray(v, dtype=np.float64) for v in (TABLE, lo, hi, [1.0]))
    common = dict(split=_lib.SPLIT_PER_START, split_times=SPLITS.ctypes.data, n_start=S, init=init.ctypes.data, rows=ROWS.ctypes.data, n_rep=3, jsfs=tab.ctypes.data,
                  n_box=lo_.shape[0], box_lo=lo_.ctypes.data, box_hi=hi_.ctypes.data, walkers=W, n_step=4, thin=1, a=2.0, seed=0)
    pa = {k: np.ascontiguousarray(prior[k], dtype=np.int32 if k in ("scale", "kind") else np.float64) for k in ("scale", "kind", "p0", "p1")}
    p = _lib.Prior(size=C.sizeof(_lib.Prior), n_prior=n_prior, **{k: v.ctypes.data for k, v in pa.items()})
    if entry == "ensemble":
        q = _lib.EnsSample(size=C.sizeof(_lib.EnsSample), n_temp=1, temperature=T.ctypes.data, **common, **{k: v.ctypes.data for k, v in out.items()})
        rc = eng._lib.misti_ensemble_sample_prior(eng._ctx, C.byref(q), None, C.byref(p))
    else:
        out.update(rung_llh=f64(S, 1), logz=f64(S))
        q = _lib.PtSample(size=C.sizeof(_lib.PtSample), n_rung=1, n_ladder=1, ladder=T.ctypes.data, swap_every=1, burn=0, **common, **{k: v.ctypes.data for k, v in out.items()})
        rc = eng._lib.misti_tempered_sample_prior(eng._ctx, C.byref(q), None, C.byref(p))
    return rc, eng._lib.misti_last_error().decode(), all((v == -777).all() for v in out.values())


@pytest.mark.parametrize("entry", ["ensemble", "tempered"])
def test_refusals_behind_the_context_write_nothing(two_rates, mixed, entry):
    init = mixed[0]
    SCALE_2 = "prior of search 1, coordinate 0: the scale 2 is neither MISTI_COORD_LINEAR nor MISTI_COORD_LOG"
    bad = lambda **kw: {k: np.array(kw.get(k, PRIOR[k]), dtype=PRIOR[k].dtype) for k in PRIOR}

    def at(k, s, c, v):
        a = PRIOR[k].copy()
        a[s, c] = v
        return {k: a}
    cases = [(bad(**at("scale", 1, 0, 2)), 3, HI, SCALE_2),
             (bad(**at("kind", 2, 1, 7)), 3, HI, "prior of search 2, coordinate 1: the kind 7 is none of MISTI_PRIOR_FLAT / NORMAL / EXPONENTIAL"),
             (bad(**at("p1", 0, 1, 0.0)), 3, HI, "prior of search 0, coordinate 1: the normal's sd 0 is not finite and positive"),
             (bad(**at("p0", 2, 0, np.inf)), 3, HI, "prior of search 2, coordinate 0: the exponential's scale inf is not finite and positive"),
             (bad(**at("p0", 0, 1, np.nan)), 3, HI, "prior of search 0, coordinate 1: the normal's mean is not finite"),
             ({k: v[0] for k, v in PRIOR.items()}, 1, np.array([[710.0, 1.0], HI[1], HI[2]]), 
              "prior of search 0, coordinate 0: the log-scale box [-4.60517, 710] leaves [-745, 709] - its natural value would leave the doubles"),
             # the box's refusals come first, the walkers' last
             (bad(**at("scale", 1, 0, 2)), 3, np.array([[np.inf, 1.0], HI[1], HI[2]]), 
              "box 0, coordinate 0: a bound is not finite (the sampler's prior is uniform on a finite box)")]
    for prior, n_prior, hi, text in cases:
        rc, why, untouched = raw_call(two_rates, entry, init, prior, n_prior, hi=hi)
        assert (rc, why) == (-1, text) and untouched
    worse = init.copy()
    worse[2, 3, 0] = 0.001
    rc, why, untouched = raw_call(two_rates, entry, worse, bad(**at("scale", 1, 0, 2)), 3)
    assert (rc, why) == (-1, SCALE_2) and untouched
    rc, why, untouched = raw_call(two_rates, entry, worse, PRIOR, 3)
    assert (rc, why) == (-1, "init[2]%s[3][0] = 0.001 is outside its box [0.01, 1]" % ("" if entry == "ensemble" else "[0]")) and untouched
    rc, why, untouched = raw_call(two_rates, entry, init, PRIOR, 3)
    assert rc == 0 and not untouched, why


def test_no_step_returns_the_initial_ensemble_with_the_values_of_its_natural_points(two_rates, mixed):
    from misti_amd.optimize import ens_natural
    init = mixed[0]
    r = two_rates.ensemble_sample(init, ROWS, TABLE, (LO, HI), split_times=SPLITS, temperature=TEMP, prior=PRIOR, n_step=0)
    assert same_bits(r["last"], init) and r["chain"].shape == (3, 0, 6, 2) and r["n_points"] == 0 and not r["accepted"].any()
    nat = ens_natural(PRIOR["scale"][:, None, :], init)
    assert not same_bits(nat, init)
    llk = two_rates.evaluate(np.repeat(SPLITS, 6), nat.reshape(-1, 2), TABLE).llk[np.arange(18), np.repeat(ROWS, 6)]
    assert same_bits(r["last_llh"], llk.reshape(3, 6)) and np.isfinite(llk).any()
    t = two_rates.tempered_sample(init[:, None], ROWS, TABLE, (LO, HI), TEMP[:, None], split_times=SPLITS, prior=PRIOR, n_step=0)
    assert same_bits(t["last"][:, 0], init) and same_bits(t["last_llh"][:, 0], llk.reshape(3, 6))


# ---- 8. the command line -----------------------------------------------------------------------------------------------------------------
def test_cli_prints_what_the_api_returns(tmp_path):
    """`--fit-st --mcmc 6 4 --mcmc-log 0 --mcmc-prior st normal 19.5 0.5` on the fixture of tests/test_gpu_pt.py's command-line test: behind
    every fit line the `mcmc:` lines of what Engine.ensemble_sample returns, with the prior, from ensemble_start around to_sampling(fit) in
    the box of logarithms - the quantiles of the log-scale rate in natural units, its mean that of the logarithm; --mcmc-out holds it."""
    from misti_amd import io as mio, synth
    from misti_amd.engine import Engine
    from misti_amd.optimize import ensemble_start, ensemble_summary, from_sampling, prior_spec, to_sampling
    g = load_golden("golden_pulse_sweep")[0]["in"]
    f1, f2, fj, fo = (str(tmp_path / n) for n in ("g1.psmc", "g2.psmc", "bs.sfs", "chain.npz"))
    open(f1, "w").write(synth.psmc_text(16, 1, synth.THETA_1))
    open(f2, "w").write(synth.psmc_text(17, 2, synth.THETA_2))
    open(fj, "w").write(mio.format_jsfs(mio.bootstrap_table(synth.chunk_rows(g["sfs"], 20), 2, random.Random(5))))
    inp = mio.read_psmc(f1, f2)
    cmd = [sys.executable, "-m", "misti_amd.cli", f1, f2, fj, "20", "-mi", "1", "2", "20", "0.1", "1", "--cpfit", "--funits", str(tmp_path / "nounits.txt"),
           "--grid-st", "19", "20", "--all-bs", "--fit-st", "--box", "0", "0.01", "1", "--box", "st", "18", "21", "--mcmc", "6", "4", "--mcmc-burn", "1",
           "--mcmc-seed", "7", "--mcmc-spread", "0.05", "--mcmc-temp", "2.5", "--mcmc-log", "0", "--mcmc-prior", "st", "normal", "19.5", "0.5", "--mcmc-out", fo]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    lines = r.stdout.splitlines()
    fit = re.compile(r"^bs_id = (\S+) \tsplitT = (\S+) \ttime = \S+ \tmigration rates optim = \[(\S+)\] \tllh = (\S+)$")
    pat = re.compile(r"^mcmc: bs_id = (\d+) \tsplitT = (\S+) \tcoordinate (\d+) \tmean = (\S+) \tmedian = (\S+) \t2\.5% = (\S+) \t97\.5% = (\S+) \ttau = (\S+) \taccepted = (\S+)( \t\(short\))?( \t\(log scale: .*\))?$")
    at = [i for i, l in enumerate(lines) if fit.match(l)]
    assert len(at) == 3, r.stdout[-1500:]
    rows, _, _ = mio.read_jsfs(fj)
    rows = np.array(rows, dtype=float)
    prior = prior_spec(2, log=(0,), normal={1: (19.5, 0.5)})
    box = tuple(to_sampling(np.array(v), prior) for v in ([0.01, 18.0], [1.0, 21.0]))
    x = np.array([[float(fit.match(lines[i]).group(3)), float(fit.match(lines[i]).group(2))] for i in at])
    init = np.stack([ensemble_start(to_sampling(np.clip(x[b], [0.01, 18.0], [1.0, 21.0]), prior, box), *box, 6, 0.05, 7, 0) for b in range(3)])
    with Engine(inp.times, inp.lambdas, [(0, 2, -1, 0.1, 0)], [], n_param=1, cpfit=True, smooth=True, unfolded=False, sample_date=inp.sampleDateDiscr) as e:
        want = e.ensemble_sample(init, np.arange(3), rows, box, fit_split=True, n_step=4, temperature=2.5, seed=7, ids=np.zeros(3, dtype=np.uint64), prior=prior)
    for n, i in enumerate(at):
        s = ensemble_summary(want["chain"][n], 1, accepted=want["accepted"][n], n_step=4)
        for c in range(2):
            m = pat.match(lines[i + 1 + c])
            assert m, lines[i + 1 + c]
            q = [from_sampling(s[k], prior)[c] for k in ("median", "q025", "q975")]
            assert int(m.group(3)) == c and [m.group(k) for k in range(4, 10)] == [str(v) for v in (s["mean"][c], *q, s["tau"][c], s["acceptance"])], (n, c, m.groups())
            assert bool(m.group(11)) == (c == 0)                                      # the line says which coordinate was sampled on the log scale
        assert s["mean"][0] < 0.0 < float(pat.match(lines[i + 1]).group(5)) <= 1.0          # the mean of a logarithm, the median of a rate
    out = np.load(fo)
    for k in ENS:
        assert same_bits(out[k], want[k]), k
    assert same_bits(out["prior_scale"], prior["scale"]) and same_bits(out["prior_p0"], prior["p0"])
    assert "coordinate 0 on the log scale, flat; coordinate 1 linear, normal(19.5, 0.5)" in r.stdout and "%d proposals evaluated" % want["n_points"] in r.stdout
