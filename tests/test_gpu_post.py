"""Posterior summaries on the device - misti_ens_summary_dev, misti_ensemble_posterior, Engine.ensemble_summary_dev /
ensemble_posterior and `--mcmc-post` - against optimize.ensemble_posterior_rule, bit for bit on every output.

The kernels are tested through misti_ens_summary_dev on chains the test uploads itself: three searches, W in {4, 6, 256}, N in {1, 3,
16}, n = K - burn in {1, 2, 63, 64, 65, 130} (lsum's lane stride and fold edges), one or eight probabilities, every kind of lag cap,
and chains that tie every radix digit, differ in the lowest byte or the sign only, hold both zeros or a NaN.  The sampler's side is
the two-rate model of tests/test_gpu_ens.py (fixtures rebuilt here): 3 searches, 8 walkers, 12 steps."""
import ctypes as C
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

OUTPUTS = ("mean", "cov", "quant", "tau", "window", "best_llh", "best_x", "best_at")
PROBS8 = (0.0, 0.025, 0.25, 0.5, 0.6180339887, 0.975, 1.0, 0.5)
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


@pytest.fixture(scope="module")
def two_rates(grid):
    """Both populations' migration from interval 2 to the split, the two rates optimised."""
    from misti_amd.engine import Engine
    e = Engine(grid[0], grid[1], bands=[(0, 2, -1, 0.2, 0), (1, 2, -1, 0.1, 1)], pulses=(), n_param=2, cpfit=True, smooth=True)
    yield e
    e.close()


# ---- synthetic chains ----------------------------------------------------------------------------------------------------------------------
FLAVOURS = ("random", "equal", "dups", "lowbyte", "sign", "zeros", "nan")


def flavour(kind, rng, K, W, N, burn):
    """One search's chain [K][W][N]."""
    shape = (K, W, N)
    if kind == "random":
        return rng.standard_normal(shape) * 30.0 - 7.0
    if kind == "equal":
        return np.full(shape, 3.25)
    if kind == "dups":                                       # three values: every digit of the key tied within a value
        return rng.choice(np.array([1.5, -2.25, 1e-3]), size=shape)
    if kind == "lowbyte":                                    # 1.0 with a random lowest byte: seven radix passes tie, the last decides
        return (np.float64(1.0).view(np.uint64) + rng.integers(0, 256, size=shape, dtype=np.uint64)).view(np.float64)
    if kind == "sign":
        return np.where(rng.random(shape) < 0.5, 1.75, -1.75)
    if kind == "zeros":
        return np.where(rng.random(shape) < 0.5, 0.0, -0.0)
    x = rng.standard_normal(shape)
    x[burn + (K - burn) // 2, W // 2, N - 1] = np.nan        # one NaN among the kept samples of the last coordinate
    return x


def synthetic(case, S, K, W, N, burn):
    rng = np.random.default_rng(100 + case)
    chain = np.stack([flavour(FLAVOURS[(3 * case + s) % len(FLAVOURS)], rng, K, W, N, burn) for s in range(S)])
    llh = np.round(rng.standard_normal((S, K, W)) * 3.0, 1)  # one decimal: ties
    llh[rng.random((S, K, W)) < 0.1] = -np.inf
    llh[rng.random((S, K, W)) < 0.05] = np.nan
    llh[rng.random((S, K, W)) < 0.05] = -0.0
    return chain, llh


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def summarise(eng, chain, llh, **kw):
    out = eng.ensemble_summary_dev(on_device(chain), None if llh is None else on_device(llh), **kw)
    eng.sync()
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_rule(dev, ref, names=OUTPUTS, where=""):
    for k in names:
        if not same_bits(dev[k], ref[k]):
            bad = np.argwhere(np.ascontiguousarray(dev[k]).view(np.int64 if dev[k].dtype == np.float64 else np.int32)
                              != np.ascontiguousarray(ref[k]).view(np.int64 if ref[k].dtype == np.float64 else np.int32))
            print(where, k, "differs at", bad[:5].tolist(), "device", dev[k][tuple(bad[0])], "rule", ref[k][tuple(bad[0])])
        assert same_bits(dev[k], ref[k]), (where, k)


# (W, N, K, burn, probs, max_lag as a function of n)
CASES = [
    (4, 3, 130, 0, PROBS8, lambda n: n - 1),
    (6, 1, 68, 3, (0.5,), lambda n: n + 5),
    (256, 16, 64, 0, PROBS8, lambda n: 1),
    (4, 16, 63, 0, (0.3,), lambda n: 0),
    (6, 3, 2, 0, PROBS8, lambda n: n - 1),
    (4, 3, 7, 6, PROBS8, lambda n: n + 5),
    (256, 1, 1, 0, (1.0,), lambda n: 0),
    (6, 16, 130, 0, (0.0,), lambda n: n + 5),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_synthetic_chains_equal_the_rule_bit_for_bit(two_rates, case):
    from misti_amd.optimize import ensemble_posterior_rule
    W, N, K, burn, probs, lag = CASES[case]
    chain, llh = synthetic(case, 3, K, W, N, burn)
    kw = dict(burn=burn, probs=probs, max_lag=lag(K - burn))
    ref = ensemble_posterior_rule(chain, llh, **kw)
    dev = summarise(two_rates, chain, llh, **kw)
    print("case", case, "flavours", [FLAVOURS[(3 * case + s) % len(FLAVOURS)] for s in range(3)], "tau", ref["tau"][:, 0], "window", ref["window"][:, 0])
    assert_rule(dev, ref, where="case %d" % case)


def test_every_flavour_of_chain_at_one_shape(two_rates):
    """All seven kinds of chain (and a search whose chain is all NaN-free ties in chain_llh) in ONE call, n = 65, every lag."""
    from misti_amd.optimize import ensemble_posterior_rule
    rng = np.random.default_rng(7)
    chain = np.stack([flavour(k, rng, 68, 6, 3, 3) for k in FLAVOURS])
    llh = np.full((7, 68, 6), 2.5)
    llh[1] = -np.inf
    llh[2] = np.nan
    ref = ensemble_posterior_rule(chain, llh, burn=3, probs=PROBS8)
    dev = summarise(two_rates, chain, llh, burn=3, probs=PROBS8)
    assert_rule(dev, ref)
    assert dev["best_at"][0].tolist() == [0, 0] and dev["best_at"][1].tolist() == [-1, -1] and np.isnan(dev["best_x"][2]).all()
    assert (dev["window"][1] == 0).all() and (dev["tau"][1] == 1.0).all() and (dev["cov"][1] == 0.0).all()            # the constant chain
    assert np.signbit(dev["quant"][5][:, 0]).all() and not np.signbit(dev["quant"][5][:, 6]).any()                     # -0.0 first, +0.0 last
    assert np.isnan(dev["quant"][6][2, 6]) and np.isfinite(dev["quant"][6][2, 0]) and np.isnan(dev["mean"][6][2])     # the NaN sorts last


# ---- a search's result is a function of its own chain ---------------------------------------------------------------------------------
def test_a_search_alone_equals_the_search_among_others_and_permuted(two_rates):
    chain, llh = synthetic(1, 5, 70, 6, 3, 5)
    kw = dict(burn=5, probs=(0.025, 0.5, 0.975))
    among = summarise(two_rates, chain, llh, **kw)
    for s in (0, 3):
        alone = summarise(two_rates, chain[s:s + 1], llh[s:s + 1], **kw)
        for k in OUTPUTS:
            assert same_bits(alone[k][0], among[k][s]), (s, k)
    perm = np.array([3, 0, 4, 2, 1])
    shuffled = summarise(two_rates, chain[perm], llh[perm], **kw)
    for k in OUTPUTS:
        assert same_bits(shuffled[k], among[k][perm]), k


# ---- NULL outputs, guard values ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain(two_rates):
    chain, llh = synthetic(0, 3, 70, 4, 3, 5)
    kw = dict(burn=5, probs=(0.1, 0.5, 0.9))
    return chain, llh, kw, summarise(two_rates, chain, llh, **kw)


@pytest.mark.parametrize("want", [("mean",), ("cov",), ("quant",), ("tau",), ("window",), ("best_llh",), ("best_x",), ("best_at",), ("tau", "best_at"),
                                  ("cov", "quant", "window"), ("mean", "cov", "quant", "tau", "window", "best_llh", "best_x"), ()])
def test_null_outputs_leave_the_others_bits_unchanged(two_rates, plain, want):
    chain, llh, kw, full = plain
    part = summarise(two_rates, chain, llh, want=want, **kw)
    assert set(part) == set(want)
    for k in want:
        assert same_bits(part[k], full[k]), k


def test_without_chain_llh_there_is_no_best_sample(two_rates, plain):
    chain, llh, kw, full = plain
    dev = summarise(two_rates, chain, None, **kw)
    for k in ("mean", "cov", "quant", "tau", "window"):
        assert same_bits(dev[k], full[k]), k
    assert (dev["best_llh"] == -np.inf).all() and (dev["best_at"] == -1).all()
    assert (dev["best_x"].view(np.uint64) == np.float64(np.nan).view(np.uint64)).all()


GUARD = 64
MARK64, MARK32 = -777.0, -777


def raw_summary(eng, chain, llh, burn, probs, max_lag, c=5.0, size=None, n_prob=None):
    """misti_ens_summary_dev through the raw descriptor on a live context, every output inside a buffer of marks with GUARD marks before
    and after it.  Returns (code, message, buffers, shapes)."""
    import torch
    from misti_amd import _lib
    S, K, W, N = chain.shape
    pr = np.asarray(probs, dtype=np.float64)
    P = pr.size
    shapes = dict(mean=(S, N), cov=(S, N, N), quant=(S, N, P), tau=(S, N), window=(S, N), best_llh=(S,), best_x=(S, N), best_at=(S, 2))
    bufs = {}
    for k, shp in shapes.items():
        i32 = k in ("window", "best_at")
        bufs[k] = torch.full((int(np.prod(shp)) + 2 * GUARD,), MARK32 if i32 else MARK64, dtype=torch.int32 if i32 else torch.float64, device="cuda")
    d_chain, d_llh = on_device(chain), on_device(llh)
    p = _lib.EnsPost(size=C.sizeof(_lib.EnsPost) if size is None else size, burn=burn, n_prob=P if n_prob is None else n_prob, probs=pr.ctypes.data,
                     max_lag=max_lag, c=c, **{k: v.data_ptr() + GUARD * v.element_size() for k, v in bufs.items()})
    rc = eng._lib.misti_ens_summary_dev(eng._ctx, S, K, W, N, C.c_void_p(d_chain.data_ptr()), C.c_void_p(d_llh.data_ptr()), C.byref(p))
    why = eng._lib.misti_last_error().decode()
    eng.sync()
    return rc, why, {k: v.cpu().numpy() for k, v in bufs.items()}, shapes


def test_guard_values_around_every_output_are_untouched(two_rates, plain):
    chain, llh, kw, full = plain
    rc, why, bufs, shapes = raw_summary(two_rates, chain, llh, kw["burn"], kw["probs"], chain.shape[1])
    assert rc == 0, why
    for k, v in bufs.items():
        assert (v[:GUARD] == -777).all() and (v[-GUARD:] == -777).all(), k
        assert same_bits(v[GUARD:-GUARD].reshape(shapes[k]), full[k]), k


@pytest.mark.parametrize("kw, code, word", [
    (dict(burn=70), -1, "burn"),
    (dict(burn=-1), -1, "burn"),
    (dict(size=12), -1, "size"),
    (dict(n_prob=9), -1, "n_prob"),
    (dict(probs=(0.5, 1.0000001)), -1, "probs[1]"),
    (dict(max_lag=-2), -1, "max_lag"),
    (dict(c=-1.0), -1, "c must be"),
])
def test_descriptor_errors_write_nothing_and_leave_the_context_usable(two_rates, plain, kw, code, word):
    chain, llh, good, full = plain
    a = dict(burn=good["burn"], probs=good["probs"], max_lag=5)
    a.update(kw)
    rc, why, bufs, _ = raw_summary(two_rates, chain, llh, **a)
    assert rc == code and word in why, (rc, why)
    assert all((v == -777).all() for v in bufs.values())
    again = summarise(two_rates, chain, llh, **good)
    for k in OUTPUTS:
        assert same_bits(again[k], full[k]), k


def test_no_search_writes_nothing(two_rates):
    rc, why, bufs, _ = raw_summary(two_rates, np.empty((0, 5, 4, 2)), np.empty((0, 5, 4)), 0, (0.5,), 3)
    assert rc == 0 and all((v == -777).all() for v in bufs.values())


# ---- end to end: the sampler, then the summary of its chain --------------------------------------------------------------------------
def start(points, lo, hi, W, spread=0.2, seed=1):
    from misti_amd.optimize import ensemble_start
    points = np.atleast_2d(points)
    lo, hi = (np.broadcast_to(np.asarray(v, dtype=float), points.shape) for v in (lo, hi))
    return np.stack([ensemble_start(p, lo[s], hi[s], W, spread, seed, s) for s, p in enumerate(points)])


RUN = dict(n_step=12, thin=2, seed=4)
POST = dict(burn=1, probs=(0.025, 0.5, 0.975))


@pytest.fixture(scope="module", params=["split per search", "fitted split"])
def sampled(two_rates, request):
    """ensemble_sample, ensemble_posterior with and without the chain, on the same arguments: 3 searches, W = 8, 12 steps, thin 2."""
    if request.param == "fitted split":
        box = (np.array([0.01, 0.01, 9.0]), np.array([1.0, 1.0, 13.5]))
        init = start([[0.2, 0.1, 11.0], [0.3, 0.1, 12.0], [0.1, 0.2, 10.0]], *box, 8, spread=0.05)
        kw = dict(fit_split=True, temperature=3.0, **RUN)
    else:
        box = (np.array([0.01, 0.01]), np.array([1.0, 1.0]))
        init = start([[0.2, 0.1], [0.3, 0.1], [0.1, 0.2]], *box, 8, spread=0.05)
        kw = dict(split_times=SPLITS, **RUN)
    sample = two_rates.ensemble_sample(init, ROWS, TABLE, box, **kw)
    kept = two_rates.ensemble_posterior(init, ROWS, TABLE, box, keep_chain=True, **POST, **kw)
    lean = two_rates.ensemble_posterior(init, ROWS, TABLE, box, **POST, **kw)
    return sample, kept, lean


def test_the_posterior_call_samples_what_ensemble_sample_samples(sampled):
    sample, kept, lean = sampled
    assert sample["chain"].shape[:3] == (3, 6, 8)
    for k in ("chain", "chain_llh", "last", "last_llh", "accepted"):
        assert same_bits(kept[k], sample[k]), k
    assert kept["n_points"] == sample["n_points"] == lean["n_points"] and sample["accepted"].sum() > 0


def test_the_summaries_are_the_rule_on_that_chain_with_or_without_it(sampled):
    from misti_amd.optimize import ensemble_posterior_rule
    sample, kept, lean = sampled
    ref = ensemble_posterior_rule(sample["chain"], sample["chain_llh"], **POST)
    assert_rule(kept, ref, where="keep_chain")
    assert_rule(lean, ref, where="no chain")
    assert "chain" not in lean and "chain_llh" not in lean
    for k in ("last", "last_llh", "accepted"):
        assert same_bits(lean[k], sample[k]), k
    # (a search none of whose walkers ever has a value - the fitted-split case has one - has no best sample: -inf on both sides)
    assert np.isfinite(ref["best_llh"]).any() and (ref["best_llh"] == sample["chain_llh"][:, 1:].max(axis=(1, 2))).all()


def test_a_refused_walker_never_wins_the_best_sample(two_rates):
    """Search 0: a box that allows a negative rate and two walkers inside that region - the engine refuses them (llh -inf) until they
    accept a proposal that has a value.  Search 1: a box wholly inside the negative region - no sample of it ever has a value."""
    from misti_amd.optimize import ensemble_posterior_rule
    lo, hi = np.array([[-0.3, 0.01], [-0.3, 0.01]]), np.array([[1.0, 1.0], [-0.05, 1.0]])
    init = start([[0.2, 0.1], [-0.2, 0.2]], lo, hi, 6, spread=0.1)
    init[0, 1], init[0, 4] = [-0.29, 0.1], [-0.28, 0.3]        # deep inside: a stretch of z >= 1 / 2 rarely brings them out
    r = two_rates.ensemble_posterior(init, ROWS[:2], TABLE, (lo, hi), split_times=SPLITS[:2], n_step=3, seed=1, burn=0, keep_chain=True)
    assert (r["chain_llh"][1] == -np.inf).all() and (r["chain_llh"][0] == -np.inf).any() and np.isfinite(r["chain_llh"][0]).any()
    assert_rule(r, ensemble_posterior_rule(r["chain"], r["chain_llh"], burn=0))
    t, w = r["best_at"][0]
    assert np.isfinite(r["best_llh"][0]) and r["chain_llh"][0, t, w] == r["best_llh"][0] == r["chain_llh"][0][np.isfinite(r["chain_llh"][0])].max()
    assert r["best_llh"][1] == -np.inf and r["best_at"][1].tolist() == [-1, -1] and np.isnan(r["best_x"][1]).all()


def test_errors_of_the_posterior_call_write_nothing(two_rates):
    box = (np.array([0.01, 0.01]), np.array([1.0, 1.0]))
    init = start([[0.2, 0.1]], *box, 4)
    from misti_amd._lib import MistiError
    for kw, word in ((dict(burn=3), "burn"), (dict(probs=(2.0,)), "probs[0]"), (dict(n_step=0), "burn"), (dict(n_step=10 ** 9), "device chain")):
        a = dict(n_step=3, burn=0)
        a.update(kw)
        with pytest.raises(MistiError, match=re.escape(word)):
            two_rates.ensemble_posterior(init, ROWS[:1], TABLE, box, split_times=SPLITS[:1], **a)
    r = two_rates.ensemble_posterior(np.empty((0, 4, 2)), np.empty(0, dtype=np.int32), TABLE, box, split_times=np.empty(0), n_step=3)
    assert r["mean"].shape == (0, 2) and r["n_points"] == 0


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def test_cli_mcmc_post_prints_what_the_api_returns_and_mcmc_alone_is_unchanged(tmp_path):
    """`--grid-solve --mcmc 8 12 --mcmc-post` on the fixture of tests/test_gpu_ens.py's command-line test: behind every fit line one
    `post:` line per coordinate whose numbers are posterior_table of what Engine.ensemble_posterior returns from ensemble_start around
    that fit, and no chain is written; the same command without --mcmc-post prints the `mcmc:` lines of ensemble_summary as before."""
    from misti_amd import io as mio, synth
    from misti_amd.engine import Engine
    from misti_amd.optimize import ensemble_start, ensemble_summary, posterior_table
    g = load_golden("golden_pulse_sweep")[0]["in"]
    f1, f2, fj = (str(tmp_path / n) for n in ("g1.psmc", "g2.psmc", "bs.sfs"))
    open(f1, "w").write(synth.psmc_text(16, 1, synth.THETA_1))
    open(f2, "w").write(synth.psmc_text(17, 2, synth.THETA_2))
    open(fj, "w").write(mio.format_jsfs(mio.bootstrap_table(synth.chunk_rows(g["sfs"], 20), 3, random.Random(5))))
    inp = mio.read_psmc(f1, f2)
    cmd = [sys.executable, "-m", "misti_amd.cli", f1, f2, fj, "20", "-mi", "1", "2", "20", "0.1", "1", "--cpfit", "--funits", str(tmp_path / "nounits.txt"),
           "--grid-st", "19", "20", "--all-bs", "--grid-solve", "--box", "0", "0.01", "1", "--mcmc", "8", "12", "--mcmc-seed", "7"]
    before = sorted(p.name for p in tmp_path.iterdir())
    r = subprocess.run(cmd + ["--mcmc-post"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    assert sorted(p.name for p in tmp_path.iterdir()) == before and "mcmc:" not in r.stdout
    lines = r.stdout.splitlines()
    fit = re.compile(r"^bs_id = (\S+) \tsplitT = (\S+) \ttime = \S+ \tmigration rates optim = \[(\S+)\] \tllh = (\S+)$")
    pat = re.compile(r"^post: bs_id = (\d+) \tsplitT = (\S+) \tcoordinate (\d+) \tmean = (\S+) \tsd = (\S+) \tq0\.025 = (\S+) \tq0\.5 = (\S+) \tq0\.975 = (\S+) "
                     r"\ttau = (\S+) \tn_eff = (\S+)( \t\(short\))? \tcorr = \[(\S+)\] \tbest llh = (\S+) at = \((-?\d+), (-?\d+)\) x = (\S+)$")
    at = [i for i, l in enumerate(lines) if fit.match(l)]
    assert len(at) == 8, r.stdout[-1500:]
    rows, _, _ = mio.read_jsfs(fj)
    rows = np.array(rows, dtype=float)
    lo, hi = np.array([0.01]), np.array([1.0])
    x = np.array([float(fit.match(lines[i]).group(3)) for i in at]).reshape(4, 2, 1)
    init = np.stack([[ensemble_start(x[b, j], lo, hi, 8, 1e-2, 7, j) for j in range(2)] for b in range(4)]).reshape(8, 8, 1)
    args = (init, np.repeat(np.arange(4), 2), rows, (lo, hi))
    kw = dict(split_times=np.tile([19.0, 20.0], 4), n_step=12, seed=7, ids=np.tile([0, 1], 4))
    with Engine(inp.times, inp.lambdas, [(0, 2, -1, 0.1, 0)], [], n_param=1, cpfit=True, smooth=True, unfolded=False, sample_date=inp.sampleDateDiscr) as e:
        want = e.ensemble_posterior(*args, burn=6, **kw)
        chain = e.ensemble_sample(*args, **kw)
    for n, i in enumerate(at):
        m = pat.match(lines[i + 1])
        assert m, lines[i + 1]
        t = posterior_table({k: want[k][n] for k in ("mean", "cov", "quant", "tau", "window", "last")}, 6)
        assert int(m.group(1)) == n // 2 and int(m.group(3)) == 0
        assert [m.group(k) for k in range(4, 11)] == [str(v) for v in (t["mean"][0], t["sd"][0])] + [repr(float(v)) for v in t["quant"][0]] + [
            str(t["tau"][0]), str(t["n_eff"][0])], (n, m.groups())
        assert bool(m.group(11)) == bool(t["short"][0]) and m.group(12) == repr(float(t["corr"][0][0]))
        assert m.group(13) == str(want["best_llh"][n]) and [int(m.group(14)), int(m.group(15))] == want["best_at"][n].tolist()
        assert m.group(16) == str(want["best_x"][n][0])
    assert "ensemble MCMC with 8 walkers, 12 steps, thin 1, burn 6" in r.stdout and "%d proposals evaluated" % want["n_points"] in r.stdout
    # without --mcmc-post: the `mcmc:` lines of before, from the chain on the host
    r0 = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r0.returncode == 0, r0.stderr[-1500:]
    old = re.compile(r"^mcmc: bs_id = (\d+) \tsplitT = (\S+) \tcoordinate (\d+) \tmean = (\S+) \tmedian = (\S+) \t2\.5% = (\S+) \t97\.5% = (\S+) \ttau = (\S+) \taccepted = (\S+)( \t\(short\))?$")
    lines0 = r0.stdout.splitlines()
    at0 = [i for i, l in enumerate(lines0) if fit.match(l)]
    assert [lines0[i] for i in at0] == [lines[i] for i in at] and "post:" not in r0.stdout
    for n, i in enumerate(at0):
        m = old.match(lines0[i + 1])
        assert m, lines0[i + 1]
        s = ensemble_summary(chain["chain"][n], 6, accepted=chain["accepted"][n], n_step=12)
        assert [m.group(k) for k in range(4, 10)] == [str(v) for v in (s["mean"][0], s["median"][0], s["q025"][0], s["q975"][0], s["tau"][0], s["acceptance"])], (n, m.groups())
        assert bool(m.group(10)) == bool(s["short"][0])
