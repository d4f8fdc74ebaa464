"""Shortest (HPD) intervals and the sorted marginals on the device - the hpd, hpd_at and order outputs of misti_ens_summary_dev, the
sampling doors and `--mcmc-hpd` - against optimize.ensemble_hpd_rule, bit for bit.

The sort is tested through Engine.ensemble_summary_dev on chains the test uploads itself, at the smallest shapes where a tiled sort and
a window reduction can go wrong.  With T = _lib.POST_SORT_TILE, m = n W samples per marginal takes every value of {1, 2, 63, 64, 65,
255, 257, T - 1, T, T + 1, 2 T + 1, 3 T + 5} (one sample; the bitonic network's power-of-two padding; the 256 threads of the window
reduction; one tile, one short of it, one over it: a merge with a run of one key; three and four runs: a merge pass with a run that has
no partner, and two passes) - with W = 1, since most of them are prime to 2 and 6; W = 2 and W = 6 take the nearest multiples.  N in
{1, 3, 16}, burn 0 and > 0, two searches per case so that every flavour of chain meets every size.  The sampler's side is the two-rate
model of tests/test_gpu_post.py (fixtures rebuilt here): 2 searches, 8 walkers, 40 steps."""
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

OLD = ("mean", "cov", "quant", "tau", "window", "best_llh", "best_x", "best_at")
NEW = ("hpd", "hpd_at", "order")
MASSES = (0.95, 0.5, 1.0, 1e-9)
TABLE = np.array([[3e7, 9000, 2500, 10000, 6000, 4000, 2600, 4100], [2.9e7, 9100, 2400, 10100, 6100, 3900, 2500, 4000]])
ROWS = np.array([0, 1], dtype=np.int32)
SPLITS = np.array([11.0, 12.5])


def tile():
    from misti_amd import _lib
    return _lib.POST_SORT_TILE


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def grid():
    from misti_amd import synth
    inp = synth.psmc_pair(8, 9)
    times, lh, _ = synth.self_consistent(inp, 11, [[1, 2, 11, 0.2, 0]], [])
    return times, lh


@pytest.fixture(scope="module")
def two_rates(grid):
    from misti_amd.engine import Engine
    e = Engine(grid[0], grid[1], bands=[(0, 2, -1, 0.2, 0), (1, 2, -1, 0.1, 1)], pulses=(), n_param=2, cpfit=True, smooth=True)
    yield e
    e.close()


# ---- synthetic chains ----------------------------------------------------------------------------------------------------------------------
FLAVOURS = ("sorted", "reverse", "equal", "dups", "signs", "nonfinite", "random")


def flavour(kind, rng, K, W, N, burn):
    """One search's chain [K][W][N]."""
    shape = (K, W, N)
    if kind in ("sorted", "reverse"):                        # every marginal ascending (descending) in the order the sort reads it
        v = np.sort(rng.standard_normal(shape).reshape(-1, N), axis=0)
        return np.ascontiguousarray(v if kind == "sorted" else v[::-1]).reshape(shape)
    if kind == "equal":
        return np.full(shape, -3.25)
    if kind == "dups":                                       # a set of five: long runs of equal keys across every merge cut
        return rng.choice(np.array([1.5, -2.25, 1e-3, 7.0, -0.5]), size=shape)
    if kind == "signs":                                      # both signs, both zeros
        return rng.choice(np.array([0.0, -0.0, 1.75, -1.75, 2.0 ** -1074, -2.0 ** -1074]), size=shape) * rng.choice(np.array([1.0, 3.0]), size=shape)
    x = rng.standard_normal(shape) * 30.0 - 7.0
    if kind == "nonfinite":                                  # among the kept samples of every coordinate: a NaN and both infinities
        flat = x[burn:].reshape(-1, N)
        for j in range(N):
            at = rng.permutation(flat.shape[0])[:3]
            for i, v in zip(at, (np.nan, np.inf, -np.inf)):
                flat[i, j] = v
        x[burn:] = flat.reshape(x[burn:].shape)
    return x


def synthetic(case, S, K, W, N, burn):
    rng = np.random.default_rng(500 + case)
    return np.stack([flavour(FLAVOURS[(2 * case + s) % len(FLAVOURS)], rng, K, W, N, burn) for s in range(S)])


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def summarise(eng, chain, llh=None, **kw):
    out = eng.ensemble_summary_dev(on_device(chain), None if llh is None else on_device(llh), **kw)
    eng.sync()
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_rule(dev, ref, names=NEW, where=""):
    for k in names:
        if not same_bits(dev[k], ref[k]):
            kind = np.int64 if dev[k].dtype == np.float64 else np.int32
            bad = np.argwhere(np.ascontiguousarray(dev[k]).view(kind) != np.ascontiguousarray(ref[k]).view(kind))
            print(where, k, "differs at", bad[:5].tolist(), "device", dev[k][tuple(bad[0])], "rule", ref[k][tuple(bad[0])])
        assert same_bits(dev[k], ref[k]), (where, k)


def cases():
    """(m, W, N, burn): every m of the issue's list at W = 1, N and burn going round; W = 2 and 6 at the multiples nearest to the edges."""
    T = tile()
    out = []
    for i, m in enumerate((1, 2, 63, 64, 65, 255, 257, T - 1, T, T + 1, 2 * T + 1, 3 * T + 5)):
        out.append((m, 1, (1, 3, 16)[i % 3], (0, 3)[i % 2]))
    out += [(2, 2, 3, 0), (64, 2, 16, 2), (T, 2, 1, 1), (T + 2, 2, 3, 0), (6, 6, 1, 0), (258, 6, 16, 1), (T - 2, 6, 3, 0), (T + 4, 6, 1, 5),
            (3 * T + 6, 6, 3, 0), (2 * T + 2, 2, 16, 0)]
    return out


CASES = cases()


@pytest.mark.parametrize("case", range(len(CASES)), ids=["m%d-W%d-N%d-burn%d" % c for c in CASES])
def test_synthetic_chains_equal_the_rule_bit_for_bit(two_rates, case):
    from misti_amd.optimize import ensemble_hpd_rule
    m, W, N, burn = CASES[case]
    chain = synthetic(case, 2, m // W + burn, W, N, burn)
    ref = ensemble_hpd_rule(chain, burn=burn, masses=MASSES, order=True)
    dev = summarise(two_rates, chain, burn=burn, masses=MASSES, want=NEW)
    assert set(dev) == set(NEW) and dev["order"].shape == (2, N, m)
    assert_rule(dev, ref, where="case %r %r" % (CASES[case], [FLAVOURS[(2 * case + s) % len(FLAVOURS)] for s in range(2)]))


def test_every_flavour_of_chain_across_four_tiles(two_rates):
    """All seven kinds of chain in ONE call at m = 3 T + 5 (two merge passes, the last run five keys long), eight masses."""
    from misti_amd.optimize import ensemble_hpd_rule
    rng = np.random.default_rng(11)
    m, masses = 3 * tile() + 5, (0.95, 0.9, 0.5, 1.0, 1e-9, 0.3333, 0.68, 0.999)
    chain = np.stack([flavour(k, rng, m, 1, 3, 0) for k in FLAVOURS])
    ref = ensemble_hpd_rule(chain, masses=masses, order=True)
    dev = summarise(two_rates, chain, masses=masses, want=NEW)
    assert_rule(dev, ref)
    nf = FLAVOURS.index("nonfinite")
    assert np.isnan(dev["order"][nf, :, -1]).all() and (dev["order"][nf, :, 0] == -np.inf).all() and np.isfinite(dev["hpd"][nf, :, 2]).all()
    assert (dev["hpd_at"][FLAVOURS.index("equal")] == 0).all()


def test_no_search_writes_nothing(two_rates):
    import ctypes as C
    import torch
    from misti_amd import _lib
    bufs = {k: torch.full((64,), -777, dtype=torch.int32 if k == "hpd_at" else torch.float64, device="cuda") for k in NEW}
    pr, ms = np.array([0.5]), np.array([0.95])
    p = _lib.EnsPost(size=C.sizeof(_lib.EnsPost), burn=0, n_prob=1, probs=pr.ctypes.data, max_lag=3, c=5.0, n_mass=1, masses=ms.ctypes.data,
                     **{k: v.data_ptr() for k, v in bufs.items()})
    rc = two_rates._lib.misti_ens_summary_dev(two_rates._ctx, 0, 5, 4, 2, None, None, C.byref(p))
    two_rates.sync()
    assert rc == 0 and all((v.cpu().numpy() == -777).all() for v in bufs.values())
    out = summarise(two_rates, np.empty((0, 5, 4, 2)), masses=(0.95,), want=NEW)
    assert out["hpd"].shape == (0, 2, 1, 2) and out["order"].shape == (0, 2, 20)


def test_a_search_alone_equals_the_search_among_others(two_rates):
    chain = synthetic(3, 3, tile() + 9, 2, 3, 4)
    among = summarise(two_rates, chain, burn=4, masses=MASSES, want=NEW)
    alone = summarise(two_rates, chain[2:], burn=4, masses=MASSES, want=NEW)
    for k in NEW:
        assert same_bits(alone[k][0], among[k][2]), k


def test_the_eight_older_outputs_keep_their_bits(two_rates):
    """... with and without the new ones asked, each new output alone equals itself among the others, and the default keys are the
    eight - plus hpd and hpd_at where masses are given."""
    from misti_amd.optimize import ensemble_hpd_rule, ensemble_posterior_rule
    rng = np.random.default_rng(12)
    chain = synthetic(5, 2, 300, 4, 3, 5)
    llh = np.round(rng.standard_normal((2, 300, 4)) * 3.0, 1)
    kw = dict(burn=5, probs=(0.1, 0.5, 0.9))
    old = summarise(two_rates, chain, llh, **kw)
    both = summarise(two_rates, chain, llh, masses=MASSES, want=OLD + NEW, **kw)
    assert tuple(old) == OLD and tuple(both) == OLD + NEW
    for k in OLD:
        assert same_bits(old[k], both[k]), k
    assert_rule(both, ensemble_posterior_rule(chain, llh, **kw), OLD)
    assert_rule(both, ensemble_hpd_rule(chain, burn=5, masses=MASSES, order=True))
    default = summarise(two_rates, chain, llh, masses=MASSES, **kw)
    assert tuple(default) == OLD + ("hpd", "hpd_at")
    for want in (("hpd",), ("hpd_at",), ("order",), ("quant", "hpd")):
        part = summarise(two_rates, chain, llh, masses=MASSES, want=want, **kw)
        assert tuple(part) == want
        for k in want:
            assert same_bits(part[k], both[k]), (want, k)
    assert same_bits(summarise(two_rates, chain, want=("order",), **kw)["order"], both["order"])           # the sort needs no mass


def test_the_workspace_regrows_between_calls_of_different_size(two_rates, grid):
    """A small call, a large one and the small one again on ONE context equal the same calls on fresh contexts."""
    from misti_amd.engine import Engine
    small, large = synthetic(6, 1, 70, 2, 3, 0), synthetic(7, 3, 2 * tile() + 7, 2, 3, 0)
    seq = [summarise(two_rates, c, masses=MASSES, want=NEW + ("mean", "tau")) for c in (small, large, small)]
    for c, got in zip((small, large), seq):
        with Engine(grid[0], grid[1], bands=[(0, 2, -1, 0.2, 0), (1, 2, -1, 0.1, 1)], pulses=(), n_param=2, cpfit=True, smooth=True) as fresh:
            want = summarise(fresh, c, masses=MASSES, want=NEW + ("mean", "tau"))
        for k in want:
            assert same_bits(got[k], want[k]), k
    for k in seq[0]:
        assert same_bits(seq[0][k], seq[2][k]), k


# ---- the sampling doors ---------------------------------------------------------------------------------------------------------------------
def start(points, lo, hi, W, spread=0.05, seed=1):
    from misti_amd.optimize import ensemble_start
    return np.stack([ensemble_start(np.asarray(p), lo, hi, W, spread, seed, s) for s, p in enumerate(points)])


BOX = (np.array([0.01, 0.01]), np.array([1.0, 1.0]))
RUN = dict(split_times=SPLITS, n_step=40, seed=4)


def test_ensemble_posterior_returns_the_rule_on_its_chain(two_rates):
    from misti_amd.optimize import ensemble_hpd_rule, ensemble_posterior_rule
    init = start([[0.2, 0.1], [0.3, 0.1]], *BOX, 8)
    plain = two_rates.ensemble_posterior(init, ROWS, TABLE, BOX, burn=5, **RUN)
    r = two_rates.ensemble_posterior(init, ROWS, TABLE, BOX, burn=5, masses=(0.95, 0.5), keep_chain=True, want=OLD + NEW, **RUN)
    assert "hpd" not in plain and r["chain"].shape == (2, 40, 8, 2) and r["order"].shape == (2, 2, 35 * 8)
    assert_rule(r, ensemble_hpd_rule(r["chain"], burn=5, masses=(0.95, 0.5), order=True))
    assert_rule(r, ensemble_posterior_rule(r["chain"], r["chain_llh"], burn=5), OLD)
    for k in OLD + ("last", "last_llh", "accepted"):
        assert same_bits(plain[k], r[k]), k
    lean = two_rates.ensemble_posterior(init, ROWS, TABLE, BOX, burn=5, masses=(0.95, 0.5), **RUN)              # the default keys: no order, no chain
    assert "order" not in lean and "chain" not in lean and same_bits(lean["hpd"], r["hpd"]) and same_bits(lean["hpd_at"], r["hpd_at"])


def test_tempered_sample_returns_the_rule_on_its_cold_chain(two_rates):
    from misti_amd.optimize import ensemble_hpd_rule
    init = np.ascontiguousarray(np.repeat(start([[0.2, 0.1], [0.3, 0.1]], *BOX, 8)[:, None], 2, axis=1))
    r = two_rates.tempered_sample(init, ROWS, TABLE, BOX, np.array([1.0, 4.0]), burn=5, post=dict(masses=(0.9,), want=OLD + NEW, keep_chain=True), **RUN)
    assert r["chain"].shape == (2, 40, 8, 2)
    assert_rule(r, ensemble_hpd_rule(r["chain"], burn=5, masses=(0.9,), order=True))


def test_the_prior_door_returns_the_rule_in_sampling_coordinates(two_rates):
    from misti_amd.optimize import ensemble_hpd_rule, posterior_table, prior_spec, to_sampling
    prior = prior_spec(2, log=(0,), exponential={1: 0.2})
    box = tuple(to_sampling(v, prior) for v in BOX)
    init = to_sampling(start([[0.2, 0.1], [0.3, 0.1]], *BOX, 8), prior, box)
    r = two_rates.ensemble_posterior(init, ROWS, TABLE, box, burn=5, masses=(0.95,), keep_chain=True, prior=prior, **RUN)
    assert_rule(r, ensemble_hpd_rule(r["chain"], burn=5, masses=(0.95,)), ("hpd", "hpd_at"))
    t = posterior_table(r, 35, prior=prior)
    assert same_bits(t["hpd"], r["hpd"]) and (t["hpd_natural"][:, 0] == np.exp(r["hpd"][:, 0])).all() and (t["hpd_natural"][:, 1] == r["hpd"][:, 1]).all()


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def test_cli_mcmc_hpd_prints_the_interval_on_every_post_line(tmp_path):
    """`--grid-solve --mcmc 8 12 --mcmc-post --mcmc-hpd 0.9 0.5` on the fixture of tests/test_gpu_post.py's command-line test: every
    `post:` line carries ` hpd 0.9 = [lo, hi]` and ` hpd 0.5 = [lo, hi]` behind its quantiles, and the numbers are what
    Engine.ensemble_posterior returns with masses=(0.9, 0.5) from ensemble_start around that fit."""
    from misti_amd import io as mio, synth
    from misti_amd.engine import Engine
    from misti_amd.optimize import ensemble_start
    g = load_golden("golden_pulse_sweep")[0]["in"]
    f1, f2, fj = (str(tmp_path / n) for n in ("g1.psmc", "g2.psmc", "bs.sfs"))
    open(f1, "w").write(synth.psmc_text(16, 1, synth.THETA_1))
    open(f2, "w").write(synth.psmc_text(17, 2, synth.THETA_2))
    open(fj, "w").write(mio.format_jsfs(mio.bootstrap_table(synth.chunk_rows(g["sfs"], 20), 3, random.Random(5))))
    inp = mio.read_psmc(f1, f2)
    cmd = [sys.executable, "-m", "misti_amd.cli", f1, f2, fj, "20", "-mi", "1", "2", "20", "0.1", "1", "--cpfit", "--funits", str(tmp_path / "nounits.txt"),
           "--grid-st", "19", "20", "--all-bs", "--grid-solve", "--box", "0", "0.01", "1", "--mcmc", "8", "12", "--mcmc-seed", "7",
           "--mcmc-post", "--mcmc-hpd", "0.9", "0.5"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    lines = r.stdout.splitlines()
    fit = re.compile(r"^bs_id = (\S+) \tsplitT = (\S+) \ttime = \S+ \tmigration rates optim = \[(\S+)\] \tllh = (\S+)$")
    pat = re.compile(r"^post: bs_id = (\d+) \tsplitT = (\S+) \tcoordinate 0 .*\tq0\.975 = (\S+) \thpd 0\.9 = \[(\S+), (\S+)\] \thpd 0\.5 = \[(\S+), (\S+)\] \ttau = ")
    at = [i for i, l in enumerate(lines) if fit.match(l)]
    assert len(at) == 8 and sum(l.startswith("post:") for l in lines) == 8, r.stdout[-1500:]
    rows, _, _ = mio.read_jsfs(fj)
    rows = np.array(rows, dtype=float)
    lo, hi = np.array([0.01]), np.array([1.0])
    x = np.array([float(fit.match(lines[i]).group(3)) for i in at]).reshape(4, 2, 1)
    init = np.stack([[ensemble_start(x[b, j], lo, hi, 8, 1e-2, 7, j) for j in range(2)] for b in range(4)]).reshape(8, 8, 1)
    with Engine(inp.times, inp.lambdas, [(0, 2, -1, 0.1, 0)], [], n_param=1, cpfit=True, smooth=True, unfolded=False, sample_date=inp.sampleDateDiscr) as e:
        want = e.ensemble_posterior(init, np.repeat(np.arange(4), 2), rows, (lo, hi), split_times=np.tile([19.0, 20.0], 4), n_step=12, seed=7,
                                    ids=np.tile([0, 1], 4), burn=6, masses=(0.9, 0.5))
    for n, i in enumerate(at):
        m = pat.match(lines[i + 1])
        assert m, lines[i + 1]
        assert [m.group(k) for k in range(4, 8)] == [repr(float(v)) for v in want["hpd"][n, 0].reshape(-1)], (n, m.groups())
