"""Joint regions of coordinate pairs on the device - misti_ens_joint_dev, the two sampling doors that end in it and `--mcmc-joint` -
against optimize.ensemble_joint_rule, bit for bit.

The kernels are tested through Engine.ensemble_joint_dev on chains the test uploads itself, at the smallest shapes where a slabbed
histogram and a block reduction can go wrong.  With T = _lib.JOINT_SLAB, m = n W samples takes every value of {1, 2, 63, 64, 65, 255,
256, 257, T - 1, T, T + 1, 2 T + 1, 3 T + 5} (one sample; a wave; the 256 threads of a workgroup; one slab - plain stores -, one short of
it, one over it - the memset and the global atomics -, three and four slabs) with W = 1, since most of them are prime to 2 and 6; W = 2
and W = 6 take the nearest multiples.  N in {2, 3, 16}, burn 0 and > 0, every bin shape of {(1, 1), (1, 128), (2, 3), (63, 65), (64,
64), (128, 127), (128, 128)}, the pairs (0, 1), (1, 0), (N - 1, 0) - at N = 16 all 120 pairs in one call -, two searches per case so
that every flavour of chain meets every size, and every case once with the ranges taken from the data and once with given ranges that
leave samples outside, one of them lo > hi and one NaN.  The sampler's side is the two-rate model of tests/test_gpu_post.py (fixtures
rebuilt here): 2 searches, 8 walkers, 40 steps."""
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

OUT = ("counts", "range", "inside", "mode", "level", "cells", "held")
MASSES = (0.95, 0.5, 1.0, 1e-9)
BINS = ((1, 1), (1, 128), (2, 3), (63, 65), (64, 64), (128, 127), (128, 128))
WINDOW = (-0.75, 1.0)
TABLE = np.array([[3e7, 9000, 2500, 10000, 6000, 4000, 2600, 4100], [2.9e7, 9100, 2400, 10100, 6100, 3900, 2500, 4000]])
ROWS = np.array([0, 1], dtype=np.int32)
SPLITS = np.array([11.0, 12.5])


def slab():
    from misti_amd import _lib
    return _lib.JOINT_SLAB


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
FLAVOURS = ("normal", "equal", "five", "lattice", "signs", "nonfinite", "edges")


def edge_values():
    """The interior edges of WINDOW for the bin counts of BINS, and one ulp either side of each."""
    lo, hi = WINDOW
    e = np.array([lo + i * (hi - lo) / B for B in (2, 3, 63, 64, 65, 127, 128) for i in range(1, B)])
    return np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), [lo, hi]])


def flavour(kind, rng, K, W, N, burn):
    """One search's chain [K][W][N]."""
    shape = (K, W, N)
    if kind == "equal":
        return np.full(shape, 0.3125)
    if kind == "five":                                       # a few cells with huge counts: the LDS atomics under contention
        return rng.choice(np.array([0.5, -0.25, 1e-3, 0.96875, -0.5]), size=shape)
    if kind == "lattice":                                    # every cell of a 4 x 4 lattice equally often (where m is a multiple of 16)
        i = np.arange(K * W)
        return np.stack([(((i // 4 ** (j % 2)) % 4) + 0.5) / 4.0 - 0.25 * (j % 3 == 2) for j in range(N)], axis=-1).reshape(shape)
    if kind == "signs":                                      # both zeros, subnormals
        return rng.choice(np.array([0.0, -0.0, 0.75, -0.5, 2.0 ** -1074, -2.0 ** -1074, 2.0 ** -1030]), size=shape)
    if kind == "edges":                                      # exactly on interior edges of the given window, and one ulp either side
        return rng.choice(edge_values(), size=shape)
    x = rng.standard_normal(shape) * 0.6 + 0.2
    if kind == "nonfinite":                                  # among the kept samples of every coordinate: a NaN and both infinities
        flat = x[burn:].reshape(-1, N)
        for j in range(N):
            at = rng.permutation(flat.shape[0])[:3]
            for i, v in zip(at, (np.nan, np.inf, -np.inf)):
                flat[i, j] = v
        x[burn:] = flat.reshape(x[burn:].shape)
    return x


def synthetic(case, S, K, W, N, burn):
    rng = np.random.default_rng(900 + case)
    return np.stack([flavour(FLAVOURS[(2 * case + s) % len(FLAVOURS)], rng, K, W, N, burn) for s in range(S)])


def given_ranges(S, P):
    """[S][P][2][2]: WINDOW on every axis - it leaves samples of every random flavour outside -, narrowed a little per pair; in the
    LAST search pair 0 has lo > hi on its first axis and pair 1 a NaN on its second."""
    r = np.empty((S, P, 2, 2))
    r[..., 0], r[..., 1] = WINDOW
    r[:, :, 1, 1] -= 0.125 * (np.arange(P) % 3)[None, :]
    r[S - 1, 0, 0] = (1.0, -0.75)
    r[S - 1, 1 % P, 1] = (-0.75, np.nan)
    return r


def pairs_and_bins(case, N):
    if N == 16:
        pairs = [(a, b) if (a + b) % 2 else (b, a) for a in range(16) for b in range(a)]
        return pairs, [BINS[(case + q) % len(BINS)] for q in range(120)]
    return [(0, 1), (1, 0), (N - 1, 0)], [BINS[(case + q) % len(BINS)] for q in range(3)]


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def reduce_dev(eng, chain, pairs, **kw):
    out = eng.ensemble_joint_dev(on_device(chain), pairs, **kw)
    eng.sync()
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}


def assert_rule(dev, ref, names=OUT, where=""):
    for k in names:
        if not same_bits(dev[k], ref[k]):
            kind = np.int64 if dev[k].dtype == np.float64 else np.int32
            bad = np.argwhere(np.ascontiguousarray(dev[k]).view(kind) != np.ascontiguousarray(ref[k]).view(kind))
            print(where, k, "differs at", bad[:5].tolist(), "device", dev[k][tuple(bad[0])], "rule", ref[k][tuple(bad[0])])
        assert same_bits(dev[k], ref[k]), (where, k)


def cases():
    """(m, W, N, burn): every m of the list at W = 1, N and burn going round; W = 2 and 6 at the multiples nearest to the edges."""
    T = slab()
    out = []
    for i, m in enumerate((1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1, 3 * T + 5)):
        out.append((m, 1, (2, 3, 16)[i % 3], (0, 3)[i % 2]))
    out += [(2, 2, 3, 0), (64, 2, 16, 2), (256, 2, 2, 1), (T, 2, 3, 1), (T + 2, 2, 2, 0), (6, 6, 2, 0), (258, 6, 16, 1), (T - 4, 6, 3, 0), (T + 2, 6, 2, 5),
            (3 * T + 6, 6, 3, 0), (2 * T + 2, 2, 16, 0)]
    return out


CASES = cases()


@pytest.mark.parametrize("case", range(len(CASES)), ids=["m%d-W%d-N%d-burn%d" % c for c in CASES])
def test_synthetic_chains_equal_the_rule_bit_for_bit(two_rates, case):
    from misti_amd.optimize import ensemble_joint_rule, joint_counts
    m, W, N, burn = CASES[case]
    chain = synthetic(case, 2, m // W + burn, W, N, burn)
    pairs, bins = pairs_and_bins(case, N)
    where = "case %r %r" % (CASES[case], [FLAVOURS[(2 * case + s) % len(FLAVOURS)] for s in range(2)])
    for rng in (None, given_ranges(2, len(pairs))):
        ref = ensemble_joint_rule(chain, pairs, bins=bins, burn=burn, range=rng, masses=MASSES)
        dev = reduce_dev(two_rates, chain, pairs, bins=bins, burn=burn, range=rng, masses=MASSES)
        assert set(OUT) <= set(dev) and dev["counts"].shape == (2, int(ref["offsets"][-1]))
        assert_rule(dev, ref, where=where + (" data" if rng is None else " given"))
        for q in range(len(pairs)):
            assert (joint_counts(dev, q).sum(axis=(1, 2)) + ref["outside"][:, q] == m).all() and (dev["inside"][:, q] + ref["outside"][:, q] == m).all()
        if rng is not None:
            assert dev["inside"][1, 0] == 0 and dev["inside"][1, 1] == 0 and tuple(dev["mode"][1, 0]) == (-1, -1) and not dev["level"][1, :2].any()
            assert same_bits(dev["range"], rng)


def test_every_flavour_of_chain_across_four_slabs(two_rates):
    """All seven kinds of chain in ONE call at m = 3 T + 5, eight masses, the largest and the smallest pair side by side."""
    from misti_amd.optimize import ensemble_joint_rule, joint_counts
    rng = np.random.default_rng(21)
    m, masses = 3 * slab() + 5, (0.95, 0.9, 0.5, 1.0, 1e-9, 0.3333, 0.68, 0.999)
    chain = np.stack([flavour(k, rng, m, 1, 3, 0) for k in FLAVOURS])
    pairs, bins = [(0, 1), (2, 1), (1, 2)], [(128, 128), (1, 1), (4, 4)]
    for window in (None, given_ranges(len(FLAVOURS), 3)):
        ref = ensemble_joint_rule(chain, pairs, bins=bins, range=window, masses=masses)
        dev = reduce_dev(two_rates, chain, pairs, bins=bins, range=window, masses=masses)
        assert_rule(dev, ref)
    dev = reduce_dev(two_rates, chain, pairs, bins=bins, masses=masses)
    eq, nf, five = (FLAVOURS.index(k) for k in ("equal", "nonfinite", "five"))
    assert (dev["inside"][eq] == m).all() and (dev["mode"][eq] == 0).all() and (dev["level"][eq] == m).all() and (dev["cells"][eq] == 1).all()
    assert (dev["inside"][nf] <= m - 3).all() and np.isfinite(dev["range"][nf]).all()
    assert joint_counts(dev, 0, five).max() > m // 25 and np.count_nonzero(joint_counts(dev, 0, five)) <= 25
    lattice = reduce_dev(two_rates, flavour("lattice", rng, 3 * slab(), 1, 2, 0)[None], [(0, 1)], bins=4, range=np.array([[0.0, 1.0], [0.0, 1.0]]), masses=MASSES)
    assert set(lattice["counts"].reshape(-1).tolist()) == {3 * slab() // 16} and (lattice["cells"] == 16).all() and (lattice["held"] == 3 * slab()).all()


def test_no_search_writes_nothing(two_rates):
    import ctypes as C
    import torch
    from misti_amd import _lib
    bufs = {k: torch.full((64,), -777, dtype=torch.float64 if k == "range_out" else torch.int32, device="cuda")
            for k in ("counts", "range_out", "inside", "mode", "level", "cells", "held")}
    pr, bn, ms = np.array([[0, 1]], dtype=np.int32), np.array([[4, 4]], dtype=np.int32), np.array([0.95])
    j = _lib.EnsJoint(size=C.sizeof(_lib.EnsJoint), burn=0, n_pair=1, pairs=pr.ctypes.data, bins=bn.ctypes.data, n_mass=1, masses=ms.ctypes.data,
                      **{k: v.data_ptr() for k, v in bufs.items()})
    rc = two_rates._lib.misti_ens_joint_dev(two_rates._ctx, 0, 5, 4, 2, None, C.byref(j))
    two_rates.sync()
    assert rc == 0 and all((v.cpu().numpy() == -777).all() for v in bufs.values())
    out = reduce_dev(two_rates, np.empty((0, 5, 4, 2)), [(0, 1)], bins=4)
    assert out["counts"].shape == (0, 16) and out["level"].shape == (0, 1, 1)


def test_a_search_alone_equals_the_search_among_others(two_rates):
    chain = synthetic(3, 5, slab() // 2 + 9, 2, 3, 4)
    pairs, bins, window = [(0, 1), (2, 0)], [(63, 65), (128, 128)], given_ranges(5, 2)
    for rng_all, rng_one in ((None, None), (window, window[4:])):
        among = reduce_dev(two_rates, chain, pairs, bins=bins, burn=4, range=rng_all, masses=MASSES)
        alone = reduce_dev(two_rates, chain[4:], pairs, bins=bins, burn=4, range=rng_one, masses=MASSES)
        for k in OUT:
            assert same_bits(alone[k][0], among[k][4]), k


def test_every_output_alone_has_the_bytes_it_has_among_the_others(two_rates):
    from misti_amd.optimize import ensemble_joint_rule
    chain = synthetic(5, 2, slab() + 300, 2, 3, 5)
    pairs, bins = [(0, 1), (1, 2), (2, 0)], [(64, 64), (2, 3), (128, 127)]
    for window in (None, given_ranges(2, 3)):
        kw = dict(bins=bins, burn=5, range=window, masses=MASSES)
        full = reduce_dev(two_rates, chain, pairs, **kw)
        assert_rule(full, ensemble_joint_rule(chain, pairs, **kw))
        for want in [(k,) for k in OUT] + [("mode", "held"), ("range", "inside")]:
            part = reduce_dev(two_rates, chain, pairs, want=want, **kw)
            assert set(want) <= set(part) and not (set(OUT) - set(want)) & set(part)
            for k in want:
                assert same_bits(part[k], full[k]), (want, k)
    no_mass = reduce_dev(two_rates, chain, pairs, bins=bins, burn=5, masses=())                # a histogram needs no mass
    assert "level" not in no_mass and same_bits(no_mass["counts"], reduce_dev(two_rates, chain, pairs, bins=bins, burn=5)["counts"])


def test_a_small_call_behind_a_large_one_on_one_context(two_rates, grid):
    """Stale counts are not added to and the workspace only grows: large, small, large on ONE context equal fresh contexts - with the
    counts in the caller's buffer and with the counts in the context's workspace (only what is read off them asked for)."""
    from misti_amd.engine import Engine
    large, small = synthetic(7, 3, 2 * slab() + 7, 2, 3, 0), synthetic(6, 1, 70, 2, 3, 0)
    pairs = [(0, 1), (2, 1)]
    for want in (OUT, ("inside", "mode", "level", "cells", "held")):
        kw = dict(bins=[(128, 128), (63, 65)], masses=MASSES, want=want)
        seq = [reduce_dev(two_rates, c, pairs, **kw) for c in (large, small, large)]
        for c, got in zip((large, small), seq):
            with Engine(grid[0], grid[1], bands=[(0, 2, -1, 0.2, 0), (1, 2, -1, 0.1, 1)], pulses=(), n_param=2, cpfit=True, smooth=True) as fresh:
                ref = reduce_dev(fresh, c, pairs, **kw)
            for k in want:
                assert same_bits(got[k], ref[k]), k
        for k in want:
            assert same_bits(seq[0][k], seq[2][k]), k


# ---- the sampling doors ---------------------------------------------------------------------------------------------------------------------
def start(points, lo, hi, W, spread=0.05, seed=1):
    from misti_amd.optimize import ensemble_start
    return np.stack([ensemble_start(np.asarray(p), lo, hi, W, spread, seed, s) for s, p in enumerate(points)])


BOX = (np.array([0.01, 0.01]), np.array([1.0, 1.0]))
RUN = dict(split_times=SPLITS, n_step=40, seed=4)
JOINT = dict(pairs=[(0, 1), (1, 0)], bins=[(16, 16), (128, 3)], masses=(0.95, 0.5))
POST = ("mean", "cov", "quant", "tau", "window", "best_llh", "best_x", "best_at")


def test_ensemble_posterior_returns_the_rule_on_its_chain(two_rates):
    from misti_amd.optimize import ensemble_joint_rule
    init = start([[0.2, 0.1], [0.3, 0.1]], *BOX, 8)
    plain = two_rates.ensemble_posterior(init, ROWS, TABLE, BOX, burn=5, keep_chain=True, **RUN)
    r = two_rates.ensemble_posterior(init, ROWS, TABLE, BOX, burn=5, keep_chain=True, joint=JOINT, **RUN)
    assert "joint" not in plain and r["chain"].shape == (2, 40, 8, 2)
    assert_rule(r["joint"], ensemble_joint_rule(r["chain"], burn=5, **JOINT))
    for k in POST + ("last", "last_llh", "accepted", "chain", "chain_llh"):                 # the sampler's and post's outputs keep their bits
        assert same_bits(plain[k], r[k]), k
    assert plain["n_points"] == r["n_points"]
    boxed = two_rates.ensemble_posterior(init, ROWS, TABLE, BOX, burn=5, joint=dict(JOINT, range="box", burn=7), **RUN)      # no chain comes back
    assert "chain" not in boxed and (boxed["joint"]["range"] == np.array([0.01, 1.0])).all()
    assert_rule(boxed["joint"], ensemble_joint_rule(r["chain"], burn=7, range=np.array([0.01, 1.0]), **JOINT))
    with pytest.raises(ValueError, match="finite box"):
        two_rates._joint(2, 2, [(0, 1)], range="box", box=(np.array([0.0, 0.0]), np.array([1.0, np.inf])))


def test_ensemble_sample_with_and_without_joint(two_rates):
    """The plain door without summaries: joint=None IS the older entry, and a joint leaves the sampler's outputs their bits."""
    import ctypes as C
    from misti_amd.optimize import ensemble_joint_rule
    init = start([[0.2, 0.1], [0.3, 0.1]], *BOX, 8)
    old = two_rates.ensemble_sample(init, ROWS, TABLE, BOX, **RUN)
    r = two_rates.ensemble_sample(init, ROWS, TABLE, BOX, joint=dict(JOINT, burn=3, want=("counts", "inside", "level")), **RUN)
    assert set(k for k in r["joint"] if k in OUT) == {"counts", "inside", "level"}
    assert_rule(r["joint"], ensemble_joint_rule(r["chain"], burn=3, **JOINT), ("counts", "inside", "level"))
    for k in ("chain", "chain_llh", "accepted", "last", "last_llh"):
        assert same_bits(old[k], r[k]), k
    # the new entry with joint == NULL against the older entry, through the binding's own marshalling
    calls = []
    real = two_rates._lib.misti_ensemble_sample
    try:
        two_rates._lib.misti_ensemble_sample = lambda ctx, q: (calls.append(1), two_rates._lib.misti_ensemble_sample_joint(ctx, q, None, None, None))[1]
        via = two_rates.ensemble_sample(init, ROWS, TABLE, BOX, **RUN)
    finally:
        two_rates._lib.misti_ensemble_sample = real
    assert calls == [1]
    for k in ("chain", "chain_llh", "accepted", "last", "last_llh"):
        assert same_bits(old[k], via[k]), k


def test_tempered_sample_returns_the_rule_on_its_cold_chain(two_rates):
    from misti_amd.optimize import ensemble_joint_rule
    init = np.ascontiguousarray(np.repeat(start([[0.2, 0.1], [0.3, 0.1]], *BOX, 8)[:, None], 2, axis=1))
    ladder = np.array([1.0, 4.0])
    old = two_rates.tempered_sample(init, ROWS, TABLE, BOX, ladder, burn=5, post=dict(keep_chain=True), **RUN)
    r = two_rates.tempered_sample(init, ROWS, TABLE, BOX, ladder, burn=5, post=dict(keep_chain=True), joint=JOINT, **RUN)
    assert r["chain"].shape == (2, 40, 8, 2)
    assert_rule(r["joint"], ensemble_joint_rule(r["chain"], burn=5, **JOINT))
    for k in POST + ("chain", "chain_llh", "accepted", "swap_proposed", "swap_accepted", "last", "last_llh", "rung_llh", "logz"):
        assert same_bits(old[k], r[k]), k
    lean = two_rates.tempered_sample(init, ROWS, TABLE, BOX, ladder, burn=5, joint=JOINT, **RUN)                  # without summaries
    assert_rule(lean["joint"], r["joint"])
    assert same_bits(lean["logz"], r["logz"])


def test_the_prior_door_returns_the_rule_in_sampling_coordinates(two_rates):
    from misti_amd.optimize import ensemble_joint_rule, joint_table, prior_spec, to_sampling
    prior = prior_spec(2, log=(0,), exponential={1: 0.2})
    box = tuple(to_sampling(v, prior) for v in BOX)
    init = to_sampling(start([[0.2, 0.1], [0.3, 0.1]], *BOX, 8), prior, box)
    old = two_rates.ensemble_posterior(init, ROWS, TABLE, box, burn=5, keep_chain=True, prior=prior, **RUN)
    r = two_rates.ensemble_posterior(init, ROWS, TABLE, box, burn=5, keep_chain=True, prior=prior, joint=dict(JOINT, range="box"), **RUN)
    window = np.stack([np.stack([box[0][[a, b]], box[1][[a, b]]], axis=-1) for a, b in JOINT["pairs"]])
    assert_rule(r["joint"], ensemble_joint_rule(r["chain"], burn=5, range=window, **JOINT))
    for k in POST + ("chain", "chain_llh", "last"):
        assert same_bits(old[k], r[k]), k
    t = joint_table(r["joint"], prior=prior)[0][0]
    assert t["coordinate"] == ("log", "linear") and t["natural_is_image"] and t["window_natural"][0] == tuple(np.exp(box[i][0]) for i in (0, 1))


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def test_cli_mcmc_joint_prints_a_line_per_fit_and_pair_and_writes_the_counts(tmp_path):
    """`--grid-solve --mcmc 8 12 --mcmc-joint 0 1 16 --mcmc-joint 1 0` on a two-rate model over the fixture of tests/test_gpu_post.py's
    command-line test: a `joint:` line per fit and pair, and the counts of `--mcmc-joint-out` equal the rule on the chain `--mcmc-out`
    wrote in the same run, over the box."""
    from misti_amd import io as mio, synth
    from misti_amd.optimize import ensemble_joint_rule
    g = load_golden("golden_pulse_sweep")[0]["in"]
    f1, f2, fj, fc, fo = (str(tmp_path / n) for n in ("g1.psmc", "g2.psmc", "bs.sfs", "chain.npz", "joint.npz"))
    open(f1, "w").write(synth.psmc_text(16, 1, synth.THETA_1))
    open(f2, "w").write(synth.psmc_text(17, 2, synth.THETA_2))
    open(fj, "w").write(mio.format_jsfs(mio.bootstrap_table(synth.chunk_rows(g["sfs"], 20), 1, random.Random(5))))
    cmd = [sys.executable, "-m", "misti_amd.cli", f1, f2, fj, "20", "-mi", "1", "2", "20", "0.1", "1", "-mi", "2", "2", "20", "0.1", "1", "--cpfit",
           "--funits", str(tmp_path / "nounits.txt"), "--grid-st", "19", "20", "--all-bs", "--grid-solve", "--box", "0", "0.01", "1", "--box", "1", "0.01", "1",
           "--mcmc", "8", "12", "--mcmc-seed", "7", "--mcmc-out", fc, "--mcmc-joint", "0", "1", "16", "--mcmc-joint", "1", "0", "--mcmc-joint-mass", "0.9", "0.5",
           "--mcmc-joint-out", fo]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("joint:")]
    pat = re.compile(r"^joint: bs_id = \d+ \tsplitT = \S+ \tcoordinates \((\d), (\d)\) \tbins = (\d+) x \d+ \twindow = \[0\.01, 1\.0\] x \[0\.01, 1\.0\] \tinside = 48 "
                     r"\tmode = \(\S+, \S+\) \tmass 0\.9: level = \d+ cells = \d+ held = \d+ / 48 extent = \[\S+, \S+\] x \[\S+, \S+\] \tmass 0\.5: level = ")
    chain, out = np.load(fc), np.load(fo)
    S = chain["chain"].shape[0]
    assert S == 4 and len(lines) == 2 * S and all(pat.match(l) for l in lines), r.stdout[-1500:]
    assert [pat.match(l).groups() for l in lines[:2]] == [("0", "1", "16"), ("1", "0", "32")]
    ref = ensemble_joint_rule(chain["chain"], [(0, 1), (1, 0)], bins=[(16, 16), (32, 32)], burn=6, range=np.array([0.01, 1.0]), masses=(0.9, 0.5))
    for k in OUT:
        assert same_bits(out[k], ref[k]), k
    assert out["edges_0_0"].shape == (S, 17) and out["edges_1_1"].shape == (S, 33) and out["offsets"].tolist() == [0, 256, 1280]
