"""Ensemble MCMC per search without a GPU: the stream (optimize.ens_draws against NumPy's Philox at the stated blocks, misti_ens_draws -
the very functions the kernels call - against ens_draws), the sampler's own exponential against 50-digit arithmetic and its host entry
bit for bit, the decision on a table that covers every branch, the rule's half-steps and ensemble bookkeeping on analytic objectives
(optimize.ensemble_rule - what the device result is compared against in tests/test_gpu_ens.py), three sampling tests with fixed
seeds, the host helpers, and the argument checks misti_ensemble_sample makes before it looks at a context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

E_ARG, E_LIMIT = -1, -4


def lib():
    from misti_amd import _lib
    return _lib.load()


def c_draws(seed, id_, t, i, W):
    p, uz, ua = C.c_int32(-7), C.c_double(-7.0), C.c_double(-7.0)
    rc = lib().misti_ens_draws(seed, id_, t, i, W, C.byref(p), C.byref(uz), C.byref(ua))
    assert rc == 0, lib().misti_last_error()
    return dict(partner=p.value, u_z=uz.value, u_acc=ua.value)


def c_exp(x):
    y = C.c_double(-7.0)
    assert lib().misti_ens_exp(float(x), C.byref(y)) == 0
    return y.value


def c_accept(z, d, old, new, T, u):
    a = C.c_int32(-7)
    assert lib().misti_ens_accept(z, d, old, new, T, u, C.byref(a)) == 0, lib().misti_last_error()
    return a.value


def bits(v):
    return np.asarray(v, dtype=np.float64).tobytes()


# ---- the stream ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [4, 256])
@pytest.mark.parametrize("seed, id_", [(0, 0), (2 ** 64 - 1, 2 ** 40 + 5)])
def test_ens_draws_are_numpys_philox_at_the_stated_blocks(seed, id_, W):
    """Walker i of step t owns block t W + i of numpy.random.Philox(key=[seed, id]) - words 4 (t W + i) ... of its random_raw stream from
    counter 0: w[0] the partner (the high 64 bits of raw x W / 2, Python integers here), w[1] and w[2] the uniforms (raw >> 11) 2^-53."""
    from misti_amd.optimize import ens_draws
    T = 4
    raw = [int(v) for v in np.random.Philox(key=np.array([seed, id_], dtype=np.uint64)).random_raw(T * W * 4)]
    for t in range(T):
        for i in (0, 1, W // 2 - 1, W // 2, W - 1):
            w = raw[4 * (t * W + i):4 * (t * W + i) + 4]
            want = dict(partner=(w[0] * (W // 2)) >> 64, u_z=(w[1] >> 11) * 2.0 ** -53, u_acc=(w[2] >> 11) * 2.0 ** -53)
            assert ens_draws(seed, id_, t, i, W) == want, (t, i)
            assert c_draws(seed, id_, t, i, W) == want, (t, i)
            assert 0 <= want["partner"] < W // 2 and 0 <= want["u_z"] < 1 and 0 <= want["u_acc"] < 1


def test_the_library_draws_what_ens_draws_states_far_into_the_stream():
    from misti_amd.optimize import ens_draws
    for W, t, i in ((6, 100000, 5), (16, 2 ** 31, 0), (256, 12345, 200)):
        assert c_draws(11, 6, t, i, W) == ens_draws(11, 6, t, i, W)


def test_draws_argument_checks():
    L = lib()
    p = (C.byref(C.c_int32()), C.byref(C.c_double()), C.byref(C.c_double()))
    assert L.misti_ens_draws(0, 0, -1, 0, 4, *p) == E_ARG
    assert L.misti_ens_draws(0, 0, 0, 0, 2, *p) == E_ARG
    assert L.misti_ens_draws(0, 0, 0, 0, 5, *p) == E_ARG and b"even" in L.misti_last_error()
    assert L.misti_ens_draws(0, 0, 0, 0, 258, *p) == E_LIMIT
    assert L.misti_ens_draws(0, 0, 0, 4, 4, *p) == E_ARG
    assert L.misti_ens_draws(0, 0, 0, 0, 4, None, p[1], p[2]) == E_ARG
    assert L.misti_ens_exp(0.0, None) == E_ARG and L.misti_ens_accept(1.0, 0, 0.0, 0.0, 1.0, 0.5, None) == E_ARG
    a = C.byref(C.c_int32())
    assert L.misti_ens_accept(1.0, -1, 0.0, 0.0, 1.0, 0.5, a) == E_ARG and L.misti_ens_accept(1.0, 16, 0.0, 0.0, 1.0, 0.5, a) == E_ARG
    assert L.misti_ens_accept(1.0, 0, 0.0, 0.0, 0.0, 0.5, a) == E_ARG and L.misti_ens_accept(1.0, 0, 0.0, 0.0, float("inf"), 0.5, a) == E_ARG


# ---- the exponential ----------------------------------------------------------------------------------------------------------------------
def exp_grid():
    """A fixed grid: the reduction's breakpoints (k + 1/2) ln 2 and k ln 2 with their neighbours, 0, +-tiny, the subnormal results, the
    underflow and overflow edges, and a regular sweep of [-745, 709]."""
    ln2 = float.fromhex("0x1.62e42fefa39efp-1")
    g = [0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300, 2.0 ** -54, -2.0 ** -54, 1.0, -1.0, 709.0, -745.0, 709.782712893384, 709.7827128933841,
         710.0, np.nextafter(710.0, np.inf), 711.0, 1e308, -708.3964185322641, -708.5, -744.4400719213812, -745.1332191019411, -745.2, -746.0,
         np.nextafter(-746.0, -np.inf), -747.0, -1e308]
    for k in list(range(-1076, -1060)) + list(range(-1025, -1018)) + list(range(-40, 41)) + list(range(1018, 1025)):
        for c in ((k + 0.5) * ln2, k * ln2):
            g += [np.nextafter(c, -np.inf), c, np.nextafter(c, np.inf)]
    g += list(np.linspace(-745.0, 709.0, 2909)) + list(np.linspace(-1.0, 1.0, 401))
    return np.array([v for v in g if np.isfinite(v)], dtype=np.float64)


def test_ens_exp_is_within_4_ulp_of_the_exponential():
    import mpmath
    from misti_amd.optimize import ens_exp
    mpmath.mp.dps = 50
    x = exp_grid()
    y = ens_exp(x)
    worst = 0.0
    for xi, yi in zip(x[(x >= -745.0) & (x <= 709.0)], y[(x >= -745.0) & (x <= 709.0)]):
        exact = mpmath.exp(mpmath.mpf(float(xi)))
        ulp = float(np.spacing(np.float64(float(exact)))) if float(exact) > 0 else 5e-324
        err = float(abs(mpmath.mpf(float(yi)) - exact) / mpmath.mpf(ulp))
        worst = max(worst, err)
        assert err <= 4.0, (xi, yi, err)
    print("ens_exp: largest error on the grid %.3f ulp" % worst)
    assert ens_exp(0.0) == 1.0 and ens_exp(-0.0) == 1.0 and ens_exp(5e-324) == 1.0 and ens_exp(-5e-324) == 1.0
    assert ens_exp(np.nextafter(-746.0, -np.inf)) == 0.0 and ens_exp(-1e308) == 0.0 and ens_exp(-747.0) == 0.0
    assert ens_exp(np.nextafter(710.0, np.inf)) == np.inf and ens_exp(1e308) == np.inf and ens_exp(710.0) == np.inf
    assert np.isnan(ens_exp(np.nan)) and isinstance(ens_exp(1.0), float)
    sweep = ens_exp(np.linspace(-745.0, 709.0, 2909))
    assert (np.diff(sweep) >= 0).all() and (np.diff(sweep[20:]) > 0).all()                # (the first results are one or two subnormal steps)


def test_the_library_exponential_equals_ens_exp_bit_for_bit():
    from misti_amd.optimize import ens_exp
    x = exp_grid()
    want = ens_exp(x)
    got = np.array([c_exp(v) for v in x])
    bad = [float(v) for v, a, b in zip(x, got, want) if bits(a) != bits(b)]
    assert not bad, bad[:5]
    assert np.isnan(c_exp(float("nan"))) and c_exp(float("inf")) == np.inf and c_exp(float("-inf")) == 0.0


# ---- the decision -------------------------------------------------------------------------------------------------------------------------
def test_the_library_decision_equals_the_rules_on_every_branch():
    from misti_amd.optimize import ens_decision, ens_exp
    inf, nan = float("inf"), float("nan")
    table = [  # z, d, llk_old, llk_new, T, u_acc, want (None: whatever the rule says)
        (1.3, 2, -10.0, -inf, 1.0, 0.0, 0), (1.3, 2, -10.0, nan, 1.0, 0.0, 0), (1.3, 2, -inf, -inf, 1.0, 0.0, 0),          # no new value
        (1.3, 2, -inf, -1e6, 1.0, 0.999, 1), (0.6, 3, nan, -5.0, 2.0, 0.999, 1),                                          # no old value
        (0.5, 0, -3.0, -3.0, 1.0, 0.999999, 1), (0.5, 0, -3.0, -4.0, 1.0, 0.3, 1), (0.5, 0, -3.0, -4.0, 1.0, 0.4, 0),      # d = 0: p = exp(e)
        (0.9, 1, -3.0, -2.0, 1.0, 0.999, 1), (0.5, 1, -3.0, -3.0, 1.0, 0.5, 0), (0.5, 1, -3.0, -3.0, 1.0, 0.4999, 1),       # e >= 0
        (0.5, 3, -3.0, 5.0, 4.0, 0.9, 1), (0.5, 15, -3.0, -3.0, 1.0, 2.0 ** -15, 0), (0.5, 15, -3.0, -3.0, 1.0, 2.0 ** -16, 1),
        (1.9, 4, 0.0, -800.0, 1.0, 0.0, 0), (1.9, 4, 0.0, -740.0, 1.0, 0.0, 1), (1.9, 4, 0.0, -1e9, 1.0, 0.0, 0),            # a deep underflow
        (1.9, 4, -1e9, 0.0, 1.0, 0.999, 1), (1.2, 2, -5.0, -6.0, 1e-300, 0.0, 0), (1.2, 2, -6.0, -5.0, 1e-300, 0.999, 1),   # e = -+inf
    ]
    for z, d, old, new, T, e in ((0.7, 2, -12.5, -13.25, 1.0, None), (1.1, 5, -100.0, -103.0, 2.5, None), (0.51, 1, -3.0, -3.0, 1.0, None)):
        g = 1.0
        for _ in range(d):
            g = g * z
        p = g * ens_exp((new - old) / T)
        assert 0 < p < 1
        table += [(z, d, old, new, T, float(np.nextafter(p, 0.0)), 1), (z, d, old, new, T, p, 0), (z, d, old, new, T, float(np.nextafter(p, 1.0)), 0)]
    for z, d, old, new, T, u, want in table:
        rule = int(ens_decision(z, d, old, new, T, u))
        assert rule == want, (z, d, old, new, T, u)
        assert c_accept(z, d, old, new, T, u) == rule, (z, d, old, new, T, u)


# ---- the rule: half-steps and the ensemble -----------------------------------------------------------------------------------------------
def normal(X, s):
    return 0.5 * (X * X).sum(axis=1)


def flat(X, s):
    return np.zeros(len(X))


def stretch(u, a=2.0):
    s = (a - 1.0) * u + 1.0
    return (s * s) / a


def test_half_1_sees_what_half_0_accepted():
    """One free coordinate (d = 0) on a constant objective: p = 1, every proposal inside the box is accepted.  Step 1 by hand from
    ens_draws: the second half moves against the first half AS HALF 0 LEFT IT."""
    from misti_amd.optimize import ens_draws, ensemble_rule
    x0 = np.array([[[1.0], [2.0], [4.0], [8.0]]])
    r = ensemble_rule(flat, x0, [-1e6], [1e6], 1, seed=5, ids=[9])
    x = x0[0, :, 0].copy()
    stale = x.copy()
    for i in range(4):
        d = ens_draws(5, 9, 1, i, 4)
        j = (2 if i < 2 else 0) + d["partner"]
        z = stretch(d["u_z"])
        stale[i] = x0[0, j, 0] + z * (x0[0, i, 0] - x0[0, j, 0])
        x[i] = x[j] + z * (x[i] - x[j])
    assert bits(r["last"][0, :, 0]) == bits(x) and bits(x[:2]) == bits(stale[:2]) and (x[2:] != stale[2:]).any()
    assert r["accepted"].tolist() == [[1, 1, 1, 1]] and r["n_points"] == 4 and bits(r["chain"][0, 0]) == bits(r["last"][0])


def test_a_proposal_outside_the_box_is_never_evaluated_and_a_fixed_coordinate_stays():
    from misti_amd.optimize import ensemble_rule, ensemble_start
    lo, hi = np.array([-0.5, 0.25, -0.5]), np.array([0.5, 0.25, 0.5])
    seen = []

    def fun(X, s):
        seen.append(X.copy())
        return normal(X, s)
    x0 = np.stack([ensemble_start([0.1, 0.25, -0.1], lo, hi, 8, 0.4, 3, s) for s in range(2)])
    r = ensemble_rule(fun, x0, lo, hi, 40, seed=3)
    X = np.concatenate(seen)
    assert (X >= lo).all() and (X <= hi).all() and len(X) == 2 * 8 + r["n_points"]
    assert 0 < r["n_points"] < 40 * 2 * 8                                   # some proposals were rejected in advance
    assert (r["chain"][:, :, :, 1] == 0.25).all() and (X[:, 1] == 0.25).all()
    assert (r["chain"] >= lo).all() and (r["chain"] <= hi).all()
    assert r["accepted"].sum() > 0 and (r["accepted"] <= 40).all()
    assert len(seen) <= 1 + 2 * 40                                                        # one batch per half-step


def test_a_search_alone_equals_the_search_among_others_and_in_another_order():
    from misti_amd.optimize import ensemble_rule
    rng = np.random.default_rng(1)
    x0 = rng.uniform(-1, 1, (4, 6, 2))
    lo, hi = np.tile([-3.0, -3.0], (4, 1)), np.tile([3.0, 3.0], (4, 1))
    lo[2], hi[2] = [-1.0, -1.0], [1.0, 1.0]
    T, ids = np.array([1.0, 2.0, 0.5, 1.0]), np.array([7, 3, 11, 5], dtype=np.uint64)
    kw = dict(n_step=12, thin=2, seed=9)
    fields = ("chain", "chain_llh", "accepted", "last", "last_llh")
    together = ensemble_rule(normal, x0, lo, hi, temperature=T, ids=ids, **kw)
    n = 0
    for s in range(4):
        alone = ensemble_rule(normal, x0[s:s + 1], lo[s], hi[s], temperature=T[s], ids=ids[s:s + 1], **kw)
        n += alone["n_points"]
        for k in fields:
            assert np.array_equal(alone[k][0], together[k][s]), (s, k)
    assert n == together["n_points"]
    perm = np.array([2, 0, 3, 1])
    shuffled = ensemble_rule(normal, x0[perm], lo[perm], hi[perm], temperature=T[perm], ids=ids[perm], **kw)
    for k in fields:
        assert np.array_equal(shuffled[k], together[k][perm]), k
    default = ensemble_rule(normal, x0, lo, hi, temperature=T, ids=np.arange(4), **kw)           # ids default to 0 ... S - 1
    assert all(np.array_equal(default[k], ensemble_rule(normal, x0, lo, hi, temperature=T, **kw)[k]) for k in fields)


def test_no_step_thinning_and_continuing_from_last():
    from misti_amd.optimize import ens_draws, ensemble_rule
    rng = np.random.default_rng(2)
    x0 = rng.uniform(-1, 1, (2, 4, 3))
    box = ([-4.0] * 3, [4.0] * 3)
    r0 = ensemble_rule(normal, x0, *box, 0)
    assert r0["chain"].shape == (2, 0, 4, 3) and bits(r0["last"]) == bits(x0) and bits(r0["last_llh"]) == bits(-normal(x0.reshape(-1, 3), None).reshape(2, 4))
    assert r0["n_points"] == 0 and not r0["accepted"].any()
    every = ensemble_rule(normal, x0, *box, 11, thin=1, seed=4)
    third = ensemble_rule(normal, x0, *box, 11, thin=3, seed=4)
    assert third["chain"].shape == (2, 3, 4, 3) and bits(third["chain"]) == bits(every["chain"][:, 2::3]) and bits(third["chain_llh"]) == bits(every["chain_llh"][:, 2::3])
    assert bits(third["last"]) == bits(every["last"]) == bits(every["chain"][:, -1]) and third["n_points"] == every["n_points"]
    # a later call continues from `last`; with shifted ids it draws from streams the first call did not use: its first half-step by hand
    # from ens_draws of the NEW streams at step 1 - every walker of the first half is where it was or at that proposal
    more = ensemble_rule(normal, every["last"], *box, 5, seed=4, ids=[100, 101])
    assert more["chain"].shape == (2, 5, 4, 3)
    moved = 0
    for s, id_ in enumerate((100, 101)):
        for i in range(2):
            d = ens_draws(4, id_, 1, i, 4)
            xi, xj = every["last"][s, i], every["last"][s, 2 + d["partner"]]
            y = xj + stretch(d["u_z"]) * (xi - xj)
            got = more["chain"][s, 0, i]
            assert bits(got) in (bits(xi), bits(y)), (s, i)
            moved += bits(got) == bits(y)
    assert moved > 0
    assert bits(ensemble_rule(normal, every["last"], *box, 5, seed=4, ids=[0, 1])["chain"]) != bits(more["chain"])      # the ids matter


def test_a_walker_without_a_value_accepts_the_first_proposal_that_has_one():
    """Walker 0 starts where the objective has no value (x[0] > 0).  Replayed from ens_draws and the kept chain: until a proposal of
    its own lands where there is a value it stays put without one, and it takes that proposal whatever u_acc says."""
    from misti_amd.optimize import ens_draws, ensemble_rule

    def hole(X, s):
        return np.where(X[:, 0] > 0, np.inf, normal(X, s))
    x0 = np.array([[[0.5, 0, 0], [-0.5, 0, 0], [-0.2, 0.1, 0], [-0.3, 0, 0.1]]])
    r = ensemble_rule(hole, x0, [-4.0] * 3, [4.0] * 3, 30, seed=1)
    first = None
    for t in range(1, 31):
        before = x0[0] if t == 1 else r["chain"][0, t - 2]
        d = ens_draws(1, 0, t, 0, 4)
        y = before[2 + d["partner"]] + stretch(d["u_z"]) * (before[0] - before[2 + d["partner"]])
        if y[0] <= 0 and (np.abs(y) <= 4).all():
            first = t
            break
        assert r["chain_llh"][0, t - 1, 0] == -np.inf and bits(r["chain"][0, t - 1, 0]) == bits(x0[0, 0]), t
    assert first is not None and first > 1                                               # (with this seed: not at once, and within the run)
    assert bits(r["chain"][0, first - 1, 0]) == bits(y) and r["chain_llh"][0, first - 1, 0] == -0.5 * (y * y).sum()
    assert np.isfinite(r["chain_llh"][0, first - 1:]).all() and (r["chain"][0, first - 1:, :, 0] <= 0).all()   # a point without a value is never taken
    assert r["accepted"][0, 0] >= 1


def test_the_rule_refuses_what_the_library_refuses():
    from misti_amd.optimize import ensemble_rule
    x0 = np.zeros((1, 4, 2))
    for kw in (dict(lo=[0.0, -np.inf], hi=[1.0, 1.0]), dict(lo=[2.0, 0.0], hi=[1.0, 1.0]), dict(lo=[0.0, 0.0], hi=[0.0, 0.0]),
               dict(lo=[0.5, -1.0], hi=[1.0, 1.0]), dict(n_step=-1), dict(thin=0), dict(a=1.0), dict(a=np.inf), dict(temperature=0.0),
               dict(temperature=np.nan)):
        a = dict(lo=[-1.0, -1.0], hi=[1.0, 1.0], n_step=2)
        a.update(kw)
        with pytest.raises(ValueError):
            ensemble_rule(normal, x0, **a)
    for W in (2, 5, 258):
        with pytest.raises(ValueError):
            ensemble_rule(normal, np.zeros((1, W, 2)), [-1.0, -1.0], [1.0, 1.0], 2)


# ---- sampling: deterministic, the seeds are fixed ------------------------------------------------------------------------------------------
def batch_means(series, n_batch=25):
    """The mean of a series and its Monte Carlo standard error from the means of n_batch consecutive batches."""
    y = np.asarray(series)[:len(series) // n_batch * n_batch].reshape(n_batch, -1).mean(axis=1)
    return y.mean(), y.std(ddof=1) / np.sqrt(n_batch)


def moments(chain, burn, mean, var):
    """z-scores of the mean and of the variance (about the known mean) of every coordinate of chain[n_keep][W][N]."""
    c = chain[burn:]
    out = []
    for k in range(c.shape[2]):
        m, se_m = batch_means(c[:, :, k].mean(axis=1))
        v, se_v = batch_means(((c[:, :, k] - mean[k]) ** 2).mean(axis=1))
        out += [(m - mean[k]) / se_m, (v - var[k]) / se_v]
    return np.array(out)


@pytest.fixture(scope="module")
def sampled():
    from misti_amd.optimize import ensemble_rule, ensemble_start
    W, steps = 16, 4000
    wide = (np.array([-60.0, -60.0]), np.array([60.0, 60.0]))
    x0 = np.stack([ensemble_start([0.0, 0.0], *wide, W, 0.01, 17, s) for s in range(2)])
    nrm = ensemble_rule(normal, x0, *wide, steps, temperature=[1.0, 4.0], seed=17)
    box = (np.array([-1.0, 0.0]), np.array([2.0, 5.0]))
    uni = ensemble_rule(flat, ensemble_start([0.5, 2.5], *box, W, 0.3, 17, 2)[None], *box, steps, seed=17, ids=[2])
    return nrm, uni


def test_a_standard_normal_is_sampled_with_its_mean_and_variance(sampled):
    z = moments(sampled[0]["chain"][0], 500, [0.0, 0.0], [1.0, 1.0])
    print("standard normal, z-scores (mean, variance per coordinate):", np.round(z, 2))
    assert (np.abs(z) < 5).all(), z
    assert 0.5 < sampled[0]["accepted"][0].mean() / 4000 < 0.9


def test_the_temperature_scales_the_variance(sampled):
    z = moments(sampled[0]["chain"][1], 500, [0.0, 0.0], [4.0, 4.0])
    print("normal at T = 4, z-scores:", np.round(z, 2))
    assert (np.abs(z) < 5).all(), z


def test_a_constant_objective_samples_the_box_uniformly(sampled):
    z = moments(sampled[1]["chain"][0], 500, [0.5, 2.5], [9.0 / 12, 25.0 / 12])
    print("uniform on the box, z-scores:", np.round(z, 2))
    assert (np.abs(z) < 5).all(), z
    assert sampled[1]["n_points"] < 4000 * 16                                         # proposals left the box and cost nothing


# ---- host helpers ---------------------------------------------------------------------------------------------------------------------------
def test_composite_temperature():
    from misti_amd.optimize import composite_temperature
    H = -np.array([[4.0, 1.0], [1.0, 3.0]])
    assert composite_temperature(H, H) == pytest.approx(1.0, rel=1e-14) and composite_temperature(H, -H) == pytest.approx(1.0, rel=1e-14)
    assert composite_temperature(H, -7.5 * H) == pytest.approx(7.5, rel=1e-14)
    J = np.array([[8.0, 0.0], [0.0, 3.0]])
    assert composite_temperature(H, J) == pytest.approx(abs(np.trace(np.linalg.inv(H) @ J)) / 2, rel=1e-14)
    for bad in (np.array([[4.0, 1.0], [1.0, 3.0]]), np.array([[-4.0, 0.0], [0.0, 1.0]]), np.array([[-4.0, 0.0], [0.0, np.nan]])):
        with pytest.raises(ValueError, match="not negative definite"):
            composite_temperature(bad, J)
    with pytest.raises(ValueError):
        composite_temperature(H, np.full((2, 2), np.nan))


def test_ensemble_start_stays_inside_the_box_and_walker_0_is_the_point():
    from misti_amd.optimize import ensemble_start
    lo, hi = np.array([0.0, 1.0, 5.0, -1.0, 0.0]), np.array([1.0, 1.0, 50.0, 1.0, 1e-3])
    p = ensemble_start([0.999, 7.0, 20.0, -3.0, 5e-4], lo, hi, 32, 0.05, 4, 1)
    assert p.shape == (32, 5) and (p >= lo).all() and (p <= hi).all()
    assert p[0].tolist() == [0.999, 1.0, 20.0, -1.0, 5e-4] and (p[:, 1] == 1.0).all()
    assert (p[:, 0] == 1.0).any() and len(set(p[:, 2])) == 32 and np.abs(p[:, 2] - 20.0).max() <= 0.05 * 45
    assert bits(p) == bits(ensemble_start([0.999, 7.0, 20.0, -3.0, 5e-4], lo, hi, 32, 0.05, 4, 1)) != bits(ensemble_start([0.999, 7.0, 20.0, -3.0, 5e-4], lo, hi, 32, 0.05, 4, 2))
    # the uniforms come from the sampler's key with the second counter word 1: no step of a sampler reads them
    raw = np.random.Philox(key=np.array([4, 1], dtype=np.uint64), counter=np.array([0, 1, 0, 0], dtype=np.uint64)).random_raw(32 * 5)
    u = ((raw >> np.uint64(11)).astype(float) * 2.0 ** -53).reshape(32, 5)
    assert p[3, 2] == 20.0 + 0.05 * 45.0 * (2.0 * u[3, 2] - 1.0)


def test_ensemble_summary_on_an_ar1_series_of_known_autocorrelation_time():
    from misti_amd.optimize import autocorrelation_time, ensemble_summary
    rng = np.random.default_rng(8)
    # tau = (1 + phi) / (1 - phi) = 9.  The windowed estimate (window M = 5 tau) has a relative standard error of about
    # sqrt(2 (2 M + 1) / n) = 0.03 at n = 199 000: the 15 % below are five of them.
    phi, n, W = 0.8, 200000, 4
    e = rng.standard_normal((n, W, 2)) * np.sqrt(1 - phi * phi)
    y = np.empty((n, W, 2))
    y[0] = rng.standard_normal((W, 2))
    for t in range(1, n):
        y[t] = phi * y[t - 1] + e[t]
    y[:, :, 1] = 3.0 + 2.0 * y[:, :, 1]
    s = ensemble_summary(y, burn=1000)
    assert s["tau"] == pytest.approx([9.0, 9.0], rel=0.15) and not s["short"].any() and s["n"] == 199000
    assert s["mean"] == pytest.approx([0.0, 3.0], abs=0.1) and s["median"] == pytest.approx([0.0, 3.0], abs=0.1)
    assert s["q025"] == pytest.approx([-1.96, 3 - 3.92], abs=0.15) and s["q975"] == pytest.approx([1.96, 3 + 3.92], abs=0.15)
    assert ensemble_summary(y[:300], burn=0)["short"].all()                              # under 50 autocorrelation times
    assert autocorrelation_time(rng.standard_normal(5000)) == pytest.approx(1.0, abs=0.2) and autocorrelation_time(np.ones(10)) == 1.0
    acc = np.full(W, 30, dtype=np.int32)
    assert ensemble_summary(y[:100], 0, accepted=acc, n_step=100)["acceptance"] == pytest.approx(0.3)
    with pytest.raises(ValueError):
        ensemble_summary(y[:10], burn=10)


# ---- what the ABI refuses before it looks at a context ----------------------------------------------------------------------------------
def ens_sample(ctx=None, size=None, null=(), **kw):
    """misti_ensemble_sample WITHOUT a context: every check below comes before the context is looked at, and a descriptor that passes
    them ends at "ctx is NULL".  No output is ever written."""
    from misti_amd import _lib
    S = kw.pop("n_start", 2)
    W = kw.get("walkers", 6)
    n = max(S, 1)
    a = dict(init=np.full((n, max(W, 1), 2), 0.5), rows=np.zeros(n, dtype=np.int32), jsfs=np.ones((3, 8)), box_lo=np.zeros((1, 2)), box_hi=np.ones((1, 2)),
             temperature=np.ones(n), last=np.zeros((n, max(W, 1), 2)), last_llh=np.zeros((n, max(W, 1))), split_times=np.full(n, 5.0))
    for k in list(kw):
        if k in a:
            a[k] = np.ascontiguousarray(kw.pop(k), dtype=a[k].dtype)
    f = dict(size=C.sizeof(_lib.EnsSample) if size is None else size, split=_lib.SPLIT_PER_START, n_start=S, n_rep=3, n_box=1, walkers=W, n_step=5, thin=1,
             n_temp=1, a=2.0, seed=0)
    f.update(kw)
    q = _lib.EnsSample(**f, **{k: (None if k in null else v.ctypes.data) for k, v in a.items()})
    rc = lib().misti_ensemble_sample(ctx, C.byref(q))
    assert not a["last"].any() and not a["last_llh"].any()
    return rc, lib().misti_last_error().decode()


@pytest.mark.parametrize("kw, code, word", [
    (dict(), E_ARG, "ctx is NULL"),                                                 # the descriptor passes: only the context is missing
    (dict(n_start=0, n_box=0), E_ARG, "ctx is NULL"),
    (dict(n_step=0), E_ARG, "ctx is NULL"),
    (dict(size=8), E_ARG, "size"),
    (dict(split=0), E_ARG, "split mode"),
    (dict(n_start=-1), E_ARG, "negative"),
    (dict(null=("init",)), E_ARG, "NULL"),
    (dict(null=("temperature",)), E_ARG, "NULL"),
    (dict(null=("last_llh",)), E_ARG, "NULL"),
    (dict(null=("split_times",)), E_ARG, "split_times"),
    (dict(null=("split_times",), split=2), E_ARG, "ctx is NULL"),                   # a fitted split needs none
    (dict(n_rep=0), E_ARG, "n_rep"),
    (dict(walkers=5), E_ARG, "walkers must be even"),
    (dict(walkers=2), E_ARG, "walkers must be even and >= 4"),
    (dict(walkers=258), E_LIMIT, "MISTI_ENS_MAX_WALKERS"),
    (dict(n_step=-1), E_ARG, "n_step"),
    (dict(thin=0), E_ARG, "thin"),
    (dict(a=1.0), E_ARG, "a must be"),
    (dict(a=float("inf")), E_ARG, "a must be"),
    (dict(n_temp=3), E_ARG, "n_temp"),
    (dict(temperature=[0.0, 1.0]), E_ARG, "temperature[0]"),
    (dict(n_temp=2, temperature=[1.0, float("nan")]), E_ARG, "temperature[1]"),
    (dict(n_temp=2, temperature=[1.0, float("inf")]), E_ARG, "temperature[1]"),
    (dict(n_box=3), E_ARG, "n_box"),
    (dict(rows=[0, 3]), E_ARG, "rows[1]"),
    (dict(split_times=[5.0, float("inf")]), E_ARG, "split_times[1]"),
    # the header's order: of two faults the earlier one is named
    (dict(walkers=5, thin=0), E_ARG, "walkers"),
    (dict(thin=0, a=0.5), E_ARG, "thin"),
    (dict(a=0.5, n_box=3), E_ARG, "a must be"),
    (dict(temperature=[-1.0, 1.0], rows=[0, 9]), E_ARG, "temperature[0]"),
])
def test_ensemble_sample_argument_checks(kw, code, word):
    rc, why = ens_sample(**kw)
    assert rc == code and word in why, (rc, why)


def test_a_null_descriptor_is_refused():
    assert lib().misti_ensemble_sample(None, None) == E_ARG and b"NULL" in lib().misti_last_error()


# ---- header, binding --------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_entry_points():
    from misti_amd import _lib, build, optimize
    hdr = open(os.path.join(ROOT, "include", "misti_hip.h")).read()
    assert re.search(r"^int misti_ensemble_sample\(misti_ctx\* ctx, const misti_ens_t\* sampler\);", hdr, flags=re.M)
    for name in ("misti_ens_draws", "misti_ens_exp", "misti_ens_accept"):
        assert re.search(r"^int %s\(" % name, hdr, flags=re.M) and name in _lib.SYMBOLS
    flat_ = " ".join(hdr.split()).replace("* ", "")
    assert "optimize.ensemble_rule" in hdr and "rejected WITHOUT an evaluation" in flat_ and "0x1.62e42feep-1" in hdr
    assert "#define MISTI_ENS_MAX_WALKERS 256" in hdr and _lib.ENS_MAX_WALKERS == optimize.ENS_MAX_WALKERS == 256
    assert "misti_ens.hip" in build.SOURCES and "misti_ens.h" in build.HEADERS
    body = hdr[:hdr.index("} misti_ens_t;")].rsplit("typedef struct {", 1)[1]
    names = [n for line in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", line.strip())]
    assert names == [n for n, _ in _lib.EnsSample._fields_], names
    # the rule's constants are the header's
    assert (optimize._ENS_INV_LN2.hex(), optimize._ENS_LN2_HI.hex(), optimize._ENS_LN2_LO.hex()) == ("0x1.71547652b82fep+0", "0x1.62e42fee00000p-1", "0x1.a39ef35793c76p-33")


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
BASE = ["a.psmc", "b.psmc", "d.sfs", "20"]
SOLVE = ["--grid-solve", "--grid-st", "15", "17", "-mi", "1", "4", "16", "0.2", "1", "--box", "0", "0.01", "5"]
FIT = ["--fit-st", "--grid-st", "15", "17", "-mi", "1", "4", "16", "0.2", "1", "--box", "0", "0.01", "5", "--box", "st", "14", "18"]


def test_parser_accepts_mcmc():
    from misti_amd import cli
    a = cli.build_parser().parse_args(BASE + SOLVE + ["--mcmc", "8", "50", "--mcmc-burn", "10", "--mcmc-thin", "2", "--mcmc-seed", "3", "--mcmc-spread", "0.1",
                                                       "--mcmc-temp", "2.5", "--mcmc-out", "c.npz"])
    assert cli.mcmc_error(a) is None
    assert cli._mcmc_options(a) == dict(walkers=8, n_step=50, thin=2, burn=10, seed=3, spread=0.1, temperature=2.5)
    a = cli.build_parser().parse_args(BASE + FIT + ["--all-bs", "--mcmc", "16", "40", "--mcmc-temp", "auto", "--de", "16", "5"])
    assert cli.mcmc_error(a) is None and cli._mcmc_options(a) == dict(walkers=16, n_step=40, thin=1, burn=20, seed=0, spread=1e-2, temperature="auto")
    assert cli.mcmc_error(cli.build_parser().parse_args(BASE)) is None
    assert "--mcmc W STEPS" in cli.__doc__ or "--mcmc" in cli.build_parser().format_help()


@pytest.mark.parametrize("args, word", [
    (["--mcmc-seed", "3"], "give --mcmc W STEPS"),
    (["--mcmc-temp", "auto"], "give --mcmc W STEPS"),
    (["--mcmc", "3", "5"] + SOLVE, "even, 4 ... 256"),
    (["--mcmc", "7", "5"] + SOLVE, "even, 4 ... 256"),
    (["--mcmc", "258", "5"] + SOLVE, "even, 4 ... 256"),
    (["--mcmc", "8", "0"] + SOLVE, "at least 1"),
    (["--mcmc", "8", "5", "--grid-st", "15", "17"], "--fit-st or --grid-solve"),
    (["--mcmc", "8", "5"] + SOLVE + ["--se"], "--se"),
    (["--mcmc", "8", "5"] + SOLVE + ["--gpus", "2"], "one GPU"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-thin", "0"], "--mcmc-thin"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-thin", "6"], "--mcmc-thin"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-burn", "5"], "--mcmc-burn"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-seed", "-1"], "uint64"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-spread", "-0.1"], "--mcmc-spread"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-temp", "0"], "--mcmc-temp"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-temp", "hot"], "--mcmc-temp"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-temp", "auto"], "needs --all-bs"),
    (["--mcmc", "8", "5"] + SOLVE[:-4], "no --box 0"),
    (["--mcmc", "8", "5"] + FIT[:-4], "no --box st"),
    (["--mcmc", "8", "5"] + SOLVE[:-4] + ["--box", "0", "0.01", "inf"], "finite box"),
])
def test_mcmc_error_names_the_reason(args, word):
    from misti_amd import cli
    why = cli.mcmc_error(cli.build_parser().parse_args(BASE + args))
    assert why is not None and word in why, why


def test_mcmc_is_refused_before_a_file_is_read(capsys):
    from misti_amd import cli
    assert cli.main(["no.psmc", "no.psmc", "no.sfs", "20", "--mcmc", "8", "5"] + SOLVE[:-4]) == 2      # (the files do not exist)
    assert "--box" in capsys.readouterr().err
