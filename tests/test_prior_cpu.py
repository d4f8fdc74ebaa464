"""Priors and log-scale coordinates of the ensemble samplers without a GPU: the host entries misti_ens_log_prior and
misti_ens_accept_prior - the very functions the kernels call - against the rule's own NumPy statements bit for bit, the structural
identities of optimize.ensemble_prior_rule / tempered_prior_rule (what the device result is compared against in
tests/test_gpu_prior.py), sampling tests with fixed seeds on a constant objective (the posterior is the prior), the refusals
misti_ensemble_sample_prior and misti_tempered_sample_prior make before they look at a context, the binding, and the command line."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from conftest import ROOT

E_ARG = -1


def lib():
    from misti_amd import _lib
    return _lib.load()


def bits(v):
    return np.asarray(v, dtype=np.float64).tobytes()


def c_log_prior(scale, kind, p0, p1, lo, hi, y, natural=True):
    scale, kind = (np.ascontiguousarray(v, dtype=np.int32) for v in (scale, kind))
    p0, p1, lo, hi, y = (np.ascontiguousarray(v, dtype=np.float64) for v in (p0, p1, lo, hi, y))
    lp, nat = C.c_double(-7.0), np.full(y.size, -7.0)
    rc = lib().misti_ens_log_prior(y.size, *(v.ctypes.data for v in (scale, kind, p0, p1, lo, hi, y)), C.byref(lp), nat.ctypes.data if natural else None)
    return rc, lp.value, nat


def c_accept(z, d, old, new, T, lp_old, lp_new, u):
    a = C.c_int32(-7)
    assert lib().misti_ens_accept_prior(z, d, old, new, T, lp_old, lp_new, u, C.byref(a)) == 0, lib().misti_last_error()
    return a.value


# ---- host functions against the rule ---------------------------------------------------------------------------------------------------
def test_the_library_log_prior_and_natural_point_equal_the_rules():
    """Every kind x both scales at once (N = 6), then the same with each coordinate in turn fixed among free ones; y at both box edges,
    +-0.0 and inside; p0 / p1 entries a kind does not read are NaN: they are not looked at."""
    from misti_amd import optimize as o
    nan = float("nan")
    scale = [s for s in (o.COORD_LINEAR, o.COORD_LOG) for _ in range(3)]
    kind = [o.PRIOR_FLAT, o.PRIOR_NORMAL, o.PRIOR_EXPONENTIAL] * 2
    p0 = np.array([nan, 0.3, 0.7, nan, -2.5, 1.3])
    p1 = np.array([nan, 0.5, nan, nan, 1.7, nan])
    lo = np.array([-1.0, -4.0, -0.0, -6.9, -5.0, -3.0])
    hi = np.array([1.0, 4.0, 8.0, 2.3, 1.0, 3.0])
    inside = np.array([0.25, -1.1, 0.0, -0.3, 0.1, -2.9])
    n = 0
    for fixed in (None, 0, 1, 2, 3, 4, 5):
        l, h = lo.copy(), hi.copy()
        if fixed is not None:
            h[fixed] = l[fixed]
        for y in (l, h, inside if fixed is None else np.where(np.arange(6) == fixed, l, inside), np.where(np.arange(6) == 2, -0.0, l)):
            rc, lp, nat = c_log_prior(scale, kind, p0, p1, l, h, y)
            assert rc == 0, lib().misti_last_error()
            assert bits(lp) == bits(o.ens_log_prior(kind, p0, p1, l, h, y)), (fixed, y)
            assert bits(nat) == bits(o.ens_natural(scale, y))
            exp = np.empty(6)
            for k in range(6):
                v = C.c_double()
                assert lib().misti_ens_exp(float(y[k]), C.byref(v)) == 0
                exp[k] = v.value
            assert bits(nat[3:]) == bits(exp[3:]) and bits(nat[:3]) == bits(y[:3])              # LOG: misti_ens_exp(y) bit for bit
            n += 1
    assert n == 28
    # by hand: one normal and one exponential term, each operation rounded on its own, summed in increasing k from +0.0
    y = inside
    u = (y[1] - 0.3) / 0.5
    t1, t2 = -0.5 * (u * u), -((y[2] - lo[2]) / 0.7)
    u4 = (y[4] - -2.5) / 1.7
    want = (((0.0 + t1) + t2) + -0.5 * (u4 * u4)) + -((y[5] - lo[5]) / 1.3)
    assert bits(c_log_prior(scale, kind, p0, p1, lo, hi, y)[1]) == bits(want)
    # an all-flat prior: +0.0, and natural may be NULL
    rc, lp, nat = c_log_prior([0, 1], [0, 0], [nan, nan], [nan, nan], [0.0, -1.0], [1.0, 1.0], [0.5, 0.5], natural=False)
    assert rc == 0 and bits(lp) == bits(0.0) and (nat == -7.0).all()


def test_the_library_decision_with_a_prior_equals_the_rules_on_every_branch():
    from misti_amd.optimize import ens_decision, ens_decision_prior, ens_exp
    inf, nan = float("inf"), float("nan")
    table = [  # z, d, llk_old, llk_new, T, lp_old, lp_new, u_acc, want (None: whatever the rule says)
        (1.3, 2, -10.0, -inf, 1.0, 0.0, 5.0, 0.0, 0), (1.3, 2, -10.0, nan, 1.0, 0.0, 5.0, 0.0, 0), (1.3, 2, -inf, -inf, 1.0, 0.0, 0.0, 0.0, 0),   # no new value
        (1.3, 2, -inf, -1e6, 1.0, 0.0, -50.0, 0.999, 1), (0.6, 3, nan, -5.0, 2.0, -1.0, -9.0, 0.999, 1),                                        # no old value
        (0.5, 0, -3.0, -3.0, 1.0, -1.0, -2.0, 0.3, 1), (0.5, 0, -3.0, -3.0, 1.0, -1.0, -2.0, 0.4, 0),                                           # the prior alone decides
        (0.5, 0, -3.0, -4.0, 2.0, -2.0, -1.0, 0.999, 1),                                                                                        # ... and is not tempered: e = -0.5 + 1
        (0.5, 0, -3.0, -4.0, 2.0, -1.0, -1.0, 0.61, 0), (0.5, 0, -3.0, -4.0, 2.0, -1.0, -1.0, 0.60, 1),
        (2.0, 3, -3.0, -3.0, 1.0, 0.0, 0.0, 0.999999, 1), (0.5, 2, -3.0, -3.0, 1.0, 0.0, 0.0, 0.25, 0), (0.5, 2, -3.0, -3.0, 1.0, 0.0, 0.0, 0.2499, 1),
        (1.0, 1, -3.0, -1e4, 1.0, 0.0, 0.0, 0.0, 0), (1.0, 1, -3.0, -3.0, 1.0, 0.0, -1e4, 0.0, 0),                                               # p underflows: u = 0 is not below 0
        (1.7, 4, -2.0, -2.5, 0.7, -0.125, -3.5, 0.01, None), (0.8, 2, -7.0, -6.5, 3.0, -4.0, -0.5, 0.9, None),
    ]
    for z, d, old, new, T, lo_, ln_, u, want in table:
        got = c_accept(z, d, old, new, T, lo_, ln_, u)
        assert got == int(ens_decision_prior(z, d, old, new, T, lo_, ln_, u)), (z, d, old, new, T, lo_, ln_, u)
        if want is not None:
            assert got == want, (z, d, old, new, T, lo_, ln_, u)
    # on both sides of the threshold p = g ens_exp(e), e = (new - old) / T + (lp_new - lp_old)
    for z, d, old, new, T, lo_, ln_ in ((0.7, 2, -12.5, -13.25, 1.0, -0.5, -0.75), (1.1, 5, -100.0, -103.0, 2.5, -1.25, -3.0), (0.51, 1, -3.0, -3.0, 1.0, -2.0, -2.5)):
        g = 1.0
        for _ in range(d):
            g = g * z
        p = g * ens_exp((new - old) / T + (ln_ - lo_))
        assert 0.0 < p < 1.0
        assert c_accept(z, d, old, new, T, lo_, ln_, np.nextafter(p, 0.0)) == 1 and c_accept(z, d, old, new, T, lo_, ln_, p) == 0
    # equal log priors: the prior-less decision
    for z, d, old, new, T, u in itertools.product((0.6, 1.4), (0, 2), (-3.0,), (-3.5, -2.0), (1.0, 4.0), (0.1, 0.5, 0.9)):
        assert c_accept(z, d, old, new, T, -1.5, -1.5, u) == int(ens_decision(z, d, old, new, T, u))
    a = C.c_int32()
    assert lib().misti_ens_accept_prior(1.0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5, C.byref(a)) == E_ARG
    assert lib().misti_ens_accept_prior(1.0, 16, 0.0, 0.0, 1.0, 0.0, 0.0, 0.5, C.byref(a)) == E_ARG
    assert lib().misti_ens_accept_prior(1.0, 0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.5, None) == E_ARG


@pytest.mark.parametrize("kw, word", [
    (dict(scale=[0, 2]), "coordinate 1: the scale 2"),
    (dict(kind=[3, 0]), "coordinate 0: the kind 3"),
    (dict(kind=[0, 1], p1=[0.0, 0.0]), "coordinate 1: the normal's sd"),
    (dict(kind=[0, 1], p1=[0.0, float("inf")]), "coordinate 1: the normal's sd"),
    (dict(kind=[2, 0], p0=[-1.0, 0.0]), "coordinate 0: the exponential's scale"),
    (dict(kind=[2, 0], p0=[float("nan"), 0.0]), "coordinate 0: the exponential's scale"),
    (dict(kind=[0, 1], p0=[0.0, float("nan")], p1=[0.0, 1.0]), "coordinate 1: the normal's mean"),
    (dict(scale=[0, 1], hi=[1.0, 709.5]), "coordinate 1: the log-scale box"),
    (dict(scale=[1, 0], lo=[-745.5, 0.0]), "coordinate 0: the log-scale box"),
    (dict(scale=[0, 2], kind=[3, 0]), "coordinate 0: the kind 3"),                     # coordinate by coordinate, and per coordinate in the header's order
    (dict(scale=[2, 0], kind=[3, 0]), "the scale 2"),
    (dict(kind=[1, 0], p0=[float("nan"), 0.0], p1=[-1.0, 0.0]), "sd"),
])
def test_log_prior_refuses_what_the_samplers_refuse_per_coordinate(kw, word):
    """The per-coordinate refusals of the two samplers stand behind the context (they need N); misti_ens_log_prior makes the same checks
    through the same function, as search 0.  The rule refuses them too."""
    from misti_amd.optimize import ensemble_prior_rule
    a = dict(scale=[0, 0], kind=[0, 0], p0=[0.0, 0.0], p1=[0.0, 0.0], lo=[0.0, 0.0], hi=[1.0, 1.0])
    a.update(kw)
    rc, lp, nat = c_log_prior(a["scale"], a["kind"], a["p0"], a["p1"], a["lo"], a["hi"], a["lo"])
    why = lib().misti_last_error().decode()
    assert rc == E_ARG and "search 0" in why and word in why, why
    assert lp == -7.0 and (nat == -7.0).all()
    with pytest.raises(ValueError):
        ensemble_prior_rule(flat, np.tile(np.array(a["lo"], dtype=float), (1, 4, 1)), a["lo"], a["hi"], 1, {k: a[k] for k in ("scale", "kind", "p0", "p1")})


# ---- structural identities -----------------------------------------------------------------------------------------------------------------
def normal(X, s):
    return 0.5 * (np.asarray(X) ** 2).sum(axis=1)


def flat(X, s):
    return np.zeros(len(X))


def two_wells(X, s):
    X = np.asarray(X)
    a = -0.5 * ((X - 2.0) ** 2).sum(axis=1) / 0.25 ** 2
    b = -0.5 * ((X + 2.0) ** 2).sum(axis=1) / 0.25 ** 2
    return -np.logaddexp(a, b)


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        va, vb = np.asarray(a[k]), np.asarray(b[k])
        assert va.shape == vb.shape and va.dtype == vb.dtype and va.tobytes() == vb.tobytes(), k


def test_a_prior_that_says_nothing_is_the_rule_without_one():
    from misti_amd.optimize import ensemble_prior_rule, ensemble_rule, prior_spec, tempered_prior_rule, tempered_rule
    rng = np.random.default_rng(3)
    lo, hi = np.array([[-4.0, -4.0], [-3.0, 1.0]]), np.array([[4.0, 4.0], [3.0, 1.0]])
    x0 = np.clip(rng.uniform(-3, 3, (2, 3, 6, 2)), lo[:, None, None], hi[:, None, None])
    none = prior_spec(2)
    assert not none["scale"].any() and not none["kind"].any()
    for fun in (two_wells, normal):
        kw = dict(n_step=12, thin=2, temperature=[1.0, 2.5], seed=4, ids=[3, 9])
        want = ensemble_rule(fun, x0[:, 0], lo, hi, **kw)
        assert want["accepted"].sum() > 0
        same(ensemble_prior_rule(fun, x0[:, 0], lo, hi, prior=None, **kw), want)
        same(ensemble_prior_rule(fun, x0[:, 0], lo, hi, prior=none, **kw), want)
        same(ensemble_prior_rule(fun, x0[:, 0], lo, hi, prior={k: np.tile(v, (2, 1)) for k, v in none.items()}, **kw), want)
        kw = dict(n_step=12, thin=2, swap_every=1, burn=1, seed=4, ids=[3, 9])
        want = tempered_rule(fun, x0, lo, hi, [1.0, 4.0, 16.0], **kw)
        assert want["swap_accepted"].sum() > 0
        same(tempered_prior_rule(fun, x0, lo, hi, [1.0, 4.0, 16.0], prior=None, **kw), want)
        same(tempered_prior_rule(fun, x0, lo, hi, [1.0, 4.0, 16.0], prior=none, **kw), want)


def test_one_rung_of_the_tempered_prior_rule_is_the_ensemble_prior_rule_and_the_prior_moves_the_chain():
    from misti_amd.optimize import ensemble_prior_rule, ensemble_rule, prior_spec, tempered_prior_rule
    rng = np.random.default_rng(5)
    lo, hi = np.array([-2.0, -3.0, 0.5]), np.array([1.5, 3.0, 0.5])
    x0 = np.clip(rng.uniform(-1, 1, (2, 1, 6, 3)), lo, hi)
    prior = prior_spec(3, log=(0, 2), normal={0: (-0.5, 0.4)}, exponential={1: 0.8})
    seen = []

    def fun(X, s):
        seen.append(np.array(X))
        return normal(X, s)
    ens = ensemble_prior_rule(fun, x0[:, 0], lo, hi, 9, prior, thin=2, temperature=[1.5, 0.5], seed=2, ids=[1, 4])
    from misti_amd.optimize import ens_exp
    assert all(bits(X[:, 2]) == bits(np.full(len(X), ens_exp(0.5))) for X in seen)                 # a fixed LOG coordinate: ens_exp(lo) exactly
    assert bits(seen[0][:, 0]) == bits(ens_exp(x0[:, 0].reshape(-1, 3)[:, 0])) and bits(seen[0][:, 1]) == bits(x0[:, 0].reshape(-1, 3)[:, 1])
    assert (ens["chain"][..., 2] == 0.5).all() and (ens["chain"] >= lo).all() and (ens["chain"] <= hi).all()
    for swap_every in (0, 1):
        pt = tempered_prior_rule(normal, x0, lo, hi, np.array([[1.5], [0.5]]), 9, prior, thin=2, swap_every=swap_every, seed=2, ids=[1, 4])
        for k in ("chain", "accepted", "last", "last_llh"):
            assert bits(pt[k].reshape(ens[k].shape)) == bits(ens[k]) and pt[k].dtype == ens[k].dtype, k
        assert bits(pt["chain_llh"][:, 0]) == bits(ens["chain_llh"]) and pt["n_points"] == ens["n_points"]
    plain = ensemble_rule(lambda X, s: normal(np.column_stack([np.exp(X[:, 0]), X[:, 1], np.exp(X[:, 2])]), s), x0[:, 0], lo, hi, 9, thin=2,
                          temperature=[1.5, 0.5], seed=2, ids=[1, 4])
    assert bits(plain["chain"]) != bits(ens["chain"])


# ---- sampling: deterministic, the seeds are fixed; a constant objective, so the posterior is the prior ------------------------------------------
def batch_means(series, n_batch=25):
    """The mean of a series and its Monte Carlo standard error from the means of n_batch consecutive batches (tests/test_ens_cpu.py)."""
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


W, STEPS, BURN = 16, 4000, 500


def sample(fun, prior, lo, hi, at, seed, id_):
    from misti_amd.optimize import ensemble_prior_rule, ensemble_start
    lo, hi = np.array([lo]), np.array([hi])
    x0 = ensemble_start([at], lo, hi, W, 0.3, seed, id_)[None]
    return ensemble_prior_rule(fun, x0, lo, hi, STEPS, prior, seed=seed, ids=[id_])


def test_a_normal_prior_is_sampled_with_its_mean_and_variance():
    """NORMAL(0.3, 0.5) on [-4, 4]: the box cuts the normal at -8.6 and 7.4 sd - below 1e-13 of its mass: mean 0.3, variance 0.25."""
    from misti_amd.optimize import prior_spec
    r = sample(flat, prior_spec(1, normal={0: (0.3, 0.5)}), -4.0, 4.0, 0.3, 17, 0)
    z = moments(r["chain"][0], BURN, [0.3], [0.25])
    print("NORMAL(0.3, 0.5) on [-4, 4], z-scores (mean, variance):", np.round(z, 2))
    assert (np.abs(z) < 5).all(), z


def test_an_exponential_prior_is_sampled_with_its_mean_and_variance():
    """EXPONENTIAL(0.5) on [0, 8]: the box cuts it at 16 scales (1e-7 of its mass; the moments move by 1e-6): mean 0.5, variance 0.25."""
    from misti_amd.optimize import prior_spec
    r = sample(flat, prior_spec(1, exponential={0: 0.5}), 0.0, 8.0, 0.5, 17, 1)
    z = moments(r["chain"][0], BURN, [0.5], [0.25])
    print("EXPONENTIAL(0.5) on [0, 8], z-scores (mean, variance):", np.round(z, 2))
    assert (np.abs(z) < 5).all(), z


def test_a_flat_prior_on_a_log_coordinate_is_log_uniform():
    """LOG + FLAT on [ln 1e-3, ln 10]: uniform in y - the midpoint, (hi - lo)^2 / 12 -, and half of the natural samples lie below 0.1,
    the geometric midpoint.  The objective saw natural values only."""
    from misti_amd.optimize import from_sampling, prior_spec
    lo, hi = float(np.log(1e-3)), float(np.log(10.0))
    prior = prior_spec(1, log=(0,))
    seen = [np.inf, -np.inf]

    def fun(X, s):
        seen[0], seen[1] = min(seen[0], X.min()), max(seen[1], X.max())
        return np.zeros(len(X))
    r = sample(fun, prior, lo, hi, 0.5 * (lo + hi), 17, 2)
    assert 1e-3 * (1 - 1e-12) <= seen[0] and seen[1] <= 10.0 * (1 + 1e-12)
    z = moments(r["chain"][0], BURN, [0.5 * (lo + hi)], [(hi - lo) ** 2 / 12.0])
    print("LOG + FLAT on [ln 1e-3, ln 10], z-scores (mean, variance):", np.round(z, 2))
    assert (np.abs(z) < 5).all(), z
    below = from_sampling(r["chain"][0][BURN:], prior)[:, :, 0] < 0.1
    share, se = batch_means(below.mean(axis=1))
    print("share of natural samples below 0.1: %.4f, z = %.2f" % (share, (share - 0.5) / se))
    assert abs(share - 0.5) < 5 * se


def test_a_normal_prior_on_a_normal_objective_halves_the_variance():
    from misti_amd.optimize import prior_spec
    r = sample(normal, prior_spec(1, normal={0: (0.0, 1.0)}), -60.0, 60.0, 0.0, 17, 3)
    z = moments(r["chain"][0], BURN, [0.0], [0.5])
    print("standard normal objective x NORMAL(0, 1), z-scores (mean, variance):", np.round(z, 2))
    assert (np.abs(z) < 5).all(), z


# ---- host helpers -----------------------------------------------------------------------------------------------------------------------------
def test_prior_spec_and_the_coordinate_maps():
    from misti_amd import optimize as o
    p = o.prior_spec(4, log=(0, 3), normal={3: (-1.0, 2.0)}, exponential={1: 0.25})
    assert p["scale"].tolist() == [1, 0, 0, 1] and p["kind"].tolist() == [0, 2, 0, 1] and p["scale"].dtype == p["kind"].dtype == np.int32
    assert p["p0"].tolist() == [0.0, 0.25, 0.0, -1.0] and p["p1"].tolist() == [0.0, 0.0, 0.0, 2.0]
    for bad in (dict(log=(4,)), dict(normal={-1: (0.0, 1.0)}), dict(normal={1: (0.0, 1.0)}, exponential={1: 1.0})):
        with pytest.raises(ValueError):
            o.prior_spec(4, **bad)
    x = np.array([[1e-3, 0.5, 7.0, 20.0], [2.0, 0.0, -1.0, 1.0]])
    y = o.to_sampling(x, p)
    assert bits(y) == bits(np.column_stack([np.log(x[:, 0]), x[:, 1], x[:, 2], np.log(x[:, 3])]))
    assert bits(o.from_sampling(y, p)) == bits(np.column_stack([np.exp(y[:, 0]), y[:, 1], y[:, 2], np.exp(y[:, 3])]))
    # a value whose logarithm lands outside the box of logarithms is clipped into it
    lo, hi = np.array([np.log(1e-3), 0.0, -1.0, 0.0]), np.array([np.nextafter(np.log(2.0), 0.0), 1.0, 7.0, np.log(20.0)])
    y = o.to_sampling(x, p, (lo, hi))
    assert (y >= lo).all() and (y <= hi).all() and y[1, 0] == hi[0] and y[0, 3] == hi[3]


def test_posterior_table_reports_log_coordinates_in_natural_units_too():
    from misti_amd import optimize as o
    rng = np.random.default_rng(2)
    chain = rng.normal(-1.0, 0.5, (40, 6, 2))
    res = o.ensemble_posterior_rule(chain, rng.normal(size=(40, 6)), burn=4)
    res["last"] = chain[-1]
    prior = o.prior_spec(2, log=(1,))
    t0, t = o.posterior_table(res, 36), o.posterior_table(res, 36, prior=prior)
    for k in t0:
        assert bits(t[k]) == bits(t0[k]) or t[k].dtype == bool
    assert t["coordinate"].tolist() == ["linear", "log"]
    assert bits(t["quant_natural"][0]) == bits(res["quant"][0]) and bits(t["quant_natural"][1]) == bits(np.exp(res["quant"][1]))
    assert bits(t["best_x_natural"]) == bits([res["best_x"][0], np.exp(res["best_x"][1])])


# ---- what the ABI refuses before it looks at a context -----------------------------------------------------------------------------------
def sample_prior(entry, prior=None, size=None, null=(), **kw):
    """misti_ensemble_sample_prior / misti_tempered_sample_prior WITHOUT a context, on a descriptor that passes every check up to the
    context.  `prior`: dict of n_prior and the arrays.  No output is ever written."""
    from misti_amd import _lib
    S, Wk = 2, 6
    a = dict(init=np.full((S, Wk, 2), 0.5), rows=np.zeros(S, dtype=np.int32), jsfs=np.ones((3, 8)), box_lo=np.zeros((1, 2)), box_hi=np.ones((1, 2)),
             last=np.zeros((S, Wk, 2)), last_llh=np.zeros((S, Wk)), split_times=np.full(S, 5.0))
    f = dict(split=_lib.SPLIT_PER_START, n_start=S, n_rep=3, n_box=1, walkers=Wk, n_step=5, thin=1, a=2.0, seed=0)
    f.update(kw)
    if entry == "ensemble":
        a.update(temperature=np.ones(1))
        q = _lib.EnsSample(size=C.sizeof(_lib.EnsSample), n_temp=1, **f, **{k: v.ctypes.data for k, v in a.items()})
    else:
        a.update(ladder=np.ones(1), rung_llh=np.zeros(S), logz=np.zeros(S))
        q = _lib.PtSample(size=C.sizeof(_lib.PtSample), n_rung=1, n_ladder=1, swap_every=1, burn=0, **f, **{k: v.ctypes.data for k, v in a.items()})
    pa = dict(scale=np.zeros((2, 2), dtype=np.int32), kind=np.zeros((2, 2), dtype=np.int32), p0=np.zeros((2, 2)), p1=np.zeros((2, 2)))
    p = None
    if prior is not None:
        p = _lib.Prior(size=C.sizeof(_lib.Prior) if size is None else size, n_prior=prior, **{k: (None if k in null else v.ctypes.data) for k, v in pa.items()})
    fn = lib().misti_ensemble_sample_prior if entry == "ensemble" else lib().misti_tempered_sample_prior
    rc = fn(None, C.byref(q), None, C.byref(p) if p is not None else None)
    assert not a["last"].any() and not a["last_llh"].any() and (entry == "ensemble" or not (a["rung_llh"].any() or a["logz"].any()))
    return rc, lib().misti_last_error().decode()


@pytest.mark.parametrize("entry", ["ensemble", "tempered"])
@pytest.mark.parametrize("kw, word", [
    (dict(), "ctx is NULL"),                                                        # no prior: the descriptor passes, only the context is missing
    (dict(prior=1), "ctx is NULL"),
    (dict(prior=2), "ctx is NULL"),
    (dict(prior=1, size=8), "the prior descriptor's size is 8"),
    (dict(prior=3), "n_prior must be 1 or n_start (got 3 for 2"),
    (dict(prior=0), "n_prior"),
    (dict(prior=1, null=("scale",)), "scale / kind / p0 / p1 is NULL"),
    (dict(prior=1, null=("kind",)), "NULL"),
    (dict(prior=2, null=("p0",)), "NULL"),
    (dict(prior=1, null=("p1",)), "NULL"),
    # the existing order, the prior's behind the box's: of two faults the earlier one is named
    (dict(prior=1, size=8, split=0), "the prior descriptor's size"),
    (dict(prior=3, n_box=3), "n_box"),
    (dict(prior=3, thin=0), "thin"),
    (dict(prior=3, null=("scale",)), "n_prior"),
    (dict(prior=3, n_rep=0), "n_rep"),
])
def test_the_samplers_refuse_a_bad_prior_descriptor_before_the_context(entry, kw, word):
    rc, why = sample_prior(entry, **kw)
    assert rc == E_ARG and word in why, (rc, why)


def test_the_abi_version_is_still_6():
    from misti_amd import _lib
    assert _lib.ABI_VERSION == 6 and lib().misti_abi_version() == 6


# ---- header, binding --------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_prior():
    from misti_amd import _lib, build, optimize
    hdr = open(os.path.join(ROOT, "include", "misti_hip.h")).read()
    assert "#define MISTI_ABI_VERSION 6" in hdr and _lib.ABI_VERSION == 6
    assert C.sizeof(_lib.EnsSample) == 192 and C.sizeof(_lib.PtSample) == 240 and C.sizeof(_lib.Prior) == 40
    # the library's own sizeof: a descriptor of this binding's size passes the size check (it ends at the context)
    assert "ctx is NULL" in sample_prior("ensemble", prior=1)[1] and "ctx is NULL" in sample_prior("tempered", prior=1)[1]
    for name, py in (("MISTI_COORD_LINEAR", _lib.COORD_LINEAR), ("MISTI_COORD_LOG", _lib.COORD_LOG), ("MISTI_PRIOR_FLAT", _lib.PRIOR_FLAT),
                     ("MISTI_PRIOR_NORMAL", _lib.PRIOR_NORMAL), ("MISTI_PRIOR_EXPONENTIAL", _lib.PRIOR_EXPONENTIAL)):
        assert int(re.search(r"^#define %s (\d+)$" % name, hdr, flags=re.M).group(1)) == py == getattr(optimize, name[len("MISTI_"):])
    for name in ("misti_ensemble_sample_prior", "misti_tempered_sample_prior", "misti_ens_log_prior", "misti_ens_accept_prior"):
        assert re.search(r"^int %s\(" % name, hdr, flags=re.M) and name in _lib.SYMBOLS
    body = hdr[:hdr.index("} misti_prior_t;")].rsplit("typedef struct {", 1)[1]
    names = [n for line in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", line.strip())]
    assert names == [n for n, _ in _lib.Prior._fields_], names
    assert "optimize.ensemble_prior_rule" in hdr and "optimize.tempered_prior_rule" in hdr and "NOT tempered" in hdr
    assert "misti_prior.h" in build.HEADERS


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
BASE = ["a.psmc", "b.psmc", "d.sfs", "20"]
SOLVE = ["--grid-solve", "--grid-st", "15", "17", "-mi", "1", "4", "16", "0.2", "1", "--box", "0", "0.01", "5"]
FIT = ["--fit-st", "--grid-st", "15", "17", "-mi", "1", "4", "16", "0.2", "1", "--box", "0", "0.01", "5", "--box", "st", "14", "18"]


def test_parser_accepts_the_prior_options():
    from misti_amd import cli, optimize as o
    a = cli.build_parser().parse_args(BASE + FIT + ["--mcmc", "8", "50", "--mcmc-log", "0", "--mcmc-prior", "st", "normal", "16", "0.5"])
    assert cli.mcmc_error(a) is None
    p = cli._mcmc_prior(a, 1)
    assert p["scale"].tolist() == [o.COORD_LOG, o.COORD_LINEAR] and p["kind"].tolist() == [o.PRIOR_FLAT, o.PRIOR_NORMAL]
    assert p["p0"].tolist() == [0.0, 16.0] and p["p1"].tolist() == [0.0, 0.5]
    a = cli.build_parser().parse_args(BASE + SOLVE + ["--mcmc", "8", "50", "--mcmc-prior", "0", "exponential", "0.25", "--mcmc-log", "0"])
    assert cli.mcmc_error(a) is None
    p = cli._mcmc_prior(a, 1)
    assert p["scale"].tolist() == [o.COORD_LOG] and p["kind"].tolist() == [o.PRIOR_EXPONENTIAL] and p["p0"].tolist() == [0.25]
    a = cli.build_parser().parse_args(BASE + SOLVE + ["--mcmc", "8", "50"])
    assert cli.mcmc_error(a) is None and cli._mcmc_prior(a, 1) is None
    assert "--mcmc-log" in cli.build_parser().format_help() and "--mcmc-prior" in cli.__doc__


@pytest.mark.parametrize("args, word", [
    (SOLVE + ["--mcmc-log", "0"], "give --mcmc W STEPS"),
    (SOLVE + ["--mcmc-prior", "0", "normal", "0", "1"], "give --mcmc W STEPS"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-log", "1"], "no coordinate of this run"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-log", "st"], "no coordinate of this run"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-log", "0", "0"], "twice"),
    (["--mcmc", "8", "5"] + SOLVE[:-4] + ["--box", "0", "0", "5", "--mcmc-log", "0"], "LO > 0"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-prior", "2", "normal", "0", "1"], "no coordinate of this run"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-prior", "0", "cauchy", "0", "1"], "K normal MEAN SD | K exponential SCALE"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-prior", "0", "normal", "0"], "K normal MEAN SD | K exponential SCALE"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-prior", "0", "exponential", "1", "2"], "K normal MEAN SD | K exponential SCALE"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-prior", "0"], "K normal MEAN SD | K exponential SCALE"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-prior", "0", "normal", "0", "x"], "numbers"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-prior", "0", "normal", "0", "0"], "SD finite and > 0"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-prior", "0", "normal", "inf", "1"], "MEAN must be finite"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-prior", "0", "exponential", "-1"], "SCALE must be finite and > 0"),
    (["--mcmc", "8", "5"] + FIT + ["--mcmc-prior", "st", "normal", "16", "1", "--mcmc-prior", "st", "exponential", "1"], "already has a prior"),
])
def test_mcmc_error_names_the_priors_fault(args, word):
    from misti_amd import cli
    why = cli.mcmc_error(cli.build_parser().parse_args(BASE + args))
    assert why is not None and word in why, why


def test_the_prior_options_are_refused_before_a_file_is_read(capsys):
    from misti_amd import cli
    assert cli.main(["no.psmc", "no.psmc", "no.sfs", "20"] + SOLVE + ["--mcmc-log", "0"]) == 2          # (the files do not exist)
    assert "give --mcmc W STEPS" in capsys.readouterr().err
