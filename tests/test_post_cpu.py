"""Posterior summaries of a chain without a GPU: the rule (optimize.ensemble_posterior_rule - what the device result is compared
against, bit for bit, in tests/test_gpu_post.py) against NumPy's sort, quantile, mean and covariance and against
optimize.autocorrelation_time's FFT estimator, the rule's edge cases, the helper posterior_table, and the argument checks
misti_ens_summary_dev makes before it looks at a context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

E_ARG, E_LIMIT = -1, -4
EPS = 2.0 ** -53                     # unit roundoff


def lib():
    from misti_amd import _lib
    return _lib.load()


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def chains(seed, S=1, K=40, W=4, N=2):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((S, K, W, N)) * np.array([1.0, 30.0])[:N] + np.array([0.5, -7.0])[:N]


# ---- order statistics, quantiles --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("burn", [0, 7])
def test_order_statistics_are_numpys_sort(seed, burn):
    from misti_amd.optimize import ensemble_posterior_rule
    x = chains(seed)
    r = ensemble_posterior_rule(x, burn=burn, probs=(0.0, 1.0))
    flat = x[0, burn:].reshape(-1, 2)
    for j in range(2):
        assert bits(r["order"][0, j]).tolist() == bits(np.sort(flat[:, j])).tolist()
        assert r["quant"][0, j, 0] == flat[:, j].min() and r["quant"][0, j, 1] == flat[:, j].max()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_interpolated_quantiles_are_within_4_ulp_of_numpys(seed):
    """q = x_(i) + g (x_(i+1) - x_(i)) has three roundings (the difference, the product, the sum), each at most half an ulp of a
    magnitude no larger than the larger neighbouring order statistic's - and so does np.quantile's own linear interpolation: 4 ulp of
    that magnitude bound the difference of the two."""
    from misti_amd.optimize import ensemble_posterior_rule
    x = chains(seed)
    probs = (0.025, 0.1, 0.25, 0.5, 0.6180339887, 0.75, 0.975, 0.999)
    r = ensemble_posterior_rule(x, burn=3, probs=probs)
    flat = x[0, 3:].reshape(-1, 2)
    m = flat.shape[0]
    for j in range(2):
        o = np.sort(flat[:, j])
        for p, pr in enumerate(probs):
            i = int(np.floor((m - 1) * pr))
            mag = max(abs(o[i]), abs(o[min(i + 1, m - 1)]))
            assert abs(r["quant"][0, j, p] - np.quantile(flat[:, j], pr)) <= 4 * np.spacing(mag), (j, pr)
            assert o[i] <= r["quant"][0, j, p] <= o[min(i + 1, m - 1)]


# ---- mean, covariance ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_mean_and_covariance_within_the_textbook_bound(seed):
    """A sum of m terms in ANY order is within gamma_m sum|terms| of the exact sum, gamma_m = m u / (1 - m u) (Higham, Accuracy and
    Stability of Numerical Algorithms, (4.4)); the rule's and NumPy's sums both are, so they differ by at most twice that.  The
    covariance's terms carry the rounding of the centring and of the product as well: gamma_{m+4} on the sum of |products|, plus the
    effect of the two means differing within their own bound."""
    from misti_amd.optimize import ensemble_posterior_rule
    x = chains(seed)
    r = ensemble_posterior_rule(x, burn=5)
    flat = x[0, 5:].reshape(-1, 2)
    m = flat.shape[0]
    gam = lambda k: k * EPS / (1 - k * EPS)
    mean_bound = 2 * gam(m + 2) * np.abs(flat).sum(axis=0) / m
    assert (np.abs(r["mean"][0] - np.mean(flat, axis=0)) <= mean_bound).all()
    ref = np.cov(flat.T)
    d = flat - flat.mean(axis=0)
    for j in range(2):
        for k in range(2):
            terms = np.abs(d[:, j] * d[:, k]).sum()
            shift = mean_bound[j] * np.abs(d[:, k]).sum() + mean_bound[k] * np.abs(d[:, j]).sum()
            assert abs(r["cov"][0, j, k] - ref[j, k]) <= (2 * gam(m + 4) * terms + 2 * shift) / (m - 1), (j, k)
    assert bits(r["cov"][0]).tolist() == bits(r["cov"][0].T).tolist()


# ---- the autocorrelation time ------------------------------------------------------------------------------------------------------------
def ar1(seed, n, phi):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(n) * np.sqrt(1 - phi * phi)
    y = np.empty(n)
    y[0] = rng.standard_normal()
    for t in range(1, n):
        y[t] = phi * y[t - 1] + e[t]
    return y


def fft_window(y, c=5.0):
    """autocorrelation_time's own tau_M series and window decision (optimize.autocorrelation_time, line for line)."""
    n = y.size
    y = y - y.mean()
    size = 1 << (2 * n - 1).bit_length()
    f = np.fft.rfft(y, size)
    rho = np.fft.irfft(f * np.conj(f), size)[:n] / float(np.dot(y, y))
    tau = 2.0 * np.cumsum(rho) - 1.0
    ok = np.arange(n) >= c * tau
    return tau, int(np.argmax(ok)) if ok.any() else -1


def test_ar1_series_window_and_tau_are_autocorrelation_times():
    from misti_amd.optimize import autocorrelation_time, ensemble_posterior_rule
    n, phi, W = 4000, 0.5, 4
    y = ar1(11, n, phi)
    tau_fft, M = fft_window(y)
    # the precondition: the FFT estimator's window decision is not within rounding of flipping, at M and at M - 1
    assert M >= 1 and abs(M - 5.0 * tau_fft[M]) > 1e-6 and abs((M - 1) - 5.0 * tau_fft[M - 1]) > 1e-6
    # W identical walkers: the ensemble-mean series is the series itself ((4 y) / 4 is exact)
    r = ensemble_posterior_rule(np.repeat(y[:, None, None], W, axis=1), max_lag=n - 1)
    assert r["window"][0] == M
    assert r["tau"][0] == pytest.approx(autocorrelation_time(y), rel=1e-10)
    assert r["tau"][0] == pytest.approx((1 + phi) / (1 - phi), rel=0.25)
    # the cap: lags behind the window change nothing, a cap below it leaves no window
    capped = ensemble_posterior_rule(np.repeat(y[:, None, None], W, axis=1), max_lag=M)
    assert capped["window"][0] == M and bits(capped["tau"]).tolist() == bits(r["tau"]).tolist()
    assert ensemble_posterior_rule(np.repeat(y[:, None, None], W, axis=1), max_lag=M - 1)["window"][0] == -1


# ---- edge cases of the rule ----------------------------------------------------------------------------------------------------------------
def test_a_constant_series_has_tau_1_window_0_and_no_variance():
    from misti_amd.optimize import ensemble_posterior_rule
    r = ensemble_posterior_rule(np.full((1, 9, 4, 2), 2.5))
    assert (r["tau"] == 1.0).all() and (r["window"] == 0).all() and (r["cov"] == 0.0).all() and (r["mean"] == 2.5).all()
    assert (r["quant"] == 2.5).all()


def test_max_lag_0_leaves_no_window():
    from misti_amd.optimize import ensemble_posterior_rule
    r = ensemble_posterior_rule(chains(4), max_lag=0)
    assert (r["window"] == -1).all() and (r["tau"] == 1.0).all()


def test_p_0_and_p_1_are_the_minimum_and_the_maximum():
    from misti_amd.optimize import ensemble_posterior_rule
    x = chains(5, S=2)
    r = ensemble_posterior_rule(x, burn=2, probs=(0.0, 1.0, 0.0))
    flat = x[:, 2:].reshape(2, -1, 2)
    assert (r["quant"][:, :, 0] == flat.min(axis=1)).all() and (r["quant"][:, :, 1] == flat.max(axis=1)).all()
    assert (r["quant"][:, :, 2] == r["quant"][:, :, 0]).all()


def test_one_kept_step():
    from misti_amd.optimize import ensemble_posterior_rule
    x = chains(6, K=5, W=6)
    r = ensemble_posterior_rule(x, burn=4)
    for j in range(2):
        e = x[0, 4, 0, j]
        for w in range(1, 6):
            e = e + x[0, 4, w, j]
        assert r["mean"][0, j] == e / 6.0
    assert (r["tau"] == 1.0).all() and (r["window"] == -1).all()


def test_signed_zeros_follow_the_key_order():
    from misti_amd.optimize import ensemble_posterior_rule, post_order_key
    assert post_order_key(np.array([-0.0]))[0] < post_order_key(np.array([0.0]))[0]
    key = post_order_key(np.array([-np.inf, -1.0, -0.0, 0.0, 5e-324, 1.0, np.inf, np.nan]))
    assert (np.diff(key.astype(object)) > 0).all()
    x = np.zeros((1, 3, 3, 1))
    x.reshape(-1)[[1, 3, 5, 7]] = -0.0                                          # m = 9: four -0.0, five +0.0; p = k / 8 is a rank exactly
    r = ensemble_posterior_rule(x, probs=(0.0, 3 / 8, 4 / 8, 1.0))
    assert np.signbit(r["order"][0, 0]).tolist() == [True] * 4 + [False] * 5
    assert np.signbit(r["quant"][0, 0]).tolist() == [True, True, False, False]


def test_best_sample_ties_go_to_the_lowest_step_then_walker():
    from misti_amd.optimize import ensemble_posterior_rule
    x = chains(7, K=6)
    llh = np.full((1, 6, 4), -3.0)
    llh[0, 0, 0] = 9.0                                                          # burnt: never a candidate
    llh[0, 3, 2] = llh[0, 3, 1] = llh[0, 4, 0] = 1.5
    llh[0, 2, 3] = np.nan
    llh[0, 2, 0] = -np.inf
    r = ensemble_posterior_rule(x, llh, burn=2)
    assert r["best_llh"][0] == 1.5 and r["best_at"][0].tolist() == [1, 1] and bits(r["best_x"][0]).tolist() == bits(x[0, 3, 1]).tolist()
    none = ensemble_posterior_rule(x, np.full((1, 6, 4), -np.inf))
    assert none["best_llh"][0] == -np.inf and np.isnan(none["best_x"]).all() and none["best_at"][0].tolist() == [-1, -1]
    no_llh = ensemble_posterior_rule(x)
    assert no_llh["best_llh"][0] == -np.inf and np.isnan(no_llh["best_x"]).all() and no_llh["best_at"][0].tolist() == [-1, -1]
    up = ensemble_posterior_rule(x, np.where(np.arange(4) == 2, np.inf, llh), burn=2)      # +inf is a value
    assert up["best_llh"][0] == np.inf and up["best_at"][0].tolist() == [0, 2]


def test_a_search_is_a_function_of_its_own_chain():
    from misti_amd.optimize import ensemble_posterior_rule
    x = chains(8, S=3)
    llh = np.random.default_rng(8).standard_normal((3, 40, 4))
    all_ = ensemble_posterior_rule(x, llh, burn=4)
    one = ensemble_posterior_rule(x[1], llh[1], burn=4)
    for k, v in one.items():
        assert np.asarray(v).tobytes() == np.ascontiguousarray(all_[k][1]).tobytes(), k


def test_the_rule_refuses_what_the_library_refuses():
    from misti_amd.optimize import ensemble_posterior_rule
    x = chains(9)
    for kw in (dict(burn=40), dict(burn=-1), dict(probs=()), dict(probs=[0.5] * 9), dict(probs=(1.5,)), dict(probs=(float("nan"),)), dict(max_lag=-1),
               dict(c=0.0), dict(c=float("inf"))):
        with pytest.raises(ValueError):
            ensemble_posterior_rule(x, **kw)


def test_posterior_table():
    from misti_amd.optimize import ensemble_posterior_rule, posterior_table
    y = ar1(3, 3000, 0.5)
    x = np.stack([np.repeat(y[:, None], 4, axis=1), 2.0 * np.repeat(y[:, None], 4, axis=1) + 1.0], axis=2)[None]
    r = ensemble_posterior_rule(x)
    t = posterior_table(r, 3000, walkers=4)
    assert t["sd"][0] == pytest.approx(np.sqrt(np.diagonal(r["cov"][0]))) and t["corr"][0][0, 1] == pytest.approx(1.0)
    assert t["n_eff"][0] == pytest.approx(3000 * 4 / r["tau"][0]) and not t["short"].any()
    assert posterior_table(ensemble_posterior_rule(x[:, :60]), 60, walkers=4)["short"].all()          # under 50 tau
    assert posterior_table(ensemble_posterior_rule(x, max_lag=2), 3000, walkers=4)["short"].all()       # no window


# ---- what the ABI refuses before it looks at a context ----------------------------------------------------------------------------------
def summary(S=2, K=10, W=4, N=2, chain=1, size=None, probs=(0.025, 0.5, 0.975), null_probs=False, **kw):
    """misti_ens_summary_dev WITHOUT a context: every check below comes before the context is looked at, and a descriptor that passes
    them ends at "ctx is NULL"."""
    from misti_amd import _lib
    pr = np.asarray(probs, dtype=np.float64)
    f = dict(size=C.sizeof(_lib.EnsPost) if size is None else size, burn=0, n_prob=pr.size, probs=None if null_probs else pr.ctypes.data, max_lag=5, c=5.0)
    f.update(kw)
    p = _lib.EnsPost(**f)
    rc = lib().misti_ens_summary_dev(None, S, K, W, N, C.c_void_p(chain) if chain else None, None, C.byref(p))
    return rc, lib().misti_last_error().decode()


@pytest.mark.parametrize("kw, code, word", [
    (dict(), E_ARG, "ctx is NULL"),                                                 # the descriptor passes: only the context is missing
    (dict(S=0, chain=0), E_ARG, "ctx is NULL"),
    (dict(size=8), E_ARG, "size"),
    (dict(S=-1), E_ARG, "negative"),
    (dict(W=0), E_ARG, "no walker"),
    (dict(burn=-1), E_ARG, "burn"),
    (dict(burn=10), E_ARG, "burn"),
    (dict(K=0), E_ARG, "burn"),
    (dict(n_prob=0), E_ARG, "n_prob"),
    (dict(n_prob=9), E_ARG, "n_prob"),
    (dict(null_probs=True), E_ARG, "probs is NULL"),
    (dict(probs=(0.5, 1.5)), E_ARG, "probs[1]"),
    (dict(probs=(-0.1,)), E_ARG, "probs[0]"),
    (dict(probs=(float("nan"),)), E_ARG, "probs[0]"),
    (dict(max_lag=-1), E_ARG, "max_lag"),
    (dict(c=0.0), E_ARG, "c must be"),
    (dict(c=float("nan")), E_ARG, "c must be"),
    (dict(c=float("inf")), E_ARG, "c must be"),
    (dict(chain=0), E_ARG, "chain is NULL"),
    (dict(W=257), E_LIMIT, "MISTI_ENS_MAX_WALKERS"),
    (dict(N=17), E_LIMIT, "MISTI_MAX_PARAMS"),
    (dict(K=2 ** 30, W=4), E_LIMIT, "INT32_MAX"),
    # the header's order: of two faults the earlier one is named
    (dict(burn=10, n_prob=0), E_ARG, "burn"),
    (dict(n_prob=0, null_probs=True), E_ARG, "n_prob"),
    (dict(probs=(2.0,), max_lag=-1), E_ARG, "probs[0]"),
    (dict(max_lag=-1, c=0.0), E_ARG, "max_lag"),
    (dict(c=0.0, chain=0), E_ARG, "c must be"),
    (dict(chain=0, W=257), E_ARG, "chain is NULL"),
    (dict(W=257, N=17), E_LIMIT, "MISTI_ENS_MAX_WALKERS"),
])
def test_summary_argument_checks(kw, code, word):
    rc, why = summary(**kw)
    assert rc == code and word in why, (rc, why)


def test_null_descriptors_are_refused():
    from misti_amd import _lib
    assert lib().misti_ens_summary_dev(None, 1, 1, 4, 1, None, None, None) == E_ARG and b"NULL" in lib().misti_last_error()
    assert lib().misti_ensemble_posterior(None, None, None) == E_ARG and b"sampler descriptor is NULL" in lib().misti_last_error()
    q = _lib.EnsSample(size=C.sizeof(_lib.EnsSample), split=_lib.SPLIT_PER_START)
    assert lib().misti_ensemble_posterior(None, C.byref(q), None) == E_ARG and b"summary descriptor is NULL" in lib().misti_last_error()
    p = _lib.EnsPost(size=4)
    assert lib().misti_ensemble_posterior(None, C.byref(q), C.byref(p)) == E_ARG and b"misti_ens_post_t" in lib().misti_last_error()


# ---- header, binding, command line ---------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_entry_points():
    from misti_amd import _lib, build, optimize
    hdr = open(os.path.join(ROOT, "include", "misti_hip.h")).read()
    assert lib().misti_abi_version() == 6 and "#define MISTI_ABI_VERSION 6" in hdr
    assert re.search(r"^int misti_ens_summary_dev\(misti_ctx\* ctx, int64_t S, int64_t K, int32_t W, int32_t N, const double\* d_chain,", hdr, flags=re.M)
    assert re.search(r"^int misti_ensemble_posterior\(misti_ctx\* ctx, const misti_ens_t\* sampler, const misti_ens_post_t\* post\);", hdr, flags=re.M)
    assert "misti_ens_summary_dev" in _lib.SYMBOLS and "misti_ensemble_posterior" in _lib.SYMBOLS
    assert "#define MISTI_POST_MAX_PROBS 8" in hdr and _lib.POST_MAX_PROBS == optimize.POST_MAX_PROBS == 8
    assert "optimize.ensemble_posterior_rule" in hdr
    assert "misti_post.hip" in build.SOURCES and "misti_post.h" in build.HEADERS
    body = hdr[:hdr.index("} misti_ens_post_t;")].rsplit("typedef struct {", 1)[1]
    names = [n for line in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", line.strip())]
    assert names == [n for n, _ in _lib.EnsPost._fields_], names


BASE = ["a.psmc", "b.psmc", "d.sfs", "20"]
SOLVE = ["--grid-solve", "--grid-st", "15", "17", "-mi", "1", "4", "16", "0.2", "1", "--box", "0", "0.01", "5"]


def test_parser_accepts_mcmc_post():
    from misti_amd import cli
    a = cli.build_parser().parse_args(BASE + SOLVE + ["--mcmc", "8", "50", "--mcmc-post"])
    assert cli.mcmc_error(a) is None and cli._mcmc_post_options(a) == dict(probs=(0.025, 0.5, 0.975), max_lag=None)
    a = cli.build_parser().parse_args(BASE + SOLVE + ["--mcmc", "8", "50", "--mcmc-post", "0.05", "0.95", "--mcmc-lag", "20"])
    assert cli.mcmc_error(a) is None and cli._mcmc_post_options(a) == dict(probs=(0.05, 0.95), max_lag=20)
    # without --mcmc-post the options of --mcmc are what they were
    a = cli.build_parser().parse_args(BASE + SOLVE + ["--mcmc", "8", "50"])
    assert a.mcmc_post is None and cli.mcmc_error(a) is None
    for args, word in ((["--mcmc-post"], "give --mcmc W STEPS"), (["--mcmc", "8", "50", "--mcmc-lag", "3"] + SOLVE, "--mcmc-lag"),
                       (["--mcmc", "8", "50", "--mcmc-post", "1.5"] + SOLVE, "[0, 1]"),
                       (["--mcmc", "8", "50", "--mcmc-post"] + ["0.5"] * 9 + SOLVE, "at most 8"),
                       (["--mcmc", "8", "50", "--mcmc-post", "--mcmc-lag", "-1"] + SOLVE, "L >= 0")):
        why = cli.mcmc_error(cli.build_parser().parse_args(BASE + args))
        assert why is not None and word in why, why
