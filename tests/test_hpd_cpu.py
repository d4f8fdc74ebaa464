"""Shortest (HPD) intervals without a GPU: the rule (optimize.ensemble_hpd_rule - what the device result is compared against, bit for
bit, in tests/test_gpu_hpd.py) against a restatement that walks every window in pure Python, its edge cases, a posterior piled up at
the edge of its box, the helper posterior_table, the refusals misti_ens_summary_dev makes before it looks at a context, the header
against the binding, and the parser's `--mcmc-hpd`."""
import ctypes as C
import math
import os
import re
import struct

import numpy as np
import pytest

from conftest import ROOT

E_ARG, E_LIMIT = -1, -4


def lib():
    from misti_amd import _lib
    return _lib.load()


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def key_of(v):
    """post_order_key of one double, restated on Python integers."""
    b = struct.unpack("<Q", struct.pack("<d", v))[0]
    return (~b) & (2 ** 64 - 1) if b >> 63 else b ^ (1 << 63)


def brute(samples, mass):
    """The rule by the letter: sort by the key, walk i upward.  Returns (k, i*, x_(i*), x_(i*+k-1), the sorted samples)."""
    o = sorted((float(v) for v in samples), key=key_of)
    m = len(o)
    k = 1
    while float(k) < float(m) * mass:                        # the smallest integer with double(k) >= double(m) p ...
        k += 1
    k = min(max(k, 1), m)                                    # ... clamped to 1 ... m
    best, wb = 0, o[k - 1] - o[0]
    for i in range(1, m - k + 1):
        w = o[i + k - 1] - o[i]
        if w < wb or (math.isnan(wb) and not math.isnan(w)):
            best, wb = i, w
    return k, best, o[best], o[best + k - 1], o


def check(chain, burn, masses):
    """ensemble_hpd_rule on chain[S][K][W][N] against brute(), every search, coordinate and mass; returns the rule's result."""
    from misti_amd.optimize import ensemble_hpd_rule, ensemble_posterior_rule, hpd_window
    r = ensemble_hpd_rule(chain, burn=burn, masses=masses, order=True)
    S, K, W, N = chain.shape
    m = (K - burn) * W
    assert r["hpd"].shape == (S, N, len(masses), 2) and r["hpd_at"].shape == (S, N, len(masses)) and r["hpd_at"].dtype == np.int32
    assert bits(r["order"]).tolist() == bits(ensemble_posterior_rule(chain, burn=burn)["order"]).tolist()
    for s in range(S):
        for j in range(N):
            for q, p in enumerate(masses):
                k, at, lo, hi, o = brute(chain[s, burn:, :, j].reshape(-1), p)
                assert k == hpd_window(m, p)
                assert r["hpd_at"][s, j, q] == at, (s, j, p, r["hpd_at"][s, j, q], at)
                assert bits(r["hpd"][s, j, q]).tolist() == bits([lo, hi]).tolist(), (s, j, p)
                assert bits(r["order"][s, j]).tolist() == bits(o).tolist()
    return r


MASSES = (0.95, 0.5, 1.0, 1e-9, 0.3333)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("burn", [0, 7])
def test_rule_equals_the_walk_over_every_window(seed, burn):
    rng = np.random.default_rng(seed)
    check(rng.standard_normal((2, 30, 4, 3)) * np.array([1.0, 30.0, 1e-3]) + np.array([0.5, -7.0, 0.0]), burn, MASSES)


def test_ties_resolve_to_the_lowest_window():
    """0, 1, 2, ..., 11: every window of k samples is k - 1 wide - the first wins; and two equal minima apart from each other."""
    x = np.arange(12.0)[::-1].reshape(1, 12, 1, 1).copy()
    r = check(x, 0, (0.5, 0.25, 0.95))
    assert r["hpd_at"].reshape(-1).tolist() == [0, 0, 0] and r["hpd"][0, 0, 0].tolist() == [0.0, 5.0]
    y = np.array([0.0, 1.0, 5.0, 9.0, 10.0, 20.0]).reshape(1, 6, 1, 1)                  # k = 2: widths 1 4 4 1 10 - ranks 0 and 3 tie
    r = check(y, 0, (1 / 3,))
    assert r["hpd_at"][0, 0, 0] == 0 and r["hpd"][0, 0, 0].tolist() == [0.0, 1.0]


def test_duplicates_and_both_zeros():
    rng = np.random.default_rng(4)
    dup = rng.choice(np.array([1.5, -2.25, 1e-3, 7.0, -0.5]), size=(1, 25, 4, 2))
    check(dup, 3, MASSES)
    zeros = np.where(rng.random((1, 16, 2, 1)) < 0.5, 0.0, -0.0)
    r = check(zeros, 0, (1.0, 0.5))
    assert np.signbit(r["hpd"][0, 0, 0, 0]) and not np.signbit(r["hpd"][0, 0, 0, 1])   # mass 1: from -0.0 to +0.0
    assert r["hpd_at"][0, 0, 1] == 0                                                    # every width is 0: the lowest window
    mixed = np.concatenate([zeros, rng.standard_normal((1, 16, 2, 1))], axis=1)
    check(mixed, 0, MASSES)


def test_a_nan_and_infinities_in_the_chain():
    """A NaN sample sorts last and makes its windows NaN-wide; inf - inf is NaN too: any number beats them; a marginal whose every
    window is NaN gives rank 0.  hpd copies bits - a NaN's payload survives."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((1, 20, 2, 3))
    x[0, 3, 1, 0] = np.nan
    x[0, 4, 0, 1], x[0, 9, 1, 1], x[0, 11, 0, 1] = np.inf, np.inf, -np.inf
    x[0, :, :, 2] = np.inf
    x[0, 0, 0, 2] = np.array([0x7ff8000000000abc], dtype=np.uint64).view(np.float64)[0]
    r = check(x, 0, MASSES)
    assert np.isnan(r["hpd"][0, 0, 2, 1]) and np.isfinite(r["hpd"][0, 0, 0]).all()      # mass 1 reaches the NaN, 0.95 avoids it
    assert (r["hpd_at"][0, 2] == 0).all() and r["hpd"][0, 2, 2, 0] == np.inf             # inf - inf everywhere: rank 0
    assert bits(r["hpd"][0, 2, 2, 1]) == 0x7ff8000000000abc                              # the payload, not the canonical NaN
    # coordinate 1: 38 of 40 samples cannot avoid all three infinities - every window is inf wide, a tie the lowest rank wins; half can
    assert r["hpd_at"][0, 1, 0] == 0 and r["hpd"][0, 1, 0, 0] == -np.inf and np.isfinite(r["hpd"][0, 1, 0, 1])
    assert np.isfinite(r["hpd"][0, 1, 1]).all() and r["hpd"][0, 1, 2].tolist() == [-np.inf, np.inf]


def test_mass_one_tiny_mass_and_one_sample():
    from misti_amd.optimize import ensemble_hpd_rule, hpd_window
    rng = np.random.default_rng(6)
    x = rng.standard_normal((2, 9, 4, 2))
    r = check(x, 1, (1.0, 1e-300))
    flat = x[:, 1:].reshape(2, -1, 2)
    assert (r["hpd"][:, :, 0, 0] == flat.min(axis=1)).all() and (r["hpd"][:, :, 0, 1] == flat.max(axis=1)).all() and (r["hpd_at"][:, :, 0] == 0).all()
    assert (r["hpd"][:, :, 1, 0] == r["hpd"][:, :, 1, 1]).all() and (r["hpd_at"][:, :, 1] == 0).all()      # k = 1: width 0 everywhere
    one = check(x[:, :1, :1], 0, (0.95, 1.0, 1e-9))                                                          # m = 1: the sample twice
    assert (one["hpd"] == x[:, 0, 0, :, None, None]).all() and (one["hpd_at"] == 0).all()
    assert [hpd_window(m, p) for m, p in ((1, 0.95), (20, 0.95), (20, 1.0), (20, 1e-9), (3, 1 / 3), (10, 0.3), (100, 0.07))] == [1, 19, 20, 1, 1, 3, 8]
    single = ensemble_hpd_rule(x[0], burn=1)                                                                 # one search, the default mass
    assert single["hpd"].shape == (2, 1, 2) and "order" not in single
    assert bits(single["hpd"]).tolist() == bits(ensemble_hpd_rule(x, burn=1)["hpd"][0]).tolist()
    for bad in (dict(burn=9), dict(masses=(0.0,)), dict(masses=(1.5,)), dict(masses=(float("nan"),)), dict(masses=(0.5,) * 9)):
        with pytest.raises(ValueError):
            ensemble_hpd_rule(x, **bad)


def test_a_search_depends_on_its_own_chain_alone():
    from misti_amd.optimize import ensemble_hpd_rule
    rng = np.random.default_rng(7)
    x = rng.standard_normal((3, 12, 4, 2))
    whole, alone = ensemble_hpd_rule(x, masses=MASSES, order=True), ensemble_hpd_rule(x[2:], masses=MASSES, order=True)
    for k in ("hpd", "hpd_at", "order"):
        assert whole[k][2].tobytes() == alone[k][0].tobytes()


def test_an_exponential_piled_at_the_edge_keeps_its_edge():
    """The question the interval is for: a migration rate whose posterior is an exponential piled against the lower edge of its box.
    The density falls from the edge, so the shortest 95 % interval starts AT the smallest sample; the equal-tailed interval cuts
    2.5 % off the low side by construction and so excludes the edge although it is the mode."""
    from misti_amd.optimize import ensemble_hpd_rule, ensemble_posterior_rule
    rng = np.random.default_rng(8)
    x = (0.01 + rng.exponential(0.05, size=(1, 500, 8, 1)))
    x[0, 17, 3, 0] = 0.01                                                               # a walker on the edge itself
    h = ensemble_hpd_rule(x, masses=(0.95,))
    q = ensemble_posterior_rule(x, probs=(0.025, 0.975))["quant"][0, 0]
    assert h["hpd_at"][0, 0, 0] == 0 and h["hpd"][0, 0, 0, 0] == x.min() == 0.01
    assert q[0] > 0.01 + 0.5 * 0.05 * 0.025                                              # the 2.5 % quantile of the exponential: about scale x 0.0253
    assert h["hpd"][0, 0, 0, 1] - h["hpd"][0, 0, 0, 0] < q[1] - q[0]                    # and the shortest interval is the shorter one


def test_posterior_table_carries_the_interval():
    from misti_amd.optimize import COORD_LOG, ensemble_hpd_rule, ensemble_posterior_rule, posterior_table, prior_spec
    rng = np.random.default_rng(9)
    x = rng.standard_normal((2, 60, 4, 2))
    r = dict(ensemble_posterior_rule(x), **ensemble_hpd_rule(x, masses=(0.9, 0.5)))
    t = posterior_table(r, 60, walkers=4)
    assert t["hpd"].tobytes() == r["hpd"].tobytes() and "hpd_natural" not in t
    assert "hpd" not in posterior_table(ensemble_posterior_rule(x), 60, walkers=4)
    prior = prior_spec(2, log=(1,))
    assert prior["scale"][1] == COORD_LOG
    t = posterior_table(r, 60, walkers=4, prior=prior)
    assert t["hpd_natural"].shape == (2, 2, 2, 2)
    assert (t["hpd_natural"][:, 0] == r["hpd"][:, 0]).all() and (t["hpd_natural"][:, 1] == np.exp(r["hpd"][:, 1])).all()
    one = {k: v[0] for k, v in r.items()}                                               # a single search, as the command line hands it over
    assert (posterior_table(one, 60, walkers=4, prior=prior)["hpd_natural"] == t["hpd_natural"][0]).all()


# ---- what the ABI refuses before it looks at a context ----------------------------------------------------------------------------------
def summary(S=2, K=10, W=4, N=2, chain=1, masses=(0.95,), null_masses=False, hpd=0, hpd_at=0, order=0, **kw):
    """misti_ens_summary_dev WITHOUT a context: a descriptor that passes every check ends at "ctx is NULL"."""
    from misti_amd import _lib
    pr, ms = np.array([0.025, 0.5, 0.975]), np.asarray(masses, dtype=np.float64)
    f = dict(size=C.sizeof(_lib.EnsPost), burn=0, n_prob=pr.size, probs=pr.ctypes.data, max_lag=5, c=5.0, n_mass=ms.size,
             masses=None if null_masses or not ms.size else ms.ctypes.data, hpd=hpd or None, hpd_at=hpd_at or None, order=order or None)
    f.update(kw)
    p = _lib.EnsPost(**f)
    rc = lib().misti_ens_summary_dev(None, S, K, W, N, C.c_void_p(chain) if chain else None, None, C.byref(p))
    return rc, lib().misti_last_error().decode()


@pytest.mark.parametrize("kw, code, word", [
    (dict(hpd=8, hpd_at=8, order=8), E_ARG, "ctx is NULL"),                          # the descriptor passes: only the context is missing
    (dict(masses=(1.0, 1e-300, 0.5)), E_ARG, "ctx is NULL"),
    (dict(masses=(0.5,) * 8), E_ARG, "ctx is NULL"),
    (dict(masses=()), E_ARG, "ctx is NULL"),                                         # today's call
    (dict(masses=(), order=8), E_ARG, "ctx is NULL"),                                # the sorted marginal needs no mass
    (dict(n_mass=-1), E_ARG, "n_mass"),
    (dict(n_mass=9), E_ARG, "n_mass"),
    (dict(null_masses=True), E_ARG, "masses is NULL"),
    (dict(masses=(0.5, 0.0)), E_ARG, "masses[1]"),
    (dict(masses=(1.0000001,)), E_ARG, "masses[0]"),
    (dict(masses=(-0.5,)), E_ARG, "masses[0]"),
    (dict(masses=(0.5, 0.9, float("nan"))), E_ARG, "masses[2]"),
    (dict(masses=(), hpd=8), E_ARG, "n_mass == 0"),
    (dict(masses=(), hpd_at=8), E_ARG, "n_mass == 0"),
    # the header's order: of two faults the earlier one is named - every older refusal comes before the new ones ...
    (dict(n_mass=9, c=0.0), E_ARG, "c must be"),
    (dict(n_mass=9, chain=0), E_ARG, "chain is NULL"),
    (dict(masses=(2.0,), W=257), E_LIMIT, "MISTI_ENS_MAX_WALKERS"),
    (dict(null_masses=True, K=2 ** 30), E_LIMIT, "INT32_MAX"),
    (dict(n_mass=9, burn=10), E_ARG, "burn"),
    (dict(n_mass=9, size=8), E_ARG, "size"),
    # ... and the new ones keep theirs
    (dict(n_mass=9, null_masses=True), E_ARG, "n_mass"),
    (dict(masses=(2.0,), null_masses=True), E_ARG, "masses is NULL"),
    (dict(n_mass=0, masses=(2.0,), hpd=8), E_ARG, "n_mass == 0"),
])
def test_summary_argument_checks(kw, code, word):
    rc, why = summary(**kw)
    assert rc == code and word in why, (rc, why)


# ---- header, binding, command line ---------------------------------------------------------------------------------------------------------
def test_header_binding_and_tile_agree():
    from misti_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "misti_hip.h")).read()
    assert lib().misti_abi_version() == 6 and "#define MISTI_ABI_VERSION 6" in hdr
    body = hdr[:hdr.index("} misti_ens_post_t;")].rsplit("typedef struct {", 1)[1]
    names = [n for line in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", line.strip())]
    assert names == [n for n, _ in _lib.EnsPost._fields_] and names[-6:] == ["best_at", "n_mass", "masses", "hpd", "hpd_at", "order"], names
    for field, ctype in (("n_mass", "int32_t"), ("masses", "const double*"), ("hpd", "double*"), ("hpd_at", "int32_t*"), ("order", "double*")):
        assert re.search(r"^\s+%s %s;" % (re.escape(ctype), field), body, flags=re.M), field
    assert "optimize.ensemble_hpd_rule" in hdr and "need a sort and are not offered" not in hdr and "not invariant" in hdr
    post_h = open(os.path.join(ROOT, "misti_amd", "csrc", "misti_post.h")).read()
    tile = int(re.search(r"^#define MISTI_POST_SORT_TILE (\d+)", post_h, flags=re.M).group(1))
    assert _lib.POST_SORT_TILE == tile and tile >= 256 and tile & (tile - 1) == 0
    assert 2 * tile * 8 <= 64 * 1024                     # two tiles of keys fit the LDS one workgroup may statically declare
    # the size both sides give the descriptor (the library refuses another)
    rc = lib().misti_ens_summary_dev(None, 1, 1, 4, 1, None, None, C.byref(_lib.EnsPost(size=C.sizeof(_lib.EnsPost) - 8)))
    assert rc == E_ARG and b"size" in lib().misti_last_error()


BASE = ["a.psmc", "b.psmc", "d.sfs", "20"]
SOLVE = ["--grid-solve", "--grid-st", "15", "17", "-mi", "1", "4", "16", "0.2", "1", "--box", "0", "0.01", "5"]


def test_parser_accepts_mcmc_hpd():
    from misti_amd import cli
    parse = lambda args: cli.build_parser().parse_args(BASE + args)
    a = parse(SOLVE + ["--mcmc", "8", "50", "--mcmc-post", "--mcmc-hpd"])
    assert cli.mcmc_error(a) is None and cli._mcmc_hpd_masses(a) == (0.95,)
    assert cli._mcmc_post_options(a) == dict(probs=(0.025, 0.5, 0.975), max_lag=None)          # the masses travel on their own
    a = parse(SOLVE + ["--mcmc", "8", "50", "--mcmc-post", "0.05", "0.95", "--mcmc-hpd", "0.5", "0.9", "1"])
    assert cli.mcmc_error(a) is None and cli._mcmc_hpd_masses(a) == (0.5, 0.9, 1.0) and cli._mcmc_post_options(a)["probs"] == (0.05, 0.95)
    a = parse(SOLVE + ["--mcmc", "8", "50", "--mcmc-post"])
    assert a.mcmc_hpd is None and cli.mcmc_error(a) is None and cli._mcmc_hpd_masses(a) is None
    for args, word in ((["--mcmc-hpd"], "give --mcmc W STEPS"),
                       (["--mcmc", "8", "50", "--mcmc-hpd"] + SOLVE, "give --mcmc-post"),
                       (["--mcmc", "8", "50", "--mcmc-post", "--mcmc-hpd", "0"] + SOLVE, "(0, 1]"),
                       (["--mcmc", "8", "50", "--mcmc-post", "--mcmc-hpd", "1.5"] + SOLVE, "(0, 1]"),
                       (["--mcmc", "8", "50", "--mcmc-post", "--mcmc-hpd", "nan"] + SOLVE, "(0, 1]"),
                       (["--mcmc", "8", "50", "--mcmc-post", "--mcmc-hpd"] + ["0.5"] * 9 + SOLVE, "at most 8")):
        why = cli.mcmc_error(parse(args))
        assert why is not None and "--mcmc-hpd" in why and word in why, why
    assert "--mcmc-hpd" in cli.__doc__
