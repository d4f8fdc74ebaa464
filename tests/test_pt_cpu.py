"""Tempered ensemble MCMC without a GPU: the rule (optimize.tempered_rule - what the device result is compared against in
tests/test_gpu_pt.py) against optimize.ensemble_rule at one rung and against a scalar restatement of a rung at the stated blocks,
misti_pt_swap - the very function the swap kernel calls - against the rule's decision, the bookkeeping of the swap rounds counted by
hand, the thermodynamic-integration reduction on exact binary fractions, the two-well target a single-temperature ensemble never
crosses, and what misti_tempered_sample and the command line refuse before a context or a file is looked at."""
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


def bits(v):
    return np.asarray(v, dtype=np.float64).tobytes()


def normal(X, s):
    return 0.5 * (np.asarray(X) ** 2).sum(axis=1)


def flat(X, s):
    return np.zeros(len(X))


def start(S, L, W, N, lo, hi, seed=5):
    u = np.random.default_rng(seed).random((S, L, W, N))
    lo, hi = np.broadcast_to(lo, (S, N)), np.broadcast_to(hi, (S, N))
    return lo[:, None, None, :] + u * (hi - lo)[:, None, None, :]


# ---- one rung is the ensemble sampler -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("swap_every", [0, 1, 3])
def test_one_rung_equals_ensemble_rule_bit_for_bit(swap_every):
    from misti_amd.optimize import ensemble_rule, tempered_rule
    lo = np.array([[-3.0, -2.0, 0.25], [-1.0, 0.5, -4.0]])            # two searches, two boxes; search 1 holds coordinate 1 fixed
    hi = np.array([[3.0, 2.0, 1.5], [2.0, 0.5, 4.0]])
    init = start(2, 1, 6, 3, lo, hi)
    T = np.array([[1.5], [0.75]])
    e = ensemble_rule(normal, init[:, 0], lo, hi, 7, thin=2, temperature=T[:, 0], seed=11, ids=[4, 9])
    r = tempered_rule(normal, init, lo, hi, T, 7, thin=2, swap_every=swap_every, burn=1, seed=11, ids=[4, 9])
    for k in ("chain", "chain_llh", "accepted", "last", "last_llh"):
        assert bits(r[k]) == bits(e[k]) and r[k].size == e[k].size, k
    assert r["n_points"] == e["n_points"] and e["accepted"].sum() > 0
    assert r["chain_llh"].shape == (2, 1, 3, 6) and r["swap_proposed"].shape == (2, 0) and bits(r["logz"]) == bits([0.0, 0.0])


# ---- the swap function ----------------------------------------------------------------------------------------------------------------
def c_swap(T_lo, T_hi, lo, hi, u):
    a = C.c_int32(-7)
    assert lib().misti_pt_swap(float(T_lo), float(T_hi), float(lo), float(hi), float(u), C.byref(a)) == 0, lib().misti_last_error()
    return a.value


def test_the_library_swap_equals_the_rules_decision():
    from misti_amd.optimize import pt_swap_decision
    rng = np.random.default_rng(3)
    n = 3000
    T_lo = 10.0 ** rng.uniform(-3, 3, n)
    T_hi = T_lo * (1.0 + 10.0 ** rng.uniform(-6, 3, n))
    lo, hi = rng.normal(-1e3, 40.0, n), rng.normal(-1e3, 40.0, n)
    u = rng.random(n)
    # e beyond +-746 either way, equal values, u = 0 (also against an exponential of 0), walkers without a value
    lo[:200], hi[:200], T_lo[:200], T_hi[:200] = -5e3, -1e3, 1.0, 4.0
    lo[200:400], hi[200:400], T_lo[200:400], T_hi[200:400] = -1e3, -5e3, 1.0, 4.0
    hi[400:600] = lo[400:600]
    u[::7] = 0.0
    u[600:650] = 0.0
    lo[600:650], hi[600:650], T_lo[600:650], T_hi[600:650] = -1e3, -9e3, 0.5, 8.0
    lo[650:700], hi[700:750] = -np.inf, np.nan
    lo[750:760], hi[750:760] = np.inf, -np.inf
    want = pt_swap_decision(T_lo, T_hi, lo, hi, u)
    got = np.array([c_swap(*t) for t in zip(T_lo, T_hi, lo, hi, u)])
    assert (got == want).all()
    assert want[:200].all() and not want[200:400].any()             # exp(+3000) = inf, exp(-3000) = 0
    assert (want[400:600] == (u[400:600] < 1.0)).all()               # equal values: e = 0
    assert not want[600:650].any()                                   # u = 0 against 0
    assert want[::7][100:].sum() > 0                                 # u = 0 against a positive exponential
    assert not want[650:760].any()                                   # a walker without a value never swaps
    assert 0.2 < want[760:].mean() < 0.9


def test_swap_argument_checks():
    a = C.c_int32(-7)
    for args, word in (((1.0, 2.0, 0.0, 0.0, 0.5, None), "NULL"), ((0.0, 2.0, 0.0, 0.0, 0.5, C.byref(a)), "finite and positive"),
                       ((1.0, float("inf"), 0.0, 0.0, 0.5, C.byref(a)), "finite and positive"), ((2.0, 2.0, 0.0, 0.0, 0.5, C.byref(a)), "below"),
                       ((1.0, 2.0, 0.0, 0.0, 1.0, C.byref(a)), "[0, 1)"), ((1.0, 2.0, 0.0, 0.0, float("nan"), C.byref(a)), "[0, 1)")):
        assert lib().misti_pt_swap(*args) == E_ARG and word.encode() in lib().misti_last_error(), args
    assert a.value == -7


# ---- the bookkeeping ------------------------------------------------------------------------------------------------------------------
def scalar_rung(fun, x, lo, hi, T, seed, id_, steps, a=2.0):
    """One ensemble moved by the stretch move, walker by walker, with the draws of the given step indices (optimize.ens_draws)."""
    from misti_amd.optimize import ens_decision, ens_draws
    x = np.array(x, dtype=float)
    W, N = x.shape
    H = W // 2
    f = -fun(x, None)
    d = int((lo != hi).sum()) - 1
    for step in steps:
        for half in (0, 1):
            old = x.copy()
            for m in range(H):
                i = half * H + m
                dr = ens_draws(seed, id_, step, i, W)
                j = (1 - half) * H + dr["partner"]
                s = (a - 1.0) * dr["u_z"] + 1.0
                z = (s * s) / a
                y = np.where(lo == hi, lo, old[j] + z * (old[i] - old[j]))
                if ((y >= lo) & (y <= hi)).all():
                    new = -float(fun(y[None], None)[0])
                    if ens_decision(z, d, f[i], new, T, dr["u_acc"]):
                        x[i], f[i] = y, new
    return x, f


def test_walker_i_of_rung_l_of_step_t_owns_block_tL_plus_l_times_W_plus_i():
    from misti_amd.optimize import ensemble_rule, tempered_rule
    lo, hi = np.array([-3.0, -3.0]), np.array([3.0, 3.0])
    L, W = 3, 4
    init = start(1, L, W, 2, lo, hi)
    T = np.array([1.0, 2.0, 8.0])
    r = tempered_rule(normal, init, lo, hi, T, 2, swap_every=0, seed=7, ids=[13])
    for l in range(L):
        x, f = scalar_rung(normal, init[0, l], lo, hi, T[l], 7, 13, [1 * L + l, 2 * L + l])
        assert bits(r["last"][0, l]) == bits(x) and bits(r["last_llh"][0, l]) == bits(f), l
    assert r["swap_proposed"].sum() == 0 and r["accepted"].sum() > 0
    # another L: another stream for every rung - except where the blocks coincide: step t of rung 0 of L rungs is step t L of one rung
    one = ensemble_rule(normal, init[:, 0], lo, hi, 3, seed=7, ids=[13])
    first = tempered_rule(normal, init, lo, hi, T, 1, swap_every=0, seed=7, ids=[13])
    assert bits(first["last"][0, 0]) != bits(one["chain"][0, 0])
    x3, _ = scalar_rung(normal, init[0, 0], lo, hi, 1.0, 7, 13, [3])
    x1, _ = scalar_rung(normal, init[0, 0], lo, hi, 1.0, 7, 13, [1])
    assert bits(first["last"][0, 0]) == bits(x3) and bits(one["chain"][0, 0]) == bits(x1)


def test_the_pair_parity_alternates_and_the_counters_are_as_counted_by_hand():
    from misti_amd.optimize import tempered_rule
    lo, hi = np.array([0.0, 0.0]), np.array([1.0, 1.0])
    # a flat objective: every value is 0, e = 0, ens_exp(0) = 1 > u - every pair that is treated trades
    r = tempered_rule(flat, start(2, 2, 4, 2, lo, hi), lo, hi, [1.0, 2.0], 5, swap_every=1)
    assert (r["swap_proposed"] == 4 * 3).all() and (r["swap_accepted"] == 4 * 3).all()      # L = 2: rounds 1, 3, 5 treat (0, 1); 2, 4 none
    r = tempered_rule(flat, start(1, 2, 4, 2, lo, hi), lo, hi, [1.0, 2.0], 5, swap_every=2)
    assert r["swap_proposed"].tolist() == [[4]]                                              # rounds at t = 2 (n = 1) and t = 4 (n = 2: none)
    init = start(1, 3, 4, 2, lo, hi)
    r = tempered_rule(flat, init, lo, hi, [1.0, 2.0, 4.0], 4, swap_every=1, thin=2)
    assert r["swap_proposed"].tolist() == [[8, 8]] and r["swap_accepted"].tolist() == [[8, 8]]   # rounds 1, 3: pair (0, 1); 2, 4: (1, 2)
    assert r["swap_proposed"].dtype == r["swap_accepted"].dtype == np.int32 and r["accepted"].shape == (1, 3, 4)
    # the chain row of a kept step is the state AFTER its swap round: step 4 is kept and swapped
    assert bits(r["chain"][0, -1]) == bits(r["last"][0, 0]) and bits(r["chain_llh"][0, :, -1]) == bits(r["last_llh"][0])
    none = tempered_rule(flat, init, lo, hi, [1.0, 2.0, 4.0], 4, swap_every=0, thin=2)
    assert none["swap_proposed"].sum() == 0 and bits(none["chain"][0, -1]) != bits(r["chain"][0, -1])
    # a rung without a value (rung 2 sits where the objective has none, and the stretch keeps it there): its pair is never counted
    wall = lambda X, s: np.where(np.asarray(X)[:, 0] > 0.5, np.inf, 0.0)
    init[0, :2, :, 0] *= 0.4
    init[0, 2, :, 0] = 0.9 + 0.1 * init[0, 2, :, 0]
    r = tempered_rule(wall, init, lo, hi, [1.0, 2.0, 4.0], 4, swap_every=1)
    assert np.isneginf(r["last_llh"][0, 2]).all() and r["swap_proposed"].tolist() == [[8, 0]] and r["swap_accepted"].tolist() == [[8, 0]]


def test_a_fit_alone_equals_the_fit_among_others():
    from misti_amd.optimize import tempered_rule
    lo = np.array([[-3.0, -3.0], [-1.0, -2.0]])
    hi = np.array([[3.0, 3.0], [4.0, 2.0]])
    init = start(2, 3, 4, 2, lo, hi)
    T = np.array([[1.0, 3.0, 9.0], [0.5, 1.0, 6.0]])
    both = tempered_rule(normal, init, lo, hi, T, 6, thin=2, burn=1, seed=2, ids=[5, 3])
    alone = tempered_rule(normal, init[1:], lo[1], hi[1], T[1], 6, thin=2, burn=1, seed=2, ids=[3])
    for k in ("chain", "chain_llh", "accepted", "swap_proposed", "swap_accepted", "last", "last_llh", "rung_llh", "logz"):
        assert np.asarray(both[k][1:]).tobytes() == np.asarray(alone[k]).tobytes(), k
    assert 0 < both["swap_accepted"].sum() < both["swap_proposed"].sum()


# ---- the reduction --------------------------------------------------------------------------------------------------------------------
def test_the_reduction_on_exact_binary_fractions():
    from misti_amd.optimize import tempered_reduction
    E = np.array([-3.5, -6.25, -10.0, -40.5])
    T = np.array([1.0, 2.0, 8.0, 64.0])
    llh = np.broadcast_to(E[None, :, None, None], (2, 4, 70, 4)).copy()            # 70 kept steps: more than lsum's 64 partials
    llh[:, :, :3] = 1e300                                                           # the burn is respected
    rung, logz = tempered_reduction(llh, T, burn=3)
    assert bits(rung) == bits(np.broadcast_to(E, (2, 4)))
    want = 0.0 + (0.5 * (-3.5 - 6.25)) * (1.0 - 0.5) + (0.5 * (-6.25 - 10.0)) * (0.5 - 0.125) + (0.5 * (-10.0 - 40.5)) * (0.125 - 0.015625)
    assert bits(logz) == bits([want, want]) and want == -8.24609375
    llh[1, 2, 40, 1] = -np.inf
    rung, logz = tempered_reduction(llh, T, burn=3)
    assert np.isneginf(rung[1, 2]) and np.isneginf(logz[1]) and bits(rung[0]) == bits(E) and bits(rung[1, [0, 1, 3]]) == bits(E[[0, 1, 3]])
    llh[1, 1, 5, 0] = np.inf                                                        # +inf beside -inf: a NaN, stored as the canonical quiet NaN
    rung, logz = tempered_reduction(llh, T, burn=3)
    assert bits(logz[1]) == bits(np.nan) == bytes.fromhex("000000000000f87f")
    one, z1 = tempered_reduction(llh[0, :1], T[:1], burn=69)
    assert bits(one) == bits([-3.5]) and bits(z1) == bits(0.0)                      # L = 1: +0.0
    with pytest.raises(ValueError):
        tempered_reduction(llh, T, burn=70)


def test_temperature_ladder():
    from misti_amd.optimize import temperature_ladder
    assert temperature_ladder(2.5, 7.0, 1).tolist() == [2.5] and temperature_ladder(2.5, float("nan"), 1).tolist() == [2.5]
    t = temperature_ladder(0.5, 256.0, 5)
    assert np.allclose(t, [0.5, 2.0, 8.0, 32.0, 128.0], rtol=1e-14) and t[0] == 0.5 and (np.diff(t) > 0).all()
    for bad in ((1.0, 1.0, 3), (1.0, float("inf"), 2), (0.0, 4.0, 2), (1.0, 4.0, 0), (1.0, 4.0, 65)):
        with pytest.raises(ValueError):
            temperature_ladder(*bad)


# ---- two wells ------------------------------------------------------------------------------------------------------------------------
def two_wells(X, s):
    X = np.asarray(X)
    a = -0.5 * ((X - 2.0) ** 2).sum(axis=1) / 0.25 ** 2
    b = -0.5 * ((X + 2.0) ** 2).sum(axis=1) / 0.25 ** 2
    return -np.logaddexp(a, b)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_ladder_crosses_between_two_wells_and_one_temperature_does_not(seed):
    """Two Gaussian wells, sigma = 0.25, at +-(2, 2) in [-6, 6]^2; 8 walkers around (-2, -2) with spread 0.02 (ensemble_start, ids
    100 + l per rung), 400 steps.  Observed: ensemble_rule puts 0.000 of its samples at x0 > 0 on seeds 0, 1, 2; the cold rung of the
    ladder 1, 4, 16, 64, 256 puts 0.2925, 0.4625, 0.4575 of the second half of its run there, with 36 - 68 % of the swaps accepted
    per pair.  The condition is zero against not zero."""
    from misti_amd.optimize import ensemble_rule, ensemble_start, tempered_rule
    lo, hi = [-6.0, -6.0], [6.0, 6.0]
    init = np.stack([ensemble_start([-2.0, -2.0], lo, hi, 8, spread=0.02, seed=seed, id_=100 + l) for l in range(5)])[None]
    e = ensemble_rule(two_wells, init[:, 0], lo, hi, 400, seed=seed)
    assert (e["chain"][..., 0] > 0).sum() == 0
    r = tempered_rule(two_wells, init, lo, hi, [1.0, 4.0, 16.0, 64.0, 256.0], 400, swap_every=1, burn=200, seed=seed)
    share = float((r["chain"][0, 200:, :, 0] > 0).mean())
    print("seed", seed, "share beyond x0 > 0:", share, "swaps:", r["swap_accepted"] / r["swap_proposed"], "logz:", r["logz"])
    assert share > 0 and (r["swap_accepted"] > 0).all() and (r["swap_proposed"] >= r["swap_accepted"]).all()
    assert np.isfinite(r["logz"]).all() and (np.diff(r["rung_llh"][0]) < 0).all()      # the hotter, the lower the mean llh


def test_the_rule_refuses_what_the_library_refuses():
    from misti_amd.optimize import tempered_rule
    lo, hi = np.zeros(2), np.ones(2)
    x = start(1, 2, 4, 2, lo, hi)
    for kw in (dict(ladder=[2.0, 1.0]), dict(ladder=[1.0, 1.0]), dict(ladder=[0.0, 1.0]), dict(ladder=[1.0, float("inf")]), dict(swap_every=-1),
               dict(burn=5), dict(burn=-1), dict(thin=0), dict(a=1.0)):
        args = dict(ladder=[1.0, 2.0], n_step=5)
        args.update(kw)
        with pytest.raises(ValueError):
            tempered_rule(flat, x, lo, hi, **args)
    with pytest.raises(ValueError):
        tempered_rule(flat, np.zeros((1, 65, 4, 2)), lo, hi, np.arange(1.0, 66.0), 1)
    assert tempered_rule(flat, x, lo, hi, [1.0, 2.0], 0, burn=9)["chain"].shape == (1, 0, 4, 2)      # no kept step: burn is not looked at


# ---- what the ABI refuses before it looks at a context ----------------------------------------------------------------------------------
def pt_sample(ctx=None, size=None, null=(), post=None, **kw):
    """misti_tempered_sample WITHOUT a context: every check below comes before the context is looked at, and a descriptor that passes
    them ends at "ctx is NULL".  No output is ever written."""
    from misti_amd import _lib
    S, W, L = kw.pop("n_start", 2), kw.get("walkers", 6), kw.get("n_rung", 3)
    n, w, l = max(S, 1), max(W, 1), min(max(L, 1), 70)
    a = dict(init=np.full((n, l, w, 2), 0.5), rows=np.zeros(n, dtype=np.int32), jsfs=np.ones((3, 8)), box_lo=np.zeros((1, 2)), box_hi=np.ones((1, 2)),
             ladder=np.tile(2.0 ** np.arange(l), (n, 1)), last=np.zeros((n, l, w, 2)), last_llh=np.zeros((n, l, w)), rung_llh=np.zeros((n, l)),
             logz=np.zeros(n), split_times=np.full(n, 5.0))
    for k in list(kw):
        if k in a:
            a[k] = np.ascontiguousarray(kw.pop(k), dtype=a[k].dtype)
    f = dict(size=C.sizeof(_lib.PtSample) if size is None else size, split=_lib.SPLIT_PER_START, n_start=S, n_rep=3, n_box=1, walkers=W, n_rung=L, n_ladder=1,
             n_step=6, thin=2, swap_every=1, burn=0, a=2.0, seed=0)
    f.update(kw)
    q = _lib.PtSample(**f, **{k: (None if k in null else v.ctypes.data) for k, v in a.items()})
    rc = lib().misti_tempered_sample(ctx, C.byref(q), C.byref(post) if post is not None else None)
    assert not any(a[k].any() for k in ("last", "last_llh", "rung_llh", "logz"))
    return rc, lib().misti_last_error().decode()


@pytest.mark.parametrize("kw, code, word", [
    (dict(), E_ARG, "ctx is NULL"),                                                 # the descriptor passes: only the context is missing
    (dict(n_start=0, n_box=0), E_ARG, "ctx is NULL"),
    (dict(n_step=0, burn=7), E_ARG, "ctx is NULL"),                                 # no kept step: burn is not looked at
    (dict(n_rung=1), E_ARG, "ctx is NULL"),
    (dict(n_rung=64), E_ARG, "ctx is NULL"),
    (dict(swap_every=0), E_ARG, "ctx is NULL"),
    (dict(n_ladder=2), E_ARG, "ctx is NULL"),
    (dict(size=8), E_ARG, "size"),
    (dict(split=0), E_ARG, "split mode"),
    (dict(n_start=-1), E_ARG, "negative"),
    (dict(null=("init",)), E_ARG, "NULL"),
    (dict(null=("ladder",)), E_ARG, "NULL"),
    (dict(null=("rung_llh",)), E_ARG, "NULL"),
    (dict(null=("logz",)), E_ARG, "NULL"),
    (dict(null=("split_times",)), E_ARG, "split_times"),
    (dict(null=("split_times",), split=2), E_ARG, "ctx is NULL"),
    (dict(n_rep=0), E_ARG, "n_rep"),
    (dict(walkers=5), E_ARG, "walkers must be even"),
    (dict(walkers=258), E_LIMIT, "MISTI_ENS_MAX_WALKERS"),
    (dict(n_step=-1), E_ARG, "n_step"),
    (dict(thin=0), E_ARG, "thin"),
    (dict(a=1.0), E_ARG, "a must be"),
    (dict(n_rung=0), E_ARG, "n_rung must be >= 1"),
    (dict(n_rung=65), E_LIMIT, "MISTI_PT_MAX_RUNGS"),
    (dict(n_ladder=3), E_ARG, "n_ladder"),
    (dict(ladder=[[0.0, 1.0, 2.0], [1.0, 2.0, 3.0]]), E_ARG, "ladder[0][0]"),
    (dict(ladder=[[1.0, float("inf"), 2.0], [1.0, 2.0, 3.0]]), E_ARG, "ladder[0][1]"),
    (dict(ladder=[[1.0, 2.0, 2.0], [1.0, 2.0, 3.0]]), E_ARG, "ladder[0][2]"),
    (dict(n_ladder=2, ladder=[[1.0, 2.0, 3.0], [1.0, 3.0, 2.5]]), E_ARG, "ladder[1][2]"),
    (dict(n_ladder=2, ladder=[[1.0, 2.0, 3.0], [1.0, float("nan"), 2.5]]), E_ARG, "ladder[1][1]"),
    (dict(swap_every=-1), E_ARG, "swap_every"),
    (dict(burn=3), E_ARG, "burn"),
    (dict(burn=-1), E_ARG, "burn"),
    (dict(n_box=3), E_ARG, "n_box"),
    (dict(rows=[0, 3]), E_ARG, "rows[1]"),
    (dict(split_times=[5.0, float("inf")]), E_ARG, "split_times[1]"),
    # the header's order: of two faults the earlier one is named
    (dict(a=0.5, n_rung=0), E_ARG, "a must be"),
    (dict(n_rung=0, n_ladder=3), E_ARG, "n_rung"),
    (dict(n_rung=65, n_ladder=3), E_LIMIT, "MISTI_PT_MAX_RUNGS"),
    (dict(n_ladder=3, swap_every=-1), E_ARG, "n_ladder"),
    (dict(ladder=[[1.0, 1.0, 2.0], [1.0, 2.0, 3.0]], swap_every=-1), E_ARG, "ladder[0][1]"),
    (dict(swap_every=-1, burn=9), E_ARG, "swap_every"),
    (dict(burn=9, n_box=3), E_ARG, "burn"),
    (dict(burn=9, rows=[0, 9]), E_ARG, "burn"),
])
def test_tempered_sample_argument_checks(kw, code, word):
    rc, why = pt_sample(**kw)
    assert rc == code and word in why, (rc, why)


def test_a_null_or_wrong_size_descriptor_is_refused():
    from misti_amd import _lib
    assert lib().misti_tempered_sample(None, None, None) == E_ARG and b"NULL" in lib().misti_last_error()
    rc, why = pt_sample(post=_lib.EnsPost(size=4))
    assert rc == E_ARG and "summary descriptor's size" in why
    rc, why = pt_sample(post=_lib.EnsPost(size=4), split=0)                         # the sizes come before the split mode
    assert rc == E_ARG and "summary descriptor's size" in why


# ---- header, binding --------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_entry_points():
    from misti_amd import _lib, build, optimize
    hdr = open(os.path.join(ROOT, "include", "misti_hip.h")).read()
    assert re.search(r"^int misti_tempered_sample\(misti_ctx\* ctx, const misti_pt_t\* sampler, const misti_ens_post_t\* post", hdr, flags=re.M)
    assert re.search(r"^int misti_pt_swap\(", hdr, flags=re.M)
    assert "misti_tempered_sample" in _lib.SYMBOLS and "misti_pt_swap" in _lib.SYMBOLS
    flat_ = " ".join(hdr.split()).replace("* ", "")
    assert "optimize.tempered_rule" in hdr and "(t L + l) W + i" in flat_ and "p = (n - 1) & 1" in flat_ and "NOT included" in flat_
    assert "#define MISTI_ABI_VERSION 6" in hdr and lib().misti_abi_version() == 6
    assert "#define MISTI_PT_MAX_RUNGS 64" in hdr and _lib.PT_MAX_RUNGS == optimize.PT_MAX_RUNGS == 64
    assert "misti_pt.hip" in build.SOURCES and "misti_pt.h" in build.HEADERS
    body = hdr[:hdr.index("} misti_pt_t;")].rsplit("typedef struct {", 1)[1]
    names = [n for line in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", line.strip())]
    assert names == [n for n, _ in _lib.PtSample._fields_], names
    assert C.sizeof(_lib.PtSample) == 240 and C.sizeof(_lib.EnsSample) == 192       # the new descriptor; the existing one as it was


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
BASE = ["a.psmc", "b.psmc", "d.sfs", "20"]
SOLVE = ["--grid-solve", "--grid-st", "15", "17", "-mi", "1", "4", "16", "0.2", "1", "--box", "0", "0.01", "5"]


def test_parser_accepts_the_ladder():
    from misti_amd import cli
    a = cli.build_parser().parse_args(BASE + SOLVE + ["--mcmc", "8", "50", "--mcmc-ladder", "5", "256", "--mcmc-swap", "2", "--mcmc-temp", "1.5"])
    assert cli.mcmc_error(a) is None and cli._mcmc_ladder_options(a) == dict(ladder=(5, 256.0), swap_every=2)
    a = cli.build_parser().parse_args(BASE + SOLVE + ["--mcmc", "8", "50", "--mcmc-ladder", "1", "1"])
    assert cli.mcmc_error(a) is None and cli._mcmc_ladder_options(a) == dict(ladder=(1, 1.0), swap_every=1)      # one rung: the ratio is not looked at
    a = cli.build_parser().parse_args(BASE + SOLVE + ["--mcmc", "8", "50"])
    assert cli._mcmc_ladder_options(a) == dict(ladder=None, swap_every=1)
    assert "--mcmc-ladder L RATIO" in cli.__doc__


@pytest.mark.parametrize("args, word", [
    (["--mcmc-ladder", "3", "16"], "give --mcmc W STEPS"),
    (["--mcmc-swap", "2"], "give --mcmc W STEPS"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-swap", "2"], "give --mcmc-ladder"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-ladder", "3", "16", "--mcmc-swap", "-1"], "E >= 0"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-ladder", "0", "16"], "1 <= L <= 64"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-ladder", "65", "16"], "1 <= L <= 64"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-ladder", "3", "1"], "finite and > 1"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-ladder", "3", "0.5"], "finite and > 1"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-ladder", "3", "inf"], "finite and > 1"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-ladder", "3", "nan"], "finite and > 1"),
    (["--mcmc", "8", "5"] + SOLVE + ["--mcmc-ladder", "three", "16"], "an integer and a number"),
])
def test_mcmc_error_names_the_reason(args, word):
    from misti_amd import cli
    why = cli.mcmc_error(cli.build_parser().parse_args(BASE + args))
    assert why is not None and word in why, why


def test_the_ladder_is_refused_before_a_file_is_read(capsys):
    from misti_amd import cli
    assert cli.main(["no.psmc", "no.psmc", "no.sfs", "20", "--mcmc", "8", "5", "--mcmc-ladder", "3", "1"] + SOLVE) == 2      # (the files do not exist)
    assert "--mcmc-ladder" in capsys.readouterr().err
