"""The population kernels beyond one workgroup - misti_de.hip, misti_ens.hip, misti_pt.hip and the prior path of misti_prior.h - against
their NumPy rules (optimize.differential_evolution_rule, ensemble_rule, ensemble_prior_rule, tempered_rule, tempered_prior_rule) driven by
Engine.evaluate as their objective, bit for bit, over every field the method's own module compares (tests/test_gpu_de.py, test_gpu_ens.py,
test_gpu_pt.py, test_gpu_prior.py; their helpers are used here by import), n_points included.

Those modules stay inside one workgroup: at most 4 searches, 7 members, 8 walkers, 3 rungs, 3 coordinates.  The shapes here are the
smallest that reach each edge beyond it, at 2 - 5 generations or steps:

  1  DE, 100 searches x 7 members: 36 searches per selection workgroup, so three of them and 700 trial threads; the searches stop at
     different generations (the compaction of the live searches over several workgroups, the host's stale bound -> put_none)
  2  DE, 85 / 128 / 129 / 255 / 256 members: idle tail threads of the selection workgroup, one search per workgroup, a full workgroup
  3  DE, N = 16 (MISTI_MAX_PARAMS: a member's last uniform is the last word of its fifth block) and N = 15 + the fitted split
  4  ensemble, 70 searches x 8 walkers: 280 proposal threads, 560 initial ones - t / H, s W + i, row W + w past one workgroup; with a
     prior per search as well
  5  ensemble, W = 256 (MISTI_ENS_MAX_WALKERS): one proposal workgroup per two searches, one and a half for three
  6  ensemble, N = 16 at 34 walkers
  7  tempered, L = 64 (MISTI_PT_MAX_RUNGS): even and odd swap rounds of 32 and 31 pairs, 256 and 384 swap threads, E[64] of the reduction
  8  tempered, 50 fits x 3 rungs x 6 walkers: 300 swap threads, a kept row rewritten by a second workgroup; with one prior for all
  9  case 8 with post=: the summaries and the shortest intervals on the cold chain.  The plain sampler's half at W = 256 is left out:
     tests/test_gpu_post.py holds the summary kernels at W = 256 already

The small model is the two-rate model of tests/test_gpu_de.py on its 16-interval grid, with its table, the rows and the splits going
round the searches.  The 16-coordinate model has the structure of tests/test_gpu_limits.py::test_largest_model_structure (8 bands + 8
pulses on the 32-interval grid of PSMC files of 16 and 17 intervals) in the box PAR x (1 -+ 0.2) around that test's `par`, with a split
per search from {17, 17.5, 17.75, 18, 19}: measured on the device, this model has a value at every point of that box for splits from
16.5 to 19 and at none from 19.5 on (the lambda correction fails, status 2 - that test's own split, 20, included), so at these splits
every final value of the rule's side is finite.  Its N = 15 variant holds the last pulse's fraction at PAR[15] and fits the split in
[16.5, 19] instead.

What keeps a case from passing vacuously is asserted on the RULE's output.  The rule's side of a case is computed once."""
import numpy as np
import pytest

import test_gpu_de as de
import test_gpu_ens as ens
import test_gpu_pt as pt
from test_gpu_de import grid, same_bits, two_rates          # grid, two_rates: the small model's fixtures
from test_gpu_limits import grid as psmc_grid

pytestmark = pytest.mark.gpu

POST_OLD = ("mean", "cov", "quant", "tau", "window", "best_llh", "best_x", "best_at")
POST_NEW = ("hpd", "hpd_at", "order")
ENS = ens.FIELDS
PT = pt.FIELDS
LOG, NORMAL, EXPONENTIAL = 1, 1, 2                  # MISTI_COORD_LOG; MISTI_PRIOR_NORMAL, MISTI_PRIOR_EXPONENTIAL


def going_round(S):
    """rows[S], splits[S] of the small model: the table's three rows and the four splits of tests/test_gpu_de.py going round."""
    s = np.arange(S)
    return (s % 3).astype(np.int32), de.SPLITS[s % 4]


def held(dev, ref, fields, where):
    for k in fields:
        want = np.asarray(ref[k])
        got = np.asarray(dev[k], dtype=want.dtype)
        if not same_bits(got, want):
            bad = [s for s in range(min(len(got), len(want))) if not same_bits(got[s], want[s])]
            print(where, k, "differs in", len(bad), "of", len(want), "searches:", bad[:12], "device", got[bad[0]].ravel()[:6], "rule", want[bad[0]].ravel()[:6])
        assert same_bits(got, want), (where, k)
    assert dev["n_points"] == ref["n_points"], where


def same_per_search(part, whole, searches, fields, where):
    """Search searches[j] of `whole` is search j of `part`, bit for bit."""
    for k in fields:
        for j, s in enumerate(searches):
            assert same_bits(part[k][j], whole[k][s]), (where, k, int(s))


def moved(ref, skip=()):
    """DE: the final population of every search (but the refused ones) holds more than three distinct finite values."""
    for s, f in enumerate(ref["population_llh"]):
        if s not in skip:
            assert len({float(v) for v in f[np.isfinite(f)]}) > 3, (s, f)


def decided_both_ways(ref):
    """The samplers: proposals were accepted and proposals were refused."""
    assert 0 < int(ref["accepted"].sum()) < ref["n_points"], (int(ref["accepted"].sum()), ref["n_points"])


# ---- the 16-coordinate model ------------------------------------------------------------------------------------------------------------
PAR = np.array([0.05 + 0.01 * k for k in range(8)] + [0.02 + 0.01 * k for k in range(8)])
BANDS = [(k % 2, 2 * (k // 2), 2 * (k // 2) + 2, 0.0, k) for k in range(8)]
WIDE_SPLITS = np.array([18.0, 17.75, 19.0, 17.5, 17.0])
SPLIT_BOX = (16.5, 19.0)
BOX_REL = 0.2


def wide_engine(n_param):
    from misti_amd.engine import Engine
    inp = psmc_grid(16, 17)
    pulses = [((k + 1) % 2, 9 + k, 0.0, 8 + k) if 8 + k < n_param else ((k + 1) % 2, 9 + k, float(PAR[8 + k]), -1) for k in range(8)]
    return Engine(inp.times, inp.lambdas, BANDS, pulses, n_param=n_param, cpfit=True, smooth=True)


@pytest.fixture(scope="module")
def wide():
    e = wide_engine(16)
    yield e
    e.close()


@pytest.fixture(scope="module")
def wide15():
    e = wide_engine(15)
    yield e
    e.close()


def wide_problem(S, fit_split):
    """rows, splits (None: fitted), the centre [S][16] and the box PAR x (1 -+ BOX_REL) per search (SPLIT_BOX for a fitted split)."""
    s = np.arange(S)
    rows, splits = (s % 3).astype(np.int32), WIDE_SPLITS[s % 5]
    if not fit_split:
        return rows, splits, np.tile(PAR, (S, 1)), np.tile(PAR * (1.0 - BOX_REL), (S, 1)), np.tile(PAR * (1.0 + BOX_REL), (S, 1))
    x = np.column_stack([np.tile(PAR[:15], (S, 1)), splits])
    lo = np.column_stack([np.tile(PAR[:15] * (1.0 - BOX_REL), (S, 1)), np.full(S, SPLIT_BOX[0])])
    hi = np.column_stack([np.tile(PAR[:15] * (1.0 + BOX_REL), (S, 1)), np.full(S, SPLIT_BOX[1])])
    return rows, None, x, lo, hi


def mostly_finite(values, where):
    share = float(np.isfinite(values).mean())
    print(where, "share of final values that are finite on the rule's side:", share)
    assert share >= 0.75, (where, share)


# ---- 1. DE: searches over several workgroups, stopping at different generations -------------------------------------------------------
DE_MANY = dict(pop=7, maxiter=5, tol=1e-6, atol=0.0, F=(0.5, 1.0), CR=0.7, seed=3)
S_DE = 100


@pytest.fixture(scope="module")
def de_many(two_rates):
    """Around (0.2, 0.1) a box per search whose share of the ordinary box [0.01, 1]^2 runs geometrically from 1e-9 (the hair of
    tests/test_gpu_de.py: its values agree to far less than tol |mean|, it stops after the initial population) to 1, in an order that
    mixes the widths over the workgroups; every tenth search has the all-negative box the engine refuses; every seventh starts outside
    its box."""
    s = np.arange(S_DE)
    refused = s % 10 == 0
    c = np.array([0.2, 0.1])
    share = 1e-9 ** (1.0 - ((s * 37) % S_DE) / (S_DE - 1.0))
    lo, hi = c - share[:, None] * (c - 0.01), c + share[:, None] * (1.0 - c)
    lo[refused], hi[refused] = -0.5, -0.1
    starts = np.tile(c, (S_DE, 1))
    starts[s % 7 == 3] = [5.0, 0.3]
    starts[refused] = -0.2
    rows, splits = going_round(S_DE)
    ref = de.rule(two_rates, starts, rows, (lo, hi), split_times=splits, **DE_MANY)
    dev = de.device(two_rates, starts, rows, (lo, hi), split_times=splits, **DE_MANY)
    return starts, rows, splits, lo, hi, np.flatnonzero(refused), ref, dev


def test_1_de_searches_over_several_workgroups_stop_at_different_generations(de_many):
    starts, rows, splits, lo, hi, refused, ref, dev = de_many
    print("rule: searches per nit", np.bincount(ref["nit"], minlength=6).tolist(), "status", np.bincount(ref["status"], minlength=3).tolist())
    stops = set(ref["nit"].tolist())
    assert len(stops) >= 3 and {0, DE_MANY["maxiter"]} <= stops, stops
    moved(ref, skip=set(refused.tolist()))
    assert (ref["llh"][refused] == -np.inf).all() and (ref["status"][refused] == 2).all() and np.isfinite(np.delete(ref["llh"], refused)).all()
    held(dev, ref, de.FIELDS, "100 searches")
    assert ref["n_points"] == int(ref["nfev"].sum())


def test_1_de_permuted_and_a_slice_alone(two_rates, de_many):
    starts, rows, splits, lo, hi, refused, ref, dev = de_many
    perm = np.random.default_rng(1).permutation(S_DE)
    shuffled = de.device(two_rates, starts[perm], rows[perm], (lo[perm], hi[perm]), split_times=splits[perm], ids=perm, **DE_MANY)
    same_per_search(shuffled, dev, perm, de.FIELDS, "permuted")
    assert shuffled["n_points"] == dev["n_points"]
    part = np.arange(48, 53)                                                          # search 50 is a refused one
    alone = de.device(two_rates, starts[part], rows[part], (lo[part], hi[part]), split_times=splits[part], ids=part, **DE_MANY)
    same_per_search(alone, dev, part, de.FIELDS, "a slice alone")
    assert alone["n_points"] == int(dev["nfev"][part].sum())


# ---- 2. DE: population sizes at the workgroup's edges -----------------------------------------------------------------------------------
@pytest.mark.parametrize("pop, S", [(85, 3), (128, 3), (129, 3), (255, 3), (256, 3), (256, 1)], ids=lambda v: str(v))
def test_2_de_population_sizes_at_the_workgroups_edges(two_rates, pop, S):
    """85: three searches and one idle thread per workgroup; 128: two searches; 129 and 255: one search and idle threads; 256: a search
    fills the workgroup.  Search 0 an ordinary box, search 1 the hair (it stops after the initial population: the live searches are
    compacted), search 2 its second rate held fixed, its start outside the box."""
    lo = np.array([[0.01, 0.01], [0.2, 0.1], [0.01, 0.15]])[:S]
    hi = np.array([[1.0, 1.0], [0.2 + 1e-9, 0.1 + 1e-9], [1.0, 0.15]])[:S]
    starts = np.array([[0.2, 0.1], [0.2, 0.1], [5.0, 0.3]])[:S]
    kw = dict(pop=pop, maxiter=2, tol=1e-6, atol=0.0, F=(0.5, 1.0), CR=0.7, seed=5)
    ref = de.rule(two_rates, starts, de.ROWS[:S], (lo, hi), split_times=de.SPLITS[:S], **kw)
    dev = de.device(two_rates, starts, de.ROWS[:S], (lo, hi), split_times=de.SPLITS[:S], **kw)
    print("rule nit", ref["nit"].tolist(), "distinct values", [len(set(f.tolist())) for f in ref["population_llh"]])
    assert ref["nit"].tolist() == [2, 0, 2][:S]
    moved(ref)
    held(dev, ref, de.FIELDS, "pop %d" % pop)
    assert dev["population"].shape == (S, pop, 2)


# ---- 3. DE: N = 16 and N = 15 + the fitted split ----------------------------------------------------------------------------------------
DE_WIDE = dict(pop=8, maxiter=3, tol=1e-9, atol=0.0, F=(0.5, 1.0), CR=0.7, seed=7)


@pytest.mark.parametrize("fit_split", [False, True], ids=["N16", "N15-and-the-split"])
def test_3_de_sixteen_coordinates(wide, wide15, fit_split):
    """70 searches x 8 members in the box PAR x (1 -+ 0.2) (a fitted split in [16.5, 19]); every third search holds coordinate s % 16
    fixed at its centre."""
    eng, S = (wide15 if fit_split else wide), 70
    rows, splits, x, lo, hi = wide_problem(S, fit_split)
    for s in range(0, S, 3):
        lo[s, s % 16] = hi[s, s % 16] = x[s, s % 16]
    ref = de.rule(eng, x, rows, (lo, hi), split_times=splits, **DE_WIDE)
    dev = de.device(eng, x, rows, (lo, hi), split_times=splits, **DE_WIDE)
    mostly_finite(ref["population_llh"], "DE, 16 coordinates")
    moved(ref)
    held(dev, ref, de.FIELDS, "16 coordinates")
    for s in range(0, S, 3):
        assert (dev["population"][s][:, s % 16] == x[s, s % 16]).all()
    if fit_split:
        assert same_bits(dev["split"], dev["x"][:, 15]) and (dev["split"] != np.floor(dev["split"])).any()


# ---- 4. ensemble: many searches, with and without a prior per search -------------------------------------------------------------------
ENS_MANY = dict(n_step=4, thin=2, a=2.0, seed=3)
S_ENS = 70


def ens_many_problem():
    """The four kinds of search of tests/test_gpu_ens.py's mixed call going round: an ordinary box, a tight box around the ensemble, the
    second rate held fixed, a hot ensemble in a wide box; a temperature per search."""
    s = np.arange(S_ENS)
    kind = s % 4
    lo = np.array([[0.01, 0.01], [0.15, 0.06], [0.01, 0.15], [0.001, 0.001]])[kind]
    hi = np.array([[1.0, 1.0], [0.25, 0.14], [1.0, 0.15], [3.0, 3.0]])[kind]
    T = np.array([1.0, 2.0, 0.5, 50.0])[kind] * (1.0 + s / 100.0)
    init = ens.start(np.array([[0.2, 0.1], [0.2, 0.1], [0.3, 0.15], [0.5, 0.4]])[kind], lo, hi, 8, spread=np.array([0.05, 0.3, 0.05, 0.05])[kind])
    return init, lo, hi, T


@pytest.fixture(scope="module")
def ens_many(two_rates):
    init, lo, hi, T = ens_many_problem()
    rows, splits = going_round(S_ENS)
    ref = ens.rule(two_rates, init, rows, (lo, hi), split_times=splits, temperature=T, **ENS_MANY)
    dev = ens.device(two_rates, init, rows, (lo, hi), split_times=splits, temperature=T, **ENS_MANY)
    return init, rows, splits, lo, hi, T, ref, dev


def test_4_ensemble_many_searches(ens_many):
    init, rows, splits, lo, hi, T, ref, dev = ens_many
    decided_both_ways(ref)
    assert ref["n_points"] < ENS_MANY["n_step"] * S_ENS * 8                             # the rule rejected proposals in advance
    held(dev, ref, ENS, "70 searches")
    assert dev["chain"].shape == (S_ENS, 2, 8, 2) and (dev["chain"][2::4][..., 1] == 0.15).all()


def test_4_ensemble_permuted_and_a_slice_alone(two_rates, ens_many):
    init, rows, splits, lo, hi, T, ref, dev = ens_many
    perm = np.random.default_rng(2).permutation(S_ENS)
    shuffled = ens.device(two_rates, init[perm], rows[perm], (lo[perm], hi[perm]), split_times=splits[perm], temperature=T[perm], ids=perm, **ENS_MANY)
    same_per_search(shuffled, dev, perm, ENS, "permuted")
    assert shuffled["n_points"] == dev["n_points"]
    part = np.arange(30, 36)
    alone = ens.device(two_rates, init[part], rows[part], (lo[part], hi[part]), split_times=splits[part], temperature=T[part], ids=part, **ENS_MANY)
    same_per_search(alone, dev, part, ENS, "a slice alone")


def test_4_ensemble_many_searches_with_a_prior_per_search(two_rates):
    """The same call in sampling coordinates with n_prior = n_start: coordinate 0 on the log scale in every second search, its prior
    NORMAL (mean 0.4 of the way into the box, sd 0.15 of its width) in one group of four searches and EXPONENTIAL (scale a quarter of the
    width) in the next."""
    from misti_amd.optimize import ensemble_prior_rule, to_sampling
    init, lo, hi, T = ens_many_problem()
    rows, splits = going_round(S_ENS)
    s = np.arange(S_ENS)
    prior = dict(scale=np.zeros((S_ENS, 2), dtype=np.int32), kind=np.zeros((S_ENS, 2), dtype=np.int32), p0=np.zeros((S_ENS, 2)), p1=np.zeros((S_ENS, 2)))
    prior["scale"][s % 2 == 0, 0] = LOG
    lo, hi = to_sampling(lo, prior), to_sampling(hi, prior)
    init = to_sampling(init, {"scale": prior["scale"][:, None, :]}, (lo[:, None, :], hi[:, None, :]))
    width = hi[:, 0] - lo[:, 0]
    normal = (s // 4) % 2 == 0
    prior["kind"][:, 0] = np.where(normal, NORMAL, EXPONENTIAL)
    prior["p0"][:, 0] = np.where(normal, lo[:, 0] + 0.4 * width, 0.25 * width)
    prior["p1"][:, 0] = np.where(normal, 0.15 * width, 0.0)
    ref = ensemble_prior_rule(pt.objective(two_rates, rows, splits), init, lo, hi, prior=prior, temperature=T, **ENS_MANY)
    dev = ens.device(two_rates, init, rows, (lo, hi), split_times=splits, temperature=T, prior=prior, **ENS_MANY)
    decided_both_ways(ref)
    held(dev, ref, ENS, "70 searches with a prior")
    assert (dev["chain"][0::2][..., 0] <= 0.0).all() and (dev["chain"][1::2][..., 0] > 0.0).all()      # logarithms of rates below 1 | rates


# ---- 5. ensemble: W = 256 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 3])
def test_5_ensemble_256_walkers(two_rates, S):
    """H = 128: half a proposal workgroup for one search, exactly one for two, one and a half for three."""
    lo, hi = np.array([0.01, 0.01]), np.array([1.0, 1.0])
    init = ens.start(np.array([[0.2, 0.1], [0.3, 0.2], [0.15, 0.3]])[:S], lo, hi, 256, spread=0.1)
    kw = dict(split_times=de.SPLITS[:S], temperature=np.array([1.0, 3.0, 0.5])[:S], n_step=2, thin=1, seed=4)
    ref = ens.rule(two_rates, init, de.ROWS[:S], (lo, hi), **kw)
    dev = ens.device(two_rates, init, de.ROWS[:S], (lo, hi), **kw)
    decided_both_ways(ref)
    held(dev, ref, ENS, "W = 256, %d searches" % S)
    assert dev["chain"].shape == (S, 2, 256, 2)


# ---- 6. ensemble: N = 16 -------------------------------------------------------------------------------------------------------------------
def test_6_ensemble_sixteen_coordinates(wide):
    """20 searches x 34 walkers (more than 2 N) started within 0.2 of the half-width around PAR, in the box PAR x (1 -+ 0.2)."""
    S = 20
    rows, splits, x, lo, hi = wide_problem(S, False)
    init = ens.start(x, lo, hi, 34, spread=0.2)
    kw = dict(split_times=splits, temperature=1.0 + np.arange(S), n_step=3, thin=1, seed=6)
    ref = ens.rule(wide, init, rows, (lo, hi), **kw)
    dev = ens.device(wide, init, rows, (lo, hi), **kw)
    mostly_finite(ref["last_llh"], "ensemble, 16 coordinates")
    decided_both_ways(ref)
    held(dev, ref, ENS, "16 coordinates")


# ---- 7. tempered: the deepest ladder -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fits", [2, 3])
def test_7_tempered_sixty_four_rungs(two_rates, fits):
    """Rounds 1 and 3 treat the 32 pairs (0, 1), (2, 3), ..., rounds 2 and 4 the 31 pairs (1, 2), ..., (61, 62): with 4 walkers 256 and
    248 swap threads for two fits, 384 and 372 for three."""
    from misti_amd.optimize import temperature_ladder
    L, W = 64, 4
    ladder = temperature_ladder(1.0, 1e6, L)
    lo, hi = pt.LO[:fits], pt.HI[:fits]
    init = pt.start([[0.2, 0.1], [0.2, 0.1], [0.3, 0.15]][:fits], lo, hi, L, W, spread=0.1)
    kw = dict(split_times=pt.SPLITS[:fits], n_step=4, thin=1, swap_every=1, burn=1, a=2.0, seed=3)
    ref = pt.rule(two_rates, init, pt.ROWS[:fits], (lo, hi), ladder, **kw)
    dev = pt.device(two_rates, init, pt.ROWS[:fits], (lo, hi), ladder, **kw)
    decided_both_ways(ref)
    proposed, accepted = ref["swap_proposed"], ref["swap_accepted"]
    assert proposed.shape == (fits, L - 1) and ((accepted > 0) & (accepted < proposed)).any()
    assert proposed[:, 0::2].sum() > 0 and proposed[:, 1::2].sum() > 0                    # even and odd rounds
    held(dev, ref, PT, "64 rungs, %d fits" % fits)
    assert dev["chain_llh"].shape == (fits, L, 4, W) and dev["rung_llh"].shape == (fits, L)


# ---- 8. tempered: many fits, with and without one prior for all; 9. the summaries --------------------------------------------------------
TEMPERED = dict(n_step=4, thin=2, swap_every=1, burn=1, a=2.0, seed=3)
S_PT = 50


def pt_many_problem():
    """The three fits of tests/test_gpu_pt.py's mixed call going round (the third holds its second rate fixed), a ladder per fit."""
    s = np.arange(S_PT)
    lo, hi = pt.LO[s % 3], pt.HI[s % 3]
    ladder = pt.LADDER[s % 3] * (1.0 + s / 50.0)[:, None]
    init = pt.start(np.array([[0.2, 0.1], [0.2, 0.1], [0.3, 0.15]])[s % 3], lo, hi, 3, 6, spread=0.1)
    return init, lo, hi, ladder


@pytest.fixture(scope="module")
def pt_many(two_rates):
    init, lo, hi, ladder = pt_many_problem()
    rows, splits = going_round(S_PT)
    ref = pt.rule(two_rates, init, rows, (lo, hi), ladder, split_times=splits, **TEMPERED)
    dev = pt.device(two_rates, init, rows, (lo, hi), ladder, split_times=splits, **TEMPERED)
    return init, rows, splits, lo, hi, ladder, ref, dev


def test_8_tempered_many_fits(two_rates, pt_many):
    init, rows, splits, lo, hi, ladder, ref, dev = pt_many
    decided_both_ways(ref)
    assert ref["swap_accepted"].sum() > 0 and (ref["swap_proposed"] - ref["swap_accepted"]).sum() > 0
    assert ref["swap_proposed"][:, 0].sum() > 0 and ref["swap_proposed"][:, 1].sum() > 0
    held(dev, ref, PT, "50 fits")
    s = 37
    alone = pt.device(two_rates, init[s:s + 1], rows[s:s + 1], (lo[s:s + 1], hi[s:s + 1]), ladder[s], split_times=splits[s:s + 1], ids=[s], **TEMPERED)
    same_per_search(alone, dev, [s], PT, "a fit alone")


def test_8_tempered_many_fits_with_one_prior_for_all(two_rates):
    """The first rate on the log scale, the second under a normal prior (where it is not held fixed): n_prior = 1."""
    from misti_amd.optimize import prior_spec, tempered_prior_rule, to_sampling
    init, lo, hi, ladder = pt_many_problem()
    rows, splits = going_round(S_PT)
    prior = prior_spec(2, log=(0,), normal={1: (0.12, 0.05)})
    lo, hi = to_sampling(lo, prior), to_sampling(hi, prior)
    init = to_sampling(init, prior, (lo[:, None, None, :], hi[:, None, None, :]))
    ref = tempered_prior_rule(pt.objective(two_rates, rows, splits), init, lo, hi, ladder, prior=prior, **TEMPERED)
    dev = pt.device(two_rates, init, rows, (lo, hi), ladder, split_times=splits, prior=prior, **TEMPERED)
    decided_both_ways(ref)
    assert ref["swap_accepted"].sum() > 0 and (ref["swap_proposed"] - ref["swap_accepted"]).sum() > 0
    held(dev, ref, PT, "50 fits with a prior")


def test_9_tempered_many_fits_with_post(two_rates, pt_many):
    """The eight summaries, the shortest intervals and the sorted marginals of the cold chains of case 8 (two kept steps x 6 walkers),
    against the rules on the chain that comes back; the sampler's outputs keep their bits."""
    from misti_amd.optimize import ensemble_hpd_rule, ensemble_posterior_rule
    init, rows, splits, lo, hi, ladder, ref, dev = pt_many
    post = dict(burn=0, probs=(0.1, 0.5, 0.9), masses=(0.9, 0.5))
    got = pt.device(two_rates, init, rows, (lo, hi), ladder, split_times=splits, post=dict(post, want=POST_OLD + POST_NEW, keep_chain=True), **TEMPERED)
    for k in PT:
        assert same_bits(got[k], dev[k]), k
    want = ensemble_posterior_rule(got["chain"], got["chain_llh"][:, 0], burn=0, probs=post["probs"])
    want.update(ensemble_hpd_rule(got["chain"], burn=0, masses=post["masses"], order=True))
    assert got["order"].shape == (S_PT, 2, 12)
    for k in POST_OLD + POST_NEW:
        assert same_bits(got[k], want[k]), k
