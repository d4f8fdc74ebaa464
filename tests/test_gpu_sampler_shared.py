"""What the plain and the tempered ensemble sampler share on the host: one check, one run and one carve of the context's search
buffers (misti_sampler.cpp: SamplerArgs, sampler_run).  Seven calls one after another on ONE context, consecutive calls carving layouts
of different sizes and different optional parts - rungs, the reduction's arrays, the swap counters, a prior's arrays, the summaries'
workspace, a chain kept on the device or not at all - and every one of them must equal the same call on a fresh context, field by
field and bit for bit; the first and the last call are the same call; and the tempered call of one rung is the plain call.  Once with
a split per search, once with the split as the last coordinate.

The model and the S = 3 problem are those of tests/test_gpu_search_shared.py: every search with a row, a split, band bounds, pulse
times, a box of its own (n_box == S) and explicit ids, the middle search refused by the engine, so that slots without a point and
-inf values are on the path.  4 walkers, 4 steps, thin = 2: two kept rows and a swap round of each parity; a half-step is at most
3 x 3 x 2 = 18 points.  Every call is a valid call."""
import numpy as np
import pytest

from test_gpu_de import same_bits
from test_gpu_search_shared import BOUNDS, HI, IDS, LO, PULSES, ROWS, STARTS, model, problem

pytestmark = pytest.mark.gpu

STEPS = dict(n_step=4, thin=2, a=2.0, seed=1)
POST = dict(burn=0, probs=(0.25, 0.5))
LADDER = np.array([1.0, 3.0, 9.0])
PLAIN_FIELDS = ("chain", "chain_llh", "last", "last_llh", "accepted", "n_points")


def arguments(fit):
    """The S = 3 problem with the initial rungs [S][3][W][N] (rung 0: the plain call's ensemble) and a prior that says something on
    linear coordinates, so that box and init serve the calls with and without it."""
    from misti_amd.optimize import prior_spec
    from test_gpu_ens import start
    p = problem(fit)
    lo, hi = p["box"]
    at = np.clip(STARTS, LO, HI)[:, :lo.shape[1]]                         # where rung 0 starts: the hotter rungs around it too, from other draws
    p["rungs"] = np.stack([p["init"]] + [start(at, lo, hi, 4, spread=0.05, seed=7 + l) for l in (1, 2)], axis=1)
    p["prior"] = prior_spec(lo.shape[1], normal={0: (0.2, 0.1)}, exponential={1: 0.1})
    p["common"] = dict(split_times=p["split_times"], fit_split=p["split_times"] is None, band_bounds=BOUNDS, pulse_times=PULSES, ids=IDS, **STEPS)
    return p


def plain(e, table, p, **kw):
    return e.ensemble_sample(p["init"], ROWS, table, p["box"], **p["common"], **kw)


def posterior(e, table, p):
    return e.ensemble_posterior(p["init"], ROWS, table, p["box"], **p["common"], **POST)


def tempered(e, table, p, L, **kw):
    return e.tempered_sample(p["rungs"][:, :L], ROWS, table, p["box"], LADDER[:L], **p["common"], **kw)


RUNS = (("plain", plain),
        ("three_rungs_summaries_no_chain", lambda e, t, p: tempered(e, t, p, 3, swap_every=1, post=POST)),
        ("posterior_no_chain", posterior),
        ("one_rung", lambda e, t, p: tempered(e, t, p, 1, swap_every=1)),
        ("plain_prior", lambda e, t, p: plain(e, t, p, prior=p["prior"])),
        ("two_rungs_prior", lambda e, t, p: tempered(e, t, p, 2, swap_every=2, prior=p["prior"])),
        ("plain_again", plain))


@pytest.fixture(scope="module")
def world():
    """(engine factory, table, {(fit, name): result}): the seven calls per split mode, all fourteen on one context, in RUNS' order."""
    make, table = model()
    out = {}
    with make() as e:
        for fit in (False, True):
            p = arguments(fit)
            for name, run in RUNS:
                out[fit, name] = run(e, table, p)
    return make, table, out


def assert_same(a, b, what, fields=None):
    assert fields is not None or list(a) == list(b), (what, list(a), list(b))
    for k in fields or a:
        print(what, k, np.asarray(a[k]).ravel()[:6], np.asarray(b[k]).ravel()[:6])
        assert same_bits(np.asarray(a[k]), np.asarray(b[k])), (what, k)


@pytest.mark.parametrize("fit", [False, True])
def test_every_call_equals_itself_on_a_fresh_context(world, fit):
    make, table, shared = world
    p = arguments(fit)
    for name, run in RUNS[:6]:
        with make() as e:
            alone = run(e, table, p)
        assert_same(shared[fit, name], alone, (fit, name))


@pytest.mark.parametrize("fit", [False, True])
def test_the_first_call_is_the_same_before_and_after_the_others(world, fit):
    shared = world[2]
    assert_same(shared[fit, "plain"], shared[fit, "plain_again"], (fit, "plain"))
    r = shared[fit, "plain"]
    assert r["chain"].shape[:3] == (3, 2, 4) and (r["last_llh"][1] == -np.inf).all() and np.isfinite(r["last_llh"][[0, 2]]).any(axis=1).all()
    assert r["accepted"][[0, 2]].sum() > 0 and r["n_points"] > 0


@pytest.mark.parametrize("fit", [False, True])
def test_one_rung_is_the_plain_call(world, fit):
    shared = world[2]
    one, r = shared[fit, "one_rung"], shared[fit, "plain"]
    assert one["chain_llh"].shape == (3, 1, 2, 4) and one["swap_proposed"].shape == (3, 0) and same_bits(one["logz"], np.zeros(3))
    squeezed = dict(one, chain_llh=one["chain_llh"][:, 0], last=one["last"][:, 0], last_llh=one["last_llh"][:, 0], accepted=one["accepted"][:, 0])
    assert_same(squeezed, r, (fit, "one_rung"), PLAIN_FIELDS)


@pytest.mark.parametrize("fit", [False, True])
def test_the_sequence_went_through_every_optional_part(world, fit):
    shared = world[2]
    three, post, two = shared[fit, "three_rungs_summaries_no_chain"], shared[fit, "posterior_no_chain"], shared[fit, "two_rungs_prior"]
    assert "chain" not in three and "chain" not in post and "mean" in three and "mean" in post and two["chain"].shape[:3] == (3, 2, 4)
    assert (three["swap_proposed"][[0, 2]].sum(axis=0) > 0).all() and (three["swap_proposed"][1] == 0).all()      # both parities; the refused fit has no pair
    assert two["swap_proposed"][[0, 2], 0].sum() > 0 and shared[fit, "plain_prior"]["chain"].shape == shared[fit, "plain"]["chain"].shape
