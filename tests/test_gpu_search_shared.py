"""What Nelder-Mead, differential evolution and the ensemble sampler share on the device (PointSource, put_point / put_none) and on
the host (the rows problem: per-search arrays, table, layout, uploads): the three searches one after another on ONE context, each
with S = 3 searches that carry everything a search can hand its points at once - a row, a split, band bounds, pulse times, a box
of their own (n_box == S) and explicit ids - the middle search with pulse times the engine refuses, so that slots without a point
and -inf results are on the path.  Once with a split per search, once with the split as the last coordinate.

S = 3 is the smallest S at which "one box for all" and "a box per search" index differently and a refused middle search has a
neighbour on each side.  The model is the pulse model of tests/test_gpu_de.py / tests/test_gpu_ens.py (the 32-interval grid of
tests/golden/golden_pulse_sweep.json: a band's rate and the second pulse's fraction searched); populations of 4, 2 generations,
4 walkers, 2 steps, 25 Nelder-Mead iterations: a batch is at most 18 points."""
import random

import numpy as np
import pytest

from conftest import load_golden
from test_gpu_de import rule as de_rule, same_bits
from test_gpu_ens import rule as ens_rule, start as ens_start

pytestmark = pytest.mark.gpu

S = 3
ROWS = np.array([2, 0, 1], dtype=np.int32)
SPLITS = np.array([20.0, 20.5, 20.0])
BOUNDS = np.array([[[4, -1]], [[5, -1]], [[5, -1]]], dtype=np.int32)
PULSES = np.array([[10, 3], [10, 99], [10, 3]], dtype=np.int32)          # search 1: a pulse beyond the grid - no point of it has a value
IDS = np.array([5, 2, 9], dtype=np.uint64)
LO = np.array([[0.01, 0.0, 17.0], [0.02, 0.0, 18.0], [0.01, 0.01, 17.5]])
HI = np.array([[0.5, 0.3, 21.5], [0.4, 0.25, 21.0], [0.6, 0.3, 21.0]])
STARTS = np.array([[0.2, 0.1, 20.0], [0.9, 0.1, 20.5], [0.25, 0.12, 20.0]])   # search 1 starts outside its box: clipped
NM = dict(tol=1e-4, maxiter=25)
DE = dict(pop=4, maxiter=2, tol=1e-9, atol=0.0, F=(0.5, 1.0), CR=0.7, seed=1)
ENS = dict(n_step=2, thin=1, a=2.0, seed=1)
NM_FIELDS = ("x", "llh", "nit", "nfev", "status", "split")
DE_FIELDS = ("x", "llh", "nit", "nfev", "status", "population", "population_llh", "split", "n_points")
ENS_FIELDS = ("chain", "chain_llh", "accepted", "last", "last_llh", "n_points")


def model():
    """(engine factory, table[3][8]) of the pulse model."""
    from misti_amd import io as mio, synth
    from misti_amd.engine import Engine
    g = load_golden("golden_pulse_sweep")[0]["in"]
    table = np.array(mio.bootstrap_table(synth.chunk_rows(g["sfs"], 20), 3, random.Random(3)), dtype=np.float64)

    def make():
        return Engine(g["times"], g["lambdas"], [(0, 4, -1, 0.2, 0)], [(0, 10, 0.05, -1), (1, 3, 0.0, 1)], n_param=2, cpfit=True, smooth=True,
                      unfolded=True)
    return make, table


def problem(fit):
    """The arguments the three searches share: N = 2 at SPLITS, or N = 3 with the split as the last coordinate."""
    n = 3 if fit else 2
    return dict(starts=STARTS[:, :n].copy(), box=(LO[:, :n].copy(), HI[:, :n].copy()), split_times=None if fit else SPLITS,
                init=ens_start(np.clip(STARTS, LO, HI)[:, :n], LO[:, :n], HI[:, :n], 4, spread=0.05))


def run_nm(e, table, p):
    return e.nm_solve_box(p["starts"], ROWS, table, p["box"], split_times=p["split_times"], band_bounds=BOUNDS, pulse_times=PULSES, **NM)


def run_de(e, table, p):
    return e.differential_evolution(p["starts"], ROWS, table, p["box"], split_times=p["split_times"], fit_split=p["split_times"] is None,
                                    band_bounds=BOUNDS, pulse_times=PULSES, ids=IDS, return_population=True, **DE)


def run_ens(e, table, p):
    return e.ensemble_sample(p["init"], ROWS, table, p["box"], split_times=p["split_times"], fit_split=p["split_times"] is None,
                             band_bounds=BOUNDS, pulse_times=PULSES, ids=IDS, **ENS)


RUNS = (("nm", run_nm, NM_FIELDS), ("de", run_de, DE_FIELDS), ("ens", run_ens, ENS_FIELDS), ("nm_again", run_nm, NM_FIELDS))


def shared_context_results(make, table):
    """{(fit, name): result} of the four calls per split mode, all eight on one context, in the order of RUNS."""
    out = {}
    with make() as e:
        for fit in (False, True):
            p = problem(fit)
            for name, run, _ in RUNS:
                out[fit, name] = run(e, table, p)
    return out


@pytest.fixture(scope="module")
def world():
    make, table = model()
    return make, table, shared_context_results(make, table)


def assert_fields(a, b, fields, what):
    for k in fields:
        print(what, k, np.asarray(a[k]).ravel()[:6], np.asarray(b[k]).ravel()[:6])
        assert same_bits(np.asarray(a[k]), np.asarray(b[k])), (what, k)


@pytest.mark.parametrize("fit", [False, True])
def test_every_search_equals_itself_on_a_fresh_context(world, fit):
    make, table, shared = world
    p = problem(fit)
    for name, run, fields in RUNS[:3]:
        with make() as e:
            alone = run(e, table, p)
        assert_fields(shared[fit, name], alone, fields, (fit, name))


@pytest.mark.parametrize("fit", [False, True])
def test_nelder_mead_is_the_same_before_and_after_the_other_searches(world, fit):
    make, table, shared = world
    assert_fields(shared[fit, "nm"], shared[fit, "nm_again"], NM_FIELDS, (fit, "nm"))
    r = shared[fit, "nm"]
    assert r["llh"][1] == -np.inf and np.isfinite(r["llh"][[0, 2]]).all()
    assert (r["x"] >= LO[:, :r["x"].shape[1]]).all() and (r["x"] <= HI[:, :r["x"].shape[1]]).all()


@pytest.mark.parametrize("fit", [False, True])
def test_the_population_searches_equal_their_rules(world, fit):
    make, table, shared = world
    p = problem(fit)
    with make() as e:
        de = de_rule(e, p["starts"], ROWS, p["box"], split_times=p["split_times"], band_bounds=BOUNDS, pulse_times=PULSES, table=table, ids=IDS, **DE)
        ens = ens_rule(e, p["init"], ROWS, p["box"], split_times=p["split_times"], band_bounds=BOUNDS, pulse_times=PULSES, table=table, ids=IDS, **ENS)
    dev = shared[fit, "de"]
    for k in DE_FIELDS[:7]:
        assert same_bits(np.asarray(dev[k], dtype=de[k].dtype), de[k]), (fit, "de", k)
    assert dev["n_points"] == de["n_points"]
    assert dev["llh"][1] == -np.inf and (dev["population_llh"][1] == -np.inf).all() and np.isfinite(dev["llh"][[0, 2]]).all()
    dev = shared[fit, "ens"]
    for k in ENS_FIELDS[:5]:
        assert same_bits(np.asarray(dev[k], dtype=ens[k].dtype), ens[k]), (fit, "ens", k)
    assert dev["n_points"] == ens["n_points"]
    assert (dev["last_llh"][1] == -np.inf).all() and np.isfinite(dev["last_llh"][[0, 2]]).any(axis=1).all()
