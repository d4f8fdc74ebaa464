"""misti_search against the ten older entry points, bit for bit: Engine travels through the descriptor alone, so the wrappers are held
to it here by direct calls.  The pulse-sweep golden's model (one band, a fixed and an optimised pulse, two parameters), five starts
whose every per-start array differs between starts - a field wired to the wrong pointer is all that can go wrong."""
import ctypes as C

import numpy as np
import pytest

import search_forms as F
from conftest import load_golden

pytestmark = pytest.mark.gpu

S = 5
INF = np.inf
SPLITS = np.array([20.0, 19.0, 21.0, 18.0, 22.0])
RATES = np.array([[0.2, 0.1], [0.15, 0.05], [0.1, 0.2], [0.25, 0.02], [0.05, 0.15]])
ROWS = np.array([0, 2, 1, 1, 0], dtype=np.int32)
BOUNDS = np.array([[[b, -1]] for b in (4, 6, 2, 8, 5)], dtype=np.int32)
TIMES = np.array([[10, t] for t in (5, 12, 15, 3, 7)], dtype=np.int32)
SEARCH_OUT, HOP_OUT = ("x", "llh", "nit", "nfev", "status"), ("x", "llh", "nfev", "failures", "accepted")


@pytest.fixture(scope="module")
def model():
    from misti_amd.engine import Engine
    grid = load_golden("golden_pulse_sweep")[0]["in"]
    table = np.array([grid["sfs"], [v * 2 for v in grid["sfs"]], [v * 3 for v in grid["sfs"]]], dtype=np.float64)
    with Engine(grid["times"], grid["lambdas"], [(0, 4, -1, 0.2, 0)], [(0, 10, 0.05, -1), (1, 5, 0.0, 1)], n_param=2, cpfit=True, smooth=True,
                unfolded=True) as eng:
        assert (eng.n_param, eng.n_band, eng.n_pulse) == (2, 1, 2)
        yield eng, table


def full(table, fitted, open_box=False):
    """Every field of a search and of its hops, with the inputs of 5 starts; ``fitted``: the split as the last coordinate."""
    from misti_amd.engine import draw_uniforms
    N = 3 if fitted else 2
    starts = np.hstack([RATES, SPLITS[:, None]]) if fitted else RATES.copy()
    lo = np.array([[0.0, 0.0], [0.01, 0.0], [0.0, 0.01], [0.02, 0.0], [0.0, 0.02]])
    hi = np.array([[0.15 + 0.01 * s, INF] for s in range(S)])
    if fitted:
        lo, hi = np.hstack([lo, SPLITS[:, None] - 1.0 - 0.1 * np.arange(S)[:, None]]), np.hstack([hi, SPLITS[:, None] + 1.0 + 0.1 * np.arange(S)[:, None]])
    if open_box:
        lo, hi = np.full((S, N), -INF), np.full((S, N), INF)
    return dict(split_time=20.0, split_times=None if fitted else SPLITS.copy(), n_start=S, starts=np.ascontiguousarray(starts), rows=ROWS.copy(),
                n_rep=3, jsfs=table, band_bounds=BOUNDS.copy(), pulse_times=TIMES.copy(), n_box=S, box_lo=np.ascontiguousarray(lo),
                box_hi=np.ascontiguousarray(hi), xatol=1e-4, fatol=1e-4, maxiter=30,
                hops=dict(niter=2, T=0.5, stepsize=0.5, interval=50, target_accept_rate=0.5, stepwise_factor=0.9, nm_maxfev=60,
                          uniforms=draw_uniforms([11, 12, 13, 14, 15], S, 2, N)))


def run(eng, symbol, f, door):
    """``symbol``'s form of ``f`` through the symbol itself (``door`` "old") or through misti_search; the outputs start as -7s."""
    hop = F.is_hop_form(symbol)
    N = f["starts"].shape[1]
    f = F.form_of(symbol, f)
    out = dict(x=np.full((S, N), -7.0), llh=np.full(S, -7.0), **{k: np.full(S, -7, dtype=np.int32) for k in (HOP_OUT if hop else SEARCH_OUT)[2:]})
    f.update(x=out["x"], llh=out["llh"])
    if hop:
        f["maxiter"] = 60
        f["hops"].update({k: out[k] for k in HOP_OUT[2:]})
    else:
        f.update({k: out[k] for k in SEARCH_OUT[2:]})
    lib = eng._lib
    rc = getattr(lib, symbol)(eng._ctx, *F.legacy_args(symbol, f)) if door == "old" else lib.misti_search(eng._ctx, C.byref(F.descriptor(f)))
    assert rc == 0, (symbol, door, lib.misti_last_error())
    return out


def same(a, b):
    return a.keys() == b.keys() and all(a[k].tobytes() == b[k].tobytes() for k in a)


FORMS = [(s, False) for s in F.LEGACY if not s.endswith("_split")] + [(s, True) for s in F.LEGACY if s.endswith(("_split", "_box"))]


@pytest.mark.parametrize("symbol, fitted", FORMS)
def test_each_older_entry_point_equals_its_descriptor_bit_for_bit(model, symbol, fitted):
    eng, table = model
    old, new = (run(eng, symbol, full(table, fitted), door) for door in ("old", "new"))
    assert set(old) == set(HOP_OUT if F.is_hop_form(symbol) else SEARCH_OUT)
    assert same(old, new), (old, new)
    assert np.isfinite(new["llh"]).any() and not (new["x"] == -7.0).any() and (new["nfev"] > 0).all()       # the searches did run


def test_null_for_the_argument_each_form_adds_is_the_form_before_it(model):
    """_rows = _bounds = _pulses at NULL bounds and times; _box with an all-infinite box = _pulses / _split (and so under hops)."""
    eng, table = model
    f = full(table, False)
    plain = dict(f, band_bounds=None, pulse_times=None)
    rows = run(eng, "misti_nm_solve_rows", f, "old")
    assert same(rows, run(eng, "misti_nm_solve_bounds", plain, "old")) and same(rows, run(eng, "misti_nm_solve_pulses", plain, "old"))
    assert same(run(eng, "misti_nm_solve_bounds", f, "old"), run(eng, "misti_nm_solve_pulses", dict(f, pulse_times=None), "old"))
    assert not same(rows, run(eng, "misti_nm_solve_pulses", f, "old"))               # the bounds and times do matter here
    for fitted, nm, bh in ((False, "misti_nm_solve_pulses", "misti_basinhopping_rows"), (True, "misti_nm_solve_split", "misti_basinhopping_split")):
        f, open_ = full(table, fitted), full(table, fitted, open_box=True)
        assert same(run(eng, nm, f, "old"), run(eng, "misti_nm_solve_box", open_, "old")), fitted
        assert same(run(eng, bh, f, "old"), run(eng, "misti_basinhopping_box", open_, "old")), fitted
        assert not same(run(eng, nm, f, "old"), run(eng, "misti_nm_solve_box", f, "old")), fitted       # the closed box does bind


@pytest.mark.parametrize("symbol", ["misti_nm_solve", "misti_nm_solve_box", "misti_basinhopping", "misti_basinhopping_box"])
def test_no_starts_return_0_and_write_nothing_through_both_doors(model, symbol):
    eng, table = model
    for door in ("old", "new"):
        out = run(eng, symbol, dict(full(table, False), n_start=0, n_box=1), door)
        assert all((a == -7).all() for a in out.values()), (door, out)
