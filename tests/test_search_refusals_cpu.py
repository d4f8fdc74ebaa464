"""Every refusal misti_search, misti_de_search, misti_ensemble_sample and misti_tempered_sample make before they look at a context, and
the prior-shape refusals of the two samplers' prior doors, with its exact code and its exact misti_last_error() text - the doors share
their checks of the rows problem (rows, split times, the limits, the box), the two samplers share one check altogether, and of two
faults each names the one its header puts first.  The existing tests (test_search_cpu.py, test_de_cpu.py, test_ens_cpu.py,
test_pt_cpu.py, test_prior_cpu.py, whose descriptor builders these are) assert a code and one word per refusal; the texts below are
the library's as they stood before the checks were shared."""
import ctypes as C

import numpy as np
import pytest

import search_forms as F
from test_de_cpu import de_search
from test_ens_cpu import ens_sample
from test_prior_cpu import sample_prior
from test_pt_cpu import pt_sample
from test_search_cpu import _full

E_ARG, E_LIMIT = -1, -4
INF, NAN = float("inf"), float("nan")


def nm_search(form="misti_nm_solve_box", fitted=False, split=None, **change):
    """misti_search WITHOUT a context on the descriptor that `form` is (test_search_cpu's valid fields), with `change` applied."""
    from misti_amd import _lib
    f = F.form_of(form, _full(N=3 if fitted else 2))
    for k, v in change.items():
        f[k] = dict(f[k], **v) if k == "hops" else v
    if split is not None:
        f["split"] = split
    lib = _lib.load()
    rc = lib.misti_search(None, C.byref(F.descriptor(f)))
    return rc, lib.misti_last_error().decode()


ROWS_PER, ROWS_FIT, ONE, HOP = "misti_nm_solve_box", "misti_nm_solve_split", "misti_nm_solve", "misti_basinhopping_box"
I32 = lambda *v: np.array(v, dtype=np.int32)      # noqa: E731

PT_NULL = "init / rows / jsfs / box_lo / box_hi / ladder / last / last_llh / rung_llh / logz"

CASES = [
    # ---- misti_search -------------------------------------------------------------------------------------------------------------
    (nm_search, dict(n_start=-1), E_ARG, "negative number of starts"),
    (nm_search, dict(form=ONE, starts=None), E_ARG, "starts / jsfs_row / x / llh is NULL"),
    (nm_search, dict(form=ONE, jsfs=None), E_ARG, "starts / jsfs_row / x / llh is NULL"),
    (nm_search, dict(starts=None), E_ARG, "starts / split_times / rows / jsfs / x / llh is NULL"),
    (nm_search, dict(rows=None), E_ARG, "starts / split_times / rows / jsfs / x / llh is NULL"),
    (nm_search, dict(split_times=None, split=1), E_ARG, "starts / split_times / rows / jsfs / x / llh is NULL"),
    (nm_search, dict(x=None), E_ARG, "starts / split_times / rows / jsfs / x / llh is NULL"),
    (nm_search, dict(form=ROWS_FIT, fitted=True, llh=None), E_ARG, "starts / rows / jsfs / x / llh is NULL"),
    (nm_search, dict(form=ROWS_FIT, fitted=True, rows=None), E_ARG, "starts / rows / jsfs / x / llh is NULL"),
    (nm_search, dict(n_rep=0), E_ARG, "n_rep must be >= 1 (got 0)"),
    (nm_search, dict(n_rep=-4), E_ARG, "n_rep must be >= 1 (got -4)"),
    (nm_search, dict(maxiter=0), E_ARG, "maxiter must be >= 1"),
    (nm_search, dict(form=HOP, hops=dict(niter=-1)), E_ARG, "negative number of hops"),
    (nm_search, dict(form=HOP, hops=dict(uniforms=None)), E_ARG, "uniforms is NULL"),
    (nm_search, dict(form=HOP, maxiter=0), E_ARG, "nm_maxiter, nm_maxfev and interval must be >= 1"),
    (nm_search, dict(form=HOP, hops=dict(nm_maxfev=0)), E_ARG, "nm_maxiter, nm_maxfev and interval must be >= 1"),
    (nm_search, dict(form=HOP, hops=dict(interval=0)), E_ARG, "nm_maxiter, nm_maxfev and interval must be >= 1"),
    (nm_search, dict(rows=I32(0, 3)), E_ARG, "rows[1] = 3 is outside the table (n_rep = 3)"),
    (nm_search, dict(rows=I32(-1, 0)), E_ARG, "rows[0] = -1 is outside the table (n_rep = 3)"),
    (nm_search, dict(form=ROWS_FIT, fitted=True, rows=I32(0, 7)), E_ARG, "rows[1] = 7 is outside the table (n_rep = 3)"),
    (nm_search, dict(split_times=np.array([20.0, INF])), E_ARG, "split_times[1] is not finite"),
    (nm_search, dict(split_times=np.array([NAN, 20.0])), E_ARG, "split_times[0] is not finite"),
    (nm_search, dict(), E_ARG, "ctx is NULL"),
    (nm_search, dict(form=ONE), E_ARG, "ctx is NULL"),
    (nm_search, dict(form=HOP, fitted=True), E_ARG, "ctx is NULL"),
    (nm_search, dict(n_box=5), E_ARG, "ctx is NULL"),                           # this door's box needs the model: behind the context
    (nm_search, dict(n_start=0), E_ARG, "ctx is NULL"),
    # two faults: the earlier one is named
    (nm_search, dict(n_start=-1, starts=None), E_ARG, "negative number of starts"),
    (nm_search, dict(x=None, n_rep=0), E_ARG, "starts / split_times / rows / jsfs / x / llh is NULL"),
    (nm_search, dict(n_rep=0, maxiter=0), E_ARG, "n_rep must be >= 1 (got 0)"),
    (nm_search, dict(maxiter=0, rows=I32(0, 3)), E_ARG, "maxiter must be >= 1"),
    (nm_search, dict(rows=I32(0, 3), split_times=np.array([INF, 20.0])), E_ARG, "split_times[0] is not finite"),
    (nm_search, dict(rows=I32(3, 0), split_times=np.array([INF, 20.0])), E_ARG, "rows[0] = 3 is outside the table (n_rep = 3)"),
    (nm_search, dict(form=HOP, hops=dict(niter=-1, interval=0), rows=I32(9, 9)), E_ARG, "negative number of hops"),
    # ---- misti_de_search ----------------------------------------------------------------------------------------------------------
    (de_search, dict(n_start=-1), E_ARG, "negative number of searches"),
    (de_search, dict(null=("starts",)), E_ARG, "starts / rows / jsfs / box_lo / box_hi / x / llh / split_times is NULL"),
    (de_search, dict(null=("rows",)), E_ARG, "starts / rows / jsfs / box_lo / box_hi / x / llh / split_times is NULL"),
    (de_search, dict(null=("box_hi",)), E_ARG, "starts / rows / jsfs / box_lo / box_hi / x / llh / split_times is NULL"),
    (de_search, dict(null=("split_times",)), E_ARG, "starts / rows / jsfs / box_lo / box_hi / x / llh / split_times is NULL"),
    (de_search, dict(null=("jsfs",), split=2), E_ARG, "starts / rows / jsfs / box_lo / box_hi / x / llh is NULL"),
    (de_search, dict(n_rep=0), E_ARG, "n_rep must be >= 1 (got 0)"),
    (de_search, dict(pop=3), E_ARG, "pop must be >= 4 (got 3)"),
    (de_search, dict(pop=257), E_LIMIT, "pop = 257 exceeds MISTI_DE_MAX_POP = 256"),
    (de_search, dict(maxiter=0), E_ARG, "maxiter must be >= 1"),
    (de_search, dict(tol=-1.0), E_ARG, "tol and atol must be finite and not negative"),
    (de_search, dict(atol=NAN), E_ARG, "tol and atol must be finite and not negative"),
    (de_search, dict(F_lo=1.0, F_hi=0.5), E_ARG, "F must be a finite range 0 <= F_lo <= F_hi (got 1, 0.5)"),
    (de_search, dict(F_hi=INF), E_ARG, "F must be a finite range 0 <= F_lo <= F_hi (got 0.5, inf)"),
    (de_search, dict(CR=1.5), E_ARG, "CR must lie in [0, 1] (got 1.5)"),
    (de_search, dict(n_box=3), E_ARG, "n_box must be 1 or n_start (got 3 for 2 searches)"),
    (de_search, dict(n_box=0), E_ARG, "n_box must be 1 or n_start (got 0 for 2 searches)"),
    (de_search, dict(rows=[0, 3]), E_ARG, "rows[1] = 3 is outside the table (n_rep = 3)"),
    (de_search, dict(rows=[-1, 0]), E_ARG, "rows[0] = -1 is outside the table (n_rep = 3)"),
    (de_search, dict(split_times=[5.0, INF]), E_ARG, "split_times[1] is not finite"),
    (de_search, dict(), E_ARG, "ctx is NULL"),
    (de_search, dict(null=("split_times",), split=2), E_ARG, "ctx is NULL"),
    (de_search, dict(n_start=0, n_box=0), E_ARG, "ctx is NULL"),
    # two faults
    (de_search, dict(pop=3, n_box=3), E_ARG, "pop must be >= 4 (got 3)"),
    (de_search, dict(n_box=3, rows=[0, 3]), E_ARG, "n_box must be 1 or n_start (got 3 for 2 searches)"),
    (de_search, dict(CR=NAN, split_times=[NAN, 5.0]), E_ARG, "CR must lie in [0, 1] (got nan)"),
    (de_search, dict(rows=[0, 3], split_times=[NAN, 5.0]), E_ARG, "split_times[0] is not finite"),
    # ---- misti_ensemble_sample ----------------------------------------------------------------------------------------------------
    (ens_sample, dict(n_start=-1), E_ARG, "negative number of searches"),
    (ens_sample, dict(null=("init",)), E_ARG, "init / rows / jsfs / box_lo / box_hi / temperature / last / last_llh / split_times is NULL"),
    (ens_sample, dict(null=("temperature",)), E_ARG, "init / rows / jsfs / box_lo / box_hi / temperature / last / last_llh / split_times is NULL"),
    (ens_sample, dict(null=("split_times",)), E_ARG, "init / rows / jsfs / box_lo / box_hi / temperature / last / last_llh / split_times is NULL"),
    (ens_sample, dict(null=("last",), split=2), E_ARG, "init / rows / jsfs / box_lo / box_hi / temperature / last / last_llh is NULL"),
    (ens_sample, dict(n_rep=0), E_ARG, "n_rep must be >= 1 (got 0)"),
    (ens_sample, dict(walkers=5), E_ARG, "walkers must be even and >= 4 (got 5)"),
    (ens_sample, dict(walkers=258), E_LIMIT, "walkers = 258 exceeds MISTI_ENS_MAX_WALKERS = 256"),
    (ens_sample, dict(n_step=-1), E_ARG, "n_step must not be negative"),
    (ens_sample, dict(thin=0), E_ARG, "thin must be >= 1"),
    (ens_sample, dict(a=1.0), E_ARG, "a must be finite and > 1 (got 1)"),
    (ens_sample, dict(n_temp=3), E_ARG, "n_temp must be 1 or n_start (got 3 for 2 searches)"),
    (ens_sample, dict(temperature=[0.0, 1.0]), E_ARG, "temperature[0] = 0 is not finite and positive"),
    (ens_sample, dict(n_temp=2, temperature=[1.0, INF]), E_ARG, "temperature[1] = inf is not finite and positive"),
    (ens_sample, dict(n_box=3), E_ARG, "n_box must be 1 or n_start (got 3 for 2 searches)"),
    (ens_sample, dict(rows=[0, 3]), E_ARG, "rows[1] = 3 is outside the table (n_rep = 3)"),
    (ens_sample, dict(split_times=[5.0, INF]), E_ARG, "split_times[1] is not finite"),
    (ens_sample, dict(), E_ARG, "ctx is NULL"),
    (ens_sample, dict(n_start=0, n_box=0), E_ARG, "ctx is NULL"),
    # two faults
    (ens_sample, dict(a=0.5, n_box=3), E_ARG, "a must be finite and > 1 (got 0.5)"),
    (ens_sample, dict(temperature=[-1.0, 1.0], rows=[0, 9]), E_ARG, "temperature[0] = -1 is not finite and positive"),
    (ens_sample, dict(n_box=3, split_times=[INF, 5.0]), E_ARG, "n_box must be 1 or n_start (got 3 for 2 searches)"),
    (ens_sample, dict(rows=[0, 3], split_times=[INF, 5.0]), E_ARG, "split_times[0] is not finite"),
    # ---- misti_tempered_sample: every case of test_pt_cpu.py::test_tempered_sample_argument_checks --------------------------------
    (pt_sample, dict(), E_ARG, "ctx is NULL"),
    (pt_sample, dict(n_start=0, n_box=0), E_ARG, "ctx is NULL"),
    (pt_sample, dict(n_step=0, burn=7), E_ARG, "ctx is NULL"),
    (pt_sample, dict(n_rung=1), E_ARG, "ctx is NULL"),
    (pt_sample, dict(n_rung=64), E_ARG, "ctx is NULL"),
    (pt_sample, dict(swap_every=0), E_ARG, "ctx is NULL"),
    (pt_sample, dict(n_ladder=2), E_ARG, "ctx is NULL"),
    (pt_sample, dict(size=8), E_ARG, "the sampler descriptor's size is 8, this library's misti_pt_t has 240 bytes"),
    (pt_sample, dict(split=0), E_ARG, "the sampler descriptor's split mode 0 is neither MISTI_SPLIT_PER_START nor MISTI_SPLIT_FITTED"),
    (pt_sample, dict(n_start=-1), E_ARG, "negative number of fits"),
    (pt_sample, dict(null=("init",)), E_ARG, PT_NULL + " / split_times is NULL"),
    (pt_sample, dict(null=("ladder",)), E_ARG, PT_NULL + " / split_times is NULL"),
    (pt_sample, dict(null=("rung_llh",)), E_ARG, PT_NULL + " / split_times is NULL"),
    (pt_sample, dict(null=("logz",)), E_ARG, PT_NULL + " / split_times is NULL"),
    (pt_sample, dict(null=("split_times",)), E_ARG, PT_NULL + " / split_times is NULL"),
    (pt_sample, dict(null=("split_times",), split=2), E_ARG, "ctx is NULL"),
    (pt_sample, dict(null=("last",), split=2), E_ARG, PT_NULL + " is NULL"),
    (pt_sample, dict(n_rep=0), E_ARG, "n_rep must be >= 1 (got 0)"),
    (pt_sample, dict(walkers=5), E_ARG, "walkers must be even and >= 4 (got 5)"),
    (pt_sample, dict(walkers=258), E_LIMIT, "walkers = 258 exceeds MISTI_ENS_MAX_WALKERS = 256"),
    (pt_sample, dict(n_step=-1), E_ARG, "n_step must not be negative"),
    (pt_sample, dict(thin=0), E_ARG, "thin must be >= 1"),
    (pt_sample, dict(a=1.0), E_ARG, "a must be finite and > 1 (got 1)"),
    (pt_sample, dict(n_rung=0), E_ARG, "n_rung must be >= 1 (got 0)"),
    (pt_sample, dict(n_rung=65), E_LIMIT, "n_rung = 65 exceeds MISTI_PT_MAX_RUNGS = 64"),
    (pt_sample, dict(n_ladder=3), E_ARG, "n_ladder must be 1 or n_start (got 3 for 2 fits)"),
    (pt_sample, dict(ladder=[[0.0, 1.0, 2.0], [1.0, 2.0, 3.0]]), E_ARG, "ladder[0][0] = 0 is not finite and positive"),
    (pt_sample, dict(ladder=[[1.0, INF, 2.0], [1.0, 2.0, 3.0]]), E_ARG, "ladder[0][1] = inf is not finite and positive"),
    (pt_sample, dict(ladder=[[1.0, 2.0, 2.0], [1.0, 2.0, 3.0]]), E_ARG, "ladder[0][2] = 2 is not above ladder[0][1] = 2: a ladder is strictly increasing"),
    (pt_sample, dict(n_ladder=2, ladder=[[1.0, 2.0, 3.0], [1.0, 3.0, 2.5]]), E_ARG,
     "ladder[1][2] = 2.5 is not above ladder[1][1] = 3: a ladder is strictly increasing"),
    (pt_sample, dict(n_ladder=2, ladder=[[1.0, 2.0, 3.0], [1.0, NAN, 2.5]]), E_ARG, "ladder[1][1] = nan is not finite and positive"),
    (pt_sample, dict(swap_every=-1), E_ARG, "swap_every must not be negative (got -1)"),
    (pt_sample, dict(burn=3), E_ARG, "burn must be 0 ... K - 1 (got 3 for 3 kept steps)"),
    (pt_sample, dict(burn=-1), E_ARG, "burn must be 0 ... K - 1 (got -1 for 3 kept steps)"),
    (pt_sample, dict(n_box=3), E_ARG, "n_box must be 1 or n_start (got 3 for 2 fits)"),
    (pt_sample, dict(rows=[0, 3]), E_ARG, "rows[1] = 3 is outside the table (n_rep = 3)"),
    (pt_sample, dict(split_times=[5.0, INF]), E_ARG, "split_times[1] is not finite"),
    # two faults
    (pt_sample, dict(a=0.5, n_rung=0), E_ARG, "a must be finite and > 1 (got 0.5)"),
    (pt_sample, dict(n_rung=0, n_ladder=3), E_ARG, "n_rung must be >= 1 (got 0)"),
    (pt_sample, dict(n_rung=65, n_ladder=3), E_LIMIT, "n_rung = 65 exceeds MISTI_PT_MAX_RUNGS = 64"),
    (pt_sample, dict(n_ladder=3, swap_every=-1), E_ARG, "n_ladder must be 1 or n_start (got 3 for 2 fits)"),
    (pt_sample, dict(ladder=[[1.0, 1.0, 2.0], [1.0, 2.0, 3.0]], swap_every=-1), E_ARG,
     "ladder[0][1] = 1 is not above ladder[0][0] = 1: a ladder is strictly increasing"),
    (pt_sample, dict(swap_every=-1, burn=9), E_ARG, "swap_every must not be negative (got -1)"),
    (pt_sample, dict(burn=9, n_box=3), E_ARG, "burn must be 0 ... K - 1 (got 9 for 3 kept steps)"),
    (pt_sample, dict(burn=9, rows=[0, 9]), E_ARG, "burn must be 0 ... K - 1 (got 9 for 3 kept steps)"),
    # ---- the prior's shape at both samplers' prior doors: behind n_box, before the context ------------------------------------------
    (sample_prior, dict(entry="ensemble", prior=1), E_ARG, "ctx is NULL"),
    (sample_prior, dict(entry="tempered", prior=2), E_ARG, "ctx is NULL"),
    (sample_prior, dict(entry="ensemble", prior=1, size=8), E_ARG, "the prior descriptor's size is 8, this library's misti_prior_t has 40 bytes"),
    (sample_prior, dict(entry="tempered", prior=1, size=8), E_ARG, "the prior descriptor's size is 8, this library's misti_prior_t has 40 bytes"),
    (sample_prior, dict(entry="ensemble", prior=3), E_ARG, "n_prior must be 1 or n_start (got 3 for 2 searches)"),
    (sample_prior, dict(entry="tempered", prior=3), E_ARG, "n_prior must be 1 or n_start (got 3 for 2 fits)"),
    (sample_prior, dict(entry="ensemble", prior=0), E_ARG, "n_prior must be 1 or n_start (got 0 for 2 searches)"),
    (sample_prior, dict(entry="tempered", prior=0), E_ARG, "n_prior must be 1 or n_start (got 0 for 2 fits)"),
    (sample_prior, dict(entry="ensemble", prior=1, null=("scale",)), E_ARG, "the prior's scale / kind / p0 / p1 is NULL"),
    (sample_prior, dict(entry="tempered", prior=1, null=("kind",)), E_ARG, "the prior's scale / kind / p0 / p1 is NULL"),
    (sample_prior, dict(entry="ensemble", prior=2, null=("p0",)), E_ARG, "the prior's scale / kind / p0 / p1 is NULL"),
    (sample_prior, dict(entry="tempered", prior=2, null=("p1",)), E_ARG, "the prior's scale / kind / p0 / p1 is NULL"),
    # two faults
    (sample_prior, dict(entry="ensemble", prior=1, size=8, split=0), E_ARG, "the prior descriptor's size is 8, this library's misti_prior_t has 40 bytes"),
    (sample_prior, dict(entry="ensemble", prior=3, n_box=3), E_ARG, "n_box must be 1 or n_start (got 3 for 2 searches)"),
    (sample_prior, dict(entry="tempered", prior=3, n_box=3), E_ARG, "n_box must be 1 or n_start (got 3 for 2 fits)"),
    (sample_prior, dict(entry="ensemble", prior=3, null=("scale",)), E_ARG, "n_prior must be 1 or n_start (got 3 for 2 searches)"),
    (sample_prior, dict(entry="tempered", prior=3, null=("scale",)), E_ARG, "n_prior must be 1 or n_start (got 3 for 2 fits)"),
    (sample_prior, dict(entry="tempered", prior=3, thin=0), E_ARG, "thin must be >= 1"),
    (sample_prior, dict(entry="ensemble", prior=3, n_rep=0), E_ARG, "n_rep must be >= 1 (got 0)"),
]


@pytest.mark.parametrize("door, kw, code, text", CASES, ids=["%s-%d" % (c[0].__name__, i) for i, c in enumerate(CASES)])
def test_the_refusal_and_its_text(door, kw, code, text):
    rc, why = door(**kw)
    print(door.__name__, kw, rc, repr(why))
    assert (rc, why) == (code, text)
