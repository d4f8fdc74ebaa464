"""Host side of the search descriptor (no GPU): misti_search_t / misti_hops_t in the header against the ctypes structures, the size
check, the refusals of misti_search against those of the older entry points, and which fields Engine's ten search methods and
optimize's six fits hand to misti_search."""
import ctypes as C

import numpy as np
import pytest

import search_forms as F

E_ARG = -1


def _full(N=2, n_start=2, hops=True):
    """Valid fields for 2 starts of a 2-parameter model against a 3-row table; N = 3: the split as the last coordinate."""
    S = n_start
    f = dict(split_time=20.0, split_times=np.array([20.0, 21.5]) if N == 2 else None, n_start=S, starts=np.full((2, N), 0.5),
             rows=np.array([0, 2], dtype=np.int32), n_rep=3, jsfs=np.ones((3, 8)), band_bounds=None, pulse_times=None,
             n_box=1, box_lo=np.zeros((1, N)), box_hi=np.ones((1, N)), xatol=1e-4, fatol=1e-4, maxiter=400,
             x=np.empty((2, N)), llh=np.empty(2), nit=None, nfev=None, status=None)
    f["hops"] = dict(niter=2, T=0.5, stepsize=0.5, interval=50, target_accept_rate=0.5, stepwise_factor=0.9, nm_maxfev=400,
                     uniforms=np.full((2, 2, N + 1), 0.5)) if hops else None
    return f


# ---- the structures ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c_name, py_name", [("misti_search_t", "Search"), ("misti_hops_t", "Hops")])
def test_header_declares_the_fields_of_the_structures_in_their_order(c_name, py_name):
    from misti_amd import _lib
    assert F.struct_fields(c_name) == [n for n, _ in getattr(_lib, py_name)._fields_]


def test_the_header_names_the_split_modes_as_the_binding_does():
    from misti_amd import _lib
    hdr = F.header()
    for name in ("ONE", "PER_START", "FITTED"):
        assert "#define MISTI_SPLIT_%s" % name in hdr
        assert int(hdr.split("#define MISTI_SPLIT_%s" % name)[1].split()[0]) == getattr(_lib, "SPLIT_" + name)


def test_sizes_agree_with_the_library():
    """A well-formed descriptor gets past the size check to the NULL context; the size off by 8 does not; NULL is refused."""
    from misti_amd import _lib
    lib = _lib.load()
    f = F.form_of("misti_basinhopping_box", _full())
    q = F.descriptor(f)
    assert q.size == C.sizeof(_lib.Search)
    assert lib.misti_search(None, C.byref(q)) == E_ARG and b"ctx is NULL" in lib.misti_last_error()
    for off in (-8, 8):
        q.size = C.sizeof(_lib.Search) + off
        assert lib.misti_search(None, C.byref(q)) == E_ARG
        msg = lib.misti_last_error().decode()
        assert "size" in msg and str(C.sizeof(_lib.Search)) in msg and "ctx" not in msg, msg
    assert lib.misti_search(None, None) == E_ARG and b"descriptor is NULL" in lib.misti_last_error()
    # the hops record has no size of its own: a Hops of another layout would move niter / interval / nm_maxfev / uniforms, and the
    # library would refuse one of them - here every one of them is read where the binding put it
    for change, text in ((dict(niter=-1), "negative number of hops"), (dict(interval=0), "must be >= 1"), (dict(nm_maxfev=0), "must be >= 1"),
                         (dict(uniforms=None), "uniforms is NULL")):
        g = dict(f, hops=dict(f["hops"], **change))
        assert lib.misti_search(None, C.byref(F.descriptor(g))) == E_ARG and text in lib.misti_last_error().decode(), change


def test_descriptor_only_refusals():
    from misti_amd import _lib
    lib = _lib.load()
    f = F.form_of("misti_basinhopping_rows", _full())
    f["nit"] = np.empty(2, dtype=np.int32)
    assert lib.misti_search(None, C.byref(F.descriptor(f))) == E_ARG and b"with hops, nit / nfev / status" in lib.misti_last_error()
    f = F.form_of("misti_nm_solve_rows", _full())
    f["split"] = 3
    assert lib.misti_search(None, C.byref(F.descriptor(f))) == E_ARG and b"split mode 3" in lib.misti_last_error()


# ---- the same refusals through both doors ------------------------------------------------------------------------------------------
# what nm_check decides before it looks at the context: (name, the fields it changes, the fields the symbol must have for the case)
BAD = [("negative n_start", dict(n_start=-1), ()),
       ("NULL starts", dict(starts=None), ()), ("NULL x", dict(x=None), ()), ("NULL llh", dict(llh=None), ()),
       ("n_rep == 0", dict(n_rep=0), ("n_rep",)),
       ("row out of range", dict(rows=np.array([0, 3], dtype=np.int32)), ("rows",)),
       ("negative row", dict(rows=np.array([-1, 0], dtype=np.int32)), ("rows",)),
       ("non-finite split time", dict(split_times=np.array([20.0, np.inf])), ("split_times",)),
       ("maxiter == 0", dict(maxiter=0), ()),
       ("NULL uniforms", dict(hops=dict(uniforms=None)), ("hops",)),
       ("interval == 0", dict(hops=dict(interval=0)), ("hops",)),
       ("nothing wrong but the context", dict(), ())]
# (misti_basinhopping keeps its own, older order of checks - the context first - and is not in this table)
DOORS = [s for s in F.LEGACY if s != "misti_basinhopping"]


@pytest.mark.parametrize("symbol", DOORS)
def test_the_same_refusals_through_both_doors(symbol):
    from misti_amd import _lib
    lib = _lib.load()
    ran = 0
    for fitted in ((False, True) if symbol.endswith("_box") else (symbol.endswith("_split"),)):
        for name, change, needs in BAD:
            f = F.form_of(symbol, _full(N=3 if fitted else 2))
            names = [F.RENAMED.get(n, n) for n in F.prototype_names(symbol)]
            if not all(F.is_hop_form(symbol) if k == "hops" else k in names and f[k] is not None for k in needs):
                continue                                                # the symbol has no such argument
            for k, v in change.items():
                f[k] = dict(f[k], **v) if k == "hops" else v
            rc_old = getattr(lib, symbol)(None, *F.legacy_args(symbol, f))
            msg_old = lib.misti_last_error()
            rc_new = lib.misti_search(None, C.byref(F.descriptor(f)))
            msg_new = lib.misti_last_error()
            assert rc_old == rc_new == E_ARG, (name, rc_old, rc_new)
            assert msg_old == msg_new and msg_old, (name, msg_old, msg_new)
            assert (b"ctx is NULL" in msg_old) == (not change), (name, msg_old)
            ran += 1
    assert ran >= 5, ran


# ---- the fields Engine and optimize choose -----------------------------------------------------------------------------------------
POINTERS = ("split_times", "rows", "band_bounds", "pulse_times", "box_lo", "box_hi", "nit", "nfev", "status")


@pytest.fixture
def seen(monkeypatch):
    """An Engine without a device (2 parameters, 1 band, 2 pulses) whose misti_search calls are recorded instead of run."""
    from misti_amd import _lib
    from misti_amd.engine import Engine
    lib = _lib.load()
    calls = []

    def misti_search(ctx, ref):
        q = ref._obj
        assert q.size == C.sizeof(_lib.Search) and q.starts and q.jsfs and q.x and q.llh
        N = 2 + (q.split == _lib.SPLIT_FITTED)
        C.memset(q.x, 0, 8 * N * q.n_start)
        C.memset(q.llh, 0, 8 * q.n_start)
        rec = dict(split=q.split, n_start=q.n_start, n_rep=q.n_rep, n_box=q.n_box, maxiter=q.maxiter, tol=(q.xatol, q.fatol),
                   given={k for k in POINTERS if getattr(q, k)}, hops=None)
        if q.hops:
            h = q.hops.contents
            assert h.uniforms and h.nfev and h.failures and h.accepted
            rec["hops"] = (h.niter, h.T, h.stepsize, h.interval, h.target_accept_rate, h.stepwise_factor, h.nm_maxfev)
        calls.append(rec)
        return 0
    monkeypatch.setattr(lib, "misti_search", misti_search)
    monkeypatch.setattr(lib, "misti_nm_last_stats", lambda ctx, stats: 0)
    monkeypatch.setattr(lib, "misti_nm_last_spec_iterations", lambda ctx, n: 0)
    e = Engine.__new__(Engine)
    e._lib, e._ctx, e._pid = lib, C.c_void_p(), -1                      # (another process' context: close() leaves it alone)
    e.n_param, e.n_band, e.n_pulse = 2, 1, 2
    return e, calls


S = 4
ST2, ST3 = np.full((S, 2), 0.1), np.full((S, 3), 0.1)
SP, RW, TAB = np.arange(20.0, 20.0 + S), np.zeros(S, dtype=np.int32), np.ones((3, 8))
BB, PT = np.zeros((S, 1, 2), dtype=np.int32), np.zeros((S, 2), dtype=np.int32)
BOX2, BOX3 = (np.zeros(2), np.ones(2)), (np.zeros((S, 3)), np.ones((S, 3)))
OUT = {"nit", "nfev", "status"}
HOP = dict(niter=3, T=0.25, stepsize=0.125, interval=7, target_accept_rate=0.75, stepwise_factor=0.5, nm_maxfev=90)
HOP_T = (3, 0.25, 0.125, 7, 0.75, 0.5, 90)


def test_engine_methods_choose_the_fields(seen):
    """Per public method: the split mode, which pointers are set, the box, the hops - what each older entry point is."""
    from misti_amd import _lib
    e, calls = seen
    ONE, PER, FIT = _lib.SPLIT_ONE, _lib.SPLIT_PER_START, _lib.SPLIT_FITTED
    table = [
        (lambda: e.nm_solve(ST2, 20.0, TAB[0], tol=1e-3, maxiter=50), ONE, set(), 0, False),
        (lambda: e.nm_solve_rows(ST2, SP, RW, TAB, tol=1e-3, maxiter=50), PER, {"split_times", "rows"}, 0, False),
        (lambda: e.nm_solve_bounds(ST2, SP, RW, TAB, BB, tol=1e-3, maxiter=50), PER, {"split_times", "rows", "band_bounds"}, 0, False),
        (lambda: e.nm_solve_bounds(ST2, SP, RW, TAB, None, tol=1e-3, maxiter=50), PER, {"split_times", "rows"}, 0, False),
        (lambda: e.nm_solve_pulses(ST2, SP, RW, TAB, BB, PT, tol=1e-3, maxiter=50), PER, {"split_times", "rows", "band_bounds", "pulse_times"}, 0, False),
        (lambda: e.nm_solve_pulses(ST2, SP, RW, TAB, None, PT, tol=1e-3, maxiter=50), PER, {"split_times", "rows", "pulse_times"}, 0, False),
        (lambda: e.nm_solve_split(ST3, RW, TAB, BB, PT, tol=1e-3, maxiter=50), FIT, {"rows", "band_bounds", "pulse_times"}, 0, False),
        (lambda: e.nm_solve_split(ST3, RW, TAB, tol=1e-3, maxiter=50), FIT, {"rows"}, 0, False),
        (lambda: e.nm_solve_box(ST2, RW, TAB, BOX2, split_times=SP, band_bounds=BB, tol=1e-3, maxiter=50), PER,
         {"split_times", "rows", "band_bounds", "box_lo", "box_hi"}, 1, False),
        (lambda: e.nm_solve_box(ST3, RW, TAB, BOX3, pulse_times=PT, tol=1e-3, maxiter=50), FIT, {"rows", "pulse_times", "box_lo", "box_hi"}, S, False),
        (lambda: e.basinhopping(ST2, 20.0, TAB[0], range(S), nm_maxiter=50, xatol=1e-3, fatol=1e-3, **HOP), ONE, set(), 0, True),
        (lambda: e.basinhopping_rows(ST2, SP, RW, TAB, range(S), BB, PT, nm_maxiter=50, xatol=1e-3, fatol=1e-3, **HOP), PER,
         {"split_times", "rows", "band_bounds", "pulse_times"}, 0, True),
        (lambda: e.basinhopping_rows(ST2, SP, RW, TAB, range(S), nm_maxiter=50, xatol=1e-3, fatol=1e-3, **HOP), PER, {"split_times", "rows"}, 0, True),
        (lambda: e.basinhopping_split(ST3, RW, TAB, range(S), BB, nm_maxiter=50, xatol=1e-3, fatol=1e-3, **HOP), FIT, {"rows", "band_bounds"}, 0, True),
        (lambda: e.basinhopping_box(ST2, RW, TAB, range(S), BOX2, split_times=SP, nm_maxiter=50, xatol=1e-3, fatol=1e-3, **HOP), PER,
         {"split_times", "rows", "box_lo", "box_hi"}, 1, True),
        (lambda: e.basinhopping_box(ST3, RW, TAB, range(S), BOX3, band_bounds=BB, pulse_times=PT, nm_maxiter=50, xatol=1e-3, fatol=1e-3, **HOP), FIT,
         {"rows", "band_bounds", "pulse_times", "box_lo", "box_hi"}, S, True),
    ]
    for i, (call, split, given, n_box, hops) in enumerate(table):
        del calls[:]
        r = call()
        assert len(calls) == 1, i
        c = calls[0]
        assert (c["split"], c["n_box"], c["n_start"], c["n_rep"]) == (split, n_box, S, 1 if split == ONE else 3), (i, c)
        assert c["given"] == given | (set() if hops else OUT), (i, c)
        assert c["maxiter"] == 50 and c["tol"] == (1e-3, 1e-3), (i, c)
        assert c["hops"] == (HOP_T if hops else None), (i, c)
        assert r["x"].shape == (S, 3 if split == FIT else 2) and set(r) >= ({"nfev", "failures", "accepted"} if hops else OUT), i
    # the defaults: SciPy's budgets for the coordinates the search has, the reference's 1000 without hops
    del calls[:]
    e.nm_solve_rows(ST2, SP, RW, TAB)
    e.basinhopping_rows(ST2, SP, RW, TAB, range(S), niter=1)
    e.basinhopping_split(ST3, RW, TAB, range(S), niter=1)
    assert [c["maxiter"] for c in calls] == [1000, 400, 600]
    assert calls[1]["hops"] == (1, 0.5, 0.5, 50, 0.5, 0.9, 400) and calls[2]["hops"][-1] == 600
    # the result keys each form has had
    assert "speculative_iterations" not in e.basinhopping(ST2, 20.0, TAB[0], range(S), niter=1)
    assert "speculative_iterations" in e.basinhopping_rows(ST2, SP, RW, TAB, range(S), niter=1)
    assert "split" not in e.nm_solve_pulses(ST2, SP, RW, TAB, None, None) and "split" not in e.basinhopping_rows(ST2, SP, RW, TAB, range(S), niter=1)
    for r in (e.nm_solve_split(ST3, RW, TAB), e.basinhopping_split(ST3, RW, TAB, range(S), niter=1)):
        assert np.array_equal(r["split"], r["x"][:, -1])
    for r in (e.nm_solve_box(ST2, RW, TAB, BOX2, split_times=SP), e.basinhopping_box(ST2, RW, TAB, range(S), BOX2, split_times=SP, niter=1)):
        assert np.array_equal(r["split"], SP)


def test_optimize_fits_choose_the_fields(seen, monkeypatch):
    """Each of the six fits is ONE misti_search call with the fields its arguments ask for."""
    from misti_amd import _lib, optimize
    e, calls = seen
    PER, FIT = _lib.SPLIT_PER_START, _lib.SPLIT_FITTED
    rows, starts, splits = np.ones((2, 8)), [[0.1, 0.2]], [20.0, 21.0]
    bb, pt = [[4, -1]], [10, 5]
    b2, b3 = (np.zeros(2), np.ones(2)), (np.zeros(3), np.full(3, 30.0))
    best = np.array([[1, 0], [2, -1]])
    monkeypatch.setattr(optimize, "scan_best", lambda *a, **k: (best, np.zeros(best.shape), np.zeros(3, dtype=np.int32)))
    polish = lambda **k: optimize.scan_polish(e, [20.0, 21.0, 22.0], np.full((3, 2), 0.1), rows, 2, **k)
    models2 = [(20.0, [[4, -1]]), (21.0, [[5, -1]])]
    models3 = [m + ([10, 5],) for m in models2]
    h = dict(niter=2, interval=9)
    table = [
        (lambda: polish(), PER, {"split_times", "rows"}, 0, None, 3),
        (lambda: polish(band_bounds=np.zeros((3, 1, 2), dtype=np.int32)), PER, {"split_times", "rows", "band_bounds"}, 0, None, 3),
        (lambda: polish(band_bounds=np.zeros((3, 1, 2), dtype=np.int32), pulse_times=np.zeros((3, 2), dtype=np.int32)), PER,
         {"split_times", "rows", "band_bounds", "pulse_times"}, 0, None, 3),
        (lambda: polish(box=b2), PER, {"split_times", "rows", "box_lo", "box_hi"}, 1, None, 3),
        (lambda: optimize.bootstrap_profile(e, splits, rows, starts), PER, {"split_times", "rows"}, 0, None, 4),
        (lambda: optimize.bootstrap_profile(e, splits, rows, starts, box=b2), PER, {"split_times", "rows", "box_lo", "box_hi"}, 1, None, 4),
        (lambda: optimize.bootstrap_profile_global(e, splits, rows, starts, **h), PER, {"split_times", "rows"}, 0, (2, 9, 400), 4),
        (lambda: optimize.bootstrap_profile_global(e, splits, rows, starts, box=b2, **h), PER, {"split_times", "rows", "box_lo", "box_hi"}, 1, (2, 9, 400), 4),
        (lambda: optimize.split_fit(e, rows, starts, splits), FIT, {"rows"}, 0, None, 4),
        (lambda: optimize.split_fit(e, rows, starts, splits, band_bounds=bb, pulse_times=pt, box=b3), FIT,
         {"rows", "band_bounds", "pulse_times", "box_lo", "box_hi"}, 1, None, 4),
        (lambda: optimize.split_fit_global(e, rows, starts, splits, pulse_times=pt, **h), FIT, {"rows", "pulse_times"}, 0, (2, 9, 600), 4),
        (lambda: optimize.split_fit_global(e, rows, starts, splits, box=b3, **h), FIT, {"rows", "box_lo", "box_hi"}, 1, (2, 9, 600), 4),
        (lambda: optimize.sweep_profile(e, models2, rows, starts), PER, {"split_times", "rows", "band_bounds"}, 0, None, 4),
        (lambda: optimize.sweep_profile(e, models3, rows, starts), PER, {"split_times", "rows", "band_bounds", "pulse_times"}, 0, None, 4),
    ]
    for i, (call, split, given, n_box, hops, n_start) in enumerate(table):
        del calls[:]
        call()
        assert len(calls) == 1, (i, len(calls))
        c = calls[0]
        assert (c["split"], c["n_box"], c["n_start"], c["n_rep"]) == (split, n_box, n_start, 2), (i, c)
        assert c["given"] == given | (OUT if hops is None else set()), (i, c)
        assert (c["hops"] and (c["hops"][0], c["hops"][3], c["hops"][6])) == hops, (i, c)
