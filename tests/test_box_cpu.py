"""Host side of the box constraints (no GPU): optimize.box_initial_simplex / box_clip against SciPy's own bounded Nelder-Mead, the
binding of misti_nm_solve_box / misti_basinhopping_box against their prototypes in include/misti_hip.h, what the two entry points
answer without a context, and the `--box` refusals."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

from conftest import ROOT

INF = np.inf


def scipy_first_points(x0, lo, hi):
    """The first N + 1 points scipy.optimize.minimize(method='Nelder-Mead', bounds=Bounds(lo, hi)) evaluates: its initial simplex."""
    from scipy import optimize
    seen = []

    def f(x):
        seen.append(np.array(x, dtype=np.float64))
        return float(np.sum((x - 0.3) ** 2))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                  # "Initial guess is not within the specified bounds"; maxfev reached
        optimize.minimize(f, np.asarray(x0, dtype=float), method="Nelder-Mead", bounds=optimize.Bounds(lo, hi),
                          options=dict(maxfev=len(x0) + 1))
    return np.array(seen[:len(x0) + 1])


# per N: x0 inside, outside (below and above), exactly on hi (the 2 ub - sim branch), a zero coordinate (the 0.00025 step), lo == hi,
# +-inf bounds, a start so close under hi that its 5 % step crosses it and the reflection falls below lo
CASES = [
    ([0.2], [0.0], [1.0]),
    ([1.7], [0.0], [1.0]),
    ([-0.4], [0.1], [1.0]),
    ([1.0], [0.0], [1.0]),
    ([0.0], [-1.0], [1.0]),
    ([0.0], [0.0], [0.0001]),
    ([0.5], [0.5], [0.5]),
    ([0.7], [-INF], [INF]),
    ([63.0], [61.5], [INF]),
    ([0.99], [0.98], [1.0]),
    ([0.2, 63.0], [0.0, 61.5], [1.0, 64.5]),
    ([1.7, 70.0], [0.0, 61.5], [1.0, 64.5]),
    ([0.35, 64.5], [0.0, 61.5], [0.35, 64.5]),
    ([0.0, 63.0], [0.0, 63.0], [0.0001, 63.0]),
    ([0.2, 63.0], [-INF, -INF], [INF, INF]),
    ([0.2, 64.4], [-INF, 64.3], [0.2, 64.5]),
    ([0.2, 0.05, 63.0], [0.0, 0.0, 61.5], [1.0, 1.0, 64.5]),
    ([0.2, 0.05, 63.0], [0.0, 0.05, 61.5], [0.1, 0.05, 62.0]),
    ([0.1, 0.0, 64.5], [0.0, 0.0, 61.5], [0.1, 1.0, 64.5]),
    ([0.2, 0.0, 63.0], [-INF, -1.0, 61.5], [INF, 0.0, INF]),
    ([-3.0, 5.0, 63.0], [0.0, 0.0, 63.0], [INF, 0.01, 63.0]),
]


@pytest.mark.parametrize("x0, lo, hi", CASES)
def test_box_initial_simplex_equals_scipys_bit_for_bit(x0, lo, hi):
    from misti_amd.optimize import box_initial_simplex
    ref = scipy_first_points(x0, lo, hi)
    got = box_initial_simplex(x0, lo, hi)
    assert got.shape == ref.shape == (len(x0) + 1, len(x0))
    assert got.tobytes() == ref.tobytes(), (got, ref)
    lo_, hi_ = np.asarray(lo), np.asarray(hi)
    assert (got >= lo_).all() and (got <= hi_).all()


def test_every_branch_of_the_rule_is_among_the_cases():
    """The cases above are not idle: some start lies outside its box, some vertex is reflected at the upper bound, some reflection
    is clipped at the lower bound, some coordinate takes the zero step, some is fixed, some box is infinite - and N is 1, 2 and 3."""
    from misti_amd.optimize import initial_simplex
    outside = reflected = clipped_low = zero = fixed = infinite = 0
    for x0, lo, hi in CASES:
        x0, lo, hi = (np.asarray(v, dtype=float) for v in (x0, lo, hi))
        outside += bool(((x0 < lo) | (x0 > hi)).any())
        c = np.clip(x0, lo, hi)
        sim = initial_simplex(c[None])[0]
        over = sim > hi
        reflected += bool(over.any())
        with np.errstate(invalid="ignore"):
            clipped_low += bool((over & (2 * hi - sim < lo)).any())
        zero += bool((c == 0).any())
        fixed += bool((lo == hi).any())
        infinite += bool(np.isinf(lo).any() or np.isinf(hi).any())
    assert min(outside, reflected, clipped_low, zero, fixed, infinite) >= 2, (outside, reflected, clipped_low, zero, fixed, infinite)
    assert {len(c[0]) for c in CASES} == {1, 2, 3}


def test_box_initial_simplex_per_start_boxes_and_box_clip():
    from misti_amd.optimize import box_clip, box_initial_simplex
    x0 = np.array([[0.2, 63.0], [1.7, 70.0], [0.35, 64.5]])
    lo = np.array([[0.0, 61.5], [0.0, 61.5], [0.0, 61.5]])
    hi = np.array([[1.0, 64.5], [1.0, 64.5], [0.35, 64.5]])
    got = box_initial_simplex(x0, lo, hi)
    assert got.shape == (3, 3, 2)
    for s in range(3):
        assert got[s].tobytes() == scipy_first_points(x0[s], lo[s], hi[s]).tobytes()
    assert box_initial_simplex(x0[:2], lo[0], hi[0]).tobytes() == got[:2].tobytes()          # one box for every start
    x = np.array([-1.0, 0.5, 2.0, np.nan, -0.0, 7.0])
    c = box_clip(x, [0.0, 0.0, 0.0, 0.0, 0.0, -INF], [1.0, 1.0, 1.0, 1.0, 1.0, INF])
    assert np.array_equal(c, [0.0, 0.5, 1.0, np.nan, 0.0, 7.0], equal_nan=True)
    assert c.tobytes() == np.clip(x, [0.0, 0.0, 0.0, 0.0, 0.0, -INF], [1.0, 1.0, 1.0, 1.0, 1.0, INF]).tobytes()


C_TYPES = {"misti_ctx*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double, "const double*": C.c_void_p,
           "const int32_t*": C.c_void_p, "double*": C.c_void_p, "int32_t*": C.c_void_p}


def prototype(symbol):
    hdr = open(os.path.join(ROOT, "include", "misti_hip.h")).read()
    m = re.search(r"^int %s\s*\(([^;]*)\);" % symbol, hdr, re.M)
    assert m, "no prototype of " + symbol
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    types = []
    for a in args:
        t, name = a.rsplit(" ", 1)
        if name.startswith("*"):
            t += "*"
        types.append(C_TYPES[t])
    return args, types


@pytest.mark.parametrize("symbol, n_args", [("misti_nm_solve_box", 20), ("misti_basinhopping_box", 28)])
def test_bindings_match_the_header_prototypes(symbol, n_args):
    from misti_amd import _lib
    args, types = prototype(symbol)
    res, bound = _lib.SYMBOLS[symbol]
    assert res is C.c_int
    assert len(bound) == len(types) == n_args
    assert bound == types, [(a, b, t) for a, b, t in zip(args, bound, types) if b is not t]
    # the search arguments are the same in both, and behind them the tails of the forms without a box
    assert bound[:12] == _lib.SYMBOLS["misti_nm_solve_box"][1][:12]
    tail_of = {"misti_nm_solve_box": "misti_nm_solve_split", "misti_basinhopping_box": "misti_basinhopping_split"}[symbol]
    assert bound[12:] == _lib.SYMBOLS[tail_of][1][8:]


def test_the_abi_version_stays_6():
    from misti_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "misti_hip.h")).read()
    assert re.search(r"^#define MISTI_ABI_VERSION 6$", hdr, re.M)
    assert _lib.ABI_VERSION == 6
    assert _lib.load().misti_abi_version() == 6


def test_without_a_context_both_entry_points_return_e_arg():
    """The library loads without a device; every check of the arguments comes before the first HIP call."""
    from misti_amd import _lib
    lib = _lib.load()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    starts, rows, table = np.array([[0.1, 0.2, 63.0]]), np.zeros(1, dtype=np.int32), np.ones((1, 8))
    lo, hi = np.zeros((1, 3)), np.ones((1, 3))
    x, llh, uni = np.empty((1, 3)), np.empty(1), np.zeros((1, 2, 4))
    search = [1, ptr(starts), None, ptr(rows), 1, ptr(table), None, None, 1, ptr(lo), ptr(hi)]
    assert lib.misti_nm_solve_box(None, *search, 1e-4, 1e-4, 10, ptr(x), ptr(llh), None, None, None) == -1
    assert b"ctx is NULL" in lib.misti_last_error()
    assert lib.misti_basinhopping_box(None, *search, 2, 0.5, 0.5, 50, 0.5, 0.9, 1e-4, 1e-4, 60, 60, ptr(uni),
                                      ptr(x), ptr(llh), None, None, None) == -1
    assert b"ctx is NULL" in lib.misti_last_error()


BASE = ["a.psmc", "b.psmc", "d.sfs", "20", "-mi", "1", "4", "20", "0.2", "1"]


@pytest.mark.parametrize("extra, text", [
    (["--box", "0", "0", "1"], "--box constrains the searches of --grid-solve, --fit-st or --polish"),
    (["--grid-st", "18", "20", "--box", "0", "0", "1"], "--box constrains the searches of --grid-solve, --fit-st or --polish"),
    (["--grid-st", "18", "20", "--top", "2", "--box", "0", "0", "1"], "--box constrains the searches of --grid-solve, --fit-st or --polish"),
    (["--grid-st", "18", "20", "--grid-solve", "--box", "st", "18", "20"], "--box st bounds the FITTED split: it needs --fit-st"),
    (["--grid-st", "18", "20", "--top", "2", "--polish", "--box", "st", "18", "20"], "--box st bounds the FITTED split: it needs --fit-st"),
    (["--grid-st", "18", "20", "--fit-st", "--box", "0", "1", "0.5"], "--box 0: the lower bound 1 is greater than the upper bound 0.5"),
    (["--grid-st", "18", "20", "--fit-st", "--box", "st", "inf", "-inf"], "--box st: the lower bound inf is greater than the upper bound -inf"),
    (["--grid-st", "18", "20", "--grid-solve", "--hops", "2", "--box", "0", "0.5", "0.1"], "--box 0: the lower bound 0.5 is greater"),
    (["--grid-st", "18", "20", "--fit-st", "--box", "1", "0", "1"], "--box 1: no such coordinate"),
    (["--grid-st", "18", "20", "--fit-st", "--box", "0", "nan", "1"], "--box 0: a bound is NaN"),
    (["--grid-st", "18", "20", "--fit-st", "--box", "0", "0", "1", "--box", "0", "0", "2"], "--box 0 is given twice"),
    (["--grid-st", "18", "20", "--fit-st", "--box", "0", "zero", "1"], "LO and HI are numbers"),
])
def test_cli_box_refusals_come_before_any_file_or_device(capsys, monkeypatch, extra, text):
    """The files do not exist and opening a device would raise: the refusal comes first."""
    from misti_amd import cli, engine

    def no_device(*a, **k):
        raise AssertionError("a device was opened")
    monkeypatch.setattr(engine.Engine, "__init__", no_device)
    monkeypatch.setattr(cli, "Engine", no_device)
    rc = cli.main(BASE + extra)
    assert rc == 2 and text in capsys.readouterr().err


def test_cli_box_is_not_offered_with_a_sweep(capsys):
    from misti_amd import cli
    rc = cli.main(["a.psmc", "b.psmc", "d.sfs", "20", "-mi", "1", "{a}", "20", "0.2", "1", "--grid-solve", "--sweep", "a", "4", "5", "--box", "0", "0", "1"])
    assert rc == 2 and "--box constrains the searches of ONE model: --sweep / --sweep-pu are not offered" in capsys.readouterr().err


def test_cli_box_builds_the_arrays_of_the_search():
    from misti_amd import cli
    a = cli.build_parser().parse_args(BASE + ["--grid-st", "18", "20", "--fit-st", "--box", "0", "0", "0.5", "--box", "st", "-inf", "19.5"])
    assert cli.box_error(a) is None
    lo, hi = cli._box(a, 1)
    assert np.array_equal(lo, [0.0, -INF]) and np.array_equal(hi, [0.5, 19.5])
    a = cli.build_parser().parse_args(BASE + ["--grid-st", "18", "20", "--grid-solve", "--hops", "3", "--box", "0", "0.1", "0.1"])
    assert cli.box_error(a) is None
    lo, hi = cli._box(a, 1)
    assert np.array_equal(lo, [0.1]) and np.array_equal(hi, [0.1])
    a = cli.build_parser().parse_args(BASE + ["--grid-st", "18", "20", "--top", "2", "--polish", "--box", "0", "0", "inf"])
    assert cli.box_error(a) is None and cli.top_error(a) is None
    a = cli.build_parser().parse_args(BASE + ["--grid-st", "18", "20", "--fit-st"])
    assert cli.box_error(a) is None and cli._box(a, 1) is None


class FakeEngine:
    """Stands for the Engine's searches: records which one was called and with which box."""
    n_param = 2
    n_band = n_pulse = 0

    def __init__(self):
        self.calls = []

    def _res(self, S, N, hops):
        x = np.zeros((S, N))
        r = dict(x=x, llh=-np.arange(S, dtype=float), split=x[:, -1].copy(), iterations_issued=1, slots=1, speculative_iterations=0)
        z = lambda: np.zeros(S, dtype=np.int32)
        r.update(dict(nfev=z(), failures=z(), accepted=z()) if hops else dict(nit=z(), nfev=z(), status=z()))
        return r

    def nm_solve_rows(self, starts, split_times, rows, jsfs, tol=1e-4, maxiter=1000):
        self.calls.append(("nm_solve_rows", None))
        return self._res(len(rows), 2, False)

    def nm_solve_split(self, starts, rows, table, band_bounds=None, pulse_times=None, tol=1e-4, maxiter=1000):
        self.calls.append(("nm_solve_split", None))
        return self._res(len(rows), 3, False)

    def nm_solve_box(self, starts, rows, table, box, split_times=None, band_bounds=None, pulse_times=None, tol=1e-4, maxiter=1000):
        self.calls.append(("nm_solve_box", box, None if split_times is None else np.array(split_times)))
        return self._res(len(rows), np.asarray(starts).shape[1], False)

    def basinhopping_rows(self, starts, split_times, rows, table, rngs, **kw):
        self.calls.append(("basinhopping_rows", None))
        return self._res(len(rows), 2, True)

    def basinhopping_split(self, starts, rows, table, rngs, **kw):
        self.calls.append(("basinhopping_split", None))
        return self._res(len(rows), 3, True)

    def basinhopping_box(self, starts, rows, table, rngs, box, split_times=None, **kw):
        self.calls.append(("basinhopping_box", box, None if split_times is None else np.array(split_times)))
        return self._res(len(rows), np.asarray(starts).shape[1], True)


def test_the_fits_pass_the_box_through_and_leave_the_old_calls_alone():
    from misti_amd import optimize
    rows = np.ones((2, 8))
    e = FakeEngine()
    optimize.bootstrap_profile(e, [62.0, 63.0], rows, [[0.1, 0.2]])
    optimize.split_fit(e, rows, [[0.1, 0.2]], [62.0, 63.0])
    optimize.bootstrap_profile_global(e, [62.0, 63.0], rows, [[0.1, 0.2]], niter=2)
    optimize.split_fit_global(e, rows, [[0.1, 0.2]], [62.0, 63.0], niter=2)
    assert [c[0] for c in e.calls] == ["nm_solve_rows", "nm_solve_split", "basinhopping_rows", "basinhopping_split"]
    e = FakeEngine()
    b2, b3 = ([0.0, 0.0], [1.0, 1.0]), ([0.0, 0.0, 61.0], [1.0, 1.0, 64.0])
    optimize.bootstrap_profile(e, [62.0, 63.0], rows, [[0.1, 0.2]], box=b2)
    optimize.split_fit(e, rows, [[0.1, 0.2]], [62.0, 63.0], box=b3)
    optimize.bootstrap_profile_global(e, [62.0, 63.0], rows, [[0.1, 0.2]], niter=2, box=b2)
    optimize.split_fit_global(e, rows, [[0.1, 0.2]], [62.0, 63.0], niter=2, box=b3)
    assert [c[0] for c in e.calls] == ["nm_solve_box", "nm_solve_box", "basinhopping_box", "basinhopping_box"]
    assert [c[1] for c in e.calls] == [b2, b3, b2, b3]
    assert np.array_equal(e.calls[0][2], [62.0, 63.0, 62.0, 63.0]) and e.calls[1][2] is None
    assert np.array_equal(e.calls[2][2], [62.0, 63.0, 62.0, 63.0]) and e.calls[3][2] is None
