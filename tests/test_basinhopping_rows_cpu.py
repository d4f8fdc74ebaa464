"""Host side of basin hopping per bootstrap row (no GPU): the `--hops` refusals, the order in which draw_uniforms draws against
SciPy's own runner with the split as one coordinate more, optimize.split_fit_global / bootstrap_profile_global on an engine-shaped
double that IS SciPy on an analytic objective, the bindings against their prototypes, and the argument errors of
misti_basinhopping_rows / misti_basinhopping_split that need no context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- --hops ------------------------------------------------------------------------------------------------------------------------
BASE = ["a.psmc", "b.psmc", "d.sfs", "20", "-mi", "1", "4", "20", "0.2", "1"]
FIT = ["--grid-st", "18", "20", "--fit-st"]
SOLVE = ["--grid-st", "18", "20", "--grid-solve"]


@pytest.mark.parametrize("extra, text", [
    (["--hops", "2"], "give one of them"),                                              # neither --fit-st nor --grid-solve
    (["--grid-st", "18", "20", "--hops", "2"], "give one of them"),
    (FIT + ["--hops", "0"], "at least 1"),
    (SOLVE + ["--hops", "-3"], "at least 1"),
    (FIT + ["--hops", "2", "--gpus", "2"], "--hops runs on one GPU"),
    (SOLVE + ["--hops", "2", "--gpus", "2"], "--hops runs on one GPU"),
    (FIT + ["--hops", "2", "--devices", "0,1"], "--hops runs on one GPU"),
    (SOLVE + ["--hops", "2", "--devices", "0,1"], "--hops runs on one GPU"),
    (["--grid-solve", "--hops", "2", "--sweep", "a", "4", "5"], "--sweep / --sweep-pu are not offered"),
    (["--grid-solve", "--hops", "2", "--sweep-pu", "t", "4", "5"], "--sweep / --sweep-pu are not offered"),
    (FIT + ["--hops", "2", "--sweep", "a", "4", "5"], "--sweep / --sweep-pu are not offered"),
    (FIT + ["--hops", "2", "--hop-step", "0"], "--hop-step must be positive"),
    (FIT + ["--hops", "2", "--hop-step", "nan"], "--hop-step must be positive"),
    (SOLVE + ["--hops", "2", "--hop-seed", "-1"], "--hop-seed must not be negative"),
    (["--hop-step", "0.25"], "give --hops N"),                                         # the companions alone: nothing would heed them
    (FIT + ["--hop-seed", "3"], "give --hops N"),
])
def test_hops_refusals_come_before_any_file_or_device(capsys, monkeypatch, extra, text):
    """The files do not exist and opening a device would raise: the refusal comes first, and it is hops_error's."""
    from misti_amd import cli, engine

    def no_device(*a, **k):
        raise AssertionError("a device was opened")
    monkeypatch.setattr(engine.Engine, "__init__", no_device)
    monkeypatch.setattr(cli, "Engine", no_device)
    a = cli.build_parser().parse_args(BASE + extra)
    assert text in cli.hops_error(a)
    rc = cli.main(BASE + extra)
    assert rc == 2 and text in capsys.readouterr().err


@pytest.mark.parametrize("argv", [
    BASE + FIT + ["--hops", "2"],
    BASE + FIT + ["--hops", "1", "--all-bs", "--hop-step", "0.25", "--hop-seed", "7"],
    BASE + SOLVE + ["--hops", "100"],
    BASE + ["--all-bs", "--grid-solve", "--hops", "3"],
    ["a.psmc", "b.psmc", "d.sfs", "20"] + FIT + ["--hops", "2"],                        # the no-migration model: a 1-D global search
    BASE + FIT,                                                                        # no hops: nothing to refuse
])
def test_hops_accepted_combinations(argv):
    from misti_amd import cli
    a = cli.build_parser().parse_args(argv)
    assert cli.hops_error(a) is None
    assert cli.fit_st_error(a) is None and cli.grid_solve_error(a) is None and cli.top_error(a) is None and cli.profile_error(a) is None


def test_hops_defaults_and_documents():
    from misti_amd import cli
    a = cli.build_parser().parse_args(BASE + FIT)
    assert a.hops is None and a.hop_step is None and a.hop_seed is None and cli._hop_step_seed(a) == (0.5, 0)
    a = cli.build_parser().parse_args(BASE + FIT + ["--hops", "2", "--hop-step", "0.25", "--hop-seed", "7"])
    assert cli._hop_step_seed(a) == (0.25, 7)
    assert "-tol does not apply" in cli.__doc__
    for flag in ("--hops N", "--hop-step S", "--hop-seed K"):
        assert flag in cli.__doc__
    readme = open(os.path.join(ROOT, "README.md")).read()
    for flag in ("--hops", "--hop-step", "--hop-seed"):
        assert flag in readme


# ---- draw_uniforms against SciPy's runner ------------------------------------------------------------------------------------------
class Recording(np.random.Generator):
    """A Generator that records every uniform() call SciPy's basin hopping makes: (low, high, size, what it returned)."""

    def __init__(self, seed):
        super().__init__(np.random.PCG64(seed))
        self.calls = []

    def uniform(self, low=0.0, high=1.0, size=None):
        v = super().uniform(low, high, size)
        self.calls.append((low, high, size, np.array(v, dtype=np.float64)))
        return v


def wells(x):
    """Three coordinates, many basins."""
    x = np.asarray(x, dtype=float)
    return float(np.sum((x - [0.3, -0.2, 1.5]) ** 2) + 0.3 * np.sum(np.cos(9.0 * x)))


def test_draw_uniforms_draws_what_scipys_runner_draws_with_one_coordinate_more():
    """n_param = 2 and the split: three coordinates.  SciPy draws, per hop, one uniform(-step, step, (3,)) for the displacement and
    then one uniform() for the Metropolis test, and nothing else from the generator; draw_uniforms(…, N = 3) holds exactly those
    numbers in that order: Generator.uniform is low + (high - low) * next_double."""
    from scipy import optimize
    from misti_amd.engine import draw_uniforms
    niter, N = 7, 3
    rec = Recording(12345)
    optimize.basinhopping(wells, np.array([0.1, 0.2, 1.0]), niter=niter, T=0.5, stepsize=0.4, interval=3,
                          minimizer_kwargs=dict(method="Nelder-Mead", options=dict(maxfev=40)), rng=rec)
    uni = draw_uniforms([np.random.Generator(np.random.PCG64(12345))], 1, niter, N)
    assert uni.shape == (1, niter, N + 1)
    assert len(rec.calls) == 2 * niter                                          # the count: (N + 1) numbers per hop in two calls
    steps = set()
    for h in range(niter):
        lo, hi, size, v = rec.calls[2 * h]
        assert tuple(np.atleast_1d(size)) == (N,) and lo == -hi
        steps.add(hi)
        assert same_bits(v, lo + (hi - lo) * uni[0, h, :N]), h
        lo, hi, size, v = rec.calls[2 * h + 1]
        assert (lo, hi, size) == (0.0, 1.0, None)
        assert same_bits(v.reshape(()), np.float64(uni[0, h, N]).reshape(())), h
    assert len(steps) > 1                                                       # the step adjustment fired: it draws nothing
    # one generator per start, seeds allowed (the [seed, j] lists of optimize.*_global)
    two = draw_uniforms([[5, 0], np.random.default_rng([5, 1])], 2, 2, N)
    assert same_bits(two[0], draw_uniforms([np.random.default_rng([5, 0])], 1, 2, N)[0])
    assert same_bits(two[1], draw_uniforms([[5, 1]], 1, 2, N)[0])
    with pytest.raises(ValueError):
        draw_uniforms([1, 2], 3, 2, N)


# ---- optimize.*_global on a double that is SciPy itself ----------------------------------------------------------------------------
class SciPyEngine:
    """Engine-shaped: basinhopping_rows / basinhopping_split are scipy.optimize.basinhopping on an analytic, multimodal objective whose
    minimum depends on the data row (its first entry), one independent search per start from the start's own generator."""
    n_param = 2

    def __init__(self):
        self.asked = []

    @staticmethod
    def value(x, split, row):
        x = np.asarray(x, dtype=float)
        c = 0.1 * row[0]
        return float(np.sum((x - c) ** 2) + (split - 60.0 - row[0]) ** 2 / 4.0 + 0.2 * np.cos(7.0 * x).sum() + 0.2 * np.cos(5.0 * split))

    def _hop(self, f, x0, rng, niter, T, stepsize, opt):
        from scipy import optimize
        options = {k[3:]: opt[k] for k in ("nm_maxiter", "nm_maxfev") if k in opt}
        options.update({k: opt[k] for k in ("xatol", "fatol") if k in opt})
        kw = {k: opt[k] for k in ("interval", "target_accept_rate", "stepwise_factor") if k in opt}
        assert isinstance(rng, np.random.Generator)
        res = optimize.basinhopping(f, np.asarray(x0, dtype=float), niter=niter, T=T, stepsize=stepsize, rng=rng,
                                    minimizer_kwargs=dict(method="Nelder-Mead", options=options), **kw)
        return res

    def _collect(self, results):
        return dict(x=np.array([r.x for r in results]), llh=np.array([-r.fun for r in results]),
                    nfev=np.array([r.nfev for r in results], dtype=np.int32),
                    failures=np.array([r.minimization_failures for r in results], dtype=np.int32),
                    accepted=np.array([r.nit - r.minimization_failures for r in results], dtype=np.int32),      # (a stand-in: any per-start number)
                    iterations_issued=3, slots=5, speculative_iterations=1)

    def basinhopping_split(self, starts, rows, table, rngs, band_bounds=None, pulse_times=None, niter=100, T=0.5, stepsize=0.5, **opt):
        self.asked.append(dict(starts=np.array(starts), rows=np.array(rows), bounds=band_bounds, times=pulse_times, niter=niter, T=T,
                               stepsize=stepsize, opt=dict(opt)))
        assert len(rngs) == len(rows) == len(starts)
        out = self._collect([self._hop(lambda v, r=r: self.value(v[:-1], v[-1], table[r]), x0, g, niter, T, stepsize, opt)
                             for x0, r, g in zip(starts, rows, rngs)])
        out["split"] = out["x"][:, -1].copy()
        self.last = out
        return out

    def basinhopping_rows(self, starts, split_times, rows, table, rngs, band_bounds=None, pulse_times=None, niter=100, T=0.5, stepsize=0.5, **opt):
        self.asked.append(dict(starts=np.array(starts), splits=np.array(split_times), rows=np.array(rows), niter=niter, T=T, stepsize=stepsize,
                               opt=dict(opt)))
        assert len(rngs) == len(rows) == len(starts) == len(split_times)
        return self._collect([self._hop(lambda v, r=r, st=st: self.value(v, st, table[r]), x0, g, niter, T, stepsize, opt)
                              for x0, st, r, g in zip(starts, split_times, rows, rngs)])


TABLE = np.arange(24, dtype=float).reshape(3, 8) % 5                      # rows differ in their first entry: 0, 3, 1
HOPS = dict(niter=3, T=0.5, stepsize=0.3, interval=2, nm_maxfev=300)
STARTS = [[0.1, 0.2], [0.4, -0.3]]
SPLITS = [60.0, 62.5, 64.0]


def test_split_fit_global_layout_generators_best_rule_and_row_independence():
    from misti_amd.optimize import split_fit_global, split_fit_interval
    e = SciPyEngine()
    out = split_fit_global(e, TABLE, STARTS, SPLITS, band_bounds=[[4, -1]], seed=11, **HOPS)
    asked, all18 = e.asked[-1], e.last
    pairs = np.array([s + [st] for s in STARTS for st in SPLITS])                  # start outermost, initial split innermost
    assert np.array_equal(asked["starts"], np.vstack([pairs] * 3))                 # row outermost
    assert np.array_equal(asked["rows"], np.repeat([0, 1, 2], 6)) and asked["rows"].dtype == np.int32
    assert asked["bounds"].shape == (18, 1, 2) and asked["times"] is None
    assert (asked["niter"], asked["T"], asked["stepsize"]) == (3, 0.5, 0.3) and asked["opt"] == dict(interval=2, nm_maxfev=300)
    # the generator of search j of a row is default_rng([seed, j]): every search equals SciPy run with that generator
    direct = e.basinhopping_split(np.vstack([pairs] * 3), np.repeat([0, 1, 2], 6), TABLE,
                                  [np.random.default_rng([11, j]) for _ in range(3) for j in range(6)], **HOPS)
    llh = direct["llh"].reshape(3, 6)
    best = np.argmax(llh, axis=1)
    assert np.array_equal(out["start"], best)
    for r in range(3):
        s = 6 * r + best[r]
        assert same_bits(out["x"][r], direct["x"][s]) and out["llh"][r] == direct["llh"][s] and out["split"][r] == direct["x"][s, -1]
        for k in ("nfev", "failures", "accepted"):
            assert out[k][r] == direct[k][s], k
    assert "nit" not in out and "status" not in out
    assert (out["iterations_issued"], out["slots"], out["speculative_iterations"]) == (3, 5, 1)
    assert len(set(best)) > 1 or len(set(np.round(out["split"], 3))) > 1           # the rows do differ
    # a row's result does not depend on which other rows were in the call
    for r in range(3):
        alone = split_fit_global(e, TABLE[r:r + 1], STARTS, SPLITS, band_bounds=[[4, -1]], seed=11, **HOPS)
        for k in ("x", "split", "llh", "nfev", "failures", "accepted", "start"):
            assert same_bits(alone[k][0], out[k][r]), (r, k)
    # another seed is another search
    split_fit_global(e, TABLE, STARTS, SPLITS, seed=12, **HOPS)
    assert not same_bits(e.last["nfev"], all18["nfev"]) and not same_bits(e.last["x"], all18["x"])
    # split_fit_interval takes the output unchanged
    iv = split_fit_interval(out["split"], out["llh"])
    assert iv["data_split"] == out["split"][0] and iv["n_boot"] == 2 and iv["interval"] is not None


def test_split_fit_global_best_rule_ties_and_nan():
    """The rule is _best_start_profile's: the first maximum, NaN never wins."""
    from misti_amd.optimize import split_fit_global

    class Fixed(SciPyEngine):
        def basinhopping_split(self, starts, rows, table, rngs, **kw):
            S = len(rows)
            llh = np.array([-5.0, -3.0, -3.0, np.nan, -np.inf, np.nan, -7.0, np.nan])
            assert S == llh.size
            x = np.array(starts, dtype=float) + 0.25
            return dict(x=x, llh=llh, nfev=np.arange(S, dtype=np.int32), failures=np.ones(S, dtype=np.int32), accepted=2 * np.arange(S, dtype=np.int32),
                        split=x[:, -1].copy(), iterations_issued=1, slots=1, speculative_iterations=0)
    out = split_fit_global(Fixed(), np.ones((2, 8)), [[0.1, 0.2], [0.3, 0.4]], [61.0, 62.0], niter=1)
    assert np.array_equal(out["start"], [1, 2]) and np.array_equal(out["llh"], [-3.0, -7.0])
    assert np.array_equal(out["nfev"], [1, 6]) and np.array_equal(out["accepted"], [2, 12]) and np.array_equal(out["split"], [62.25, 61.25])


def test_split_fit_global_on_a_model_without_parameters():
    from misti_amd.optimize import split_fit_global
    e = SciPyEngine()
    e.n_param = 0
    out = split_fit_global(e, TABLE[:2], None, [59.0, 61.5], seed=3, **HOPS)
    assert np.array_equal(e.asked[-1]["starts"], [[59.0], [61.5]] * 2) and out["x"].shape == (2, 1)
    assert np.array_equal(out["split"], out["x"][:, 0])


def test_bootstrap_profile_global_layout_generators_best_rule_and_row_independence():
    from misti_amd.optimize import bootstrap_profile_global, bootstrap_profile_interval
    e = SciPyEngine()
    out = bootstrap_profile_global(e, SPLITS, TABLE, STARTS, seed=4, **HOPS)
    asked = e.asked[-1]
    r_of, p_of, q_of = (a.ravel() for a in np.meshgrid(np.arange(3), np.arange(3), np.arange(2), indexing="ij"))
    assert np.array_equal(asked["rows"], r_of) and asked["rows"].dtype == np.int32          # row outermost, start innermost
    assert np.array_equal(asked["splits"], np.array(SPLITS)[p_of]) and np.array_equal(asked["starts"], np.array(STARTS)[q_of])
    assert asked["opt"] == dict(interval=2, nm_maxfev=300)
    direct = e.basinhopping_rows(np.array(STARTS)[q_of], np.array(SPLITS)[p_of], r_of, TABLE,
                                 [np.random.default_rng([4, j]) for _ in range(3) for j in range(6)], **HOPS)
    best = np.argmax(direct["llh"].reshape(3, 3, 2), axis=2)
    assert out["x"].shape == (3, 3, 2) and out["llh"].shape == (3, 3) and np.array_equal(out["start"], best)
    for r in range(3):
        for p in range(3):
            s = (r * 3 + p) * 2 + best[r, p]
            assert same_bits(out["x"][r, p], direct["x"][s]) and out["llh"][r, p] == direct["llh"][s]
            for k in ("nfev", "failures", "accepted"):
                assert out[k][r, p] == direct[k][s], k
    assert "nit" not in out and "status" not in out and out["slots"] == 5
    for r in range(3):
        alone = bootstrap_profile_global(e, SPLITS, TABLE[r:r + 1], STARTS, seed=4, **HOPS)
        for k in ("x", "llh", "nfev", "failures", "accepted", "start"):
            assert same_bits(alone[k][0], out[k][r]), (r, k)
    iv = bootstrap_profile_interval(out["llh"], SPLITS, out["x"])
    assert iv["data_split"] in SPLITS and iv["n_boot"] == 2


def test_local_profiles_keep_their_keys():
    """bootstrap_profile's own keys are untouched by the shared reduction's new argument."""
    from misti_amd.optimize import bootstrap_profile

    class Local:
        n_param = 2

        def nm_solve_rows(self, st, splits, rows, table, tol, maxiter):
            S = len(rows)
            return dict(x=np.array(st), llh=-np.arange(S, dtype=float), nit=np.arange(S, dtype=np.int32), nfev=np.arange(S, dtype=np.int32),
                        status=np.zeros(S, dtype=np.int32), iterations_issued=1, slots=2, speculative_iterations=0)
    out = bootstrap_profile(Local(), [61.0, 62.0], np.ones((2, 8)), STARTS)
    assert set(out) == {"x", "llh", "nit", "nfev", "status", "start", "iterations_issued", "slots", "speculative_iterations"}


# ---- the bindings ------------------------------------------------------------------------------------------------------------------
C_TYPES = {"misti_ctx*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double, "const double*": C.c_void_p,
           "const int32_t*": C.c_void_p, "double*": C.c_void_p, "int32_t*": C.c_void_p}


def _prototype(name):
    hdr = open(os.path.join(ROOT, "include", "misti_hip.h")).read()
    m = re.search(r"^int %s\s*\(([^;]*)\);" % name, hdr, re.M)
    assert m, "no prototype of " + name
    out = []
    for a in (" ".join(a.split()) for a in m.group(1).split(",")):
        t, n = a.rsplit(" ", 1)
        out.append((C_TYPES[t + "*" if n.startswith("*") else t], n.lstrip("*")))
    return out


def test_bindings_match_the_header_prototypes():
    from misti_amd import _lib
    rows = _prototype("misti_basinhopping_rows")
    split = _prototype("misti_basinhopping_split")
    old = _prototype("misti_basinhopping")
    assert [n for _, n in rows] == ["ctx", "n_start", "starts", "split_times", "rows", "band_bounds", "pulse_times", "n_rep", "jsfs"] + [n for _, n in old[5:]]
    assert [n for _, n in split] == [n for _, n in rows if n != "split_times"]
    for name, proto in (("misti_basinhopping_rows", rows), ("misti_basinhopping_split", split)):
        res, bound = _lib.SYMBOLS[name]
        assert res is C.c_int and bound == [t for t, _ in proto], name
    hdr = open(os.path.join(ROOT, "include", "misti_hip.h")).read()
    assert "#define MISTI_ABI_VERSION 6" in hdr and _lib.ABI_VERSION == 6


# ---- argument errors that need no context ------------------------------------------------------------------------------------------
def _args(form, **change):
    """A valid argument list of misti_basinhopping_rows / _split (2 starts of a 2-parameter model, a 3-row table), by name."""
    n = 3 if form == "split" else 2
    a = dict(ctx=None, n_start=2, starts=np.full((2, n), 0.5), split_times=np.array([20.0, 21.5]), rows=np.array([0, 2], dtype=np.int32),
             band_bounds=None, pulse_times=None, n_rep=3, jsfs=np.ones((3, 8)), niter=2, T=0.5, stepsize=0.5, interval=50,
             target_accept_rate=0.5, stepwise_factor=0.9, xatol=1e-4, fatol=1e-4, nm_maxiter=400, nm_maxfev=400,
             uniforms=np.full((2, 2, n + 1), 0.5), x=np.empty((2, n)), llh=np.empty(2), nfev=None, failures=None, accepted=None)
    a.update(change)
    if form == "split":
        del a["split_times"]
    return [v.ctypes.data_as(C.c_void_p) if isinstance(v, np.ndarray) else v for v in a.values()], a


@pytest.mark.parametrize("form", ["rows", "split"])
def test_argument_errors_that_need_no_context(form):
    """Everything that does not depend on the context is checked before it: with ctx = NULL each error still reports ITSELF, and valid
    arguments report the NULL context.  No device is touched: this runs where there is none."""
    from misti_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, "misti_basinhopping_" + form)
    cases = [(dict(), "ctx is NULL"),
             (dict(n_start=-1), "negative number of starts"),
             (dict(starts=None), "is NULL"), (dict(rows=None), "is NULL"), (dict(jsfs=None), "is NULL"), (dict(x=None), "is NULL"),
             (dict(llh=None), "is NULL"), (dict(uniforms=None), "uniforms is NULL"),
             (dict(n_rep=0), "n_rep must be >= 1"),
             (dict(niter=-1), "negative number of hops"),
             (dict(nm_maxiter=0), "must be >= 1"), (dict(nm_maxfev=0), "must be >= 1"), (dict(interval=0), "must be >= 1"),
             (dict(rows=np.array([0, 3], dtype=np.int32)), "outside the table"), (dict(rows=np.array([-1, 0], dtype=np.int32)), "outside the table")]
    if form == "rows":
        cases += [(dict(split_times=None), "is NULL"), (dict(split_times=np.array([20.0, np.inf])), "split_times[1] is not finite"),
                  (dict(split_times=np.array([np.nan, 20.0])), "split_times[0] is not finite")]
    for change, text in cases:
        args, named = _args(form, **change)
        assert fn(*args) == -1, change                                            # MISTI_E_ARG
        assert text in lib.misti_last_error().decode(), (change, lib.misti_last_error())
    # niter = 0 needs no uniforms: the NULL context is all that is left to refuse
    args, _ = _args(form, niter=0, uniforms=None)
    assert fn(*args) == -1 and "ctx is NULL" in lib.misti_last_error().decode()
