"""Host side of the fitted split time (no GPU): the t-interval over fitted splits, the best-per-row reduction, the `--fit-st`
refusals, and the binding of misti_nm_solve_split against its prototype in include/misti_hip.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def test_split_fit_interval_against_a_hand_computation():
    from scipy import stats
    from misti_amd.optimize import split_fit_interval
    split = np.array([63.2, 62.75, 64.5, 61.0, 63.125, 65.3])
    llh = np.array([-10.0, -11.0, -9.5, -np.inf, -12.0, -10.5])             # row 3 has no value: dropped and counted
    iv = split_fit_interval(split, llh)
    b = np.array([62.75, 64.5, 63.125, 65.3])
    half = stats.t.ppf(0.975, 3) * b.std(ddof=1) / np.sqrt(4)
    assert iv["n_boot"] == 4 and iv["n_excluded"] == 1
    assert iv["data_split"] == 63.2 and iv["data_llh"] == -10.0
    assert iv["mean"] == b.mean()
    assert iv["interval"] == (b.mean() - half, b.mean() + half)
    assert np.allclose(iv["interval"], stats.t.interval(0.95, 3, loc=b.mean(), scale=stats.sem(b)), rtol=1e-14, atol=0)
    assert np.array_equal(iv["best_split"], [63.2, 62.75, 64.5, np.nan, 63.125, 65.3], equal_nan=True)
    # another level; a data row without a value; too few bootstrap rows for an interval
    iv90 = split_fit_interval(split, llh, level=0.90)
    assert iv90["interval"][1] - iv90["interval"][0] < iv["interval"][1] - iv["interval"][0]
    none = split_fit_interval([63.0, 64.0, 62.0], [np.nan, -5.0, -np.inf])
    assert none["data_split"] is None and none["data_llh"] is None and none["mean"] == 64.0 and none["interval"] is None
    assert none["n_boot"] == 1 and none["n_excluded"] == 1


class FakeEngine:
    """Stands for Engine.nm_solve_split: returns a fixed value per (row, pair) and records what it was asked."""
    n_param = 2

    def __init__(self, llh):
        self.llh = np.asarray(llh, dtype=float)

    def nm_solve_split(self, starts, rows, table, band_bounds=None, pulse_times=None, tol=1e-4, maxiter=1000):
        self.asked = dict(starts=np.array(starts), rows=np.array(rows), table=np.array(table), bounds=band_bounds, times=pulse_times)
        S = len(rows)
        llh = self.llh.reshape(-1)
        assert llh.size == S
        x = np.array(starts, dtype=float) + 0.5
        return dict(x=x, llh=llh, nit=np.arange(S, dtype=np.int32), nfev=2 * np.arange(S, dtype=np.int32), status=np.zeros(S, dtype=np.int32),
                    split=x[:, -1].copy(), iterations_issued=7, slots=11, speculative_iterations=3)


def test_split_fit_keeps_the_best_search_per_row():
    from misti_amd.optimize import split_fit
    # 2 rows x (2 starts x 3 initial splits); row 0: a tie between pairs 1 and 4 (the lowest index wins), row 1: NaN never wins
    llh = [[-5.0, -3.0, -4.0, -6.0, -3.0, -np.inf], [np.nan, -np.inf, -9.0, -8.0, np.nan, -8.5]]
    e = FakeEngine(llh)
    rows = np.arange(16, dtype=float).reshape(2, 8)
    out = split_fit(e, rows, [[0.1, 0.2], [0.3, 0.4]], [61.0, 62.5, 64.0], band_bounds=[[4, -1], [10, -1]])
    pairs = np.array([[0.1, 0.2, 61.0], [0.1, 0.2, 62.5], [0.1, 0.2, 64.0], [0.3, 0.4, 61.0], [0.3, 0.4, 62.5], [0.3, 0.4, 64.0]])
    assert np.array_equal(e.asked["starts"], np.vstack([pairs, pairs]))
    assert np.array_equal(e.asked["rows"], [0] * 6 + [1] * 6) and e.asked["rows"].dtype == np.int32
    assert e.asked["bounds"].shape == (12, 2, 2) and e.asked["times"] is None
    assert np.array_equal(out["start"], [1, 3])
    assert np.array_equal(out["llh"], [-3.0, -8.0])
    assert np.array_equal(out["x"], [pairs[1] + 0.5, pairs[3] + 0.5]) and np.array_equal(out["split"], [63.0, 61.5])
    assert np.array_equal(out["nit"], [1, 9]) and np.array_equal(out["nfev"], [2, 18])
    assert (out["iterations_issued"], out["slots"], out["speculative_iterations"]) == (7, 11, 3)


def test_split_fit_on_a_model_without_parameters():
    from misti_amd.optimize import split_fit
    e = FakeEngine([[-2.0, -1.0], [-1.0, -3.0], [-4.0, -4.0]])
    e.n_param = 0
    out = split_fit(e, np.ones((3, 8)), None, [50.0, 51.5])
    assert np.array_equal(e.asked["starts"], [[50.0], [51.5]] * 3)
    assert np.array_equal(out["start"], [1, 0, 0]) and np.array_equal(out["split"], [52.0, 50.5, 50.5]) and out["x"].shape == (3, 1)


BASE = ["a.psmc", "b.psmc", "d.sfs", "20", "-mi", "1", "4", "20", "0.2", "1"]


@pytest.mark.parametrize("extra, text", [
    (["--grid-st", "18", "20", "--fit-st", "--gpus", "2"], "--fit-st runs on one GPU"),
    (["--grid-st", "18", "20", "--fit-st", "--devices", "0,1"], "--fit-st runs on one GPU"),
    (["--grid-st", "18", "20", "--fit-st", "--sweep", "a", "4", "5"], "--sweep / --sweep-pu are not offered"),
    (["--grid-st", "18", "20", "--fit-st", "--sweep-pu", "t", "4", "5"], "--sweep / --sweep-pu are not offered"),
    (["--fit-st", "--all-bs"], "--fit-st needs --grid-st"),
    (["--grid-st", "18", "20", "--fit-st", "--grid-solve"], "give one of them"),
])
def test_cli_fit_st_refusals_come_before_any_file_or_device(capsys, monkeypatch, extra, text):
    """The files do not exist and opening a device would raise: the refusal comes first."""
    from misti_amd import cli, engine

    def no_device(*a, **k):
        raise AssertionError("a device was opened")
    monkeypatch.setattr(engine.Engine, "__init__", no_device)
    monkeypatch.setattr(cli, "Engine", no_device)
    rc = cli.main(BASE + extra)
    assert rc == 2 and text in capsys.readouterr().err


def test_fit_st_alone_is_no_error():
    from misti_amd import cli
    a = cli.build_parser().parse_args(BASE + ["--grid-st", "18", "20", "0.5", "--fit-st", "--all-bs"])
    assert cli.fit_st_error(a) is None and a.fit_st
    a = cli.build_parser().parse_args(["a.psmc", "b.psmc", "d.sfs", "20", "--grid-st", "18", "20", "--fit-st"])      # no optimised -mi needed
    assert cli.fit_st_error(a) is None and cli.grid_solve_error(a) is None


C_TYPES = {"misti_ctx*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double, "const double*": C.c_void_p,
           "const int32_t*": C.c_void_p, "double*": C.c_void_p, "int32_t*": C.c_void_p}


def test_binding_of_nm_solve_split_matches_the_header_prototype():
    from misti_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "misti_hip.h")).read()
    m = re.search(r"^int misti_nm_solve_split\s*\(([^;]*)\);", hdr, re.M)
    assert m, "no prototype"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    types = []
    for a in args:
        t, name = a.rsplit(" ", 1) if not a.rsplit(" ", 1)[1].startswith("*") else (a.rsplit(" ", 1)[0] + "*", a.rsplit(" ", 1)[1][1:])
        types.append(C_TYPES[t])
    res, bound = _lib.SYMBOLS["misti_nm_solve_split"]
    assert res is C.c_int
    assert len(bound) == len(types) == 16
    assert bound == types, [(a, b, t) for a, b, t in zip(args, bound, types) if b is not t]
    # the pulses form minus split_times: the same tail
    assert bound[6:] == _lib.SYMBOLS["misti_nm_solve_pulses"][1][7:]
