"""The bootstrap profile without a GPU: the reduction of the reference's test.bs/bs_conf_int.ipynb (bootstrap_profile_interval) against
a literal transcription of the notebook, the argument errors of misti_nm_solve_rows through the loaded library, and the argument errors
of `--grid-solve`."""
import ctypes as C

import numpy as np
import pytest


def notebook_conf_int(tables):
    """test.bs/bs_conf_int.ipynb, conf_int_bs, as written there: ``tables[i]`` is the file LLH.bs=i.txt as an array of its lines
    (llh first, split last); row 0 is the data and left out of the interval."""
    import scipy.stats as st
    bs_mas = []
    for i in range(len(tables)):
        l = np.array(tables[i]).transpose()
        bs_mas.append(l[-1][np.argmax(l[0])])
    a = bs_mas[1:]  # zero is without bootstrap
    l = np.array(tables[0]).transpose()
    return st.t.interval(0.975, len(a) - 1, loc=np.mean(a), scale=st.sem(a)), l[-1][np.argmax(l[0])], a


def as_files(llh, splits):
    """The LLH.bs=r.txt files the test.bs loops write (`awk '{print $18, $14, ..., $6}'`: llh first, split last), one line per split."""
    return [[[llh[r, p], splits[p]] for p in range(len(splits))] for r in range(llh.shape[0])]


def check_against_notebook(llh, splits):
    from misti_amd.optimize import bootstrap_profile_interval
    iv = bootstrap_profile_interval(llh, splits)
    keep = [0] + [r for r in range(1, llh.shape[0]) if np.isfinite(llh[r]).any()]     # rows without a value: no best split
    (lo, hi), data_split, a = notebook_conf_int(as_files(llh[keep], splits))
    assert iv["data_split"] == data_split
    assert iv["n_boot"] == len(a) and iv["n_excluded"] == llh.shape[0] - len(keep)
    assert iv["mean"] == np.mean(a)
    assert iv["interval"] == (lo, hi)
    assert list(iv["best_split"][keep[1:]]) == list(a)
    return iv


def test_interval_equals_the_notebook_on_random_tables():
    rng = np.random.default_rng(11)
    splits = np.arange(15.0, 26.0)
    for R in (3, 12, 101):
        llh = -1e5 + rng.normal(size=(R, splits.size)) * 50
        iv = check_against_notebook(llh, splits)
        assert iv["n_excluded"] == 0 and iv["interval"][0] <= iv["mean"] <= iv["interval"][1]


def test_ties_go_to_the_first_split():
    splits = np.array([15.0, 15.5, 16.0, 17.0])
    llh = np.array([[-5.0, -3.0, -3.0, -4.0],
                    [-2.0, -2.0, -2.0, -2.0],
                    [-9.0, -1.0, -8.0, -1.0],
                    [-7.0, -7.0, -6.0, -6.0]])
    iv = check_against_notebook(llh, splits)
    assert list(iv["best_split"]) == [15.5, 15.0, 15.5, 16.0]
    assert iv["data_split"] == 15.5 and iv["data_llh"] == -3.0


def test_rows_without_a_value_are_excluded_and_counted():
    splits = np.array([20.0, 21.0, 22.0])
    inf = -np.inf
    llh = np.array([[-10.0, -9.0, inf],
                    [inf, inf, inf],
                    [-4.0, inf, -5.0],
                    [inf, -3.0, -3.5],
                    [np.nan, -np.inf, -np.inf],
                    [-1.0, -2.0, -0.5]])
    iv = check_against_notebook(llh, splits)
    assert iv["n_excluded"] == 2 and iv["n_boot"] == 3
    assert np.isnan(iv["best_split"][1]) and np.isnan(iv["best_split"][4])
    assert list(iv["best_split"][[2, 3, 5]]) == [20.0, 21.0, 22.0]


def test_row_zero_is_the_data_and_stays_out_of_the_interval():
    from misti_amd.optimize import bootstrap_profile_interval
    splits = np.array([10.0, 11.0, 12.0])
    boot = np.array([[-1.0, -2.0, -3.0], [-2.0, -1.0, -3.0], [-3.0, -2.0, -1.0], [-1.0, -3.0, -2.0]])
    a = bootstrap_profile_interval(np.vstack([[-9.0, -9.0, -1.0], boot]), splits)
    b = bootstrap_profile_interval(np.vstack([[-1.0, -9.0, -9.0], boot]), splits)
    assert a["data_split"] == 12.0 and b["data_split"] == 10.0
    assert a["interval"] == b["interval"] and a["mean"] == b["mean"] == np.mean([10.0, 11.0, 12.0, 10.0])
    x = np.arange(5 * 3 * 2, dtype=float).reshape(5, 3, 2)
    c = bootstrap_profile_interval(np.vstack([[-9.0, -1.0, -9.0], boot]), splits, x)
    assert list(c["data_x"]) == [2.0, 3.0]
    # the data row without a value: no data split; one bootstrap row: a mean, no interval
    d = bootstrap_profile_interval(np.array([[-np.inf] * 3, [-1.0, -2.0, -3.0]]), splits)
    assert d["data_split"] is None and d["n_boot"] == 1 and d["mean"] == 10.0 and d["interval"] is None


def test_nm_solve_rows_rejects_its_arguments_through_the_library():
    from misti_amd import _lib
    lib = _lib.load()
    d = (C.c_double * 16)()
    i = (C.c_int32 * 4)()
    rc = lib.misti_nm_solve_rows(None, 1, d, d, i, 1, d, 1e-4, 1e-4, 10, d, d, None, None, None)
    assert rc == -1                                   # MISTI_E_ARG
    assert b"ctx is NULL" in lib.misti_last_error()


@pytest.mark.parametrize("extra, why", [
    (["--grid-st", "18", "20", "--grid-solve", "-mi", "1", "4", "20", "0.1", "0"], "optimised parameter"),
    (["--grid-st", "18", "20", "--grid-solve", "-mi", "1", "4", "20", "0.1", "1", "--gpus", "2"], "--gpus"),
    (["--grid-st", "18", "20", "--grid-solve", "-mi", "1", "4", "20", "0.1", "1", "--devices", "0,1"], "--devices"),
    (["--grid-solve", "-mi", "1", "4", "20", "0.1", "1"], "--grid-st"),
])
def test_cli_grid_solve_argument_errors(capsys, extra, why):
    """--grid-solve refuses before reading any file (the inputs here do not exist) or touching the GPU."""
    from misti_amd import cli
    rc = cli.main(["a.psmc", "b.psmc", "d.sfs", "20"] + extra)
    assert rc == 2 and why in capsys.readouterr().err
