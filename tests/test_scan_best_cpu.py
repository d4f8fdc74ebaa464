"""The k-best-per-replicate scan without a GPU: the order rule stated on the host (optimize.best_k_per_replicate - what the device
result is compared against in tests/test_gpu_scan_best.py), the command line's refusals (cli.top_error) and the header."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NINF, NAN = -np.inf, np.nan


def lists(table, k):
    from misti_amd.optimize import best_k_per_replicate
    best, val = best_k_per_replicate(np.array(table, dtype=float), k)
    assert best.dtype == np.int64 and best.shape == val.shape == (np.array(table).shape[1], k)
    return best.tolist(), val.tolist()


def test_ties_go_to_the_lower_index_and_both_are_listed():
    best, val = lists([[1.0, 7.0], [3.0, 7.0], [3.0, 2.0], [0.5, 7.0]], 3)
    assert best == [[1, 2, 0], [0, 1, 3]]
    assert val == [[3.0, 3.0, 1.0], [7.0, 7.0, 7.0]]
    best, val = lists([[1.0, 7.0], [3.0, 7.0], [3.0, 2.0], [0.5, 7.0]], 1)
    assert best == [[1], [0]] and val == [[3.0], [7.0]]


def test_minus_infinity_and_nan_are_never_listed_and_short_columns_are_padded():
    table = [[NAN, 1.0, NINF, NAN],
             [2.0, NINF, NINF, NAN],
             [NINF, NAN, NINF, NINF],
             [5.0, NAN, NINF, NINF]]
    best, val = lists(table, 3)
    assert best == [[3, 1, -1], [0, -1, -1], [-1, -1, -1], [-1, -1, -1]]
    assert val == [[5.0, 2.0, NINF], [1.0, NINF, NINF], [NINF] * 3, [NINF] * 3]


def test_more_places_than_candidates():
    best, val = lists([[4.0, NINF], [6.0, 1.0]], 4)
    assert best == [[1, 0, -1, -1], [1, -1, -1, -1]]
    assert val == [[6.0, 4.0, NINF, NINF], [1.0, NINF, NINF, NINF]]


def test_one_place_is_the_arg_max_of_the_bootstrap_reduction():
    from misti_amd.dist import best_per_replicate
    from misti_amd.optimize import best_k_per_replicate
    rng = np.random.default_rng(4)
    for _ in range(40):
        t = rng.integers(0, 6, size=(rng.integers(1, 9), rng.integers(1, 12))).astype(float)      # few distinct values: many ties
        t[rng.random(t.shape) < 0.3] = NINF
        t[rng.random(t.shape) < 0.15] = NAN
        best, val = best_k_per_replicate(t, 1)
        want = best_per_replicate(t)
        assert np.array_equal(best[:, 0], want)
        has = want >= 0
        assert np.array_equal(val[has, 0], t[want[has], np.where(has)[0]]) and np.isneginf(val[~has, 0]).all()


def test_the_first_k_places_do_not_depend_on_k():
    from misti_amd.optimize import best_k_per_replicate
    rng = np.random.default_rng(5)
    t = rng.integers(0, 4, size=(11, 6)).astype(float)
    t[rng.random(t.shape) < 0.2] = NINF
    b8, v8 = best_k_per_replicate(t, 8)
    for k in (1, 2, 3):
        b, v = best_k_per_replicate(t, k)
        assert np.array_equal(b, b8[:, :k]) and np.array_equal(v, v8[:, :k])


BASE = ["a.psmc", "b.psmc", "d.sfs", "20"]
BAND = ["-mi", "1", "2", "20", "0.1", "1"]
GRID = ["--grid-st", "18", "22"]


@pytest.mark.parametrize("args, word", [
    (GRID + ["--polish"] + BAND, "give --top"),
    (GRID + ["--top", "0"], "1 ... 8"),
    (GRID + ["--top", "9"], "1 ... 8"),
    (["--top", "2"], "grid mode"),
    (["--all-bs", "--top", "2"], "grid mode"),
    (GRID + ["--top", "2", "--polish"], "optimised parameter"),
    (GRID + ["--top", "2", "--polish", "-mi", "1", "2", "20", "0.1", "0"], "optimised parameter"),
    (GRID + ["--top", "2", "--gpus", "2"], "one GPU"),
    (GRID + ["--top", "2", "--devices", "0,0"], "one GPU"),
    (GRID + ["--top", "2", "--grid-solve"] + BAND, "--grid-solve"),
    (GRID + ["--top", "2", "--fit-st"], "--fit-st"),
    (["--top", "2", "--sweep", "st", "18", "19"], "--sweep"),
    (GRID + ["--top", "2", "--sweep-pu", "t", "3", "4"], "--sweep"),
])
def test_top_error_names_the_reason(args, word):
    from misti_amd import cli
    why = cli.top_error(cli.build_parser().parse_args(BASE + args))
    assert why is not None and word in why, why


@pytest.mark.parametrize("args", [
    [], GRID, GRID + ["--grid-solve"] + BAND,
    GRID + ["--top", "1"], GRID + ["--top", "8", "--all-bs"], ["--grid-mi", "0", "0.01", "1", "4", "--top", "3"] + BAND,
    GRID + ["--top", "2", "--polish"] + BAND, GRID + ["--top", "2", "--polish", "-pu", "2", "5", "0.1", "1"], GRID + ["--top", "2", "--gpus", "1"],
])
def test_top_error_accepts(args):
    from misti_amd import cli
    assert cli.top_error(cli.build_parser().parse_args(BASE + args)) is None


def test_refused_before_a_file_is_read(capsys):
    from misti_amd import cli
    assert cli.main(["no.psmc", "no.psmc", "no.sfs", "20", "--top", "2"]) == 2           # (the files do not exist: reading them would raise)
    assert "grid mode" in capsys.readouterr().err


def test_header_declares_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "misti_hip.h")).read()
    assert re.search(r"^int misti_scan_best_dev\(misti_ctx\* ctx, int64_t n_cand, const double\* d_jafs, const int32_t\* d_status,", hdr, flags=re.M)
    assert "#define MISTI_SCAN_MAX_BEST 8" in hdr
    assert "#define MISTI_ABI_VERSION 6" in hdr
    from misti_amd import _lib
    assert "misti_scan_best_dev" in _lib.SYMBOLS and _lib.SCAN_MAX_BEST == 8
