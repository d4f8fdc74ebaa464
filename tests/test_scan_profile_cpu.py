"""The profile likelihood per group and replicate without a GPU: the rule stated on the host (optimize.profile_per_group - what the
device result is compared against in tests/test_gpu_scan_profile.py), the labels of a product grid (optimize.axis_groups), the
support interval (optimize.profile_interval), the command line's refusals (cli.profile_error) and the header."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NINF, NAN = -np.inf, np.nan


def profile(table, group, n_group):
    from misti_amd.optimize import profile_per_group
    table = np.array(table, dtype=float)
    val, best = profile_per_group(table, group, n_group)
    assert best.dtype == np.int64 and val.dtype == np.float64 and best.shape == val.shape == (table.shape[1], n_group)
    return val.tolist(), best.tolist()


# ---- profile_per_group --------------------------------------------------------------------------------------------------------------
def test_ties_inside_a_group_go_to_the_lower_index():
    table = [[1.0, 7.0], [3.0, 7.0], [3.0, 2.0], [0.5, 7.0], [3.0, 9.0]]
    val, best = profile(table, [0, 1, 0, 1, 1], 2)
    assert val == [[3.0, 3.0], [7.0, 9.0]]
    assert best == [[2, 1], [0, 4]]
    # the same labels given to the candidates in another arrangement: the lowest INDEX wins, wherever its group's other members lie
    val, best = profile(table, [1, 0, 0, 0, 1], 2)
    assert val == [[3.0, 3.0], [7.0, 9.0]] and best == [[1, 4], [1, 4]]


def test_minus_infinity_and_nan_never_win_and_an_empty_group_is_empty():
    table = [[NAN, 1.0, NINF],
             [2.0, NINF, NINF],
             [NINF, NAN, NINF],
             [5.0, NAN, NAN]]
    val, best = profile(table, [0, 0, 1, 1], 3)
    assert val == [[2.0, 5.0, NINF], [1.0, NINF, NINF], [NINF, NINF, NINF]]
    assert best == [[1, 3, -1], [0, -1, -1], [-1, -1, -1]]


def test_labels_outside_the_groups_are_ignored():
    table = [[9.0], [1.0], [8.0], [2.0], [7.0]]
    val, best = profile(table, [-1, 0, 2, 1, 5], 2)
    assert val == [[1.0, 2.0]] and best == [[1, 3]]
    val, best = profile(table, [-1, -7, 2, 2 ** 31 - 1, 5], 2)
    assert val == [[NINF, NINF]] and best == [[-1, -1]]


def test_identity_labels_give_the_transposed_table():
    from misti_amd.optimize import profile_per_group
    rng = np.random.default_rng(3)
    t = rng.integers(0, 6, size=(9, 5)).astype(float)
    t[rng.random(t.shape) < 0.3] = NINF
    t[rng.random(t.shape) < 0.15] = NAN
    val, best = profile_per_group(t, np.arange(9), 9)
    with np.errstate(invalid="ignore"):
        has = (t > NINF).T
    assert np.array_equal(val, np.where(has, t.T, NINF))
    assert np.array_equal(best, np.where(has, np.arange(9)[None, :], -1))


def test_one_group_is_the_first_place_of_the_scan():
    from misti_amd.optimize import best_k_per_replicate, profile_per_group
    rng = np.random.default_rng(4)
    for _ in range(40):
        t = rng.integers(0, 6, size=(rng.integers(1, 9), rng.integers(1, 12))).astype(float)      # few distinct values: many ties
        t[rng.random(t.shape) < 0.3] = NINF
        t[rng.random(t.shape) < 0.15] = NAN
        val, best = profile_per_group(t, np.zeros(t.shape[0], dtype=int), 1)
        want, want_val = best_k_per_replicate(t, 1)
        assert np.array_equal(best, want) and np.array_equal(val, want_val)


def test_every_group_is_the_scan_of_its_members():
    from misti_amd.optimize import best_k_per_replicate, profile_per_group
    rng = np.random.default_rng(5)
    t = rng.integers(0, 4, size=(40, 7)).astype(float)
    t[rng.random(t.shape) < 0.25] = NINF
    group = rng.integers(-1, 6, size=40)
    val, best = profile_per_group(t, group, 5)
    for g in range(5):
        members = np.where(group == g)[0]
        b, v = best_k_per_replicate(t[members], 1)
        assert np.array_equal(val[:, g], v[:, 0])
        assert np.array_equal(best[:, g], np.where(b[:, 0] >= 0, members[np.maximum(b[:, 0], 0)], -1))


def test_one_label_per_candidate():
    from misti_amd.optimize import profile_per_group
    with pytest.raises(ValueError):
        profile_per_group(np.zeros((3, 2)), [0, 1], 2)
    with pytest.raises(ValueError):
        profile_per_group(np.zeros((3, 2)), [0, 1, 0], 0)


# ---- axis_groups --------------------------------------------------------------------------------------------------------------------
def test_axis_groups_of_a_three_axis_grid():
    from misti_amd.optimize import axis_groups
    shape = (4, 3, 5)
    where = np.unravel_index(np.arange(60), shape)                        # the C order of meshgrid(..., indexing="ij") and ravel
    for axis in range(3):
        group, n_group = axis_groups(shape, axis)
        assert group.dtype == np.int32 and n_group == shape[axis] and np.array_equal(group, where[axis])
        group1, n1 = axis_groups(shape, (axis,))
        assert n1 == n_group and np.array_equal(group1, group)
    for i, j in ((0, 1), (0, 2), (1, 2), (2, 0)):
        group, n_group = axis_groups(shape, (i, j))
        assert n_group == shape[i] * shape[j] and np.array_equal(group, where[i] * shape[j] + where[j])
    group, n_group = axis_groups(shape, (0, 1, 2))
    assert n_group == 60 and np.array_equal(group, np.arange(60))
    for bad in ((0, 0), (3,), -1, ()):
        with pytest.raises(ValueError):
            axis_groups(shape, bad)


# ---- profile_interval ---------------------------------------------------------------------------------------------------------------
def test_profile_interval():
    from misti_amd.optimize import profile_interval
    values = [10.0, 11.0, 12.0, 13.0, 14.0]
    prof = [[-9.0, -5.0, -3.0, -5.0, -3.0],           # two maxima: the first one is reported
            [NINF, -2.0, -2.5, -7.0, NINF],
            [NINF, NINF, NINF, NINF, NINF],            # no value
            [-1.0, NAN, NINF, -4.0, -2.5]]
    iv = profile_interval(prof, values, 2.0)
    assert iv["best"].tolist()[:2] == [12.0, 11.0] and iv["llh"].tolist()[:2] == [-3.0, -2.0]
    assert iv["lo"].tolist()[:2] == [11.0, 11.0] and iv["hi"].tolist()[:2] == [14.0, 12.0]
    assert all(np.isnan(iv[f][2]) for f in ("best", "llh", "lo", "hi"))
    assert (iv["best"][3], iv["llh"][3], iv["lo"][3], iv["hi"][3]) == (10.0, -1.0, 10.0, 14.0)      # the hull: 11 .. 13 lie outside
    # a drop of 0: the maximal groups alone
    iv = profile_interval(prof, values, 0.0)
    assert iv["lo"].tolist()[:2] == [12.0, 11.0] and iv["hi"].tolist()[:2] == [14.0, 11.0] and np.isnan(iv["lo"][2])
    assert (iv["lo"][3], iv["hi"][3]) == (10.0, 10.0)
    with pytest.raises(ValueError):
        profile_interval(prof, values, -1.0)
    with pytest.raises(ValueError):
        profile_interval(prof, values[:4], 1.0)
    doc = profile_interval.__doc__
    assert "support" in doc.lower() and "composite" in doc and "not" in doc.lower() and "confidence" in doc


# ---- the command line ---------------------------------------------------------------------------------------------------------------
BASE = ["a.psmc", "b.psmc", "d.sfs", "20"]
BAND = ["-mi", "1", "2", "20", "0.1", "1"]
GRID = ["--grid-st", "18", "22"]
MESH = ["--grid-mi", "0", "0.01", "1", "4"]


@pytest.mark.parametrize("args, word", [
    (GRID + ["--profile", "splitT"], "unknown axis"),
    (GRID + ["--profile", "-1"], "unknown axis"),
    (["--profile", "st"], "not scanned"),
    (MESH + BAND + ["--profile", "st"], "not scanned"),
    (GRID + BAND + ["--profile", "0"], "not scanned"),
    (GRID + MESH + BAND + ["--profile", "1"], "not scanned"),
    (GRID + MESH + BAND + ["--profile", "st", "0", "st"], "at most two"),
    (GRID + ["--profile", "st", "st"], "same axis twice"),
    (GRID + MESH + BAND + ["--profile", "0", "0"], "same axis twice"),
    (GRID + ["--profile-drop", "1.5"], "give --profile"),
    (GRID + ["--profile", "st", "--profile-drop", "-0.5"], "negative"),
    (GRID + ["--profile", "st", "--top", "2"], "--top"),
    (GRID + BAND + ["--profile", "st", "--polish"], "--polish"),
    (GRID + ["--profile", "st", "--fit-st"], "--fit-st"),
    (GRID + BAND + ["--profile", "st", "--grid-solve"], "--grid-solve"),
    (GRID + ["--profile", "st", "--sweep", "x", "18", "19"], "--sweep"),
    (GRID + ["--profile", "st", "--sweep-pu", "t", "3", "4"], "--sweep"),
    (GRID + ["--profile", "st", "--gpus", "2"], "one GPU"),
    (GRID + ["--profile", "st", "--devices", "0,0"], "one GPU"),
])
def test_profile_error_names_the_reason(args, word):
    from misti_amd import cli
    why = cli.profile_error(cli.build_parser().parse_args(BASE + args))
    assert why is not None and word in why, why


@pytest.mark.parametrize("args", [
    [], GRID, GRID + ["--top", "2"], GRID + ["--grid-solve"] + BAND,
    GRID + ["--profile", "st"], GRID + ["--profile", "st", "--all-bs"], GRID + ["--profile", "st", "--profile-drop", "0"],
    MESH + BAND + ["--profile", "0"], GRID + MESH + BAND + ["--profile", "0", "--profile-drop", "3"],
    GRID + MESH + BAND + ["--profile", "st", "0"], GRID + MESH + BAND + ["--profile", "0", "st"], GRID + ["--profile", "st", "--gpus", "1"],
])
def test_profile_error_accepts(args):
    from misti_amd import cli
    assert cli.profile_error(cli.build_parser().parse_args(BASE + args)) is None


def test_refused_before_a_file_is_read(capsys):
    from misti_amd import cli
    assert cli.main(["no.psmc", "no.psmc", "no.sfs", "20", "--profile", "st"]) == 2      # (the files do not exist: reading them would raise)
    assert "not scanned" in capsys.readouterr().err
    assert cli.main(["no.psmc", "no.psmc", "no.sfs", "20", "--grid-st", "18", "22", "--profile", "st", "--top", "2"]) == 2
    assert "--profile" in capsys.readouterr().err                        # profile_error speaks before top_error


# ---- the header and the binding -----------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "misti_hip.h")).read()
    assert re.search(r"^int misti_scan_profile_dev\(misti_ctx\* ctx, int64_t n_cand, const double\* d_jafs, const int32_t\* d_status,", hdr, flags=re.M)
    assert "#define MISTI_SCAN_MAX_GROUPS 65535" in hdr
    assert "#define MISTI_ABI_VERSION 6" in hdr
    from misti_amd import _lib
    assert "misti_scan_profile_dev" in _lib.SYMBOLS and _lib.SCAN_MAX_GROUPS == 65535
    assert len(_lib.SYMBOLS["misti_scan_profile_dev"][1]) == 10
