"""The delete-m block jackknife without a GPU: the rule (optimize.jackknife_rows - what the device result is compared against in
tests/test_gpu_jackknife_rows.py) against the same rule written out with Python floats; the geometry and the argument checks the ABI
makes before it touches a context; the estimator (optimize.jackknife_estimate) against closed forms and against exact rational
arithmetic; header, binding and build lists; the command line's parsing and refusals."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT

E_ARG, E_LIMIT = -1, -4


def lib():
    from misti_amd import _lib
    return _lib.load()


def small_table(rng, n_chunk, fractional=True):
    c = np.zeros((n_chunk, 8))
    c[:, 1:] = rng.integers(0, 400, size=(n_chunk, 7))
    if fractional:
        c[:, 1:] *= 0.1                               # no longer integers: the order of the additions shows in the last bits
    c[:, 0] = rng.integers(1, 50, size=n_chunk) * (0.1 if fractional else 1.0) + c[:, 1:].sum(axis=1)
    return c


def shapes():
    """n_chunk 2, 3, 5, 40, 257 with m 1, 2, 7 and n_chunk - 1, wherever 1 <= m < n_chunk."""
    return [(n, m) for n in (2, 3, 5, 40, 257) for m in sorted({1, 2, 7, n - 1}) if 1 <= m < n]


def rule_in_python_floats(c, m, g):
    """Row g, as the issue states it: eight zeros, then every chunk outside the group added in chunk order - a chunk inside is skipped."""
    lo, hi = g * m, min((g + 1) * m, len(c))
    row = [0.0] * 8
    for i, chunk in enumerate(c):
        if i < lo or i >= hi:
            row = [a + float(b) for a, b in zip(row, chunk)]
    return row


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_chunk, m", shapes())
def test_rows_equal_the_rule_in_python_floats(n_chunk, m):
    from misti_amd.optimize import jackknife_rows, jackknife_table
    c = small_table(np.random.default_rng(n_chunk), n_chunk)
    G = -(-n_chunk // m)
    rows = jackknife_rows(c, m)
    assert rows.shape == (G, 8) and rows.dtype == np.float64
    for g in range(G):
        assert rows[g].tolist() == rule_in_python_floats(c, m, g), (n_chunk, m, g)          # the same bits
    table = jackknife_table(c, m)
    col = [0.0] * 8
    for r in c:
        col = [a + float(b) for a, b in zip(col, r)]
    assert table.shape == (1 + G, 8) and table[0].tolist() == col                          # row 0: the column sums in chunk order
    assert np.array_equal(table[1:], rows)
    # slices of the table are the table's rows
    for first, n in ((0, 0), (0, 1), (G // 2, G - G // 2), (G - 1, 1), (G, 0)):
        assert np.array_equal(jackknife_rows(c, m, first=first, n=n), rows[first:first + n])
    assert np.array_equal(jackknife_rows(c, m, first=G // 2), rows[G // 2:])


def test_row_zero_is_the_bootstrap_tables_row_zero():
    from misti_amd.optimize import block_bootstrap_table, jackknife_table
    c = small_table(np.random.default_rng(8), 23)
    assert jackknife_table(c, 3)[0].tobytes() == block_bootstrap_table(c, 0)[0].tobytes()


def test_a_ragged_last_group():
    from misti_amd.optimize import jackknife_rows
    c = small_table(np.random.default_rng(4), 40)
    rows = jackknife_rows(c, 7)                                       # 6 groups: five of 7 chunks, one of 5
    assert rows.shape == (6, 8)
    assert rows[5].tolist() == rule_in_python_floats(c, 7, 5)
    keep = [0.0] * 8
    for chunk in c[:35]:
        keep = [a + float(b) for a, b in zip(keep, chunk)]
    assert rows[5].tolist() == keep                                   # the last group is chunks 35 ... 39 only


def test_skipping_is_not_subtracting():
    """On counts that are no integers "the total minus the group" rounds differently from the sum of the others: the rule is the sum."""
    from misti_amd.optimize import jackknife_table
    c = small_table(np.random.default_rng(11), 257)
    t = jackknife_table(c, 1)
    assert any((t[0] - c[g]).tolist() != t[1 + g].tolist() for g in range(257))


@pytest.mark.parametrize("n_chunk, m", [(5, 2), (40, 7), (257, 64)])
def test_integer_counts_the_group_is_the_difference_exactly(n_chunk, m):
    from misti_amd.optimize import jackknife_table
    c = small_table(np.random.default_rng(n_chunk + 1), n_chunk, fractional=False)
    t = jackknife_table(c, m)
    for g in range(t.shape[0] - 1):
        group = [0.0] * 8
        for chunk in c[g * m:(g + 1) * m]:
            group = [a + float(b) for a, b in zip(group, chunk)]
        assert (t[0] - t[1 + g]).tolist() == group


# ---- geometry and what the ABI refuses before it looks at a context ---------------------------------------------------------------------
def geometry(n_chunk, m, out=True):
    G = C.c_int64(-7)
    rc = lib().misti_jackknife_geometry(n_chunk, m, C.byref(G) if out else None)
    return rc, G.value, lib().misti_last_error().decode()


def test_geometry():
    for n_chunk, m in shapes() + [(65535, 1), (65535, 65534), (1025, 64)]:
        rc, G, _ = geometry(n_chunk, m)
        assert rc == 0 and G == -(-n_chunk // m), (n_chunk, m)
    for n_chunk, m, code, word in ((1, 1, E_ARG, "n_chunk"), (0, 1, E_ARG, "n_chunk"), (-3, 1, E_ARG, "n_chunk"), (5, 0, E_ARG, "m must"),
                                   (5, -1, E_ARG, "m must"), (5, 5, E_ARG, "single group"), (5, 9, E_ARG, "single group"),
                                   (65536, 1, E_LIMIT, "MISTI_BOOT_MAX_CHUNKS")):
        rc, G, why = geometry(n_chunk, m)
        assert rc == code and word in why and G == -7, (n_chunk, m, rc, why)
    rc, _, why = geometry(5, 2, out=False)
    assert rc == E_ARG and "NULL" in why


def rows_dev(chunks, n_chunk=None, m=1, first=0, n_group=None, flags=0, rows=1, ctx=None):
    """misti_jackknife_rows_dev WITHOUT a context (there is no device here): every check of its arguments comes before the context is
    looked at, so each refusal below is the arguments', and a call that passes ends at "ctx is NULL".  `rows` is never written."""
    L = lib()
    c = None if chunks is None else np.ascontiguousarray(chunks, dtype=np.float64)
    nc = c.shape[0] if n_chunk is None else n_chunk
    if n_group is None:
        n_group = -(-nc // m) - first if m >= 1 else 1
    out = np.zeros((max(n_group, 1), 8)) if rows else None
    rc = L.misti_jackknife_rows_dev(ctx, nc, None if c is None else c.ctypes.data_as(C.c_void_p), m, first, n_group, flags,
                                    None if out is None else out.ctypes.data_as(C.c_void_p))
    assert out is None or not out.any()
    return rc, L.misti_last_error().decode()


GOOD = [[10.0, 1, 2, 3, 0, 0, 0, 0], [5.0, 0, 0, 0, 1, 1, 1, 1], [7.0, 2, 0, 0, 0, 1, 0, 3]]


def bad(i, k, v):
    c = [list(r) for r in GOOD]
    c[i][k] = v
    return c


@pytest.mark.parametrize("kw, code, word", [
    (dict(chunks=GOOD), E_ARG, "ctx is NULL"),                                  # the table passes: only the context is missing
    (dict(chunks=GOOD, m=2), E_ARG, "ctx is NULL"),
    (dict(chunks=GOOD, n_group=0), E_ARG, "ctx is NULL"),
    (dict(chunks=GOOD, first=3, n_group=0), E_ARG, "ctx is NULL"),
    (dict(chunks=GOOD, first=1, n_group=2), E_ARG, "ctx is NULL"),
    (dict(chunks=bad(0, 0, float(2 ** 24) * 5.0)), E_ARG, "ctx is NULL"),       # beyond the bootstrap's draw limit: nothing is drawn here
    (dict(chunks=bad(0, 0, 1e300)), E_ARG, "ctx is NULL"),
    (dict(chunks=None, n_chunk=3), E_ARG, "NULL"),
    (dict(chunks=GOOD, rows=0), E_ARG, "NULL"),
    (dict(chunks=GOOD[:1], n_group=1), E_ARG, "n_chunk"),
    (dict(chunks=GOOD, n_chunk=0, n_group=1), E_ARG, "n_chunk"),
    (dict(chunks=GOOD, n_chunk=-1, n_group=1), E_ARG, "n_chunk"),
    (dict(chunks=GOOD, m=0), E_ARG, "m must"),
    (dict(chunks=GOOD, m=-2), E_ARG, "m must"),
    (dict(chunks=GOOD, m=3, n_group=1), E_ARG, "single group"),
    (dict(chunks=GOOD, m=4, n_group=1), E_ARG, "single group"),
    (dict(chunks=GOOD, n_group=-1), E_ARG, "negative"),
    (dict(chunks=GOOD, first=-1, n_group=1), E_ARG, "negative"),
    (dict(chunks=GOOD, n_group=4), E_ARG, "of G = 3"),
    (dict(chunks=GOOD, first=2, n_group=2), E_ARG, "of G = 3"),
    (dict(chunks=GOOD, first=4, n_group=0), E_ARG, "of G = 3"),
    (dict(chunks=GOOD, m=2, n_group=3), E_ARG, "of G = 2"),
    (dict(chunks=GOOD, flags=1), E_ARG, "flag"),
    (dict(chunks=bad(1, 3, float("nan"))), E_ARG, "not finite"),
    (dict(chunks=bad(0, 0, float("inf"))), E_ARG, "not finite"),
    (dict(chunks=bad(1, 7, -1.0)), E_ARG, "negative"),
    (dict(chunks=bad(0, 0, 0.0)), E_ARG, "length"),
    (dict(chunks=bad(1, 0, -2.0)), E_ARG, "length"),
    (dict(chunks=GOOD, n_chunk=65536, n_group=1), E_LIMIT, "MISTI_BOOT_MAX_CHUNKS"),
])
def test_rows_dev_argument_checks(kw, code, word):
    rc, why = rows_dev(**kw)
    assert rc == code and word in why, (rc, why)


def test_the_bootstrap_still_has_its_draw_limit_and_its_messages():
    """The entry checks are shared; the draw limit stayed with the bootstrap."""
    L = lib()
    c = np.ascontiguousarray(bad(0, 0, float(2 ** 24) * 5.0 * 3), dtype=np.float64)
    out = np.zeros((4, 8))
    rc = L.misti_bootstrap_rows_dev(None, 3, c.ctypes.data_as(C.c_void_p), 0, 0, 4, 0, out.ctypes.data_as(C.c_void_p), None)
    assert rc == E_LIMIT and b"MISTI_BOOT_MAX_DRAWS" in L.misti_last_error() and not out.any()


def test_check_jackknife_refuses_what_the_abi_refuses():
    from misti_amd.optimize import check_chunks, check_jackknife, jackknife_rows, jackknife_table
    for c, m, word in ((bad(1, 3, float("nan")), 1, "finite"), (bad(1, 7, -1.0), 1, "negative"), (bad(0, 0, 0.0), 1, "length"),
                       (np.ones((65536, 8)), 1, "65535"), (np.zeros((0, 8)), 1, "at least 2"), (GOOD[:1], 1, "at least 2"),
                       (np.ones((4, 7)), 1, "[n_chunk][8]"), (GOOD, 0, "at least 1"), (GOOD, -1, "at least 1"), (GOOD, 3, "single group"),
                       (GOOD, 4, "single group"), (bad(0, 0, 1.7e308) + bad(0, 0, 1.7e308), 1, "finite number")):
        with pytest.raises(ValueError, match=re.escape(word)):
            check_jackknife(c, m)
        with pytest.raises(ValueError):
            jackknife_rows(c, m)
        with pytest.raises(ValueError):
            jackknife_table(c, m)
    c, G = check_jackknife(GOOD, 2)
    assert G == 2 and c.shape == (3, 8) and c.dtype == np.float64
    huge = bad(0, 0, float(2 ** 24) * 5.0)                             # the bootstrap's draw limit has no meaning here
    with pytest.raises(ValueError, match="draws"):
        check_chunks(huge)
    assert check_jackknife(huge, 1)[1] == 3
    for first, n in ((-1, 1), (0, -1), (0, 4), (3, 1)):
        with pytest.raises(ValueError):
            jackknife_rows(GOOD, 1, first=first, n=n)


# ---- the estimator ----------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("G", [2, 5, 20])
def test_equal_groups_of_a_mean_give_the_mean_and_its_standard_error(G):
    """theta-hat the mean of y, theta_(g) the leave-one-out means: the jackknife is the mean, its se the textbook one."""
    from scipy import stats
    from misti_amd.optimize import jackknife_estimate
    y = np.random.default_rng(G).normal(3.0, 1.0, size=G)
    theta = np.concatenate([[y.mean()], (y.sum() - y) / (G - 1)])
    lengths = np.concatenate([[G * 8.0], np.full(G, (G - 1) * 8.0)])
    r = jackknife_estimate(theta, lengths)
    se = y.std(ddof=1) / np.sqrt(G)
    assert r["estimate"] == theta[0] and r["n_group"] == G
    assert rel(r["jackknife"], r["estimate"]) <= 1e-12 and abs(r["bias"]) <= 1e-12 * abs(r["estimate"])
    assert rel(r["se"], se) <= 1e-12
    half = stats.t.ppf(0.975, G - 1) * r["se"]
    assert r["interval"] == (r["jackknife"] - half, r["jackknife"] + half)
    assert r["bias"] == r["estimate"] - r["jackknife"]


def test_equal_groups_and_arbitrary_leave_out_estimates():
    from misti_amd.optimize import jackknife_estimate
    G = 13
    rng = np.random.default_rng(1)
    t = rng.normal(2.0, 0.3, size=G)
    theta = np.concatenate([[2.1], t])
    r = jackknife_estimate(theta, np.concatenate([[G * 5.0], np.full(G, (G - 1) * 5.0)]))
    assert rel(r["se"] ** 2, (G - 1) / G * np.sum((t - t.mean()) ** 2)) <= 1e-12
    assert rel(r["jackknife"], G * 2.1 - (G - 1) * t.mean()) <= 1e-12


def exact(theta, lengths):
    """The formulas of the issue in rational arithmetic."""
    th = [Fraction(v) for v in theta]
    l = [Fraction(v) for v in lengths]
    n, G = l[0], len(th) - 1
    m = [n - v for v in l[1:]]
    h = [n / v for v in m]
    jack = G * th[0] - sum((1 - mg / n) * t for mg, t in zip(m, th[1:]))
    tau = [hg * th[0] - (hg - 1) * t for hg, t in zip(h, th[1:])]
    var = sum((tg - jack) ** 2 / (hg - 1) for tg, hg in zip(tau, h)) / G
    return jack, var


def test_unequal_groups_against_rational_arithmetic():
    from misti_amd.optimize import jackknife_estimate
    rng = np.random.default_rng(3)
    for G in (2, 3, 9):
        groups = rng.integers(1, 64, size=G).astype(float)            # group lengths: integers, so every input is a rational
        lengths = np.concatenate([[groups.sum()], groups.sum() - groups])
        theta = rng.integers(900, 1100, size=1 + G) / 64.0
        r = jackknife_estimate(theta, lengths)
        jack, var = exact(theta, lengths)
        assert rel(r["jackknife"], float(jack)) <= 1e-12 and rel(r["se"] ** 2, float(var)) <= 1e-12
        assert rel(r["bias"], float(Fraction(theta[0]) - jack)) <= 1e-9      # (a difference of two numbers that nearly agree)
        assert r["n_group"] == G


def test_rows_without_an_estimate_are_dropped_and_counted():
    from misti_amd.optimize import jackknife_estimate
    groups = np.array([3.0, 5.0, 2.0, 7.0, 4.0])
    lengths = np.concatenate([[groups.sum()], groups.sum() - groups])
    theta = np.array([10.0, 10.5, np.nan, 9.75, np.inf, 10.25])
    r = jackknife_estimate(theta, lengths)
    assert r["n_group"] == 3
    keep = [0, 1, 3, 5]
    th, l = [Fraction(float(theta[i])) for i in keep], [Fraction(float(lengths[i])) for i in keep]
    n, G = l[0], 3
    m = [n - v for v in l[1:]]
    jack = G * th[0] - sum((1 - mg / n) * t for mg, t in zip(m, th[1:]))
    var = sum(((n / mg) * th[0] - (n / mg - 1) * t - jack) ** 2 / (n / mg - 1) for mg, t in zip(m, th[1:])) / G
    assert rel(r["jackknife"], float(jack)) <= 1e-12 and rel(r["se"] ** 2, float(var)) <= 1e-12
    # fewer than two usable rows: no se, no interval
    one = jackknife_estimate(np.array([10.0, np.nan, np.nan, 9.75, np.nan, np.nan]), lengths)
    assert one["n_group"] == 1 and one["se"] is None and one["interval"] is None and one["estimate"] == 10.0 and one["jackknife"] is not None
    none = jackknife_estimate(np.array([10.0] + [np.nan] * 5), lengths)
    assert none["n_group"] == 0 and none["se"] is None and none["jackknife"] is None
    # no row-0 estimate: no result at all
    assert jackknife_estimate(np.array([np.nan, 1.0, 2.0, 3.0, 4.0, 5.0]), lengths) is None


def test_two_dimensional_estimates_are_handled_per_column():
    from misti_amd.optimize import jackknife_estimate
    groups = np.array([3.0, 5.0, 2.0, 7.0])
    lengths = np.concatenate([[groups.sum()], groups.sum() - groups])
    a = np.array([10.0, 10.5, 9.5, 9.75, 10.25])
    b = np.array([0.5, 0.25, np.nan, 0.75, 0.5])
    c = np.array([np.nan, 1.0, 1.0, 1.0, 1.0])
    r = jackknife_estimate(np.stack([a, b, c], axis=1), lengths)
    ra, rb = jackknife_estimate(a, lengths), jackknife_estimate(b, lengths)
    for k, one in enumerate((ra, rb)):
        for key in ("estimate", "jackknife", "bias", "se"):
            assert r[key][k] == one[key]
        assert tuple(r["interval"][k]) == one["interval"] and r["n_group"][k] == one["n_group"]
    assert r["n_group"].tolist() == [4, 3, 0] and np.isnan(r["estimate"][2]) and np.isnan(r["se"][2]) and r["interval"].shape == (3, 2)


def test_the_estimator_reads_column_zero_of_a_table_alone():
    from misti_amd.optimize import jackknife_estimate, jackknife_table, jackknife_weights
    c = small_table(np.random.default_rng(2), 40, fractional=False)
    t = jackknife_table(c, 7)
    n, m_g, h_g = jackknife_weights(t[:, 0])
    assert n == c[:, 0].sum() and m_g.tolist() == [c[g * 7:(g + 1) * 7, 0].sum() for g in range(6)] and h_g.tolist() == (n / m_g).tolist()
    assert jackknife_estimate(np.arange(7.0) + 1, t[:, 0])["n_group"] == 6
    for l in ([5.0, 4.0], [5.0, 5.0, 4.0], [5.0, 0.0, 4.0], [5.0, 6.0, 4.0], [5.0, np.nan, 4.0]):
        with pytest.raises(ValueError):
            jackknife_weights(l)
    with pytest.raises(ValueError):
        jackknife_estimate(np.arange(5.0), t[:, 0])


# ---- header, binding, build lists -------------------------------------------------------------------------------------------------------
def test_header_binding_and_build_lists_declare_the_entry_points_and_the_abi_stays_6():
    from misti_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "misti_hip.h")).read()
    assert re.search(r"^int misti_jackknife_rows_dev\(misti_ctx\* ctx, int64_t n_chunk, const double\* chunks", hdr, flags=re.M)
    assert re.search(r"^int misti_jackknife_geometry\(int64_t n_chunk, int64_t m, int64_t\* n_group\);", hdr, flags=re.M)
    assert "#define MISTI_ABI_VERSION 6" in hdr and "optimize.jackknife_rows" in hdr
    assert lib().misti_abi_version() == 6 and _lib.ABI_VERSION == 6
    assert {"misti_jackknife_rows_dev", "misti_jackknife_geometry"} <= set(_lib.SYMBOLS)
    assert len(_lib.SYMBOLS["misti_jackknife_rows_dev"][1]) == 8 and len(_lib.SYMBOLS["misti_jackknife_geometry"][1]) == 3
    assert "misti_jack.hip" in build.SOURCES and "misti_boot.hip" in build.SOURCES
    for f in build.SOURCES + build.HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, f)), f


# ---- the command line -------------------------------------------------------------------------------------------------------------------
BASE = ["a.psmc", "b.psmc", "d.sfs", "20"]
FIT = ["--fit-st", "--grid-st", "15", "17"]
SOLVE = ["--grid-solve", "--grid-st", "15", "17", "-mi", "1", "4", "16", "0.2", "1"]


def test_parser_accepts_jackknife():
    from misti_amd import cli
    a = cli.build_parser().parse_args(BASE + ["--jackknife", "2", "--jackknife-out", "t.sfs"] + FIT)
    assert (a.jackknife, a.jackknife_out) == (2, "t.sfs") and cli.jackknife_error(a) is None
    for more in (FIT + ["--hops", "3", "--hop-step", "0.25", "--hop-seed", "1"], FIT + ["--box", "st", "15", "17"], SOLVE, SOLVE + ["--hops", "2"],
                 SOLVE + ["--box", "0", "0.01", "2"], FIT + ["--all-bs"]):
        for m in ("0", "1", "7"):
            assert cli.jackknife_error(cli.build_parser().parse_args(BASE + ["--jackknife", m] + more)) is None, (m, more)
    a = cli.build_parser().parse_args(BASE)
    assert a.jackknife is None and a.jackknife_out is None and cli.jackknife_error(a) is None
    text = " ".join(cli.build_parser().format_help().split())
    assert "--jackknife M" in text and "--jackknife-out FILE" in text
    assert "--jackknife M" in cli.__doc__ and "--jackknife-out FILE" in cli.__doc__


NEEDS_A_FIT = "the arg-max over a grid does not move when one block is left out; fit with --fit-st or --grid-solve"


@pytest.mark.parametrize("args, word", [
    (["--jackknife", "2", "--bootstrap", "8"] + FIT, "--bootstrap"),
    (["--jackknife", "2", "--parametric", "8"] + FIT, "--parametric"),
    (["--jackknife", "2", "-bs", "1"] + FIT, "-bs K"),
    (["--jackknife", "2", "-bs", "0"] + FIT, "-bs K"),
    (["--jackknife", "2"], NEEDS_A_FIT),
    (["--jackknife", "2", "--grid-st", "15", "17"], NEEDS_A_FIT),
    (["--jackknife", "2", "--grid-st", "15", "17", "--all-bs"], NEEDS_A_FIT),
    (["--jackknife", "0", "--grid-st", "15", "17", "--all-bs"], NEEDS_A_FIT),
    (["--jackknife", "2", "--grid-st", "15", "17", "--top", "2"], NEEDS_A_FIT),
    (["--jackknife", "2", "--grid-st", "15", "17", "--top", "2", "--polish", "-mi", "1", "4", "16", "0.2", "1"], NEEDS_A_FIT),
    (["--jackknife", "2", "--grid-st", "15", "17", "--profile", "st"], NEEDS_A_FIT),
    (["--jackknife", "2", "--sweep", "t", "15", "16"], NEEDS_A_FIT),
    (["--jackknife", "2", "--sweep", "t", "15", "16", "--grid-solve"], NEEDS_A_FIT),
    (["--jackknife", "2", "--se"] + SOLVE, "--se"),
    (["--jackknife-out", "t.sfs"] + FIT, "give --jackknife M"),
    (["--jackknife", "0", "--jackknife-out", "t.sfs"] + FIT, "M >= 1"),
    (["--jackknife", "-1"] + FIT, "negative"),
])
def test_jackknife_error_names_the_reason(args, word):
    from misti_amd import cli
    why = cli.jackknife_error(cli.build_parser().parse_args(BASE + args))
    assert why is not None and word in why, why


def test_refused_before_a_file_is_read(capsys):
    from misti_amd import cli
    assert cli.main(["no.psmc", "no.psmc", "no.sfs", "20", "--jackknife", "2", "--grid-st", "15", "17"]) == 2      # (the files do not exist)
    err = capsys.readouterr().err.strip()
    assert NEEDS_A_FIT in err and len(err.splitlines()) == 1
    assert cli.main(["no.psmc", "no.psmc", "no.sfs", "20", "--jackknife", "2", "--bootstrap", "4"] + FIT) == 2
    assert "--bootstrap" in capsys.readouterr().err


def test_a_file_the_abi_would_refuse_is_an_argument_error(tmp_path, capsys):
    """Refused with one line when the file is read, before the PSMC files (which do not exist) or the GPU are touched."""
    from misti_amd import cli, io as mio
    fj = tmp_path / "d.sfs"
    units = ["--funits", str(tmp_path / "nounits.txt")]
    fj.write_text(mio.format_jsfs([[10.0, 1, 2, 3, 0, 0, 0, 4], [0.0, 0, 0, 0, 0, 0, 0, 0], [6.0, 1, 1, 1, 1, 1, 1, 0]]))
    rc = cli.main(["no.psmc", "no.psmc", str(fj), "20", "--jackknife", "1"] + FIT + units)
    err = capsys.readouterr().err.strip()
    assert rc == 2 and "length" in err and len(err.splitlines()) == 1
    fj.write_text(mio.format_jsfs([[10.0, 1, 2, 3, 0, 0, 0, 4], [5.0, 0, 0, 0, 0, 0, 0, 5], [6.0, 1, 1, 1, 1, 1, 1, 0]]))
    for m in ("3", "4"):                                              # M >= n_chunk
        rc = cli.main(["no.psmc", "no.psmc", str(fj), "20", "--jackknife", m] + FIT + units)
        err = capsys.readouterr().err.strip()
        assert rc == 2 and "single group" in err and len(err.splitlines()) == 1
    # --jackknife 0: the file must be a table - here row 1 keeps more than row 0 holds
    fj.write_text(mio.format_jsfs([[10.0, 1, 2, 3, 0, 0, 0, 4], [12.0, 0, 0, 0, 0, 0, 0, 5], [6.0, 1, 1, 1, 1, 1, 1, 0]]))
    rc = cli.main(["no.psmc", "no.psmc", str(fj), "20", "--jackknife", "0"] + FIT + units)
    err = capsys.readouterr().err.strip()
    assert rc == 2 and "jackknife table" in err and len(err.splitlines()) == 1
