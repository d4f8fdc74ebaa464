"""The parametric bootstrap without a GPU: the thresholds and the class counts of misti_parametric_rows_dev (the two host hooks run the very
functions the kernel calls) against the rule in NumPy (optimize.parametric_thresholds / parametric_rows - what the device result is
compared against in tests/test_gpu_parametric_rows.py), against the rule written in Python integers and fractions, and against the
independent statement Generator(Philox).random + searchsorted; the argument checks the ABI makes before it touches a context; the
launch geometry; the command line's parsing and refusals."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT

E_ARG, E_LIMIT = -1, -4
FAIR = [.3, .05, .2, .1, .15, .08, .12]


def lib():
    from misti_amd import _lib
    return _lib.load()


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def c_thresholds(p):
    p = np.ascontiguousarray(p, dtype=np.float64)
    T = np.full(6, 77, dtype=np.uint64)
    return lib().misti_parametric_thresholds(ptr(p), ptr(T)), T


def c_counts(p, n, seed, rep):
    p = np.ascontiguousarray(p, dtype=np.float64)
    out = np.full(7, -7, dtype=np.int64)
    return lib().misti_parametric_counts(ptr(p), n, seed, rep, ptr(out)), out


def spectra():
    rng = np.random.default_rng(3)
    s = {"random%d" % i: rng.random(7) for i in range(6)}
    s["normalised"] = np.array(FAIR)
    s["unnormalised"] = rng.random(7) * 1234.5
    s["tiny total"] = rng.random(7) * 1e-200
    for k in (0, 3, 6):
        s["only class %d" % k] = np.eye(7)[k] * 2.5
    s["leading zeros"] = np.array([0, 0, .2, .1, .3, .1, .3])
    s["middle zeros"] = np.array([.2, .1, 0, 0, 0, .4, .3])
    s["trailing zeros"] = np.array([.2, .1, .3, .4, 0, 0, 0])
    s["p6 = 1e-30"] = np.array([.2, .1, .2, .1, .2, .2, 1e-30])          # q5 rounds to 1: class 6 is never drawn
    s["p0 = 1e-300"] = np.array([1e-300, .1, .2, .1, .2, .2, .2])
    return s


SPECTRA = spectra()


def thresholds_in_integers(p):
    """The rule with nothing but Python floats for the sums and quotients the rule says are float64, and exact rationals behind them."""
    c, run = [], None
    for v in p:
        run = float(v) if run is None else run + float(v)
        c.append(run)
    out = []
    for k in range(6):
        x = Fraction(c[k] / c[6]) * 2 ** 53                           # the float64 quotient, scaled exactly
        out.append(-((-x.numerator) // x.denominator))                # ceil
    return out


# ---- thresholds ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SPECTRA))
def test_thresholds_of_host_hook_numpy_rule_and_integers_agree(name):
    from misti_amd.optimize import parametric_thresholds
    p = SPECTRA[name]
    rc, T = c_thresholds(p)
    want = thresholds_in_integers(p)
    assert rc == 0 and T.tolist() == want
    host = parametric_thresholds(p)
    assert host.dtype == np.uint64 and host.tolist() == want
    assert all(0 <= a <= b <= 2 ** 53 for a, b in zip([0] + want, want + [2 ** 53]))          # non-decreasing, in [0, 2^53]
    if name == "p6 = 1e-30":
        assert want[5] == 2 ** 53
    if name == "p0 = 1e-300":
        assert want[0] == 1                                           # ceil of something tiny and positive
    if name == "only class 3":
        assert want == [0, 0, 0, 2 ** 53, 2 ** 53, 2 ** 53]


# ---- counts -------------------------------------------------------------------------------------------------------------------------------
def independent_counts(p, n, seed, rep):
    c = np.cumsum(np.asarray(p, dtype=np.float64))
    x = np.random.Generator(np.random.Philox(key=np.array([seed, rep], dtype=np.uint64))).random(n)
    return np.bincount(np.searchsorted(c[:6] / c[6], x, side="right"), minlength=7)


@pytest.mark.parametrize("seed", [0, 7, 2 ** 64 - 1])
@pytest.mark.parametrize("rep", [0, 1, 2 ** 32 + 5])
def test_counts_equal_the_numpy_rule_and_the_independent_statement(seed, rep):
    from misti_amd.optimize import parametric_rows
    for name in ("random0", "unnormalised", "middle zeros", "trailing zeros", "only class 3", "p6 = 1e-30"):
        p = SPECTRA[name]
        for n in (0, 1, 3, 4, 5, 4099):
            rc, got = c_counts(p, n, seed, rep)
            rows, status = parametric_rows([p], 1, n, 12.5, seed=seed, first=rep)
            assert rc == 0 and status.tolist() == [0] and rows.dtype == np.float64 and rows[0, 0] == 12.5
            assert got.tolist() == rows[0, 1:].tolist() == independent_counts(p, n, seed, rep).tolist(), (name, n)
            assert got.sum() == n and (got >= 0).all() and (got[np.asarray(p) == 0] == 0).all()
        if name == "p6 = 1e-30":
            assert got[6] == 0


def test_counts_of_a_prefix_are_the_histogram_of_the_first_classes():
    from misti_amd.optimize import parametric_thresholds
    p, seed, rep, n_long = SPECTRA["random1"], 5, 9, 4099
    T = [int(t) for t in parametric_thresholds(p)]
    raw = np.random.Philox(key=np.array([seed, rep], dtype=np.uint64)).random_raw(n_long)
    classes = [sum((int(v) >> 11) >= t for t in T) for v in raw]      # the rule in Python integers, draw by draw
    for n in (0, 1, 3, 4, 5, 40, 1023, 4099):
        want = np.bincount(classes[:n], minlength=7).tolist()
        assert c_counts(p, n, seed, rep)[1].tolist() == want, n


def test_rows_do_not_depend_on_n_or_first():
    from misti_amd.optimize import parametric_rows, parametric_table
    sp = [SPECTRA["random0"], SPECTRA["trailing zeros"]]
    of = np.arange(9) % 2
    full, status = parametric_rows(sp, 9, 1001, 3.0, seed=11, spec_of=of)
    assert full.shape == (9, 8) and not status.any() and (full[:, 1:].sum(axis=1) == 1001).all()
    a, _ = parametric_rows(sp, 4, 1001, 3.0, seed=11, first=5, spec_of=of[5:])
    assert np.array_equal(a, full[5:])
    assert not np.array_equal(parametric_rows(sp, 9, 1001, 3.0, seed=12, spec_of=of)[0], full)        # the seed is in the key
    t = parametric_table([9.0, 1, 2, 3, 4, 5, 6, 7], full)
    assert t.shape == (10, 8) and t[0].tolist() == [9.0, 1, 2, 3, 4, 5, 6, 7] and np.array_equal(t[1:], full)


def test_the_stream_is_a_fair_multinomial():
    """A condition, not a measurement: the NumPy statement alone gives 10.79 on exactly these inputs, 22.46 is the 99.9 % point of chi-square
    with 6 degrees of freedom - only a wrong rule fails it."""
    n = 100003
    rc, got = c_counts(FAIR, n, 7, 3)
    expect = n * np.array(FAIR)
    chi2 = float(((got - expect) ** 2 / expect).sum())
    print("chi-square", chi2)
    assert rc == 0 and got.sum() == n and chi2 < 22.46


# ---- unusable spectra ---------------------------------------------------------------------------------------------------------------------
def with_entry(k, v):
    p = list(FAIR)
    p[k] = v
    return p


UNUSABLE = {"nan": with_entry(2, float("nan")), "inf": with_entry(6, float("inf")), "negative": with_entry(0, -1e-9), "all zeros": [0.0] * 7,
            "sum overflows": [1e308] * 7}


@pytest.mark.parametrize("name", sorted(UNUSABLE))
def test_an_unusable_spectrum_is_status_1_and_a_zero_row(name):
    from misti_amd.optimize import parametric_rows, parametric_thresholds
    p = UNUSABLE[name]
    rc, T = c_thresholds(p)
    assert rc == 1 and not T.any()
    rc, counts = c_counts(p, 1000, 1, 2)
    assert rc == 1 and not counts.any()
    assert parametric_thresholds(p) is None
    rows, status = parametric_rows([FAIR, p], 4, 1000, 6.5, seed=1, spec_of=[0, 1, 0, 1])
    assert status.tolist() == [0, 1, 0, 1] and rows[1].tolist() == [6.5] + [0.0] * 7 == rows[3].tolist() and rows[0, 1:].sum() == 1000


def test_a_bad_status_and_an_index_out_of_range_behave_likewise():
    from misti_amd.optimize import parametric_rows
    good, _ = parametric_rows([FAIR], 5, 100, 2.0, seed=4)
    rows, status = parametric_rows([FAIR, FAIR, FAIR], 5, 100, 2.0, seed=4, spec_of=[0, 1, 2, 3, -1], status=[0, 5, 3])
    assert status.tolist() == [0, 1, 1, 1, 1] and np.array_equal(rows[0], good[0])
    assert (rows[1:, 1:] == 0).all() and (rows[:, 0] == 2.0).all()


# ---- what the ABI refuses before it looks at a context ------------------------------------------------------------------------------------
def rows_dev(n_spec=1, spectra=True, genome=1.0, n_sites=10, first=0, n_rep=4, rows=True):
    """misti_parametric_rows_dev WITHOUT a context (there is no device here): every check comes before the context is looked at, so
    arguments that pass end at "ctx is NULL".  The pointers are never followed."""
    L = lib()
    sp, out = np.array(FAIR), np.zeros((4, 8))
    rc = L.misti_parametric_rows_dev(None, n_spec, ptr(sp) if spectra else None, None, None, genome, n_sites, 0, first, n_rep,
                                     ptr(out) if rows else None, None)
    assert not out.any()
    return rc, L.misti_last_error().decode()


@pytest.mark.parametrize("kw, code, word", [
    (dict(), E_ARG, "ctx is NULL"),
    (dict(n_rep=0, spectra=False, rows=False), E_ARG, "ctx is NULL"),
    (dict(n_sites=0), E_ARG, "ctx is NULL"),
    (dict(n_sites=1 << 36), E_ARG, "ctx is NULL"),
    (dict(n_spec=0), E_ARG, "n_spec"),
    (dict(n_spec=-2), E_ARG, "n_spec"),
    (dict(n_sites=-1), E_ARG, "negative"),
    (dict(n_rep=-1), E_ARG, "negative"),
    (dict(first=-1), E_ARG, "negative"),
    (dict(spectra=False), E_ARG, "NULL"),
    (dict(rows=False), E_ARG, "NULL"),
    (dict(genome=float("nan")), E_ARG, "genome"),
    (dict(genome=float("inf")), E_ARG, "genome"),
    (dict(n_sites=(1 << 36) + 1), E_LIMIT, "MISTI_PARAM_MAX_SITES"),
    (dict(n_rep=2 ** 31), E_LIMIT, "replicates"),
    (dict(first=2 ** 63 - 2), E_LIMIT, "replicates"),
])
def test_rows_dev_argument_checks(kw, code, word):
    rc, why = rows_dev(**kw)
    assert rc == code and word in why, (rc, why)


def test_the_host_hooks_check_their_own_arguments():
    L = lib()
    p, T, counts, b = np.array(FAIR), np.zeros(6, dtype=np.uint64), np.zeros(7, dtype=np.int64), C.c_int32(-1)
    assert L.misti_parametric_thresholds(None, ptr(T)) == E_ARG and L.misti_parametric_thresholds(ptr(p), None) == E_ARG
    assert L.misti_parametric_counts(None, 4, 0, 0, ptr(counts)) == E_ARG and L.misti_parametric_counts(ptr(p), 4, 0, 0, None) == E_ARG
    assert L.misti_parametric_counts(ptr(p), -1, 0, 0, ptr(counts)) == E_ARG and L.misti_parametric_counts(ptr(p), 4, 0, -1, ptr(counts)) == E_ARG
    assert L.misti_parametric_counts(ptr(p), (1 << 36) + 1, 0, 0, ptr(counts)) == E_LIMIT and b"MISTI_PARAM_MAX_SITES" in L.misti_last_error()
    assert L.misti_parametric_geometry(-1, 4, C.byref(b)) == E_ARG and L.misti_parametric_geometry(4, -1, C.byref(b)) == E_ARG
    assert L.misti_parametric_geometry(4, 4, None) == E_ARG
    assert L.misti_parametric_geometry((1 << 36) + 1, 4, C.byref(b)) == E_LIMIT and L.misti_parametric_geometry(4, 2 ** 31, C.byref(b)) == E_LIMIT
    assert b.value == -1                                              # a refused call writes nothing


def geometry(n_sites, n_rep):
    b = C.c_int32(-1)
    assert lib().misti_parametric_geometry(n_sites, n_rep, C.byref(b)) == 0
    return b.value


def test_geometry_is_the_stated_function_of_sites_and_replicates():
    assert geometry(1000, 1000) == 1
    assert geometry(2 ** 22 + 3, 1) > 1
    for n_sites in (0, 1, 4096 * 4, 4096 * 4 + 1, 10 ** 6, 5 * 10 ** 6, 2 ** 30, 2 ** 36):
        for n_rep in (0, 1, 2, 700, 1000, 8192, 10 ** 5, 2 ** 31 - 1):
            want = max(1, min(-(-8192 // max(n_rep, 1)), -(-(-(-n_sites // 4)) // 4096)))
            assert geometry(n_sites, n_rep) == want >= 1, (n_sites, n_rep)


# ---- header, binding, build, command line -------------------------------------------------------------------------------------------------
def test_header_binding_and_build_name_the_feature_and_the_abi_stays_6():
    from misti_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "misti_hip.h")).read()
    assert re.search(r"^int misti_parametric_rows_dev\(misti_ctx\* ctx, int64_t n_spec, const double\* d_spectra", hdr, flags=re.M)
    assert re.search(r"^int misti_parametric_thresholds\(const double p\[7\], uint64_t T\[6\]\);", hdr, flags=re.M)
    assert re.search(r"^int misti_parametric_counts\(const double p\[7\], int64_t n_sites, uint64_t seed, int64_t rep, int64_t counts\[7\]\);", hdr, flags=re.M)
    assert re.search(r"^int misti_parametric_geometry\(int64_t n_sites, int64_t n_rep, int32_t\* blocks_per_rep\);", hdr, flags=re.M)
    assert "#define MISTI_PARAM_MAX_SITES (1ll << 36)" in hdr and "#define MISTI_ABI_VERSION 6" in hdr
    assert "INDEPENDENTLY" in hdr and "2^-53" in hdr                  # the caveat and the quantisation are documented
    assert lib().misti_abi_version() == 6 and _lib.ABI_VERSION == 6 and _lib.PARAM_MAX_SITES == 1 << 36
    assert {"misti_parametric_rows_dev", "misti_parametric_thresholds", "misti_parametric_counts", "misti_parametric_geometry"} <= set(_lib.SYMBOLS)
    assert "misti_parametric.hip" in build.SOURCES and "misti_parametric.h" in build.HEADERS


BASE = ["a.psmc", "b.psmc", "d.sfs", "20"]


def test_parser_accepts_parametric():
    from misti_amd import cli
    a = cli.build_parser().parse_args(BASE + ["--parametric", "8", "--sites", "5000", "--bs-seed", "3", "--bootstrap-out", "t.sfs", "--grid-st", "15", "17"])
    assert (a.parametric, a.sites, a.bs_seed, a.bootstrap_out) == (8, 5000, 3, "t.sfs")
    assert cli.parametric_error(a) is None and cli.bootstrap_error(a) is None
    a = cli.build_parser().parse_args(BASE + ["--parametric", "1000", "--all-bs", "--gpus", "2"])
    assert cli.parametric_error(a) is None and cli.bootstrap_error(a) is None and a.sites is None
    a = cli.build_parser().parse_args(BASE)
    assert cli.parametric_error(a) is None and a.parametric is None
    text = " ".join(cli.build_parser().format_help().split())
    assert "--parametric" in text and "independently" in text and "narrower" in text               # --help states the caveat
    assert "INDEPENDENTLY" in cli.__doc__


@pytest.mark.parametrize("args, word", [
    (["--parametric", "0"], "at least 1"),
    (["--parametric", "-3"], "at least 1"),
    (["--parametric", "8", "--bootstrap", "8"], "give one of them"),
    (["--parametric", "8", "--bs-normalize"], "nothing to normalise"),
    (["--parametric", "8", "-bs", "2"], "-bs K"),
    (["--parametric", "8", "-bs", "0"], "-bs K"),
    (["--parametric", "8", "--bs-seed", "-1"], "uint64"),
    (["--parametric", "8", "--bs-seed", str(2 ** 64)], "uint64"),
    (["--parametric", "8", "--sites", "0"], "--sites M"),
    (["--parametric", "8", "--sites", str(2 ** 36 + 1)], "--sites M"),
    (["--sites", "100"], "give --parametric"),
])
def test_parametric_error_names_the_reason(args, word):
    from misti_amd import cli
    why = cli.parametric_error(cli.build_parser().parse_args(BASE + args))
    assert why is not None and word in why, why


@pytest.mark.parametrize("args, word", [
    (["--bs-seed", "3"], "give --bootstrap"),
    (["--bs-normalize"], "give --bootstrap"),
    (["--bootstrap-out", "t.sfs"], "give --bootstrap"),
    (["--bootstrap", "8", "-bs", "2"], "-bs K"),
    (["--bootstrap", "0"], "at least 1"),
])
def test_without_parametric_the_bootstrap_messages_are_untouched(args, word):
    from misti_amd import cli
    a = cli.build_parser().parse_args(BASE + args)
    assert cli.parametric_error(a) is None
    why = cli.bootstrap_error(a)
    assert why is not None and word in why, why


def test_refused_before_a_file_is_read(capsys):
    from misti_amd import cli
    assert cli.main(["no.psmc", "no.psmc", "no.sfs", "20", "--parametric", "8", "--bs-normalize"]) == 2      # (the files do not exist)
    assert "nothing to normalise" in capsys.readouterr().err
    assert cli.main(["no.psmc", "no.psmc", "no.sfs", "20", "--parametric", "8", "--bootstrap", "4"]) == 2
    assert "give one of them" in capsys.readouterr().err
