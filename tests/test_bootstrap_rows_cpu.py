"""The block bootstrap without a GPU: the generator of misti_bootstrap_rows_dev (misti_bootstrap_draws runs the very functions the
kernel calls) against NumPy's Philox and against the rule written out in Python integers; the rule itself (optimize.block_bootstrap -
what the device result is compared against in tests/test_gpu_bootstrap_rows.py); the argument checks the ABI makes before it touches a
context; the command line's parsing and refusals."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from conftest import ROOT

E_ARG, E_LIMIT = -1, -4


def lib():
    from misti_amd import _lib
    return _lib.load()


def c_draws(seed, rep, n_chunk, n):
    idx = np.full(n, -7, dtype=np.int64)
    rc = lib().misti_bootstrap_draws(seed, rep, n_chunk, n, idx.ctypes.data_as(C.c_void_p))
    assert rc == 0, lib().misti_last_error()
    return idx


def small_table(rng, n_chunk, fractional=False):
    c = np.zeros((n_chunk, 8))
    c[:, 1:] = rng.integers(0, 400, size=(n_chunk, 7))
    if fractional:
        c[:, 1:] *= 0.1                               # no longer integers: the order of the additions shows in the last bits
    c[:, 0] = rng.integers(1, 50, size=n_chunk) * (0.1 if fractional else 1.0) + c[:, 1:].sum(axis=1)
    return c


# ---- the generator --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 7, 2 ** 64 - 1])
@pytest.mark.parametrize("rep", [0, 1, 2 ** 32 + 5])
def test_draws_equal_numpys_philox_and_the_rule_in_integers(seed, rep):
    """4 099 draws cross a thousand block boundaries and end off a block.  NumPy's counter convention is part of what is checked:
    numpy.random.Philox advances the counter before its first block, and so does philox4x64_10_block."""
    from misti_amd.optimize import philox_draws
    n = 4099
    raw = np.random.Philox(key=np.array([seed, rep], dtype=np.uint64)).random_raw(n)
    for n_chunk in (1, 3, 1000, 65535):
        want = [(int(v) * n_chunk) >> 64 for v in raw]
        host = philox_draws(seed, rep, n_chunk, n)
        assert host.dtype == np.int64 and host.tolist() == want, n_chunk
        assert c_draws(seed, rep, n_chunk, n).tolist() == want, n_chunk
        assert 0 <= min(want) and max(want) < n_chunk


def test_a_prefix_of_the_stream_is_the_stream():
    from misti_amd.optimize import philox_draws
    full = c_draws(5, 9, 77, 41)
    for n in (0, 1, 3, 4, 5, 40):
        assert np.array_equal(c_draws(5, 9, 77, n), full[:n]) and np.array_equal(philox_draws(5, 9, 77, n), full[:n])


def test_draws_checks_its_own_arguments():
    L = lib()
    idx = np.zeros(8, dtype=np.int64)
    p = idx.ctypes.data_as(C.c_void_p)
    assert L.misti_bootstrap_draws(0, 0, 3, 8, None) == E_ARG and b"NULL" in L.misti_last_error()
    assert L.misti_bootstrap_draws(0, 0, 3, 0, None) == 0                    # nothing to write: no buffer needed
    assert L.misti_bootstrap_draws(0, -1, 3, 8, p) == E_ARG
    assert L.misti_bootstrap_draws(0, 0, 3, -1, p) == E_ARG
    assert L.misti_bootstrap_draws(0, 0, 0, 8, p) == E_ARG
    assert L.misti_bootstrap_draws(0, 0, -3, 8, p) == E_ARG
    assert L.misti_bootstrap_draws(0, 0, 65536, 8, p) == E_LIMIT and b"MISTI_BOOT_MAX_CHUNKS" in L.misti_last_error()
    assert L.misti_bootstrap_draws(0, 0, 3, (1 << 24) + 1, p) == E_LIMIT and b"MISTI_BOOT_MAX_DRAWS" in L.misti_last_error()
    assert L.misti_bootstrap_draws(0, 0, 65535, 8, p) == 0


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_chunk, fractional", [(1, False), (3, True), (40, False), (257, True)])
def test_structure_of_a_replicate(n_chunk, fractional):
    from misti_amd.optimize import block_bootstrap, philox_draws
    c = small_table(np.random.default_rng(n_chunk), n_chunk, fractional)
    genome = 0.0
    for v in c[:, 0]:
        genome += float(v)                            # plain additions in chunk order
    rows, draws = block_bootstrap(c, 12, seed=3, first=2, draws=True)
    assert rows.shape == (12, 8) and rows.dtype == np.float64 and draws.shape == (12,) and draws.dtype == np.int32
    for i in range(12):
        idx = philox_draws(3, 2 + i, n_chunk, int(draws[i]))
        sfs = [0.0] * 8
        before = None
        for j in idx:
            before = sfs[0]
            sfs = [a + float(b) for a, b in zip(sfs, c[j])]          # BootstrapJAFS's own statement: every column in draw order
        assert rows[i].tolist() == sfs                                # the same bits
        assert sfs[0] >= genome and before < genome                   # it stopped at the first total that reaches the genome
    if n_chunk == 1:
        assert (draws == 1).all() and (rows == c[0]).all()


def test_rows_do_not_depend_on_n_or_first():
    from misti_amd.optimize import block_bootstrap, block_bootstrap_table
    c = small_table(np.random.default_rng(8), 23, True)
    t9 = block_bootstrap_table(c, 9, seed=11)
    assert t9.shape == (10, 8)
    col = [0.0] * 8
    for r in c:
        col = [a + float(b) for a, b in zip(col, r)]
    assert t9[0].tolist() == col                                      # row 0: the column sums in chunk order
    for n in (1, 4):
        assert np.array_equal(block_bootstrap_table(c, n, seed=11), t9[:1 + n])
    assert np.array_equal(block_bootstrap(c, 4, seed=11, first=5), t9[6:10])
    assert np.array_equal(block_bootstrap(c, 0, seed=11), np.empty((0, 8)))
    assert not np.array_equal(block_bootstrap(c, 9, seed=12), t9[1:])      # the seed is in the key


class _Picks:
    """random.randint's place in io.bootstrap_jsfs, handing out a fixed sequence of picks."""

    def __init__(self, idx):
        self.idx = list(idx)

    def randint(self, lo, hi):
        return int(self.idx.pop(0))


def test_normalize_is_the_references_arithmetic_on_the_same_picks():
    from misti_amd import io as mio
    from misti_amd.optimize import block_bootstrap, philox_draws
    c = small_table(np.random.default_rng(5), 31)                     # integer counts, as a JSFS file has them
    rows, draws = block_bootstrap(c, 6, seed=2, normalize=True, draws=True)
    plain = block_bootstrap(c, 6, seed=2)
    for i in range(6):
        picks = philox_draws(2, i, 31, int(draws[i]))
        want = mio.bootstrap_jsfs([list(map(float, r)) for r in c], rng=_Picks(picks), normalize=True)
        assert rows[i].tolist() == [float(v) for v in want]
        assert plain[i].tolist() == [float(v) for v in mio.bootstrap_jsfs([list(map(float, r)) for r in c], rng=_Picks(picks))]
    # ... and stated outright on counts that are no integers: the division first, then 8 products
    c = small_table(np.random.default_rng(6), 7, True)
    rows = block_bootstrap(c, 5, seed=1, normalize=True)
    plain = block_bootstrap(c, 5, seed=1)
    seg = 0.0
    for r in c:
        seg += ((((((float(r[1]) + float(r[2])) + float(r[3])) + float(r[4])) + float(r[5])) + float(r[6])) + float(r[7]))
    for i in range(5):
        s = [float(v) for v in plain[i]]
        scale = seg / ((((((s[1] + s[2]) + s[3]) + s[4]) + s[5]) + s[6]) + s[7])
        assert rows[i].tolist() == [v * scale for v in s]


def test_the_references_own_stream_is_left_alone():
    """io.bootstrap_table keeps Python's Mersenne Twister (fixtures pin it): the new rule is beside it, not in its place."""
    from misti_amd import io as mio
    c = [list(map(float, r)) for r in small_table(np.random.default_rng(5), 9)]
    random.seed(4)
    a = mio.bootstrap_table(c, 3)
    random.seed(4)
    assert a == mio.bootstrap_table(c, 3) and len(a) == 4


# ---- what the ABI refuses before it looks at a context ----------------------------------------------------------------------------------
def rows_dev(chunks, n_chunk=None, n_rep=4, first=0, flags=0, rows=1, ctx=None):
    """misti_bootstrap_rows_dev WITHOUT a context (there is no device here): every check of its arguments comes before the context is
    looked at, so each refusal below is the table's, and a table that passes ends at "ctx is NULL".  `rows` is never written."""
    L = lib()
    c = None if chunks is None else np.ascontiguousarray(chunks, dtype=np.float64)
    out = np.zeros((max(n_rep, 1), 8)) if rows else None
    rc = L.misti_bootstrap_rows_dev(ctx, c.shape[0] if n_chunk is None else n_chunk, None if c is None else c.ctypes.data_as(C.c_void_p),
                                    0, first, n_rep, flags, None if out is None else out.ctypes.data_as(C.c_void_p), None)
    assert out is None or not out.any()
    return rc, L.misti_last_error().decode()


GOOD = [[10.0, 1, 2, 3, 0, 0, 0, 0], [5.0, 0, 0, 0, 1, 1, 1, 1]]


def bad(i, k, v):
    c = [list(r) for r in GOOD]
    c[i][k] = v
    return c


@pytest.mark.parametrize("kw, code, word", [
    (dict(chunks=GOOD), E_ARG, "ctx is NULL"),                                  # the table passes: only the context is missing
    (dict(chunks=GOOD, n_rep=0), E_ARG, "ctx is NULL"),
    (dict(chunks=None, n_chunk=2), E_ARG, "NULL"),
    (dict(chunks=GOOD, rows=0), E_ARG, "NULL"),
    (dict(chunks=GOOD, n_chunk=0), E_ARG, "n_chunk"),
    (dict(chunks=GOOD, n_chunk=-1), E_ARG, "n_chunk"),
    (dict(chunks=GOOD, n_rep=-1), E_ARG, "negative"),
    (dict(chunks=GOOD, first=-1), E_ARG, "negative"),
    (dict(chunks=GOOD, flags=2), E_ARG, "flag"),
    (dict(chunks=bad(1, 3, float("nan"))), E_ARG, "not finite"),
    (dict(chunks=bad(0, 0, float("inf"))), E_ARG, "not finite"),
    (dict(chunks=bad(1, 7, -1.0)), E_ARG, "negative"),
    (dict(chunks=bad(0, 0, 0.0)), E_ARG, "length"),
    (dict(chunks=bad(1, 0, -2.0)), E_ARG, "length"),
    (dict(chunks=GOOD, n_chunk=65536), E_LIMIT, "MISTI_BOOT_MAX_CHUNKS"),
    (dict(chunks=bad(0, 0, float(2 ** 24) * 5.0)), E_LIMIT, "MISTI_BOOT_MAX_DRAWS"),   # ceil(genome / 5) = 2^24 + 1 draws
    (dict(chunks=bad(0, 0, 1e300)), E_LIMIT, "MISTI_BOOT_MAX_DRAWS"),
])
def test_rows_dev_argument_checks(kw, code, word):
    rc, why = rows_dev(**kw)
    assert rc == code and word in why, (rc, why)


def test_the_draw_limit_is_exactly_where_the_header_puts_it():
    rc, why = rows_dev(bad(0, 0, float(2 ** 24) * 5.0 - 5.0))          # ceil(genome / 5) = 2^24: allowed
    assert rc == E_ARG and "ctx is NULL" in why


def test_check_chunks_refuses_what_the_abi_refuses():
    from misti_amd.optimize import check_chunks, block_bootstrap
    for c, word in ((bad(1, 3, float("nan")), "finite"), (bad(1, 7, -1.0), "negative"), (bad(0, 0, 0.0), "length"),
                    (bad(0, 0, float(2 ** 24) * 5.0), "draws"), (np.ones((65536, 8)), "65535"), (np.zeros((0, 8)), "at least one"),
                    (np.ones((4, 7)), "[n_chunk][8]")):
        with pytest.raises(ValueError, match=re.escape(word)):
            check_chunks(c)
        with pytest.raises(ValueError):
            block_bootstrap(c, 1)
    c, genome, seg = check_chunks(GOOD)
    assert genome == 15.0 and seg == 10.0 and c.shape == (2, 8)


# ---- header, binding, command line --------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_entry_points_and_the_abi_stays_6():
    from misti_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "misti_hip.h")).read()
    assert re.search(r"^int misti_bootstrap_rows_dev\(misti_ctx\* ctx, int64_t n_chunk, const double\* chunks", hdr, flags=re.M)
    assert re.search(r"^int misti_bootstrap_draws\(uint64_t seed, int64_t rep, int64_t n_chunk, int64_t n, int64_t\* idx", hdr, flags=re.M)
    for d in ("#define MISTI_BOOT_NORMALIZE   1u", "#define MISTI_BOOT_MAX_CHUNKS  65535", "#define MISTI_BOOT_MAX_DRAWS   (1 << 24)",
              "#define MISTI_ABI_VERSION 6"):
        assert d in hdr, d
    assert "Mersenne Twister" in hdr                                   # the header says whose stream this is not
    assert lib().misti_abi_version() == 6 and _lib.ABI_VERSION == 6
    assert {"misti_bootstrap_rows_dev", "misti_bootstrap_draws"} <= set(_lib.SYMBOLS)
    assert (_lib.BOOT_NORMALIZE, _lib.BOOT_MAX_CHUNKS, _lib.BOOT_MAX_DRAWS) == (1, 65535, 1 << 24)
    assert "misti_boot.hip" in build.SOURCES and "misti_boot.h" in build.HEADERS


BASE = ["a.psmc", "b.psmc", "d.sfs", "20"]


def test_parser_accepts_bootstrap():
    from misti_amd import cli
    a = cli.build_parser().parse_args(BASE + ["--bootstrap", "8", "--bs-seed", "3", "--bs-normalize", "--bootstrap-out", "t.sfs", "--grid-st", "15", "17"])
    assert (a.bootstrap, a.bs_seed, a.bs_normalize, a.bootstrap_out) == (8, 3, True, "t.sfs") and cli.bootstrap_error(a) is None
    a = cli.build_parser().parse_args(BASE + ["--bootstrap", "1000", "--all-bs", "--gpus", "2"])
    assert cli.bootstrap_error(a) is None and a.bs_seed is None
    assert cli.bootstrap_error(cli.build_parser().parse_args(BASE)) is None
    assert "Mersenne Twister" in " ".join(cli.build_parser().format_help().split())          # --help says whose stream this is not


@pytest.mark.parametrize("args, word", [
    (["--bootstrap", "8", "-bs", "2"], "-bs K"),
    (["--bootstrap", "8", "-bs", "0"], "-bs K"),
    (["--bootstrap", "0"], "at least 1"),
    (["--bootstrap", "-4"], "at least 1"),
    (["--bs-seed", "3"], "give --bootstrap"),
    (["--bs-normalize"], "give --bootstrap"),
    (["--bootstrap-out", "t.sfs"], "give --bootstrap"),
    (["--bootstrap", "8", "--bs-seed", "-1"], "uint64"),
    (["--bootstrap", "8", "--bs-seed", str(2 ** 64)], "uint64"),
])
def test_bootstrap_error_names_the_reason(args, word):
    from misti_amd import cli
    why = cli.bootstrap_error(cli.build_parser().parse_args(BASE + args))
    assert why is not None and word in why, why


def test_refused_before_a_file_is_read(capsys):
    from misti_amd import cli
    assert cli.main(["no.psmc", "no.psmc", "no.sfs", "20", "--bootstrap", "8", "-bs", "1"]) == 2      # (the files do not exist)
    assert "-bs K" in capsys.readouterr().err


def test_a_file_the_abi_would_refuse_is_an_argument_error(tmp_path, capsys):
    """A chunk of length 0 never lets a replicate end: refused with one line when the file is read, before the PSMC files or the GPU."""
    from misti_amd import cli, io as mio
    fj = tmp_path / "d.sfs"
    fj.write_text(mio.format_jsfs([[10.0, 1, 2, 3, 0, 0, 0, 4], [0.0, 0, 0, 0, 0, 0, 0, 0]]))
    rc = cli.main(["no.psmc", "no.psmc", str(fj), "20", "--bootstrap", "8", "--funits", str(tmp_path / "nounits.txt")])
    err = capsys.readouterr().err.strip()
    assert rc == 2 and "length" in err and len(err.splitlines()) == 1
