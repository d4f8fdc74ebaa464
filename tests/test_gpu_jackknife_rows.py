"""Delete-m block jackknife on the device (misti_jackknife_rows_dev, Engine.jackknife_rows_dev / jackknife_table, `--jackknife M`).
The reference everywhere is the rule stated in NumPy, optimize.jackknife_rows: every comparison is on the float64 bits, nothing by
tolerance.  The kernel stages the chunk table through LDS in tiles of 1 024 rows: tables one below, at and one above a tile, and of
several tiles; group counts below, at and above a wave and a workgroup; short last groups and groups that span a tile boundary."""
import contextlib
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 5, 257, 1023, 1024, 1025, 5000)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def random_table(seed, n_chunk):
    """Counts in multiples of 0.1 and lengths that are no integers either: the order of the additions shows in the last bits."""
    rng = np.random.default_rng(seed)
    c = np.zeros((n_chunk, 8))
    c[:, 1:] = rng.integers(0, 400, size=(n_chunk, 7)) * 0.1
    c[:, 0] = rng.integers(1, 50, size=n_chunk) * 0.1 + c[:, 1:].sum(axis=1)
    return c


def group_sizes(n_chunk):
    return [m for m in sorted({1, 2, 7, 64, 65, n_chunk - 1}) if 1 <= m < n_chunk]


@pytest.fixture(scope="module")
def case():
    """The tables and, computed once, the NumPy statement of every (table, m) the tests use."""
    from misti_amd.optimize import jackknife_rows
    return {n: (c, {m: jackknife_rows(c, m) for m in group_sizes(n)}) for n, c in ((n, random_table(n, n)) for n in SIZES)}


def psmc_inputs():
    from misti_amd import synth, io as mio
    return mio.merge_psmc(mio.read_psmc_file(io.StringIO(synth.psmc_text(16, 1, synth.THETA_1))),
                          mio.read_psmc_file(io.StringIO(synth.psmc_text(17, 2, synth.THETA_2))))


@pytest.fixture(scope="module")
def eng():
    from misti_amd.engine import Engine
    inp = psmc_inputs()
    with Engine(inp.times, inp.lambdas) as e:
        yield e


@pytest.mark.parametrize("n_chunk", SIZES)
def test_every_table_equals_the_numpy_rule(eng, case, n_chunk):
    c, want = case[n_chunk]
    seen = set()
    for m, rows in want.items():
        got = eng.jackknife_rows_dev(c, m)
        assert tuple(got.shape) == (-(-n_chunk // m), 8)
        assert same_bits(got.cpu().numpy(), rows), (n_chunk, m)
        seen.add(rows.shape[0])
    if n_chunk == 5000:
        # 79 groups: 78 of 64 chunks and a short one of 8, every 16th group boundary on a tile boundary; 77 groups of 65 span them
        assert {5000, 2500, 715, 79, 77, 2} == seen
    if n_chunk == 1025:
        assert {1025, 513, 147, 17, 16, 2} == seen                   # m = 64: group 16 is the one chunk of the second tile


def test_group_counts_around_a_wave_and_a_workgroup(eng):
    """63, 64 and 65 groups; 256 and 257: a full workgroup and one lane more."""
    from misti_amd.optimize import jackknife_rows
    for n_chunk, m in ((63, 1), (64, 1), (65, 1), (127, 2), (256, 1), (257, 1), (512, 2), (1799, 7)):
        c = random_table(1000 + n_chunk, n_chunk)
        assert same_bits(eng.jackknife_rows_dev(c, m).cpu().numpy(), jackknife_rows(c, m)), (n_chunk, m)


@pytest.mark.parametrize("n_chunk, m", [(257, 1), (1025, 2), (5000, 7)])
def test_two_calls_equal_one_and_nothing_is_written_beyond_the_rows(eng, case, n_chunk, m):
    """first_group = 0 and G / 2 through the C ABI into ONE buffer, with guard rows behind it."""
    import torch
    from misti_amd import _lib
    c, want = case[n_chunk]
    want = want[m]
    G = want.shape[0]
    dev = torch.device("cuda", 0)
    rows = torch.full((G + 8, 8), 7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    half = G // 2
    for first, n in ((0, half), (half, G - half)):
        _lib.check(eng._lib.misti_jackknife_rows_dev(eng._ctx, n_chunk, c.ctypes.data_as(C.c_void_p), m, first, n, 0, C.c_void_p(rows.data_ptr() + first * 64)))
    _lib.check(eng._lib.misti_jackknife_rows_dev(eng._ctx, n_chunk, c.ctypes.data_as(C.c_void_p), m, 0, 0, 0, None))       # n_group == 0: nothing
    _lib.check(eng._lib.misti_jackknife_rows_dev(eng._ctx, n_chunk, None, m, G, 0, 0, None))
    eng.sync()
    got = rows.cpu().numpy()
    assert same_bits(got[:G], want) and (got[G:] == 7.0).all()
    assert same_bits(eng.jackknife_rows_dev(c, m, first=half).cpu().numpy(), want[half:])
    assert same_bits(eng.jackknife_rows_dev(c, m, first=1, n=3).cpu().numpy(), want[1:4])
    assert tuple(eng.jackknife_rows_dev(c, m, first=G, n=0).shape) == (0, 8)


def test_the_tables(eng, case):
    from misti_amd.engine import MultiEngine
    from misti_amd.optimize import jackknife_table
    c = case[257][0]
    for m in (1, 7):
        table = eng.jackknife_table(c, m)
        assert isinstance(table, np.ndarray) and same_bits(table, jackknife_table(c, m))
    inp = psmc_inputs()
    with MultiEngine(inp.times, inp.lambdas, devices=[0, 0]) as multi:
        assert same_bits(multi.jackknife_table(c, 7), jackknife_table(c, 7))
        assert same_bits(multi.jackknife_table(case[1025][0], 64), np.vstack([jackknife_table(case[1025][0], 64)[:1], case[1025][1][64]]))


def test_a_refused_table_raises_with_the_codes_of_the_header(eng):
    from misti_amd._lib import MistiError
    bad = random_table(2, 4)
    bad[2, 0] = 0.0
    with pytest.raises(MistiError) as ei:
        eng.jackknife_rows_dev(bad, 1)
    assert ei.value.code == -1 and "length" in str(ei.value)
    with pytest.raises(MistiError) as ei:
        eng.jackknife_rows_dev(np.ones((65536, 8)), 1)
    assert ei.value.code == -4
    with pytest.raises(MistiError) as ei:
        eng.jackknife_rows_dev(random_table(2, 4), 4)
    assert ei.value.code == -1 and "single group" in str(ei.value)
    with pytest.raises(MistiError) as ei:
        eng.jackknife_rows_dev(random_table(2, 4), 2, first=1, n=2)
    assert ei.value.code == -1 and "of G = 2" in str(ei.value)
    # a table beyond the bootstrap's draw limit is a table here
    far = random_table(3, 3)
    far[0, 0], far[1, 0] = float(2 ** 24) * 5.0, 5.0
    from misti_amd.optimize import jackknife_rows
    assert same_bits(eng.jackknife_rows_dev(far, 1).cpu().numpy(), jackknife_rows(far, 1))
    with pytest.raises(MistiError) as ei:
        eng.bootstrap_rows_dev(far, 1)
    assert ei.value.code == -4


def test_the_device_rows_are_a_row_buffer(eng):
    """Engine.evaluate takes the device tensor as it is: the same log-likelihood bits as on the host table."""
    from misti_amd.optimize import jackknife_rows
    rng = np.random.default_rng(12)
    c = np.zeros((40, 8))
    c[:, 1:] = rng.integers(50, 5000, size=(40, 7))
    c[:, 0] = c[:, 1:].sum(axis=1) + rng.integers(1000, 2000, size=40)
    d_rows = eng.jackknife_rows_dev(c, 3)
    h_rows = jackknife_rows(c, 3)
    split = 8.0 + 0.25 * np.arange(3)
    a, b = eng.evaluate(split, None, d_rows), eng.evaluate(split, None, h_rows)
    assert same_bits(a.llk, b.llk) and a.llk.shape == (3, 14) and np.isfinite(a.llk).all()


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def run_cli(args):
    from misti_amd import cli
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc = cli.main(args)
    return rc, out.getvalue()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The small synthetic inputs of the other command-line tests: two PSMC files and a JSFS of 12 chunks."""
    from misti_amd import synth, io as mio
    from oracle.batch import oracle_truth_spectrum
    d = tmp_path_factory.mktemp("jackknife")
    f1, f2, fj = (str(d / n) for n in ("g1.psmc", "g2.psmc", "chunks.sfs"))
    open(f1, "w").write(synth.psmc_text(16, 1, synth.THETA_1))
    open(f2, "w").write(synth.psmc_text(17, 2, synth.THETA_2))
    inp = mio.read_psmc(f1, f2)
    jafs = oracle_truth_spectrum(inp.times, inp.lambdas, 20, [(0, 2, 20, 0.1, -1)], [], 0)
    chunks = synth.chunk_rows(synth.counts_from_spectrum(jafs, 200000), 12)
    open(fj, "w").write(mio.format_jsfs(chunks))
    return f1, f2, fj, inp, np.array(chunks, dtype=float), str(d / "nounits.txt"), str(d / "table.sfs")


LINE = re.compile(r"^jackknife: (\S+) \testimate = (\S+) \tjackknife = (\S+) \tbias = (\S+) \tse = (\S+) \tinterval = \[(\S+), (\S+)\] \tgroups = (\d+)$")


def jackknife_lines(text):
    return [l for l in text.splitlines() if l.startswith("jackknife:")]


def assert_lines_equal_the_estimate(lines, names, theta, lengths):
    from misti_amd.optimize import jackknife_estimate
    assert len(lines) == len(names), lines
    for k, (line, name) in enumerate(zip(lines, names)):
        m = LINE.match(line)
        assert m and m.group(1) == name, line
        want = jackknife_estimate(theta[:, k], lengths)
        got = [float(v) for v in m.groups()[1:7]]
        assert got == [want["estimate"], want["jackknife"], want["bias"], want["se"], want["interval"][0], want["interval"][1]], (line, want)
        assert int(m.group(8)) == want["n_group"] == len(lengths) - 1


def test_cli_fit_st_prints_the_jackknife_lines_and_the_written_table_repeats_the_run(files):
    from misti_amd import io as mio
    from misti_amd.engine import Engine
    from misti_amd.optimize import jackknife_table, split_fit
    f1, f2, fj, inp, chunks, units, out = files
    model = ["-mi", "1", "2", "20", "0.1", "1", "--cpfit", "--funits", units, "--grid-st", "19", "20", "0.5", "--fit-st"]
    rc, text = run_cli([f1, f2, fj, "20"] + model + ["--jackknife", "2", "--jackknife-out", out])
    assert rc == 0 and "Jackknife: 6 leave-out rows of 12 chunks in groups of 2 made on the device" in text
    assert "t-interval" not in text and len([l for l in text.splitlines() if l.startswith("bs_id =")]) == 7
    table, _, _ = mio.read_jsfs(out)
    assert same_bits(np.array(table), jackknife_table(chunks, 2))     # the file reads back as the table, exactly
    with Engine(inp.times, inp.lambdas, [(0, 2, -1, 0.1, 0)], [], n_param=1, cpfit=True, smooth=True, unfolded=False,
                sample_date=inp.sampleDateDiscr) as e:
        t = e.jackknife_table(chunks, 2)
        fit = split_fit(e, t, [[0.1]], [19.0, 19.5, 20.0])
    assert np.isfinite(fit["llh"]).all()
    theta = np.hstack([fit["split"][:, None], fit["x"][:, :1]])
    assert_lines_equal_the_estimate(jackknife_lines(text), ["splitT", "optim[0]"], theta, t[:, 0])
    rc2, text2 = run_cli([f1, f2, out, "20"] + model + ["--jackknife", "0", "--all-bs"])
    assert rc2 == 0 and jackknife_lines(text2) == jackknife_lines(text) and "Jackknife:" not in text2 and "t-interval" not in text2


def test_cli_grid_solve_prints_a_line_per_rate(files):
    from misti_amd.engine import Engine
    from misti_amd.optimize import bootstrap_profile
    f1, f2, fj, inp, chunks, units, _ = files
    rc, text = run_cli([f1, f2, fj, "20", "-mi", "1", "2", "20", "0.1", "1", "-mi", "2", "2", "20", "0.05", "1", "--cpfit", "--funits", units,
                        "--grid-st", "19", "20", "--grid-solve", "--jackknife", "1"])
    assert rc == 0 and "Jackknife: 12 leave-out rows of 12 chunks in groups of 1 made on the device" in text
    assert "t-interval" not in text and "grid-solve: bs_id = 0 best splitT" in text
    with Engine(inp.times, inp.lambdas, [(0, 2, -1, 0.1, 0), (1, 2, -1, 0.05, 1)], [], n_param=2, cpfit=True, smooth=True, unfolded=False,
                sample_date=inp.sampleDateDiscr) as e:
        t = e.jackknife_table(chunks, 1)
        prof = bootstrap_profile(e, [19.0, 20.0], t, np.array([[0.1, 0.05]]), tol=1e-4, maxiter=1000)
    assert np.isfinite(prof["llh"]).all()
    at = np.argmax(prof["llh"], axis=1)
    theta = prof["x"][np.arange(13), at]
    assert_lines_equal_the_estimate(jackknife_lines(text), ["optim[0]", "optim[1]"], theta, t[:, 0])
