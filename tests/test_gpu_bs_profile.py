"""Batched Nelder-Mead over (replicate row, split time) pairs - misti_nm_solve_rows, optimize.bootstrap_profile and `--grid-solve` -
on config 3's model with its band ends following the split (the test.bs scripts' `-mi 1 4 ${st} ...`) and a bootstrap table built
as workloads.config4 builds one.  Every pair must be exactly the separate search misti_nm_solve runs at that split against that row."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("x", "llh", "nit", "nfev", "status")


@pytest.fixture(scope="module")
def model():
    from misti_amd import io as mio, synth, workloads
    from misti_amd.engine import Engine, truth_spectrum
    w = workloads.config3(lambda *a: truth_spectrum(*a), n_start=4)
    bands = [(p, s, -1, v, k) for p, s, e, v, k in w.bands]          # band ends follow each candidate's split
    table = np.array(mio.bootstrap_table(synth.chunk_rows(w.jsfs[0], 20), 4, random.Random(3)), dtype=np.float64)
    kw = w.engine_kwargs()
    kw["bands"] = bands
    eng = Engine(w.times, w.lh, **kw)
    start = np.array([b[3] for b in bands])                            # the -mi initial values
    yield eng, table, start
    eng.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_against_separate(eng, table, starts, splits, rows, maxiter=1000):
    got = eng.nm_solve_rows(starts, splits, rows, table, tol=1e-4, maxiter=maxiter)
    for s in range(len(splits)):
        one = eng.nm_solve(starts[s:s + 1], float(splits[s]), table[rows[s]], tol=1e-4, maxiter=maxiter)
        for f in FIELDS:
            assert same_bits(got[f][s:s + 1], one[f]), (s, splits[s], rows[s], f, got[f][s], one[f])
    return got


@pytest.mark.parametrize("spec", ["default", "0"])
def test_rows_equal_separate_searches_bit_for_bit(model, monkeypatch, spec):
    """4 integer splits x 5 rows, one start each (the same initial values: the initial simplices share chains across pairs)."""
    eng, table, start = model
    if spec == "0":
        monkeypatch.setenv("MISTI_NM_SPEC", "0")
    splits = np.tile(np.array([62.0, 63.0, 64.0, 65.0]), 5)
    rows = np.repeat(np.arange(5), 4).astype(np.int32)
    starts = np.tile(start, (splits.size, 1))
    got = check_against_separate(eng, table, starts, splits, rows)
    assert np.isfinite(got["llh"]).all()
    assert (got["speculative_iterations"] > 0) == (spec == "default")


def test_rows_with_a_fractional_split(model):
    eng, table, start = model
    splits = np.array([62.0, 62.5, 63.0, 62.5, 64.0, 63.0])
    rows = np.array([0, 0, 1, 2, 2, 4], dtype=np.int32)
    got = check_against_separate(eng, table, np.tile(start, (splits.size, 1)), splits, rows)
    assert np.isfinite(got["llh"]).all()


def test_invalid_split_and_repeated_rows(model):
    """Split 9 leaves the second band (start 10) empty: llh = -inf for that pair, its neighbours untouched; rows in a non-identity,
    repeated order."""
    eng, table, start = model
    splits = np.array([64.0, 9.0, 64.0, 63.0, 63.0, 64.0])
    rows = np.array([3, 0, 3, 1, 3, 0], dtype=np.int32)
    starts = np.tile(start, (splits.size, 1))
    starts[5] = [0.3, 0.02]
    got = check_against_separate(eng, table, starts, splits, rows, maxiter=300)
    assert got["llh"][1] == -np.inf
    assert np.isfinite(np.delete(got["llh"], 1)).all()
    assert same_bits(got["x"][0], got["x"][2]) and got["llh"][0] == got["llh"][2]       # the same pair twice


def test_rows_equal_scipy(model):
    from scipy import optimize
    eng, table, start = model
    splits = np.array([63.0, 64.5, 65.0])
    rows = np.array([2, 1, 4], dtype=np.int32)
    got = eng.nm_solve_rows(np.tile(start, (3, 1)), splits, rows, table, tol=1e-4, maxiter=1000)
    for s in range(3):
        def obj(mu):
            if (np.asarray(mu) < 0).any():
                return np.inf
            return -float(eng.evaluate([splits[s]], [list(mu)], table[rows[s]:rows[s] + 1]).llk[0, 0])
        ref = optimize.minimize(obj, start, method="Nelder-Mead", options={"xatol": 1e-4, "fatol": 1e-4, "maxiter": 1000})
        assert np.array_equal(ref.x, got["x"][s]) and -ref.fun == got["llh"][s] and ref.nit == got["nit"][s]


def test_bootstrap_profile_keeps_the_best_start_per_pair(model):
    from misti_amd.optimize import bootstrap_profile
    eng, table, start = model
    starts = np.array([start, [0.3, 0.02], start])                     # starts 0 and 2 tie: the lowest index is kept
    splits = [63.0, 64.0]
    prof = bootstrap_profile(eng, splits, table[:3], starts)
    assert prof["x"].shape == (3, 2, 2) and prof["llh"].shape == (3, 2)
    for r in range(3):
        for p in range(2):
            each = [eng.nm_solve(starts[q:q + 1], splits[p], table[r]) for q in range(3)]
            llh = [e["llh"][0] for e in each]
            q = int(np.argmax(llh))
            assert prof["start"][r, p] == q and q != 2
            assert same_bits(prof["x"][r, p], each[q]["x"][0]) and prof["llh"][r, p] == llh[q]
            assert prof["nit"][r, p] == each[q]["nit"][0] and prof["status"][r, p] == each[q]["status"][0]


def _inputs(tmp_path):
    from misti_amd import synth, io as mio
    from oracle.batch import oracle_truth_spectrum
    f1, f2, fj = (str(tmp_path / n) for n in ("g1.psmc", "g2.psmc", "bs.sfs"))
    open(f1, "w").write(synth.psmc_text(16, 1, synth.THETA_1))
    open(f2, "w").write(synth.psmc_text(17, 2, synth.THETA_2))
    inp = mio.read_psmc(f1, f2)
    jafs = oracle_truth_spectrum(inp.times, inp.lambdas, 20, [(0, 2, 20, 0.1, -1)], [], 0)
    row = synth.counts_from_spectrum(jafs, 200000)
    open(fj, "w").write(mio.format_jsfs(mio.bootstrap_table(synth.chunk_rows(row, 20), 3, random.Random(5))))
    return f1, f2, fj


def test_cli_grid_solve_lines_equal_single_model_runs(tmp_path):
    import contextlib
    import io
    from conftest import ROOT
    from misti_amd import cli
    from misti_amd.optimize import bootstrap_profile_interval
    f1, f2, fj = _inputs(tmp_path)
    units = str(tmp_path / "nounits.txt")
    common = ["-mi", "1", "2", "20", "0.1", "1", "--cpfit", "--funits", units]
    cmd = [sys.executable, "-m", "misti_amd.cli", f1, f2, fj, "20"] + common + ["--grid-st", "19", "20", "0.5", "--all-bs", "--grid-solve"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("bs_id =")]
    assert len(lines) == 4 * 3                                         # rows 0..3 (outer) x splits 19, 19.5, 20 (inner)
    pat = re.compile(r"^bs_id = (\S+) \tsplitT = (\S+) \ttime = \S+ \tmigration rates optim = \[\S+\] \tllh = (\S+)$")
    parsed = [pat.match(l) for l in lines]
    assert all(parsed), lines
    assert [(int(m.group(1)), float(m.group(2))) for m in parsed] == [(b, s) for b in range(4) for s in (19.0, 19.5, 20.0)]
    # a pair's line is the single-model command's line for the same split and row, character for character
    for bs, st in ((1, "19.5"), (2, "20"), (0, "19")):
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            rc = cli.main([f1, f2, fj, st] + common + ["-bs", str(bs)])
        assert rc == 0
        single = [l for l in out.getvalue().splitlines() if l.startswith("bs_id =")]
        assert len(single) == 1
        assert single[0] == lines[bs * 3 + [19.0, 19.5, 20.0].index(float(st))]
    # the summary is bootstrap_profile_interval of the printed table
    llh = np.array([float(m.group(3)) for m in parsed]).reshape(4, 3)
    iv = bootstrap_profile_interval(llh, [19.0, 19.5, 20.0])
    m = re.search(r"grid-solve: bs_id = 0 best splitT = (\S+) ", r.stdout)
    assert m and float(m.group(1)) == iv["data_split"]
    m = re.search(r"grid-solve: bootstrap best splitT mean = (\S+) 97.5% t-interval = \[(\S+), (\S+)\] over (\d+) replicates", r.stdout)
    assert m, r.stdout[-800:]
    assert int(m.group(4)) == iv["n_boot"] and float(m.group(1)) == iv["mean"]
    assert np.array_equal([float(m.group(2)), float(m.group(3))], iv["interval"], equal_nan=True)     # nan: every replicate chose one split
