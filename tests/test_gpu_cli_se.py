"""`--se` on the command line: the standard errors printed behind a `--grid-solve` run are those of optimize.observed_covariance at
the printed optima, and every line that is not an `se:` line is what the same command prints without the flag."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RESULT = re.compile(r"^bs_id = (\S+) \tsplitT = (\S+) \ttime = \S+ \tmigration rates optim = \[([^\]]*)\] \tllh = (\S+)$", flags=re.M)
SE = re.compile(r"^se: bs_id = (\S+) \tsplitT = (\S+) \tse = \[([^\]]*)\] \tcorr = \[(.*)\] \tcond = (\S+) (?:\tsandwich se = \[([^\]]*)\])?$", flags=re.M)


def without_clock(text):
    """The run's lines with the wall-clock figures masked (the job's start time, the timing line, the single run's runtimes)."""
    text = re.sub(r"^Job run at .*$", "Job run at *", text, flags=re.M)
    text = re.sub(r"in one search, \S+ s;", "in one search, * s;", text)
    text = re.sub(r"^(Runtime:   optimisation|           total       ) \S+$", r"\1 *", text, flags=re.M)
    return text.splitlines()


def without_se(text):
    """... and with the new lines absent: the `se:` lines and the empty line in front of the block of a --grid-solve run."""
    lines = without_clock(text)
    first = next(i for i, l in enumerate(lines) if l.startswith("se:"))
    if lines[first - 1] == "":
        del lines[first - 1]
    return [l for l in lines if not l.startswith("se:")]


def write_inputs(tmp_path):
    """tests/test_gpu_cli.py's inputs (the small synthetic grid, 200 000 sites in 5 rows) with a truth that HAS migration in both
    directions, so that the fitted rates lie inside the positive quadrant."""
    from misti_amd import synth, io as mio
    from misti_amd.engine import truth_spectrum
    f1, f2, fj = (str(tmp_path / n) for n in ("g1.psmc", "g2.psmc", "data.sfs"))
    open(f1, "w").write(synth.psmc_text(16, 1, synth.THETA_1))
    open(f2, "w").write(synth.psmc_text(17, 2, synth.THETA_2))
    inp = mio.read_psmc(f1, f2)
    jafs = truth_spectrum(inp.times, inp.lambdas, 20, [(0, 2, 20, 0.3, -1), (1, 2, 20, 0.15, -1)], [], 0)
    open(fj, "w").write(mio.format_jsfs(synth.chunk_rows(synth.counts_from_spectrum(jafs, 200000), 5)))
    return f1, f2, fj, inp


def test_grid_solve_se_prints_the_observed_standard_errors(tmp_path):
    from misti_amd import io as mio
    from misti_amd.engine import Engine
    from misti_amd.optimize import observed_covariance, sandwich_covariance, standard_errors
    from test_gpu_cli import run_cli
    f1, f2, fj, inp = write_inputs(tmp_path)
    args = [f1, f2, fj, "20", "-mi", "1", "2", "20", "0.1", "1", "-mi", "2", "2", "20", "0.05", "1", "--cpfit", "--grid-st", "19", "20",
            "--grid-solve", "--all-bs", "--funits", str(tmp_path / "x")]
    rc0, plain = run_cli(args)
    rc1, out = run_cli(args + ["--se"])
    assert rc0 == 0 and rc1 == 0
    assert "se:" not in plain and without_se(out) == without_clock(plain)
    fits, ses = RESULT.findall(out), SE.findall(out)
    se_lines = [l for l in out.splitlines() if l.startswith("se:")]
    rows = np.array(mio.read_jsfs(fj)[0], dtype=float)
    R = rows.shape[0]
    assert R == 5 and len(fits) == 2 * R and len(se_lines) == len(fits), out[-3000:]
    x = np.array([[float(v) for v in f[2].split(", ")] for f in fits])
    splits = np.array([float(f[1]) for f in fits])
    bs = np.array([int(f[0]) for f in fits], dtype=np.int32)
    assert list(bs) == [r for r in range(R) for _ in range(2)]
    assert all(l.startswith("se: bs_id = %s \tsplitT = %s \t" % (f[0], f[1])) for l, f in zip(se_lines, fits))
    bands = [(0, 2, -1, 0.1, 0), (1, 2, -1, 0.05, 1)]
    with Engine(inp.times, inp.lambdas, bands, [], n_param=2, sample_date=inp.sampleDateDiscr, cpfit=True, smooth=True) as e:
        cur = e.curvature(x, splits, bs, rows)
    assert (cur.status == 0).all()
    obs = observed_covariance(cur.hess)
    print("fits", x, "eigenvalues of -H", obs["eigenvalues"])
    assert obs["ok"][:2].all(), "the data row's fits are maxima"
    want = standard_errors(obs["cov"])
    want_sand = standard_errors(sandwich_covariance(cur.hess, cur.dlog, rows))
    for p, l in enumerate(se_lines):
        if not obs["ok"][p]:                                             # (a bootstrap row whose fit is no maximum says so)
            assert "not positive definite" in l, l
            continue
        s = SE.match(l)
        assert s, l
        s = s.groups()
        assert [float(v) for v in s[2].split(", ")] == list(want[p]), (p, s[2], want[p])
        assert [float(v) for v in s[5].split(", ")] == list(want_sand[p]), (p, s[5], want_sand[p])
        assert float(s[4]) == float("%.6g" % obs["cond"][p])
    # another step: other figures, the same lines around them
    rc2, out2 = run_cli(args + ["--se", "--se-step", "2e-2"])
    assert rc2 == 0 and without_se(out2) == without_clock(plain) and SE.findall(out2) != ses and len(SE.findall(out2)) >= 2


def test_single_model_se(tmp_path):
    from test_gpu_cli import run_cli
    f1, f2, fj, inp = write_inputs(tmp_path)
    args = [f1, f2, fj, "20", "-mi", "1", "2", "20", "0.2", "1", "--cpfit", "-bs", "0", "--funits", str(tmp_path / "x")]
    from misti_amd.engine import MigrationInference

    def run(a):
        # (the Report lines count the calls of the PROCESS: both runs start from zero, as two processes would)
        MigrationInference.COUNT_LLH = MigrationInference.CORRECTION_CALLED = MigrationInference.CORRECTION_FAILED = 0
        return run_cli(a)
    rc0, plain = run(args)
    rc1, out = run(args + ["--se"])
    assert rc0 == 0 and rc1 == 0 and "se:" not in plain
    assert without_se(out) == without_clock(plain)
    ses = SE.findall(out)
    assert len(ses) == 1 and ses[0][:2] == ("0", "20.0") and float(ses[0][2]) > 0 and float(ses[0][5]) > 0, out[-2000:]
