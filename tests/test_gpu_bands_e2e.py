"""Trajectory bands end to end: Engine.trajectory_bands (misti_traj_bands: points on the host, the rates kept on the device) against
evaluate(want_lc=True) on the same points followed by optimize.trajectory_bands_rule, bit for bit, and against itself at other engine
batches and workspace bounds.  The model is the two-rate migration fixture of the sampler tests (tests/test_gpu_ens.py: its grid has
numT = 16 intervals, not the 20 the issue's text gives it): 2 groups x 65 points around its fit, fractional and whole splits mixed.
The CPU oracle says - without a GPU - that every point is valid, so the band test cannot pass on an empty set.  Then the command line:
`--bands` over a 1 + 8-row bootstrap table and `--mcmc-bands` (one fit; a ladder of two rungs; a log-scale coordinate) on the numT = 20
fixture of the other command-line tests, each against the rule on rates the test evaluates itself."""
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

G, M = 2, 65
PROBS = (0.025, 0.5, 0.975, 1.0 / 3.0)
BANDS = [(0, 2, -1, 0.2, 0), (1, 2, -1, 0.1, 1)]
FLAGS = dict(cpfit=True, smooth=True)
OUTPUTS = ("count", "mean", "quant", "lo", "hi")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def grid():
    from misti_amd import synth
    inp = synth.psmc_pair(8, 9)
    times, lh, _ = synth.self_consistent(inp, 11, [[1, 2, 11, 0.2, 0]], [])
    return times, lh


def points():
    """x[G M][2], split[G M]: rates around the fit (0.2, 0.1) - on the side where the lambda correction has a solution: beyond about
    (0.224, 0.09) the oracle reports that it fails -, splits in 11 ... 13, every third one whole."""
    rng = np.random.default_rng(2026)
    x = np.array([0.2, 0.1]) * rng.uniform([0.8, 0.95], [1.08, 1.3], size=(G * M, 2))
    split = rng.uniform(11.0, 13.0, size=G * M)
    split[::3] = np.floor(split[::3])
    split[1], split[2] = 11.0, 12.5                               # the smallest split, and a half
    return x, split


def test_the_oracle_accepts_every_point():
    """Not a GPU test: the condition of the band test below.  Every point is a valid candidate to the CPU oracle, and below the
    smallest split every sample is a member of every series."""
    from oracle.batch import oracle_eval
    times, lh = grid()
    x, split = points()
    assert len(lh) == 16 and split.min() == 11.0 and (split != np.floor(split)).sum() > 40 and (split == np.floor(split)).sum() > 40
    for i in range(G * M):
        assert oracle_eval(times, lh, BANDS, [], FLAGS, 0, float(split[i]), x[i], None)[2] == 0, i


@pytest.fixture(scope="module")
def two_rates():
    from misti_amd.engine import Engine
    times, lh = grid()
    e = Engine(times, lh, bands=BANDS, pulses=(), n_param=2, **FLAGS)
    yield e
    e.close()


@pytest.mark.gpu
def test_bands_equal_evaluate_and_the_rule(two_rates):
    from misti_amd.optimize import trajectory_bands_rule
    e = two_rates
    x, split = points()
    r = e.evaluate(split, x, want_lc=True)
    assert (r.status == 0).all()                                  # the condition, as the oracle says
    ref = trajectory_bands_rule(r.lc.reshape(G, M, e.numT + 1, 2), split.reshape(G, M), r.status.reshape(G, M), PROBS)
    assert (ref["count"][:, :11] == M).all() and (ref["count"][:, 13:] == 0).all() and (0 < ref["count"][:, 12]).all() and (ref["count"][:, 12] < M).all()
    dev = e.trajectory_bands(x, split, groups=G, probs=PROBS)
    for k in OUTPUTS:
        assert same_bits(dev[k], ref[k]), k
    # neither the engine's batches nor the workspace bound change a bit
    for kw in (dict(batch_limit=7), dict(batch_limit=0), dict(workspace_bytes=1), dict(batch_limit=7, workspace_bytes=1)):
        again = e.trajectory_bands(x, split, groups=G, probs=PROBS, **kw)
        for k in OUTPUTS:
            assert same_bits(again[k], dev[k]), (kw, k)
    # one output alone
    alone = e.trajectory_bands(x, split, groups=G, probs=PROBS, want=("quant",))
    assert set(alone) == {"quant", "probs"} and same_bits(alone["quant"], dev["quant"])
    # one group of all the points: another reduction of the same rates
    one = e.trajectory_bands(x, split, groups=1, probs=PROBS)
    ref1 = trajectory_bands_rule(r.lc[None], split[None], r.status[None], PROBS)
    for k in OUTPUTS:
        assert same_bits(one[k], ref1[k]), k


@pytest.mark.gpu
def test_a_failed_point_is_a_member_of_nothing(two_rates):
    """A negative rate is a soft failure of the engine: its sample leaves every series, the others stay."""
    from misti_amd.optimize import trajectory_bands_rule
    e = two_rates
    x, split = points()
    x, split = x[:M].copy(), split[:M].copy()
    x[5, 0] = -0.1
    r = e.evaluate(split, x, want_lc=True)
    assert r.status[5] != 0 and (np.delete(r.status, 5) == 0).all()
    dev = e.trajectory_bands(x, split, groups=1, probs=PROBS)
    ref = trajectory_bands_rule(r.lc[None], split[None], r.status[None], PROBS)
    for k in OUTPUTS:
        assert same_bits(dev[k], ref[k]), k
    assert (dev["count"][0, :11] == M - 1).all()


# ---- the command line ------------------------------------------------------------------------------------------------------------------------
def cli_run(tmp_path, n_boot, more, seed=5):
    """The command-line fixture of tests/test_gpu_joint.py (numT = 20, two optimised rates): runs it, returns (stdout, parsed options, inputs)."""
    from misti_amd import cli, io as mio, synth
    g = load_golden("golden_pulse_sweep")[0]["in"]
    f1, f2, fj = (str(tmp_path / n) for n in ("g1.psmc", "g2.psmc", "bs.sfs"))
    open(f1, "w").write(synth.psmc_text(16, 1, synth.THETA_1))
    open(f2, "w").write(synth.psmc_text(17, 2, synth.THETA_2))
    open(fj, "w").write(mio.format_jsfs(mio.bootstrap_table(synth.chunk_rows(g["sfs"], 20), n_boot, random.Random(seed))))
    args = [f1, f2, fj, "20", "-mi", "1", "2", "20", "0.1", "1", "-mi", "2", "2", "20", "0.1", "1", "--cpfit", "--funits", str(tmp_path / "nounits.txt"),
            "--all-bs", "--box", "0", "0.01", "1", "--box", "1", "0.01", "1"] + more
    r = subprocess.run([sys.executable, "-m", "misti_amd.cli"] + args, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    a = cli.build_parser().parse_args(args)
    inp = mio.read_psmc(f1, f2, a.sdate, a.rd, mio.Units.from_file(a.funits))
    return r.stdout, a, inp


def cli_engine(a, inp):
    from misti_amd import cli
    from misti_amd.engine import Engine
    splits, bands, pulses, k, axes = cli.grid_model(a)
    return Engine(inp.times, inp.lambdas, bands, pulses, n_param=k, sample_date=inp.sampleDateDiscr, mixture_th=a.mth, device=a.device,
                  cpfit=a.cpfit, true_eps=a.trueEPS, smooth=not a.nosmooth, unfolded=a.uf)


NUM = r"(-?(?:inf|nan|[0-9.]+(?:e[-+]?[0-9]+)?))"
POP = r"pop%d: (\d+)/(\d+) lo = " + NUM + r" q = \[([^\]]*)\] hi = " + NUM
LINE = re.compile(r"^bands: (.*) \tinterval = (\d+) \ttime = " + NUM + " \t" + POP % 1 + " \t" + POP % 2 + "$")


def parse_bands(stdout, label):
    """{interval: (count[2], m, lo[2], quant[2][P], hi[2])} of the `bands:` lines with this label; %r printed them, float() reads the bits back."""
    out = {}
    for line in stdout.splitlines():
        mt = LINE.match(line)
        if mt and mt.group(1) == label:
            v = mt.groups()
            pops = [v[3:8], v[8:13]]
            assert pops[0][1] == pops[1][1]
            out[int(v[1])] = ([int(p[0]) for p in pops], int(pops[0][1]), [float(p[2]) for p in pops],
                              [[float(t) for t in p[3].split(", ")] for p in pops], [float(p[4]) for p in pops])
    return out


def assert_lines(lines, ref, g, m):
    """The parsed lines of one group are the rule's group g: a line per interval with a member, the printed numbers the rule's bits."""
    want = [j for j in range(ref["count"].shape[1]) if ref["count"][g, j].any()]
    assert sorted(lines) == want and want
    for j in want:
        count, m_, lo, quant, hi = lines[j]
        assert m_ == m and count == ref["count"][g, j].tolist()
        for p in (0, 1):
            if count[p]:
                assert same_bits(np.array(quant[p]), ref["quant"][g, j, p]) and same_bits(np.array([lo[p], hi[p]]), np.array([ref["lo"][g, j, p], ref["hi"][g, j, p]]))


@pytest.mark.gpu
def test_cli_bootstrap_band(tmp_path):
    """`--all-bs --fit-st --bands 0.1 0.5 0.9 --bands-out` on a 1 + 8-row table: the `bands:` lines and the npz equal the rule on the
    re-evaluated rates of the fits the npz carries (rows 1 ... 8: the samples; row 0: the point estimate, reported beside)."""
    from misti_amd.optimize import trajectory_bands_rule
    fo = str(tmp_path / "bands.npz")
    stdout, a, inp = cli_run(tmp_path, 8, ["--fit-st", "--grid-st", "19", "20", "--box", "st", "18", "20.5", "--bands", "0.1", "0.5", "0.9", "--bands-out", fo])
    out = np.load(fo)
    x, split = out["x"], out["split"]
    assert x.shape == (9, 2) and split.shape == (9,) and out["probs"].tolist() == [0.1, 0.5, 0.9] and (split > 0).all()
    # the fits the npz carries are the printed ones
    printed = [float(v) for v in re.findall(r"^bs_id = \d+ \tsplitT = (\S+)", stdout, flags=re.M)]
    assert len(printed) == 9 and np.allclose(printed, split, rtol=1e-12)
    with cli_engine(a, inp) as e:
        r = e.evaluate(split, x, want_lc=True)
    ref = trajectory_bands_rule(r.lc[None, 1:], split[None, 1:], r.status[None, 1:], (0.1, 0.5, 0.9))
    for k in OUTPUTS:
        assert same_bits(out[k], ref[k][0]), k
    assert (r.status == 0).all() and (ref["count"][0, :18] == 8).all()
    assert_lines(parse_bands(stdout, "bootstrap"), ref, 0, 8)
    # row 0, the point estimate: its own rates below its split
    point = [l for l in stdout.splitlines() if l.startswith("bands: point")]
    below = int(np.ceil(split[0]))
    assert len(point) == below and same_bits(out["point"][:below], r.lc[0, :below]) and np.isnan(out["point"][below:]).all()
    assert "interval = 0 \ttime = 0.0 \tpop1: %r \tpop2: %r" % (float(r.lc[0, 0, 0]), float(r.lc[0, 0, 1])) in point[0]


@pytest.mark.gpu
@pytest.mark.parametrize("more, fitted", [([], True), (["--mcmc-ladder", "2", "4"], True), (["--mcmc-log", "0"], False)], ids=["one-fit", "ladder", "log"])
def test_cli_mcmc_bands(tmp_path, more, fitted):
    """`--mcmc 4 12 --mcmc-bands`: the `bands:` lines of every fit equal the rule on the chain `--mcmc-out` wrote in the same run - its kept
    samples behind the burn-in, in natural units, pushed through evaluate.  With --fit-st the split is the chain's last coordinate."""
    from misti_amd.optimize import from_sampling, trajectory_bands_rule
    fc = str(tmp_path / "chain.npz")
    mode = ["--fit-st", "--grid-st", "19", "20", "--box", "st", "18", "20.5"] if fitted else ["--grid-solve", "--grid-st", "19", "20"]
    stdout, a, inp = cli_run(tmp_path, 0 if fitted else 1, mode + ["--mcmc", "4", "12", "--mcmc-seed", "3", "--mcmc-out", fc, "--mcmc-bands"] + more)
    z = np.load(fc)
    chain = z["chain"][:, 6:]                                     # burn: half of the 12 kept steps
    if "prior_scale" in z:
        chain = from_sampling(chain, {k[6:]: z[k] for k in z.files if k.startswith("prior_")})
    S, n, W, N = chain.shape
    m = n * W
    assert (S, n, W) == ((1, 6, 4) if fitted else (4, 6, 4))
    pts = chain.reshape(S * m, N)
    x, split = (pts[:, :-1], pts[:, -1]) if fitted else (pts, np.repeat(z["split"], m))
    with cli_engine(a, inp) as e:
        r = e.evaluate(split, x, want_lc=True)
    ref = trajectory_bands_rule(r.lc.reshape(S, m, -1, 2), split.reshape(S, m), r.status.reshape(S, m), (0.025, 0.5, 0.975))
    labels = re.findall(r"^bands: (bs_id = \d+ \tsplitT = \S+) \tinterval = 0 ", stdout, flags=re.M)
    assert len(labels) == S and (ref["count"][:, 0] > 0).all()
    for g, label in enumerate(labels):
        assert_lines(parse_bands(stdout, label), ref, g, m)
