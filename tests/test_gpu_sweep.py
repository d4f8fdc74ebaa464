"""Per-start band bounds in the batched Nelder-Mead (misti_nm_solve_bounds, optimize.sweep_profile) and named sweeps on the command
line (`--sweep`, the reference's GNU-parallel recipe as one command).  The model and bootstrap table are built as in
test_gpu_bs_profile.py: config 3's model with its band ends following the split, a bootstrap table as workloads.config4 builds one.
Every start must be exactly the separate search misti_nm_solve runs on an engine whose bands carry that start's bounds."""
import contextlib
import io
import random
import re

import numpy as np
import pytest

from conftest import load_golden
from parity import internal_of, llk_bound, spread_of

pytestmark = pytest.mark.gpu

FIELDS = ("x", "llh", "nit", "nfev", "status")
# band bounds of config 3's two optimised bands (starts 4 and 10, ends following the split): the model's own and three boundaries
BOUNDS = [[[4, -1], [10, -1]], [[6, -1], [10, -1]], [[4, -1], [16, -1]], [[4, 40], [10, -1]]]


@pytest.fixture(scope="module")
def model():
    from misti_amd import io as mio, synth, workloads
    from misti_amd.engine import Engine, truth_spectrum
    w = workloads.config3(lambda *a: truth_spectrum(*a), n_start=4)
    bands = [(p, s, -1, v, k) for p, s, e, v, k in w.bands]
    table = np.array(mio.bootstrap_table(synth.chunk_rows(w.jsfs[0], 20), 4, random.Random(3)), dtype=np.float64)
    kw = w.engine_kwargs()
    kw["bands"] = bands
    engines = {}

    def engine_with(bounds=None):
        """An engine whose bands carry these bounds (None: the model's), one per bound set."""
        key = None if bounds is None else tuple(map(tuple, np.asarray(bounds).tolist()))
        if key not in engines:
            k2 = dict(kw)
            if key is not None:
                k2["bands"] = [(p, s, e, v, q) for (p, _, _, v, q), (s, e) in zip(bands, key)]
            engines[key] = Engine(w.times, w.lh, **k2)
        return engines[key]

    start = np.array([b[3] for b in bands])
    yield engine_with, table, start
    for e in engines.values():
        e.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_against_separate(engine_with, table, starts, splits, rows, bounds, maxiter=1000, skip=()):
    got = engine_with().nm_solve_bounds(starts, splits, rows, table, bounds, tol=1e-4, maxiter=maxiter)
    for s in range(len(splits)):
        if s in skip:
            continue
        one = engine_with(bounds[s]).nm_solve(starts[s:s + 1], float(splits[s]), table[rows[s]], tol=1e-4, maxiter=maxiter)
        for f in FIELDS:
            assert same_bits(got[f][s:s + 1], one[f]), (s, splits[s], rows[s], bounds[s], f, got[f][s], one[f])
    return got


@pytest.mark.parametrize("spec", ["default", "0"])
def test_bounds_equal_separate_searches_bit_for_bit(model, monkeypatch, spec):
    """3 integer splits x 4 bound sets x 2 rows, one start each: equal bounds and initial values share chains, different bounds
    never do."""
    engine_with, table, start = model
    if spec == "0":
        monkeypatch.setenv("MISTI_NM_SPEC", "0")
    sp, bd, rw = np.meshgrid([63.0, 64.0, 65.0], np.arange(len(BOUNDS)), [0, 3], indexing="ij")
    splits, rows = sp.ravel(), rw.ravel().astype(np.int32)
    bounds = np.array(BOUNDS, dtype=np.int32)[bd.ravel()]
    got = check_against_separate(engine_with, table, np.tile(start, (splits.size, 1)), splits, rows, bounds)
    assert np.isfinite(got["llh"]).all()
    assert (got["speculative_iterations"] > 0) == (spec == "default")
    # the boundary changes the answer: the same split and row under different bounds are different searches
    assert len({float(v) for v in got["llh"][(splits == 64.0) & (rows == 0)]}) == len(BOUNDS)


def test_fractional_splits_repeated_rows_and_an_invalid_bound(model):
    """Start 2's first band ends (8) before it starts (12), which SetModel refuses: llh = -inf, its neighbours untouched."""
    engine_with, table, start = model
    splits = np.array([62.5, 64.0, 64.0, 63.0, 62.5, 64.0, 63.5])
    rows = np.array([1, 3, 3, 0, 1, 3, 4], dtype=np.int32)
    bounds = np.array([BOUNDS[1], BOUNDS[2], [[12, 8], [10, -1]], BOUNDS[3], BOUNDS[1], BOUNDS[2], BOUNDS[0]], dtype=np.int32)
    starts = np.tile(start, (splits.size, 1))
    starts[6] = [0.3, 0.02]
    got = check_against_separate(engine_with, table, starts, splits, rows, bounds, maxiter=300, skip=(2,))
    assert got["llh"][2] == -np.inf
    assert np.isfinite(np.delete(got["llh"], 2)).all()
    assert same_bits(got["x"][1], got["x"][5]) and got["llh"][1] == got["llh"][5]        # the same (split, row, bounds) twice
    assert same_bits(got["x"][0], got["x"][4]) and got["llh"][0] == got["llh"][4]


def test_no_bounds_is_nm_solve_rows(model):
    engine_with, table, start = model
    eng = engine_with()
    splits = np.array([62.0, 63.5, 64.0, 9.0, 65.0])
    rows = np.array([0, 2, 4, 1, 2], dtype=np.int32)
    starts = np.tile(start, (splits.size, 1))
    a = eng.nm_solve_bounds(starts, splits, rows, table, None, maxiter=300)
    b = eng.nm_solve_rows(starts, splits, rows, table, maxiter=300)
    for f in FIELDS + ("iterations_issued", "slots", "speculative_iterations"):
        assert same_bits(a[f], b[f]) if isinstance(a[f], np.ndarray) else a[f] == b[f], f


def test_bounds_entry_point_rejects_its_arguments(model):
    """misti_nm_solve_bounds on a real context: every argument is checked before the device is touched, a rejected call leaves the
    context as it was."""
    import ctypes as C
    from misti_amd import _lib
    engine_with, table, start = model
    eng = engine_with()
    one = np.array(BOUNDS[1:2], dtype=np.int32)
    for kw, why in ((dict(rows=[5]), "rows[0] = 5 is outside the table"), (dict(split_times=[np.nan]), "split_times[0] is not finite"),
                    (dict(maxiter=0), "maxiter must be >= 1"), (dict(jsfs=np.zeros((0, 8))), "n_rep must be >= 1")):
        args = dict(starts=start[None], split_times=[64.0], rows=[0], jsfs=table, band_bounds=one)
        args.update(kw)
        with pytest.raises(_lib.MistiError, match=re.escape(why)):
            eng.nm_solve_bounds(**args)
    lib = _lib.load()
    d = (C.c_double * 16)()
    i = (C.c_int32 * 8)()
    assert lib.misti_nm_solve_bounds(eng._ctx, -1, d, d, i, i, 1, d, 1e-4, 1e-4, 10, d, d, None, None, None) == -1
    assert b"negative number of starts" in lib.misti_last_error()
    assert lib.misti_nm_solve_bounds(eng._ctx, 1, d, d, i, i, 1, None, 1e-4, 1e-4, 10, d, d, None, None, None) == -1
    assert b"is NULL" in lib.misti_last_error()
    check_against_separate(engine_with, table, start[None], np.array([64.0]), np.array([2], dtype=np.int32), one, maxiter=300)


def test_bounds_equal_scipy(model):
    from scipy import optimize
    engine_with, table, start = model
    eng = engine_with()
    splits = np.array([63.0, 64.5, 65.0])
    rows = np.array([2, 1, 4], dtype=np.int32)
    bounds = np.array([BOUNDS[1], BOUNDS[3], BOUNDS[2]], dtype=np.int32)
    got = eng.nm_solve_bounds(np.tile(start, (3, 1)), splits, rows, table, bounds, tol=1e-4, maxiter=1000)
    for s in range(3):
        def obj(mu):
            if (np.asarray(mu) < 0).any():
                return np.inf
            return -float(eng.evaluate([splits[s]], [list(mu)], table[rows[s]:rows[s] + 1], band_bounds=bounds[s:s + 1]).llk[0, 0])
        ref = optimize.minimize(obj, start, method="Nelder-Mead", options={"xatol": 1e-4, "fatol": 1e-4, "maxiter": 1000})
        assert np.array_equal(ref.x, got["x"][s]) and -ref.fun == got["llh"][s] and ref.nit == got["nit"][s]


def test_sweep_profile_keeps_the_best_start_per_pair(model):
    from misti_amd.optimize import sweep_profile
    engine_with, table, start = model
    starts = np.array([start, [0.3, 0.02], start])                     # starts 0 and 2 tie: the lowest index is kept
    models = [(63.0, BOUNDS[1]), (64.0, BOUNDS[2]), (64.0, BOUNDS[0])]
    prof = sweep_profile(engine_with(), models, table[:2], starts)
    assert prof["x"].shape == (2, 3, 2) and prof["llh"].shape == (2, 3)
    for r in range(2):
        for m, (st, bb) in enumerate(models):
            each = [engine_with(bb).nm_solve(starts[q:q + 1], st, table[r]) for q in range(3)]
            llh = [e["llh"][0] for e in each]
            q = int(np.argmax(llh))
            assert prof["start"][r, m] == q and q != 2
            assert same_bits(prof["x"][r, m], each[q]["x"][0]) and prof["llh"][r, m] == llh[q]
            assert prof["nit"][r, m] == each[q]["nit"][0] and prof["status"][r, m] == each[q]["status"][0]


SWEEP = load_golden("golden_sweep")


@pytest.mark.parametrize("cpfit", [True, False], ids=["cpfit", "default"])
def test_recipe_command_line_against_golden_sweep(cpfit):
    """Every case of golden_sweep.json (one reference run per grid point of the recipe): its model, obtained by expanding the
    recipe's command line, evaluates inside the parity contract."""
    from misti_amd import cli
    from misti_amd.engine import Engine
    from misti_amd.sweep import expand, sweep_error
    cases = [c for c in SWEEP if bool(c["in"]["kw"].get("cpfit")) == cpfit]
    sts = sorted({c["sweep"]["st"] for c in cases})
    mcs = sorted({c["sweep"]["mc"] for c in cases})
    n_value = 0
    for rates in sorted({tuple(c["sweep"]["rates"]) for c in cases}):
        line = ("{st} -mi 1 0 {mc} {mi1} 0 -mi 2 0 {mc} {mi2} 0 -mi 1 {mc} {st} {mi3} 0 -mi 2 {mc} {st} {mi4} 0 --sweep st %s --sweep mc %s"
                % (" ".join("%g" % v for v in sts), " ".join(str(v) for v in mcs)))
        line += "".join(" --sweep mi%d %r" % (i + 1, v) for i, v in enumerate(rates))
        a = cli.build_parser().parse_args(["g1.psmc", "g2.psmc", "sim.jafs"] + line.split())
        assert sweep_error(a) is None
        plan = expand(a)
        assert plan.n_model == len(sts) * len(mcs)
        mine = [c for c in cases if tuple(c["sweep"]["rates"]) == rates]
        idx = [plan.assign.index({"st": "%g" % c["sweep"]["st"], "mc": str(c["sweep"]["mc"]), **{"mi%d" % (i + 1): repr(v) for i, v in enumerate(rates)}})
               for c in mine]
        for c, m in zip(mine, idx):                                       # the expansion is the reference run's model
            assert plan.split[m] == c["in"]["split"] and list(plan.params[m]) == list(rates)
            ends = [int(np.ceil(plan.split[m])) if e == -1 else e for e in plan.bounds[m, :, 1]]
            assert [[s, e] for s, e in zip(plan.bounds[m, :, 0], ends)] == [el[1:3] for el in c["in"]["mi"]]
        i, kw = mine[0]["in"], mine[0]["in"]["kw"]
        with Engine(i["times"], i["lambdas"], plan.engine_bands(0), [], n_param=plan.n_param, cpfit=bool(kw.get("cpfit")),
                    smooth=bool(kw.get("smooth")), unfolded=bool(kw.get("unfolded"))) as e:
            r = e.evaluate(plan.split[idx], plan.params[idx], [i["sfs"]], band_bounds=plan.bounds[idx])
        for k, c in enumerate(mine):
            o = c["out"]
            if o["llh"] is None:
                assert r.status[k] == 2 or o["pert_finite"] > 0, (c["name"], r.status[k])
                continue
            if r.status[k] != 0:
                assert o["pert_fail"] > 0 or o.get("internal_fail", 0) > 0, (c["name"], r.status[k])
                continue
            n_value += 1
            bound, clause = llk_bound(o["llh"], c["in"]["sfs"], o["JAFS"], True, spread_of(o), internal_of(o))
            assert abs(r.llk[k, 0] - o["llh"]) <= bound, (c["name"], r.llk[k, 0], o["llh"], bound, clause)
    assert n_value >= 16


def _inputs(tmp_path):
    from misti_amd import synth, io as mio
    from oracle.batch import oracle_truth_spectrum
    f1, f2, fj = (str(tmp_path / n) for n in ("g1.psmc", "g2.psmc", "bs.sfs"))
    open(f1, "w").write(synth.psmc_text(16, 1, synth.THETA_1))
    open(f2, "w").write(synth.psmc_text(17, 2, synth.THETA_2))
    inp = mio.read_psmc(f1, f2)
    jafs = oracle_truth_spectrum(inp.times, inp.lambdas, 20, [(0, 2, 8, 0.1, -1), (0, 8, 20, 0.05, -1)], [], 0)
    row = synth.counts_from_spectrum(jafs, 200000)
    open(fj, "w").write(mio.format_jsfs(mio.bootstrap_table(synth.chunk_rows(row, 20), 3, random.Random(5))))
    return f1, f2, fj


def run_cli(args):
    from misti_amd import cli
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc = cli.main(args)
    assert rc == 0
    return out.getvalue()


def result_lines(text):
    return [l for l in text.splitlines() if l.startswith("bs_id =")]


def test_cli_fixed_rate_sweep_lines_equal_single_runs(tmp_path):
    """st x mc x one fixed rate in one evaluation: one line per valid model, each the single run's line character for character.
    mc = 19 with st = 19 leaves the band [mc, st) empty: the reference exits there, no line."""
    f1, f2, fj = _inputs(tmp_path)
    common = ["--cpfit", "-uf", "--funits", str(tmp_path / "nounits.txt")]
    sts, mcs, rs = ["19", "20", "20.5"], ["5", "8", "19"], ["0.05", "0.2"]
    text = run_cli([f1, f2, fj, "{st}", "-mi", "1", "2", "{mc}", "0.1", "0", "-mi", "1", "{mc}", "{st}", "{r}", "0",
                    "--sweep", "st"] + sts + ["--sweep", "mc"] + mcs + ["--sweep", "r"] + rs + common)
    lines = result_lines(text)
    valid = [(st, mc, r) for st in sts for mc in mcs for r in rs if not (st == "19" and mc == "19")]
    assert len(lines) == len(valid) == 16
    assert re.search(r"sweep: 18 models x 1 rows in one evaluation, \S+ s; 2 models skipped", text), text[-600:]
    for k in (0, 5, 9, 15):
        st, mc, r = valid[k]
        end = str(int(np.ceil(float(st))))
        single = result_lines(run_cli([f1, f2, fj, st, "-mi", "1", "2", mc, "0.1", "0", "-mi", "1", mc, end, r, "0"] + common))
        assert single == [lines[k]], (valid[k], single, lines[k])


def test_cli_grid_solve_sweep_lines_equal_single_runs(tmp_path):
    from misti_amd.optimize import sweep_interval
    f1, f2, fj = _inputs(tmp_path)
    common = ["--cpfit", "-uf", "--funits", str(tmp_path / "nounits.txt")]
    text = run_cli([f1, f2, fj, "{st}", "-mi", "1", "2", "{mc}", "0.1", "1", "-mi", "1", "{mc}", "{st}", "0.05", "1",
                    "--sweep", "st", "19", "20", "--sweep", "mc", "4", "8", "--grid-solve", "--all-bs"] + common)
    lines = result_lines(text)
    models = [(st, mc) for st in ("19", "20") for mc in ("4", "8")]
    assert len(lines) == 4 * len(models)                               # rows 0..3 (outer) x models
    pat = re.compile(r"^bs_id = (\S+) \tsplitT = (\S+) \ttime = \S+ \tmigration rates optim = \[\S+, \S+\] \tllh = (\S+)$")
    parsed = [pat.match(l) for l in lines]
    assert all(parsed), lines
    assert [(int(m.group(1)), float(m.group(2))) for m in parsed] == [(b, float(st)) for b in range(4) for st, _ in models]
    for bs, m in ((0, 3), (2, 0), (3, 1)):
        st, mc = models[m]
        single = result_lines(run_cli([f1, f2, fj, st, "-mi", "1", "2", mc, "0.1", "1", "-mi", "1", mc, st, "0.05", "1", "-bs", str(bs)] + common))
        assert single == [lines[bs * len(models) + m]], (bs, models[m])
    # the summary is sweep_interval of the printed table
    llh = np.array([float(m.group(3)) for m in parsed]).reshape(4, len(models))
    iv = sweep_interval(llh, np.array([[float(st), float(mc)] for st, mc in models]))
    m = re.search(r"sweep: bs_id = 0 best model st = (\S+) mc = (\S+) optim", text)
    assert m and (m.group(1), m.group(2)) == models[iv["data_model"]]
    for name, v in zip(("st", "mc"), iv["variables"]):
        m = re.search(r"sweep: %s bootstrap mean = (\S+) 97.5%% t-interval = \[(\S+), (\S+)\] over (\d+) replicates" % name, text)
        assert m, text[-800:]
        assert int(m.group(4)) == v["n_boot"] and float(m.group(1)) == v["mean"]
        assert np.array_equal([float(m.group(2)), float(m.group(3))], v["interval"], equal_nan=True)
