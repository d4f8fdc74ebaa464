"""Per-candidate pulse times (misti_eval_batch_pulses, misti_nm_solve_pulses, `--sweep-pu`): the pulse-date grid of
golden_pulse_sweep.json (one reference run per (fit, st, t, f) point; tests/golden/make_pulse_sweep.py) in ONE call per fit, and
bit identity with the only way there was before: one Engine per distinct pulse-time set, with the times in its model."""
import contextlib
import ctypes as C
import io
import random
import re

import numpy as np
import pytest

from conftest import load_golden
from parity import internal_of, llk_bound, spread_of

pytestmark = pytest.mark.gpu

PULSES = load_golden("golden_pulse_sweep")
GRID = PULSES[0]["in"]
FIELDS = ("x", "llh", "nit", "nfev", "status")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def make_engine(times, cpfit=True, sample_date=0, n_param=2):
    """One band following the split (rate: parameter 0, or fixed 0.2) and one pulse per entry of ``times``: the first fixed at
    0.05 out of population 1, the others out of population 2 with parameter 1 (n_param = 2) or parameter 0 (n_param = 1)."""
    from misti_amd.engine import Engine
    bands = [(0, max(4, sample_date), -1, 0.2, 0 if n_param == 2 else -1)]
    pulses = [(0, int(times[0]), 0.05, -1)] + [(1, int(t), 0.0, n_param - 1) for t in times[1:]]
    return Engine(GRID["times"], GRID["lambdas"], bands, pulses, n_param=n_param, cpfit=cpfit, smooth=True, unfolded=True, sample_date=sample_date)


# ---- 1. the reference's grid in one call per fit --------------------------------------------------------------------------------
def grid_in_one_call(cpfit):
    """The fixture's cases of one fit in ONE evaluate call; returns how many values were compared under the contract."""
    cases = [c for c in PULSES if bool(c["in"]["kw"].get("cpfit")) == cpfit]
    split = np.array([c["sweep"]["st"] for c in cases], dtype=float)
    params = np.array([[c["sweep"]["fractions"][1]] for c in cases], dtype=float)
    times = np.array([c["sweep"]["pulse_times"] for c in cases], dtype=np.int32)
    for c in cases:                                                  # the batch is the reference run's model
        assert c["in"]["mi"] == [[1, 4, int(np.ceil(c["sweep"]["st"])), 0.2, 0]]
        assert c["in"]["pu"] == [[1, 10, 0.05, 0], [2, c["sweep"]["pulse_times"][1], c["sweep"]["fractions"][1], 0]]
    with make_engine([10, 5], cpfit=cpfit, n_param=1) as e:
        r = e.evaluate(split, params, [GRID["sfs"]], pulse_times=times)
    n_value = 0
    for k, c in enumerate(cases):
        o = c["out"]
        if o["llh"] is None:
            assert r.status[k] == 2 or o["pert_finite"] > 0, (c["name"], r.status[k])
            continue
        if r.status[k] != 0:
            assert o["pert_fail"] > 0 or o.get("internal_fail", 0) > 0, (c["name"], r.status[k])
            continue
        n_value += 1
        bound, clause = llk_bound(o["llh"], c["in"]["sfs"], o["JAFS"], True, spread_of(o), internal_of(o))
        print(c["name"], r.llk[k, 0], o["llh"], abs(r.llk[k, 0] - o["llh"]), bound, clause)
        assert abs(r.llk[k, 0] - o["llh"]) <= bound, (c["name"], r.llk[k, 0], o["llh"], bound, clause)
    return n_value


def test_reference_grid_in_one_call_per_fit():
    """Every case under the per-candidate contract of tests/parity.py, and at least 24 values compared in all (8 per fit): the
    fixture's own conditions, so the test cannot pass on failures alone."""
    n = {cpfit: grid_in_one_call(cpfit) for cpfit in (True, False)}
    assert min(n.values()) >= 8 and sum(n.values()) >= 24, n


# ---- 2. bit identity with one Engine per pulse-time set --------------------------------------------------------------------------
TIME_SETS = [[10, 3], [10, 7], [5, 12], [10, 20], [10, 25], [16, 15], [2, 31]]


@pytest.mark.parametrize("cpfit, sample_date", [(True, 0), (False, 0), (True, 2)], ids=["cpfit", "default", "ancient"])
def test_equal_to_one_engine_per_time_set(cpfit, sample_date):
    """Two pulses per candidate, integer and fractional splits, times below, at and beyond the split (20 is the shortened interval
    of the split 20.5 and the split index of 20; 25 and 31 are never applied)."""
    sp, ts, pr = np.meshgrid([20.0, 20.5, 18.0], np.arange(len(TIME_SETS)), [0, 1], indexing="ij")
    split = sp.ravel()
    times = np.array(TIME_SETS, dtype=np.int32)[ts.ravel()]
    params = np.array([[0.2, 0.1], [0.15, 0.35]])[pr.ravel()]
    row = [GRID["sfs"]]
    with make_engine(TIME_SETS[0], cpfit, sample_date) as e:
        r = e.evaluate(split, params, row, want_lc=True, want_pr=True, pulse_times=times)
    ok = r.status == 0                      # (a correction that fails is a result like any other: it has to fail in both)
    assert ok[pr.ravel() == 0].all() and ok.sum() >= 0.75 * ok.size and np.isfinite(r.llk[ok]).all(), r.status
    assert len({float(v) for v in r.llk[:, 0]}) > len(TIME_SETS)
    for k, tset in enumerate(TIME_SETS):
        sel = np.where(ts.ravel() == k)[0]
        with make_engine(tset, cpfit, sample_date) as e:
            q = e.evaluate(split[sel], params[sel], row, want_lc=True, want_pr=True)
        for name in ("llk", "jafs", "lc", "pr", "status"):
            assert same_bits(getattr(q, name), getattr(r, name)[sel]), (tset, name)
    # a time at or beyond the split index is never applied: 25 and 20 at the integer split 20 are the same model ...
    at = lambda st, k, p: np.where((split == st) & (ts.ravel() == k) & (pr.ravel() == p))[0][0]
    assert r.llk[at(20.0, 3, 0), 0] == r.llk[at(20.0, 4, 0), 0]
    # ... and 20 IS applied in the shortened interval of the split 20.5
    assert r.llk[at(20.5, 3, 0), 0] != r.llk[at(20.5, 4, 0), 0]


# ---- 3. order, chain sharing, NULL ---------------------------------------------------------------------------------------------
def test_shuffle_distinct_times_and_null():
    from misti_amd import _lib
    rng = np.random.default_rng(11)
    n = 48
    split = rng.choice([19.0, 20.0, 20.5], size=n)
    times = np.array(TIME_SETS, dtype=np.int32)[rng.integers(0, len(TIME_SETS), size=n)]
    params = np.array([[0.2, 0.1], [0.15, 0.35]])[rng.integers(0, 2, size=n)]
    row = [GRID["sfs"]]
    with make_engine(TIME_SETS[0]) as e:
        r = e.evaluate(split, params, row, want_lc=True, pulse_times=times)
        perm = rng.permutation(n)
        r2 = e.evaluate(split[perm], params[perm], row, want_lc=True, pulse_times=times[perm])
        for name in ("llk", "jafs", "lc", "status"):
            assert same_bits(getattr(r2, name), getattr(r, name)[perm]), name
        # candidates that differ ONLY in a pulse time never share a chain: all different likelihoods
        m = 12
        t = np.stack([np.full(m, 15), np.arange(2, 2 + m)], 1).astype(np.int32)
        d = e.evaluate(np.full(m, 20.0), np.tile([0.2, 0.1], (m, 1)), row, pulse_times=t)
        assert (d.status == 0).all() and len({float(v) for v in d.llk[:, 0]}) == m
        # the model's own times, given per candidate, are the model: the bits of pulse_times=None
        own = e.evaluate(split, params, row, want_lc=True, want_pr=True, pulse_times=np.tile(TIME_SETS[0], (n, 1)))
        none = e.evaluate(split, params, row, want_lc=True, want_pr=True, pulse_times=None)
        plain = e.evaluate(split, params, row, want_lc=True, want_pr=True)
        for name in ("llk", "jafs", "lc", "pr", "status"):
            assert same_bits(getattr(own, name), getattr(none, name)), name
            assert same_bits(getattr(none, name), getattr(plain, name)), name
        # ... and NULL through the new entry point itself is misti_eval_batch
        s64, p64, rows = np.ascontiguousarray(split), np.ascontiguousarray(params), np.array(row, dtype=float)
        llk, jafs, status = np.empty((n, 1)), np.empty((n, 7)), np.empty(n, dtype=np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(e._lib.misti_eval_batch_pulses(e._ctx, n, ptr(s64), ptr(p64), None, None, 1, ptr(rows), ptr(llk), ptr(jafs), None, None, ptr(status)))
        assert same_bits(llk, plain.llk) and same_bits(jafs, plain.jafs) and same_bits(status, plain.status)


def test_device_buffer_form():
    import torch
    n = 6
    split = np.array([20.0, 20.5, 19.0, 20.0, 20.5, 19.0])
    times = np.array(TIME_SETS[:n], dtype=np.int32)
    params = np.tile([0.2, 0.1], (n, 1))
    with make_engine(TIME_SETS[0]) as e:
        want = e.evaluate(split, params, [GRID["sfs"]], pulse_times=times)
        dev = torch.device("cuda", e.device)
        d_split, d_par, d_rows = (torch.as_tensor(np.asarray(a, dtype=float), device=dev).contiguous() for a in (split, params, [GRID["sfs"]]))
        d_times = torch.as_tensor(times, device=dev).contiguous()
        d_llk = torch.empty((n, 1), dtype=torch.float64, device=dev)
        d_status = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        e.evaluate_dev(n, d_split.data_ptr(), d_par.data_ptr(), 1, d_rows.data_ptr(), d_llk.data_ptr(), d_status=d_status.data_ptr(),
                       d_pulse_times=d_times.data_ptr())
        e.sync()
        assert same_bits(d_llk.cpu().numpy(), want.llk) and same_bits(d_status.cpu().numpy(), want.status)


# ---- 4. invalid times -------------------------------------------------------------------------------------------------------------
def test_invalid_times_get_status_4_and_leave_the_neighbours_alone():
    from misti_amd import _lib
    numT = len(GRID["lambdas"])
    good = [[5, 3], [5, 7], [5, 12], [5, 16]]
    bad = [[5, 1], [7, 7], [5, numT + 1], [-1, 7], [5, 40]]           # below the sample date (2), two equal, beyond the grid, negative
    times = np.array([good[0], bad[0], good[1], bad[1], bad[2], good[2], bad[3], good[3], bad[4]], dtype=np.int32)
    is_bad = np.array([0, 1, 0, 1, 1, 0, 1, 0, 1], dtype=bool)
    n = len(times)
    split = np.full(n, 20.0)
    params = np.tile([0.2, 0.1], (n, 1))
    row = [GRID["sfs"]]
    with make_engine(good[0], sample_date=2) as e:
        r = e.evaluate(split, params, row, want_lc=True, pulse_times=times)
        alone = e.evaluate(split[~is_bad], params[~is_bad], row, want_lc=True, pulse_times=times[~is_bad])
    assert (r.status[is_bad] == 4).all() and (r.llk[is_bad, 0] == -np.inf).all()
    assert (r.status[~is_bad] == 0).all() and np.isfinite(r.llk[~is_bad]).all()
    for name in ("llk", "jafs", "lc", "status"):
        assert same_bits(getattr(r, name)[~is_bad], getattr(alone, name)), name
    # status 4 exactly where misti_create refuses the model
    for t in bad:
        with pytest.raises(_lib.MistiError):
            make_engine(t, sample_date=2)
    # the last index misti_create accepts (numT: valid, never applied) is accepted per candidate too
    with make_engine([5, numT], sample_date=2) as e:
        q = e.evaluate([20.0], [[0.2, 0.1]], row)
    with make_engine(good[0], sample_date=2) as e:
        p = e.evaluate([20.0], [[0.2, 0.1]], row, pulse_times=[[5, numT]])
    assert q.status[0] == 0 and same_bits(p.llk, q.llk)


# ---- 5. the batched search ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def search():
    from misti_amd import io as mio, synth
    table = np.array(mio.bootstrap_table(synth.chunk_rows(GRID["sfs"], 20), 3, random.Random(3)), dtype=np.float64)
    engines = {}

    def engine_with(times):
        key = tuple(int(t) for t in times)
        if key not in engines:
            engines[key] = make_engine(key)
        return engines[key]

    yield engine_with, table, np.array([0.2, 0.1])
    for e in engines.values():
        e.close()


def check_against_separate(engine_with, table, starts, splits, rows, times, maxiter=1000, skip=()):
    got = engine_with(TIME_SETS[0]).nm_solve_pulses(starts, splits, rows, table, None, times, tol=1e-4, maxiter=maxiter)
    for s in range(len(splits)):
        if s in skip:
            continue
        one = engine_with(times[s]).nm_solve(starts[s:s + 1], float(splits[s]), table[rows[s]], tol=1e-4, maxiter=maxiter)
        for f in FIELDS:
            assert same_bits(got[f][s:s + 1], one[f]), (s, splits[s], rows[s], times[s], f, got[f][s], one[f])
    return got


@pytest.mark.parametrize("spec", ["default", "0"])
def test_search_equals_separate_searches_bit_for_bit(search, monkeypatch, spec):
    """3 splits (one fractional) x 4 time sets x 2 rows, one start each."""
    engine_with, table, start = search
    if spec == "0":
        monkeypatch.setenv("MISTI_NM_SPEC", "0")
    sp, ts, rw = np.meshgrid([20.0, 20.5, 19.0], np.arange(4), [0, 2], indexing="ij")
    splits, rows = sp.ravel(), rw.ravel().astype(np.int32)
    times = np.array(TIME_SETS, dtype=np.int32)[ts.ravel()]
    got = check_against_separate(engine_with, table, np.tile(start, (splits.size, 1)), splits, rows, times, maxiter=400)
    assert np.isfinite(got["llh"]).all()
    assert (got["speculative_iterations"] > 0) == (spec == "default")
    # the pulse date changes the answer
    assert len({float(v) for v in got["llh"][(splits == 20.0) & (rows == 0)]}) == 4


def test_search_invalid_set_and_null(search):
    engine_with, table, start = search
    eng = engine_with(TIME_SETS[0])
    splits = np.array([20.0, 20.5, 20.0, 19.0])
    rows = np.array([1, 0, 1, 3], dtype=np.int32)
    times = np.array([TIME_SETS[1], TIME_SETS[2], [9, 9], TIME_SETS[1]], dtype=np.int32)     # start 2: two pulses at one time
    starts = np.tile(start, (4, 1))
    got = check_against_separate(engine_with, table, starts, splits, rows, times, maxiter=300, skip=(2,))
    assert got["llh"][2] == -np.inf and np.isfinite(np.delete(got["llh"], 2)).all()
    bounds = np.array([[[4, -1]], [[6, -1]], [[4, 12]], [[5, -1]]], dtype=np.int32)
    a = eng.nm_solve_pulses(starts, splits, rows, table, bounds, None, maxiter=300)
    b = eng.nm_solve_bounds(starts, splits, rows, table, bounds, maxiter=300)
    for f in FIELDS + ("iterations_issued", "slots", "speculative_iterations"):
        assert same_bits(a[f], b[f]) if isinstance(a[f], np.ndarray) else a[f] == b[f], f
    # bounds and times together: the start's own model
    c = eng.nm_solve_pulses(starts[:2], splits[:2], rows[:2], table, bounds[:2], times[:2], maxiter=300)
    from misti_amd.engine import Engine
    for s in range(2):
        with Engine(GRID["times"], GRID["lambdas"], [(0, int(bounds[s, 0, 0]), -1, 0.2, 0)],
                    [(0, int(times[s, 0]), 0.05, -1), (1, int(times[s, 1]), 0.0, 1)], n_param=2, cpfit=True, smooth=True, unfolded=True) as e:
            one = e.nm_solve(starts[s:s + 1], float(splits[s]), table[rows[s]], maxiter=300)
        for f in FIELDS:
            assert same_bits(c[f][s:s + 1], one[f]), (s, f)


def test_sweep_profile_with_pulse_times(search):
    from misti_amd.optimize import sweep_profile
    engine_with, table, start = search
    starts = np.array([start, [0.3, 0.3]])
    models = [(20.0, [[4, -1]], TIME_SETS[1]), (20.5, [[4, -1]], TIME_SETS[2])]
    prof = sweep_profile(engine_with(TIME_SETS[0]), models, table[:2], starts, maxiter=300)
    assert prof["x"].shape == (2, 2, 2)
    for r in range(2):
        for m, (st, _, ts) in enumerate(models):
            each = [engine_with(ts).nm_solve(starts[q:q + 1], st, table[r], maxiter=300) for q in range(2)]
            q = int(np.argmax([e["llh"][0] for e in each]))
            assert prof["start"][r, m] == q and same_bits(prof["x"][r, m], each[q]["x"][0]) and prof["llh"][r, m] == each[q]["llh"][0]
    with pytest.raises(ValueError):
        sweep_profile(engine_with(TIME_SETS[0]), [models[0], (20.0, [[4, -1]])], table[:2], starts)


# ---- 6. the command line --------------------------------------------------------------------------------------------------------
def _inputs(tmp_path):
    from misti_amd import synth, io as mio
    from oracle.batch import oracle_truth_spectrum
    f1, f2, fj = (str(tmp_path / n) for n in ("g1.psmc", "g2.psmc", "bs.sfs"))
    open(f1, "w").write(synth.psmc_text(16, 1, synth.THETA_1))
    open(f2, "w").write(synth.psmc_text(17, 2, synth.THETA_2))
    inp = mio.read_psmc(f1, f2)
    jafs = oracle_truth_spectrum(inp.times, inp.lambdas, 20, [(0, 4, 20, 0.2, -1)], [(0, 10, 0.05, -1), (1, 12, 0.1, -1)], 0)
    row = synth.counts_from_spectrum(jafs, 200000)
    open(fj, "w").write(mio.format_jsfs(mio.bootstrap_table(synth.chunk_rows(row, 20), 3, random.Random(5))))
    return f1, f2, fj, len(inp.lambdas)


def run_cli(args):
    from misti_amd import cli
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc = cli.main(args)
    assert rc == 0
    return out.getvalue()


def result_lines(text):
    return [l for l in text.splitlines() if l.startswith("bs_id =")]


def test_cli_pulse_sweep_lines_equal_single_runs(tmp_path):
    """st x t x f in one evaluation: one line per valid model, each the single run's line character for character.  t = 99 lies
    beyond the grid and t = 10 is the fixed pulse's time: the reference exits on both, no line."""
    f1, f2, fj, numT = _inputs(tmp_path)
    assert numT < 99
    common = ["--cpfit", "-uf", "--funits", str(tmp_path / "nounits.txt")]
    sts, ts, fs = ["20", "20.5"], ["3", "10", "12", "20", "99"], ["0.1", "0.35"]
    text = run_cli([f1, f2, fj, "{st}", "-mi", "1", "4", "{st}", "0.2", "0", "-pu", "1", "10", "0.05", "0", "-pu", "2", "{t}", "{f}", "0",
                    "--sweep", "st"] + sts + ["--sweep-pu", "t"] + ts + ["--sweep-pu", "f"] + fs + common)
    lines = result_lines(text)
    valid = [(st, t, f) for st in sts for t in ts for f in fs if t not in ("10", "99")]
    assert len(lines) == len(valid) == 12
    assert re.search(r"sweep: 20 models x 1 rows in one evaluation, \S+ s; 8 models skipped", text), text[-600:]
    assert len(set(lines)) == 11                     # t = 20 at the split 20 is never applied: its two lines differ in f alone, which no line prints
    for k in (0, 3, 5, 6, 10, 11):
        st, t, f = valid[k]
        end = str(int(np.ceil(float(st))))
        single = result_lines(run_cli([f1, f2, fj, st, "-mi", "1", "4", end, "0.2", "0", "-pu", "1", "10", "0.05", "0", "-pu", "2", t, f, "0"] + common))
        assert single == [lines[k]], (valid[k], single, lines[k])
    # the summary names the best t
    llh = [float(l.split("llh = ")[1]) for l in lines]
    st, t, f = valid[int(np.argmax(llh))]
    assert re.search(r"sweep: best model st = %s t = %s f = %s bs_id = -1 llh = %s" % (re.escape(st), t, re.escape(f), re.escape(str(max(llh)))), text), text[-600:]


def test_cli_grid_solve_pulse_sweep_equals_single_grid_solves(tmp_path):
    from misti_amd.optimize import sweep_interval
    f1, f2, fj, _ = _inputs(tmp_path)
    common = ["--cpfit", "-uf", "--funits", str(tmp_path / "nounits.txt"), "--grid-solve", "--all-bs"]
    models = [(st, t) for st in ("20", "20.5") for t in ("3", "12")]
    text = run_cli([f1, f2, fj, "{st}", "-mi", "1", "4", "{st}", "0.2", "0", "-pu", "1", "10", "0.05", "0", "-pu", "2", "{t}", "{f}", "1",
                    "--sweep", "st", "20", "20.5", "--sweep-pu", "t", "3", "12", "--sweep-pu", "f", "0.1"] + common)
    lines = result_lines(text)
    assert len(lines) == 4 * len(models)                               # rows 0..3 (outer) x models
    pat = re.compile(r"^bs_id = (\S+) \tsplitT = (\S+) \ttime = \S+ \tmigration rates fixed = \[0.2\]\toptim = \[\S+\] \tllh = (\S+)$")
    parsed = [pat.match(l) for l in lines]
    assert all(parsed), lines
    for m, (st, t) in enumerate(models):
        end = str(int(np.ceil(float(st))))
        single = result_lines(run_cli([f1, f2, fj, st, "-mi", "1", "4", end, "0.2", "0", "-pu", "1", "10", "0.05", "0", "-pu", "2", t, "0.1", "1"] + common))
        assert single == [lines[bs * len(models) + m] for bs in range(4)], (models[m], single)
    # the summary: the best t of the data row, and the bootstrap interval of t
    llh = np.array([float(m.group(3)) for m in parsed]).reshape(4, len(models))
    iv = sweep_interval(llh, np.array([[float(st), float(t)] for st, t in models]))
    m = re.search(r"sweep: bs_id = 0 best model st = (\S+) t = (\S+) optim", text)
    assert m and (m.group(1), m.group(2)) == models[iv["data_model"]]
    v = iv["variables"][1]
    m = re.search(r"sweep: t bootstrap mean = (\S+) 97.5% t-interval = \[(\S+), (\S+)\] over (\d+) replicates", text)
    assert m, text[-800:]
    assert int(m.group(4)) == v["n_boot"] == 3 and float(m.group(1)) == v["mean"]
    assert np.array_equal([float(m.group(2)), float(m.group(3))], v["interval"], equal_nan=True)
