"""Per-candidate pulse times without a GPU: the oracle against the reference's pulse-date grid (golden_pulse_sweep.json, one
reference run per (fit, st, t, f) point), the expansion and the refusals of `--sweep-pu`, the SetModel filter with pulses against a
transcription of the reference's checks, the header's declarations, and misti_nm_solve_pulses' argument errors through the loaded
library."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PULSES = load_golden("golden_pulse_sweep")
RTOL = 1e-12                  # the oracle restates the reference operation by operation on the same SciPy


def parse(tail):
    from misti_amd import cli
    return cli.build_parser().parse_args(["g1.psmc", "g2.psmc", "sim.jafs"] + tail.split())


def test_fixture_conditions():
    """What tests/golden/make_pulse_sweep.py --check asserts where the reference is installed, from the file alone."""
    finite = [c for c in PULSES if c["out"]["llh"] is not None]
    assert len(finite) >= 24
    for fit in (True, False):
        assert sum(1 for c in finite if bool(c["in"]["kw"].get("cpfit")) == fit) >= 8
    assert {c["sweep"]["st"] for c in PULSES} == {20, 20.5} and len({c["sweep"]["pulse_times"][1] for c in PULSES}) >= 5
    for c in PULSES:
        assert c["sweep"]["pulse_times"][0] != c["sweep"]["pulse_times"][1]          # the fixed pulse sits where the sweep never goes


@pytest.mark.parametrize("case", PULSES, ids=[c["name"] for c in PULSES])
def test_oracle_reproduces_the_reference(case):
    from oracle.misti_oracle import OracleModel
    i, o = case["in"], case["out"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = OracleModel(i["times"], i["lambdas"], i["sfs"], i["split"], i["mi"], i["pu"], **i["kw"])
        llh = m.jafs_likelihood(i["params"])
    assert m.numT == o["numT"] and m.splitT == o["splitT"]
    if o["llh"] is None:
        assert llh == -np.inf
        return
    assert llh == pytest.approx(o["llh"], rel=RTOL)
    np.testing.assert_allclose(m.JAFS, o["JAFS"], rtol=RTOL)
    np.testing.assert_allclose(np.array(m.lc, dtype=float), np.array(o["lc"]), rtol=RTOL)


# ---- the command line -----------------------------------------------------------------------------------------------------------
def test_sweep_pu_expansion():
    from misti_amd.sweep import expand, sweep_error
    a = parse("{st} -uf -mi 1 4 {st} {r} 0 -pu 1 10 0.05 0 -pu 2 {t} {f} 0 --sweep st 20 20.5 --sweep r 0.2 0.3 "
              "--sweep-pu t 3 7 12 --sweep-pu f 0.1 0.35")
    assert sweep_error(a) is None
    p = expand(a)
    # the --sweep variables in their order, then the --sweep-pu variables in theirs, the last innermost
    assert p.names == ["st", "r", "t", "f"] and p.model_names == ["st", "r", "t", "f"]
    assert p.n_model == 2 * 2 * 3 * 2
    assert p.assign[0] == dict(st="20", r="0.2", t="3", f="0.1") and p.assign[1]["f"] == "0.35" and p.assign[2]["t"] == "7"
    assert p.assign[6]["r"] == "0.3" and p.assign[12]["st"] == "20.5"
    assert np.array_equal(p.split, np.repeat([20.0, 20.5], 12))
    assert p.pulse_times.dtype == np.int32 and p.pulse_times.shape == (24, 2)
    assert np.array_equal(p.pulse_times[:, 0], np.full(24, 10)) and np.array_equal(p.pulse_times[:, 1], np.tile(np.repeat([3, 7, 12], 2), 4))
    # parameter slots: no optimised one; the swept fixed rate, then the swept fixed fraction - the same doubles as the literal values
    assert p.k == 0 and p.n_param == 2
    assert p.bands[0][4] == 0 and p.pulses[0] == (0, 10, 0.05, -1) and p.pulses[1][0] == 1 and p.pulses[1][3] == 1
    assert np.array_equal(p.params[:, 0], np.tile(np.repeat([0.2, 0.3], 6), 2)) and np.array_equal(p.params[:, 1], np.tile([0.1, 0.35], 12))
    assert np.array_equal(p.pulse_values[:, 1], p.params[:, 1]) and np.array_equal(p.pulse_values[:, 0], np.full(24, 0.05))
    assert p.pulse_swept and p.engine_pulses(2) == [(0, 10, 0.05, -1), (1, 7, 0.0, 1)]
    assert p.pu[3] == [["1", "10", "0.05", "0"], ["2", "7", "0.35", "0"]]
    assert np.array_equal(p.values[:, 2], p.pulse_times[:, 1]) and np.array_equal(p.values[:, 3], p.params[:, 1])
    assert np.array_equal(p.bounds[:, 0], np.tile([4, -1], (24, 1)))


def test_sweep_pu_alone_and_grid_solve_expansion():
    from misti_amd.sweep import expand, sweep_error
    a = parse("20 -mi 1 4 20 0.2 0 -pu 2 {t} 0.1 0 --sweep-pu t 3 7")
    assert sweep_error(a) is None
    p = expand(a)
    assert p.n_model == 2 and p.n_param == 0 and np.array_equal(p.pulse_times, [[3], [7]]) and p.pulse_swept
    # an optimised pulse: its swept fractions become the starts, the times the models
    a = parse("{st} -mi 1 4 {st} 0.2 1 -pu 2 {t} {f} 1 --sweep st 20 20.5 --sweep-pu t 3 7 12 --sweep-pu f 0.1 0.35 --grid-solve")
    assert sweep_error(a) is None
    p = expand(a)
    assert p.model_names == ["st", "t"] and p.rate_names == ["f"] and p.n_model == 6 and p.k == 2 and p.n_param == 2
    assert np.array_equal(p.starts, [[0.2, 0.1], [0.2, 0.35]])
    assert np.array_equal(p.pulse_times[:, 0], [3, 7, 12, 3, 7, 12]) and np.isnan(p.pulse_values).all()
    assert p.pulses[0][3] == 1
    # without a swept time nothing asks for per-candidate times
    a = parse("{st} -mi 1 4 {st} 0.2 0 -pu 2 6 {f} 0 --sweep st 20 21 --sweep-pu f 0.1 0.35")
    assert sweep_error(a) is None
    p = expand(a)
    assert not p.pulse_swept and p.n_param == 1 and np.array_equal(p.pulse_times, np.full((4, 1), 6))


@pytest.mark.parametrize("tail, why", [
    ("20 -mi 1 4 20 0.1 0 -pu 2 {v} {v} 0 --sweep-pu v 3 4", "a variable is either a pulse time or a pulse fraction"),
    ("20 -mi 1 4 20 0.1 0 -pu 2 {t} 0.1 0 --sweep-pu t 3 4.5", "--sweep-pu t: 4.5 is not an integer, and {t} is a pulse time"),
    ("20 -mi 1 4 20 0.1 0 -pu 2 6 {f} 0 --sweep-pu f 0.1 x", "--sweep-pu f: x is not a number"),
    ("20 -mi 1 4 20 0.1 0 -pu 2 {t} 0.1 1 --sweep-pu t 3 4", "-pu 2 {t} 0.1 1 is optimised (flag 1): --sweep alone evaluates fixed models; add --grid-solve"),
    ("20 -mi 1 4 20 0.1 0 -pu 2 {t} 0.1 0", "{t} is used but not declared: add --sweep-pu t"),
    ("20 -mi 1 4 20 0.1 0 -pu 2 6 0.1 0 --sweep-pu t 3 4", "--sweep-pu t: the name is declared but {t} is used nowhere"),
    ("{st} -mi 1 4 {st} 0.1 0 -pu 2 {t} 0.1 0 --sweep st 20 --sweep-pu t 3 --sweep-pu t 4", "--sweep-pu t: the name is declared twice"),
    ("{st} -mi 1 4 {st} 0.1 0 -pu 2 {st} 0.1 0 --sweep st 20 21", "a pulse takes no placeholder (per-candidate pulse times"),
    ("{st} -mi 1 4 {st} 0.1 0 -pu 2 {st} 0.1 0 --sweep st 20 21", "--sweep-pu NAME V1 V2 ..."),
    ("20 -mi 1 {t} 20 0.1 0 -pu 2 {t} 0.1 0 --sweep-pu t 3 4", "{t} stands in the time and fraction fields of -pu only"),
    ("{t} -mi 1 4 20 0.1 0 --sweep-pu t 20 21", "{t} stands in the time and fraction fields of -pu only"),
    ("20 -mi 1 4 20 0.1 0 -pu {p} 6 0.1 0 --sweep-pu p 1 2", "placeholders stand in the time and fraction fields of -pu only"),
    ("20 -mi 1 4 20 0.1 1 -pu 2 {t} {f} 0 --sweep-pu t 3 4 --sweep-pu f 0.1 0.2 --grid-solve", "--grid-solve: {f} is the fraction of a fixed pulse"),
    ("20 -mi 1 4 20 0.1 0 -pu 2 {t} 0.1 0 --sweep-pu t 3 4 --gpus 2", "--sweep runs on one GPU (--device): the sharded gathers"),
    ("20 -mi 1 4 20 0.1 0 -pu 2 {t} 0.1 0 --sweep-pu t 3 4 --devices 0,1", "--sweep runs on one GPU (--device): the sharded gathers"),
    ("20 -mi 1 4 20 0.1 0 -pu 2 {t} 0.1 0 --sweep-pu t 3 4 --grid-st 18 20", "--sweep and --grid-st exclude each other"),
])
def test_refusals(capsys, tail, why):
    """Each refusal is one line on stderr, before any file is read (none of the inputs exist) or the GPU is touched."""
    from misti_amd import cli
    rc = cli.main(["a.psmc", "b.psmc", "d.sfs"] + tail.split())
    err = capsys.readouterr().err
    assert rc == 2 and why in err, err
    assert len(err.strip().splitlines()) == 1


# ---- SetModel's checks ----------------------------------------------------------------------------------------------------------
def reference_set_model(split, mis, pus, sample_date, n_times):
    """MigrationInference.__init__ (:85-107) and SetModel (:229-279) of the reference, transcribed: True where it would run, False
    where it exits in PrintError or fails with IndexError.  ``mis`` are (pop 0/1, start, end) with end -1 = the split index, ``pus``
    (pop 0/1, time, value)."""
    if split < sample_date:
        return False
    frac, s = split % 1, int(split)
    if s - 1 > n_times:
        return False
    numT = n_times + 1
    if frac != 0.0:
        if s >= n_times:
            return False                         # times[splitT]: IndexError
        numT += 1
        s += 1
    mi = [[None, None] for _ in range(numT)]
    pu = [[None, None] for _ in range(numT)]
    for pop, start, end in mis:
        end = s if end == -1 else end
        if start < sample_date or end <= start:
            return False
        for i in range(start, end):
            if i >= numT:
                return False                     # self.mi[i]: IndexError
            if mi[i][pop] is not None:
                return False
            mi[i][pop] = 0.0
    for pop, t, val in pus:
        if t < sample_date:
            return False
        if val < 0 or val > 1:
            return False
        if t >= numT:
            return False                         # self.pu[puTime]: IndexError
        if pu[t][0] is not None or pu[t][1] is not None:
            return False
        pu[t][pop] = val
    return True


def test_structure_filter_with_pulses_against_set_model():
    from misti_amd.sweep import structure_error
    rng = np.random.default_rng(9)
    numT, pops = 12, [0, 1]
    n_bad = n_pulse_bad = 0
    for _ in range(4000):
        split = float(rng.integers(4, 12)) + (0.5 if rng.random() < 0.3 else 0.0)
        sd = int(rng.random() < 0.3)
        b = np.array([[sd, -1], [int(rng.integers(sd, 3)), 3]])
        times = rng.integers(0, 15, size=3)
        if rng.random() < 0.5:
            times = rng.integers(sd, 12, size=3)                                   # mostly inside the grid
        vals = np.where(rng.random(3) < 0.1, rng.choice([-0.1, 1.5], size=3), rng.random(3))
        pus = [(int(rng.integers(0, 2)), int(t), float(v)) for t, v in zip(times, vals)]
        want = reference_set_model(split, [(p, int(s), int(e)) for p, (s, e) in zip(pops, b)], pus, sd, numT - 1)
        got = structure_error(split, b, pops, sd, numT, times, vals)
        assert (got is None) == want, (split, times.tolist(), vals.tolist(), sd, got)
        n_bad += got is not None
        n_pulse_bad += got is not None and structure_error(split, b, pops, sd, numT) is None
    assert 400 < n_bad < 3600 and n_pulse_bad > 300, (n_bad, n_pulse_bad)
    # without pulse arguments the verdict is the bands' alone, as before
    assert structure_error(20.0, [[4, -1]], [0], 0, 32) is None
    assert "only single-direction" in structure_error(20.0, [[4, -1]], [0], 0, 32, [5, 5], [0.1, 0.1])
    assert structure_error(20.0, [[4, -1]], [0], 0, 32, [25, 20], [0.1, 0.1]) is None      # at or beyond the split: valid, never applied


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "misti_hip.h")).read()
    for name in ("misti_eval_batch_pulses", "misti_eval_batch_pulses_dev", "misti_nm_solve_pulses"):
        assert re.search(r"^int %s\(misti_ctx\* ctx," % name, text, re.M), name
    assert "#define MISTI_ABI_VERSION 6" in text
    from misti_amd import _lib
    lib = _lib.load()
    for name in ("misti_eval_batch_pulses", "misti_eval_batch_pulses_dev", "misti_nm_solve_pulses"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None


def test_nm_solve_pulses_rejects_its_arguments_through_the_library():
    """MISTI_E_ARG before anything touches a device: none is needed here (no context exists)."""
    from misti_amd import _lib
    lib = _lib.load()
    d = (C.c_double * 16)()
    i = (C.c_int32 * 8)()
    E_ARG = -1

    def call(ctx=None, starts=d, splits=d, rows=i, n_rep=1, jsfs=d, maxiter=10, x=d, llh=d):
        rc = lib.misti_nm_solve_pulses(ctx, 1, starts, splits, rows, i, i, n_rep, jsfs, 1e-4, 1e-4, maxiter, x, llh, None, None, None)
        return rc, lib.misti_last_error()
    for kw in (dict(starts=None), dict(splits=None), dict(rows=None), dict(jsfs=None), dict(x=None), dict(llh=None)):
        rc, why = call(**kw)
        assert rc == E_ARG and b"is NULL" in why and b"ctx" not in why, (kw, why)
    bad_row = (C.c_int32 * 8)(3)
    rc, why = call(rows=bad_row, n_rep=2)
    assert rc == E_ARG and b"rows[0] = 3 is outside the table" in why
    rc, why = call(rows=(C.c_int32 * 8)(-1))
    assert rc == E_ARG and b"outside the table" in why
    for v in (float("nan"), float("inf")):
        rc, why = call(splits=(C.c_double * 16)(v))
        assert rc == E_ARG and b"split_times[0] is not finite" in why
    rc, why = call(maxiter=0)
    assert rc == E_ARG and b"maxiter must be >= 1" in why
    rc, why = call(n_rep=0)
    assert rc == E_ARG and b"n_rep must be >= 1" in why
    rc, why = call()
    assert rc == E_ARG and b"ctx is NULL" in why
    # the evaluation entry point refuses a missing context the same way
    rc = lib.misti_eval_batch_pulses(None, 1, d, d, i, i, 1, d, d, d, None, None, None)
    assert rc == E_ARG and b"ctx is NULL" in lib.misti_last_error()
    rc = lib.misti_eval_batch_pulses_dev(None, 1, d, d, i, i, 1, d, d, d, None, None, None)
    assert rc == E_ARG and b"ctx is NULL" in lib.misti_last_error()
