"""Curvature at a point: misti_curvature_assemble_dev and misti_curvature (Engine.curvature_assemble_dev, Engine.curvature) against the
rule stated in NumPy (optimize.curvature_stencil, curvature_from_spectra, curvature_contract).

Which of "tolerance" and "bit equality" holds: the kernels perform the rule's operations in the rule's order, but the logarithm is
the device's, not NumPy's - the two may differ in the last place - so derivatives are held to the ROUNDING FLOOR, 16 ulp x the sum of
the absolute elementary terms of each output (clause 1 of tests/parity.py: FLOOR_ULPS x EPS x sum |terms|), where the elementary
terms of an output are the logs it differences, each with its factor (1 / 2h, 1 / h^2, 1 / 4 h_i h_j, and the class count for grad and
hess).  Statuses, NaN patterns, the symmetry of the Hessian, llh0 and everything that compares the device with itself are bit for
bit.  All models live on the small synthetic grid of tests/test_gpu_scan_profile.py (numT = 32)."""
import ctypes as C
import io
import random

import numpy as np
import pytest

from parity import EPS, FLOOR_ULPS, llk_summand_scale

pytestmark = pytest.mark.gpu

SPLIT = 20.0


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def grid():
    from misti_amd import synth, io as mio
    return mio.merge_psmc(mio.read_psmc_file(io.StringIO(synth.psmc_text(16, 1, synth.THETA_1))),
                          mio.read_psmc_file(io.StringIO(synth.psmc_text(17, 2, synth.THETA_2))))


def rule(jafs, status, h, unfolded, table=None, rows=None):
    """The NumPy rule and, per output, the floor: 16 ulp x the sum of the absolute elementary terms."""
    from misti_amd.optimize import _class_values, class_counts, curvature_contract, curvature_from_spectra
    dlog, d2log, pst = curvature_from_spectra(jafs, status, h, unfolded)
    P, D = h.shape
    with np.errstate(invalid="ignore", divide="ignore"):
        aL = np.zeros(jafs.shape)
        cv = np.abs(np.log(_class_values(jafs, unfolded)))
        aL[..., :cv.shape[-1]] = cv
    t1, t2 = np.zeros(dlog.shape), np.zeros(d2log.shape)
    q = 0
    for i in range(D):
        hi = h[:, i, None]
        t1[:, i] = (aL[:, 1 + 2 * i] + aL[:, 2 + 2 * i]) / (2 * hi)
        t2[:, i, i] = (aL[:, 1 + 2 * i] + 2 * aL[:, 0] + aL[:, 2 + 2 * i]) / (hi * hi)
        for j in range(i + 1, D):
            c = 1 + 2 * D + 4 * q
            t2[:, i, j] = t2[:, j, i] = aL[:, c:c + 4].sum(axis=1) / (4 * hi * h[:, j, None])
            q += 1
    out = dict(dlog=dlog, d2log=d2log, status=pst, tol_dlog=FLOOR_ULPS * EPS * t1, tol_d2log=FLOOR_ULPS * EPS * t2)
    if rows is not None:
        out["grad"], out["hess"] = curvature_contract(dlog, d2log, table, rows, unfolded)
        f = np.abs(class_counts(table, unfolded)[rows])
        out["tol_grad"] = FLOOR_ULPS * EPS * np.einsum("pk,pik->pi", f, t1)
        out["tol_hess"] = FLOOR_ULPS * EPS * np.einsum("pk,pijk->pij", f, t2)
    return out


def assert_floor(got, want, tol, ok, tag):
    """Points with a value within the floor (each figure printed first), points without one NaN throughout."""
    bad = ~ok
    assert np.isnan(got[bad]).all() and np.isnan(want[bad]).all(), tag
    if ok.any():
        err, room = np.abs(got[ok] - want[ok]), tol[ok]
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = np.nanmax(np.where(room > 0, err / room, np.where(err > 0, np.inf, 0.0)))
        print(tag, "largest error / floor = %.3g" % worst)
        assert np.isfinite(got[ok]).all() and (err <= room).all(), (tag, worst)


# ---- 1. assembly against the rule on hand-made spectra ---------------------------------------------------------------------------------
def spectra(rng, shape):
    j = rng.random(shape + (7,)) + 0.05
    return j / j.sum(axis=-1, keepdims=True)


def counts(rng, R):
    rows = np.zeros((R, 8))
    rows[:, 1:] = rng.integers(0, 50000, size=(R, 7))
    rows[:, 0] = rows[:, 1:].sum(axis=1)
    return rows


def assemble(e, D, jafs, status, h, rows, table, want_derivs=True):
    """Outputs pre-filled with sentinels, and a guard allocated right behind each: an overrun would show there."""
    import torch
    dev = torch.device("cuda", 0)
    P = h.shape[0]
    up = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=dev)
    d_j, d_s, d_h, d_r, d_t = up(jafs, np.float64), up(status, np.int32), up(h, np.float64), up(rows, np.int32), up(table, np.float64)
    outs, guards = {}, {}
    for name, shape in (("dlog", (P, D, 7)), ("d2log", (P, D, D, 7)), ("grad", (P, D)), ("hess", (P, D, D))):
        outs[name] = torch.full(shape, 7.0, dtype=torch.float64, device=dev)
        guards[name] = torch.full((64,), 7.0, dtype=torch.float64, device=dev)
    pst = torch.full((P,), -7, dtype=torch.int32, device=dev)
    guard_i = torch.full((64,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ptr = lambda t: t.data_ptr() if t is not None else 0
    with_rows = rows is not None
    e.curvature_assemble_dev(P, ptr(d_j), ptr(d_s), ptr(d_h), ptr(d_r), table.shape[0] if with_rows else 0, ptr(d_t) if with_rows else 0,
                             ptr(outs["dlog"]) if want_derivs else 0, ptr(outs["d2log"]) if want_derivs else 0,
                             ptr(outs["grad"]) if with_rows else 0, ptr(outs["hess"]) if with_rows else 0, ptr(pst))
    e.sync()
    assert all(float(g.sum().item()) == 64 * 7.0 for g in guards.values()) and int(guard_i.sum().item()) == 64 * -7
    return {k: v.cpu().numpy() for k, v in outs.items()}, pst.cpu().numpy()


@pytest.mark.parametrize("unfolded", [False, True], ids=["folded", "unfolded"])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_assembly_equals_the_rule_on_hand_made_spectra(D, unfolded):
    """P = 1, 3 and 70 (more points than a workgroup of the contraction holds entries for, and than one wave), random positive
    spectra, a few stencil candidates with a status 1 ... 6, one class value set to 0 (status MISTI_NUMERIC unless an earlier
    candidate of the point has a status), and the same call with d_status NULL.  Tolerance, not bit equality: see the module text."""
    from misti_amd.engine import Engine
    from misti_amd.optimize import curvature_size
    inp = grid()
    rng = np.random.default_rng(100 + 10 * D + unfolded)
    M = curvature_size(D)
    with Engine(inp.times, inp.lambdas, n_param=D, unfolded=unfolded) as e:
        for P in (1, 3, 70):
            jafs = spectra(rng, (P, M))
            h = 10.0 ** rng.uniform(-4, -1, size=(P, D))
            table = counts(rng, 6)
            rows = rng.integers(0, 6, size=P).astype(np.int32)
            status = np.zeros((P, M), dtype=np.int32)
            if P > 1:
                hit = rng.random((P, M)) < 0.15 / M * 3
                status[hit] = rng.integers(1, 7, size=int(hit.sum()))
                status[:2] = 0                                             # point 0 keeps its value
                status[1, M - 1], status[1, M // 2] = 3, 6                # two in one point: the first in stencil order counts
                jafs[2, M // 2, 3] = 0.0                                   # class 3 stands alone folded and unfolded
                status[2] = 0
            else:
                jafs[0, 0, 3] = 0.0
            for st in (status, None):
                want = rule(jafs, st, h, unfolded, table, rows)
                got, pst = assemble(e, D, jafs, st, h, rows, table)
                assert np.array_equal(pst, want["status"]), (P, st is None)
                ok = pst == 0
                if P > 1:
                    assert pst[2] == 5 and (st is None or pst[1] == 6) and ok.any() and not ok.all()
                else:
                    assert pst[0] == 5
                for name in ("dlog", "d2log", "grad", "hess"):
                    assert_floor(got[name], want[name], want["tol_" + name], ok, (name, D, unfolded, P, st is None))
                assert same_bits(got["d2log"], np.swapaxes(got["d2log"], 1, 2)) and same_bits(got["hess"], np.swapaxes(got["hess"], 1, 2))
                if not unfolded:
                    assert (got["dlog"][ok][..., 4:] == 0).all() and (got["d2log"][ok][..., 4:] == 0).all()
            # grad / hess alone (the derivatives go through the context's own buffers), and no contraction at all
            alone, pst2 = assemble(e, D, jafs, status, h, rows, table, want_derivs=False)
            both, pst1 = assemble(e, D, jafs, status, h, rows, table)
            assert same_bits(alone["grad"], both["grad"]) and same_bits(alone["hess"], both["hess"]) and np.array_equal(pst2, pst1)
            assert (alone["dlog"] == 7.0).all() and (alone["d2log"] == 7.0).all()
            none, pst3 = assemble(e, D, jafs, status, h, None, table)
            assert same_bits(none["dlog"], both["dlog"]) and same_bits(none["d2log"], both["d2log"]) and np.array_equal(pst3, pst2)
            assert (none["grad"] == 7.0).all() and (none["hess"] == 7.0).all()


# ---- the models of the driver tests ----------------------------------------------------------------------------------------------------
MODELS = {
    # name: (bands, pulses, n_param, flags, split, a point)
    "one_band_cpfit": ([(0, 2, -1, 0.2, 0)], [], 1, dict(cpfit=True, smooth=True), SPLIT, [0.2]),
    "two_way_cpfit": ([(0, 2, -1, 0.2, 0), (1, 2, -1, 0.1, 1)], [], 2, dict(cpfit=True, smooth=True), SPLIT, [0.2, 0.1]),
    "two_way_default": ([(0, 2, -1, 0.2, 0), (1, 2, -1, 0.1, 1)], [], 2, dict(smooth=True), SPLIT, [0.2, 0.1]),
    "two_way_fractional": ([(0, 2, -1, 0.2, 0), (1, 2, -1, 0.1, 1)], [], 2, dict(cpfit=True, smooth=True), 19.5, [0.25, 0.08]),
    "pulse_unfolded": ([(0, 4, -1, 0.2, 0), (1, 4, -1, 0.15, 1)], [(1, 8, 0.05, 2)], 3, dict(cpfit=True, smooth=True, unfolded=True), SPLIT,
                       [0.2, 0.15, 0.05]),
}


@pytest.fixture(scope="module")
def table():
    """A 7-row bootstrap table (row 0 the data) of counts drawn from the two-way model's own spectrum."""
    from misti_amd import io as mio, synth
    from misti_amd.engine import truth_spectrum
    inp = grid()
    jafs = truth_spectrum(inp.times, inp.lambdas, SPLIT, [(0, 2, 20, 0.2, -1), (1, 2, 20, 0.1, -1)], [], 0)
    row = synth.counts_from_spectrum(jafs, 200000)
    return np.array(mio.bootstrap_table(synth.chunk_rows(row, 20), 6, random.Random(3)), dtype=np.float64)


def model_engine(name):
    from misti_amd.engine import Engine
    inp = grid()
    bands, pulses, D, flags, split, x0 = MODELS[name]
    return Engine(inp.times, inp.lambdas, bands, pulses, n_param=D, **flags), D, split, np.array(x0), bool(flags.get("unfolded"))


def points_of(name, P, rng):
    """P points around the model's own, their rows, and per-point pulse times where the model has a pulse."""
    _, pulses, D, _, split, x0 = MODELS[name]
    x = np.array(x0) * rng.uniform(0.7, 1.4, size=(P, D))
    rows = (np.arange(P) % 7).astype(np.int32)
    pt = np.array([[6 + (p % 5)] for p in range(P)], dtype=np.int32) if pulses else None
    return x, np.full(P, split), rows, pt


def through_evaluate(e, x, splits, rows, table, unfolded, pulse_times=None, band_bounds=None, rel_step=1e-2, abs_step=0.0):
    """The stencil pushed through Engine.evaluate, then the NumPy rule; also the llk of every stencil candidate against its row."""
    from misti_amd.optimize import curvature_stencil
    pts, h, boundary = curvature_stencil(x, rel_step, abs_step)
    P, M, D = pts.shape
    rep = lambda a: None if a is None else np.repeat(np.asarray(a), M, axis=0)
    res = e.evaluate(np.repeat(splits, M), pts.reshape(P * M, D), table, band_bounds=rep(band_bounds), pulse_times=rep(pulse_times))
    jafs, status = res.jafs.reshape(P, M, 7), res.status.reshape(P, M)
    llk = res.llk.reshape(P, M, -1)[np.arange(P), :, rows]
    return rule(jafs, status, h, unfolded, table, rows), jafs, llk, h, boundary


# ---- 2. the driver against the assembly, 3. against differences of the llk values -----------------------------------------------------
def driver_comparison(name, e, D, unfolded, x, splits, rows, pt, table, may_fail=False):
    """The driver against the stencil pushed through Engine.evaluate and the rule (2.), and against central differences of the llk
    values themselves (3.); `e` is closed here.  Every point must come back with status 0 unless `may_fail`."""
    with e:
        got = e.curvature(x, splits, rows, table, pulse_times=pt)
        want, jafs, llk, h, boundary = through_evaluate(e, x, splits, rows, table, unfolded, pulse_times=pt)
    print(name, "status", got.status, "through evaluate", want["status"])
    assert not boundary.any() and np.array_equal(got.status, want["status"])
    ok = got.status == 0
    assert ok.any() and (ok.all() or may_fail)
    assert same_bits(got.h, h)
    assert same_bits(got.llh0[ok], llk[ok, 0]), "llh0 is the centre's evaluate value, bit for bit"
    assert np.isnan(got.llh0[~ok]).all()
    assert_floor(got.dlog, want["dlog"], want["tol_dlog"], ok, (name, "dlog"))
    assert_floor(got.grad, want["grad"], want["tol_grad"], ok, (name, "grad"))
    assert_floor(got.hess, want["hess"], want["tol_hess"], ok, (name, "hess"))
    assert same_bits(got.hess, np.swapaxes(got.hess, 1, 2))
    if pt is not None:
        assert len({float(v) for v in got.llh0}) == x.shape[0]         # the per-point pulse times reach the values
    # 3. the independent path: central differences of the llk values themselves.  eps is the clause-1 floor (tests/parity.py) of the
    # point's centre; a difference of 2 (4) such values over 2 h (h_i h_j) is allowed 2 eps / h_i (4 eps / (h_i h_j)).
    P = x.shape[0]
    eps = np.array([FLOOR_ULPS * EPS * llk_summand_scale(table[rows[p]], jafs[p, 0], unfolded) if ok[p] else np.nan for p in range(P)])
    g_fd = np.empty((P, D))
    h_fd = np.empty((P, D, D))
    q = 0
    for i in range(D):
        g_fd[:, i] = (llk[:, 1 + 2 * i] - llk[:, 2 + 2 * i]) / (2 * h[:, i])
        h_fd[:, i, i] = (llk[:, 1 + 2 * i] - 2 * llk[:, 0] + llk[:, 2 + 2 * i]) / h[:, i] ** 2
        for j in range(i + 1, D):
            c = 1 + 2 * D + 4 * q
            h_fd[:, i, j] = h_fd[:, j, i] = (llk[:, c] - llk[:, c + 1] - llk[:, c + 2] + llk[:, c + 3]) / (4 * h[:, i] * h[:, j])
            q += 1
    g_fd[~ok], h_fd[~ok] = np.nan, np.nan                              # (a point without a value has no llk differences to hold it to)
    assert_floor(got.grad, g_fd, 2 * eps[:, None] / h, ok, (name, "grad against llk differences"))
    assert_floor(got.hess, h_fd, 4 * eps[:, None, None] / (h[:, :, None] * h[:, None, :]), ok, (name, "hess against llk differences"))
    assert (np.abs(got.grad[ok]) > 0).all() and (np.abs(got.hess[ok]) > 0).all()


@pytest.mark.parametrize("name", sorted(MODELS))
def test_driver_equals_the_stencil_through_evaluate_and_llk_differences(name, table):
    e, D, split, x0, unfolded = model_engine(name)
    x, splits, rows, pt = points_of(name, 4, np.random.default_rng(7))
    # (under the default fit the lambda-correction fails at three of these four points - status 2, from evaluate and from the driver
    #  alike; the points with a value are held to the rule, the others must be NaN throughout)
    driver_comparison(name, e, D, unfolded, x, splits, rows, pt, table, may_fail=name == "two_way_default")


# ---- 4. the batch cut ------------------------------------------------------------------------------------------------------------------
FIELDS = ("llh0", "grad", "hess", "dlog", "status")


def test_the_result_does_not_move_with_the_batch_limit(table):
    from misti_amd.optimize import curvature_size
    e, D, split, x0, unfolded = model_engine("two_way_cpfit")
    M = curvature_size(D)
    with e:
        x, splits, rows, _ = points_of("two_way_cpfit", 5, np.random.default_rng(9))
        x[3] = x[1]                                                    # two points share their stencil's chains
        whole = e.curvature(x, splits, rows, table)
        assert (whole.status == 0).all()
        for limit in (M, 2 * M + 1):
            cut = e.curvature(x, splits, rows, table, batch_limit=limit)
            for k in FIELDS:
                assert same_bits(getattr(cut, k), getattr(whole, k)), (limit, k)


# ---- 5. isolation ----------------------------------------------------------------------------------------------------------------------
def test_points_without_a_value_leave_their_neighbours_alone(table):
    """A boundary point (a rate of 0 under an absolute step), a point whose split is off the grid and a point whose own band bounds
    end before they start, among four ordinary points: status 7 and the engine's status, NaN everywhere, and the four ordinary
    points bit for bit those of a batch without the three."""
    e, D, split, x0, unfolded = model_engine("two_way_cpfit")
    with e:
        x, splits, rows, _ = points_of("two_way_cpfit", 7, np.random.default_rng(11))
        bounds = np.tile(np.array([[2, -1], [2, -1]], dtype=np.int32), (7, 1, 1))
        bounds[0] = [[3, -1], [4, -1]]                                 # an ordinary point with bounds of its own
        special, ordinary = [1, 3, 6], [0, 2, 4, 5]
        x[1, 0] = 0.0
        splits[3] = 1000.0
        bounds[6] = [[12, 8], [2, -1]]
        got = e.curvature(x, splits, rows, table, band_bounds=bounds, abs_step=1e-4)
        ref_status = e.evaluate(splits[[3, 6]], x[[3, 6]], band_bounds=bounds[[3, 6]]).status
        alone = e.curvature(x[ordinary], splits[ordinary], rows[ordinary], table, band_bounds=bounds[ordinary], abs_step=1e-4)
    assert got.status[1] == 7 and list(got.status[[3, 6]]) == list(ref_status) and (ref_status != 0).all()
    assert (got.status[ordinary] == 0).all() and (alone.status == 0).all()
    for k in ("llh0", "grad", "hess", "dlog"):
        assert np.isnan(getattr(got, k)[special]).all(), k
        assert same_bits(getattr(got, k)[ordinary], getattr(alone, k)), k
    assert not same_bits(got.llh0[0], got.llh0[2])


# ---- 6. argument errors ----------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_device_work(table):
    """Every refusal with n_point huge and buffers that hold three points: a call that went on would read or write far outside them.
    (Checks that walk the points - rows, finiteness - are made on the real three points.)"""
    from misti_amd import _lib
    from misti_amd.engine import Engine
    inp = grid()
    e, D, split, x0, unfolded = model_engine("two_way_cpfit")
    lib = _lib.load()
    P = 3
    x = np.tile(x0, (P, 1))
    st = np.full(P, split)
    rows = np.zeros(P, dtype=np.int32)
    out = dict(llh0=np.full(P, 7.0), grad=np.full((P, D), 7.0), hess=np.full((P, D, D), 7.0), dlog=np.full((P, D, 7), 7.0),
               status=np.full(P, -7, dtype=np.int32))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    huge = 2 ** 40

    def code(n=huge, x_=x, st_=st, rows_=rows, n_rep=table.shape[0], tab=table, rel=1e-2, ab=0.0, limit=0, status=out["status"], ctx=None):
        r = lib.misti_curvature(e._ctx if ctx is None else ctx, n, ptr(x_), ptr(st_), ptr(rows_), None, None, n_rep, ptr(tab), rel, ab, limit,
                                ptr(out["llh0"]), ptr(out["grad"]), ptr(out["hess"]), ptr(out["dlog"]), ptr(status))
        assert r != 0 and lib.misti_last_error()
        return r

    with e:
        assert code(x_=None) == -1 and code(st_=None) == -1 and code(rows_=None) == -1 and code(tab=None) == -1 and code(status=None) == -1
        assert code(n=-1) == -1
        assert code(n_rep=0) == -1
        for rel, ab in ((0.0, 0.0), (-1e-2, 1e-3), (1e-2, -1e-3), (np.nan, 0.0), (np.inf, 0.0), (1e-2, np.inf)):
            assert code(rel=rel, ab=ab) == -1, (rel, ab)
        assert code(limit=8) == -1 and code(limit=-1) == -1              # M = 9
        assert code() == -4                                               # 2^40 points x 9 candidates
        assert code(n=2 ** 31 // 9 + 1) == -4
        bad_rows = rows.copy(); bad_rows[2] = table.shape[0]
        assert code(n=P, rows_=bad_rows) == -1
        bad_rows[2] = -1
        assert code(n=P, rows_=bad_rows) == -1
        for v in (np.nan, np.inf):
            bad = x.copy(); bad[1, 1] = v
            assert code(n=P, x_=bad) == -1
            bad = st.copy(); bad[2] = v
            assert code(n=P, st_=bad) == -1
        with Engine(inp.times, inp.lambdas) as none:                      # a model without an optimised parameter
            assert code(n=P, ctx=none._ctx) == -1
            with pytest.raises(_lib.MistiError) as err:
                none.curvature_assemble_dev(1, 8, 0, 8, 0, 0, 0, 0, 0, 0, 0, 8)
            assert err.value.code == -1
        # the device form: bogus but non-NULL addresses, refused before they are used
        def dev_code(*args):
            with pytest.raises(_lib.MistiError) as err:
                e.curvature_assemble_dev(*args)
            return err.value.code
        assert dev_code(huge, 8, 0, 8, 0, 0, 0, 8, 8, 0, 0, 8) == -4
        assert dev_code(-1, 8, 0, 8, 0, 0, 0, 8, 8, 0, 0, 8) == -1
        assert dev_code(P, 0, 0, 8, 0, 0, 0, 8, 8, 0, 0, 8) == -1         # d_jafs NULL
        assert dev_code(P, 8, 0, 0, 0, 0, 0, 8, 8, 0, 0, 8) == -1         # d_h NULL
        assert dev_code(P, 8, 0, 8, 0, 0, 0, 8, 8, 0, 0, 0) == -1         # d_point_status NULL
        assert dev_code(P, 8, 0, 8, 0, 0, 0, 8, 8, 8, 0, 8) == -1         # grad without rows
        assert dev_code(P, 8, 0, 8, 8, 0, 8, 8, 8, 8, 8, 8) == -1         # rows without a table (n_rep 0)
        assert dev_code(P, 8, 0, 8, 8, 3, 0, 8, 8, 8, 8, 8) == -1         # ... (d_jsfs NULL)
        e.curvature_assemble_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)      # no point: nothing to do
        # nothing was written, and the context still works
        assert all((v == (-7 if k == "status" else 7.0)).all() for k, v in out.items())
        assert lib.misti_curvature(e._ctx, 0, ptr(x), ptr(st), ptr(rows), None, None, table.shape[0], ptr(table), 1e-2, 0.0, 0,
                                   None, None, None, None, ptr(out["status"])) == 0
        res = e.curvature(x, st, rows, table)
        assert (res.status == 0).all() and np.isfinite(res.hess).all()
