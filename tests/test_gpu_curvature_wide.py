"""The curvature kernels at the widths and counts the C ABI promises and tests/test_gpu_curvature.py never reaches: models of 4 to
MISTI_MAX_PARAMS = 16 parameters (M = 513 stencil candidates, 28 KB of LDS in curv_assemble_kernel, 120 coordinate pairs behind
curv_stencil_kernel's pair decode and curv_pair_rank), more points than curv_slots_kernel has threads, and more points than
curv_assemble_kernel has workgroups.

 1. The assembly against ANALYTIC derivatives (tests/curvature_wide.py: class logs that are exact quadratics of the parameters; the
    NumPy rule is worded after the kernel and would share a slip in the pair order), and against the rule.
 2. The assembly against the rule on random spectra with statuses, at D = 4, 8, 16 and at 65 536 + 70 points.
 3. The driver at D = 4 and D = 16: curv_stencil_kernel's candidates against optimize.curvature_stencil's through Engine.evaluate.
 4. 600 points, boundary points among them: a run of 3 points per thread of curv_slots_kernel.

Tolerances are those of tests/test_gpu_curvature.py (the rounding floor; see that module's text), bit equality wherever the device
is compared with itself."""
import numpy as np
import pytest

import curvature_wide as cw
from test_gpu_curvature import (FIELDS, SPLIT, assemble, assert_floor, counts, driver_comparison, grid, model_engine, points_of, rule,
                                same_bits, spectra, table)  # noqa: F401  (table: the module's fixture)

pytestmark = pytest.mark.gpu

FOLDS = pytest.mark.parametrize("unfolded", [False, True], ids=["folded", "unfolded"])


def bare_engine(D, unfolded):
    from misti_amd.engine import Engine
    inp = grid()
    return Engine(inp.times, inp.lambdas, n_param=D, unfolded=unfolded)


# ---- 1. the assembly against analytic derivatives --------------------------------------------------------------------------------------
@FOLDS
@pytest.mark.parametrize("D", [4, 5, 8, 16])
def test_assembly_equals_the_analytic_derivatives_of_quadratic_class_logs(D, unfolded):
    """The arrays of tests/test_curvature_wide_cpu.py (same seeds) through misti_curvature_assemble_dev: within the floor of the
    analytic values (max(|L|, 1) for |L|: tests/curvature_wide.py) and within the module's floor of the rule; d2log and hess equal to
    their transposes bit for bit, the folded entries 4 to 6 zero, the guards behind every output untouched (assemble()).  A pair rank
    or a mirror store that goes wrong from the fourth coordinate on puts A_k[i'][j'] where A_k[i][j] belongs: 1e3 floors away or more."""
    case = cw.quadratic_case(D, unfolded, 300 + 10 * D + unfolded)
    rng = np.random.default_rng(7)
    tab = cw.counts(rng, 6)
    rows = rng.integers(0, 6, size=case["x"].shape[0]).astype(np.int32)
    with bare_engine(D, unfolded) as e:
        got, pst = assemble(e, D, case["jafs"], None, case["h"], rows, tab)
    assert (pst == 0).all()
    exact = cw.analytic(case, tab, rows, unfolded)
    tol = cw.floors(case["jafs"], case["h"], unfolded, tab, rows)
    want = rule(case["jafs"], None, case["h"], unfolded, tab, rows)
    ok = pst == 0
    for name in ("dlog", "d2log", "grad", "hess"):
        assert_floor(got[name], exact[name], tol[name], ok, ("analytic", name, D, unfolded))
        assert_floor(got[name], want[name], want["tol_" + name], ok, ("rule", name, D, unfolded))
    assert same_bits(got["d2log"], np.swapaxes(got["d2log"], 1, 2)) and same_bits(got["hess"], np.swapaxes(got["hess"], 1, 2))
    if not unfolded:
        assert (got["dlog"][..., 4:] == 0).all() and (got["d2log"][..., 4:] == 0).all()


# ---- 2. the assembly against the rule: widths, then counts -----------------------------------------------------------------------------
def against_the_rule(e, D, unfolded, jafs, status, h, rows, tab, tag):
    """With the statuses and with d_status NULL: statuses equal, values within the floor, symmetric bit for bit, folded entries 0."""
    out = {}
    for st in (status, None):
        want = rule(jafs, st, h, unfolded, tab, rows)
        got, pst = assemble(e, D, jafs, st, h, rows, tab)
        assert np.array_equal(pst, want["status"]), (tag, st is None)
        ok = pst == 0
        for name in ("dlog", "d2log", "grad", "hess"):
            assert_floor(got[name], want[name], want["tol_" + name], ok, (name,) + tag + (st is None,))
        assert same_bits(got["d2log"], np.swapaxes(got["d2log"], 1, 2)) and same_bits(got["hess"], np.swapaxes(got["hess"], 1, 2))
        if not unfolded:
            assert (got["dlog"][ok][..., 4:] == 0).all() and (got["d2log"][ok][..., 4:] == 0).all()
        out[st is None] = (got, pst)
    return out


@FOLDS
@pytest.mark.parametrize("D", [4, 8, 16])
def test_assembly_equals_the_rule_at_wide_models(D, unfolded):
    """test_assembly_equals_the_rule_on_hand_made_spectra's recipe at P = 1, 3 and 70: random spectra, steps of 1e-4 ... 1e-1, point 1
    with a status at the LAST stencil candidate (M - 1) and at the FIRST pair candidate (1 + 2 D: the earlier one counts), point 2
    with a class value of 0 in the middle of the stencil, random statuses 1 ... 6 beyond, and everything again with d_status NULL."""
    from misti_amd.optimize import curvature_size
    rng = np.random.default_rng(500 + 10 * D + unfolded)
    M = curvature_size(D)
    with bare_engine(D, unfolded) as e:
        for P in (1, 3, 70):
            jafs = spectra(rng, (P, M))
            h = 10.0 ** rng.uniform(-4, -1, size=(P, D))
            tab = counts(rng, 6)
            rows = rng.integers(0, 6, size=P).astype(np.int32)
            status = np.zeros((P, M), dtype=np.int32)
            if P > 1:
                hit = rng.random((P, M)) < 0.15 / M * 3
                status[hit] = rng.integers(1, 7, size=int(hit.sum()))
                status[:3] = 0                                             # point 0 keeps its value
                status[1, M - 1], status[1, 1 + 2 * D] = 3, 6
                jafs[2, M // 2, 3] = 0.0                                   # class 3 stands alone folded and unfolded
            else:
                jafs[0, M - 1, 3] = 0.0
            out = against_the_rule(e, D, unfolded, jafs, status, h, rows, tab, (D, unfolded, P))
            (both, pst), (_, pst_null) = out[False], out[True]
            if P > 1:
                assert pst[0] == 0 and pst[1] == 6 and pst[2] == 5 and pst_null[1] == 0 and pst_null[2] == 5
                assert P == 3 or (np.isin(pst[3:], (1, 2, 3, 4, 5, 6)).any() and (pst[3:] == 0).sum() > 20)
            else:
                assert pst[0] == 5 and pst_null[0] == 5
            # grad / hess alone (the derivatives go through the context's own buffers), and no contraction at all
            alone, pst2 = assemble(e, D, jafs, status, h, rows, tab, want_derivs=False)
            assert same_bits(alone["grad"], both["grad"]) and same_bits(alone["hess"], both["hess"]) and np.array_equal(pst2, pst)
            assert (alone["dlog"] == 7.0).all() and (alone["d2log"] == 7.0).all()
            none, pst3 = assemble(e, D, jafs, status, h, None, tab)
            assert same_bits(none["dlog"], both["dlog"]) and same_bits(none["d2log"], both["d2log"]) and np.array_equal(pst3, pst)
            assert (none["grad"] == 7.0).all() and (none["hess"] == 7.0).all()


def test_assembly_walks_a_second_point_per_workgroup():
    """D = 1, folded, 65 536 + 70 points: curv_assemble_kernel launches 65 536 workgroups, so the first 70 walk a second point each
    (11 MB of spectra).  Points on both sides of index 65 536 carry a status or a class value of 0; every point is held to the rule."""
    D, M, P = 1, 3, 65536 + 70
    rng = np.random.default_rng(565)
    jafs = spectra(rng, (P, M))
    h = 10.0 ** rng.uniform(-4, -1, size=(P, D))
    tab = counts(rng, 6)
    rows = rng.integers(0, 6, size=P).astype(np.int32)
    status = np.zeros((P, M), dtype=np.int32)
    marked = {3: (1, 2), 69: (2, 4), 65535: (0, 1), 65536: (2, 6), 65540: (1, 3), 65536 + 69: (0, 2)}
    for p, (m, s) in marked.items():
        status[p, m] = s
    zero = (5, 65537, 65536 + 68)
    for p in zero:
        jafs[p, 1, 3] = 0.0
    with bare_engine(D, False) as e:
        out = against_the_rule(e, D, False, jafs, status, h, rows, tab, ("second point",))
    pst, pst_null = out[False][1], out[True][1]
    assert all(pst[p] == s and pst_null[p] == 0 for p, (m, s) in marked.items())
    assert all(pst[p] == 5 and pst_null[p] == 5 for p in zero)
    assert (pst != 0).sum() == len(marked) + len(zero) and (pst_null != 0).sum() == len(zero)


# ---- 3. the driver at D = 4 and at the limit -------------------------------------------------------------------------------------------
WIDE_MODELS = {
    # name: (bands, pulses, n_param, flags, a point, points)
    # two bands per population on disjoint intervals
    "four_bands_cpfit": ([(0, 2, 6, 0.2, 0), (0, 8, -1, 0.15, 1), (1, 2, 6, 0.1, 2), (1, 8, -1, 0.12, 3)], [], 4, dict(cpfit=True, smooth=True),
                         [0.2, 0.15, 0.1, 0.12], 3),
    # tests/test_gpu_limits.py::test_largest_model_structure: both directions over intervals 0 ... 8, one pulse per interval 9 ... 16
    "largest_true_eps": ([(k % 2, 2 * (k // 2), 2 * (k // 2) + 2, 0.0, k) for k in range(8)], [((k + 1) % 2, 9 + k, 0.0, 8 + k) for k in range(8)], 16,
                         dict(true_eps=True), [0.05 + 0.01 * k for k in range(8)] + [0.02 + 0.01 * k for k in range(8)], 2),
}


def wide_points(name):
    bands, pulses, D, flags, x0, P = WIDE_MODELS[name]
    x = np.array(x0) * np.random.default_rng(D).uniform(0.7, 1.4, size=(P, D))
    return x, np.full(P, SPLIT), (np.arange(P) % 7).astype(np.int32)


@pytest.mark.parametrize("name", sorted(WIDE_MODELS))
def test_driver_equals_the_stencil_through_evaluate_at_wide_models(name, table):
    """test_driver_equals_the_stencil_through_evaluate_and_llk_differences' comparison for a model of 4 parameters (33 candidates per
    point, 6 pairs) and for the largest the ABI takes (16 parameters, 513 candidates per point, 1 026 in one batch): a pair decode of
    curv_stencil_kernel that differs from optimize.curvature_stencil's order moves another coordinate than the rule differences, and
    dlog / grad / hess leave the floor; the llk differences hold the Hessian to an independent path.  Every point must have status 0.
    Checked with the project's oracle (OracleModel, CPU) before any device run: at these points the likelihood is finite at both
    centres of the 16-parameter model under true_eps (under cpfit this structure may lose its correction: test_gpu_limits.py), and at
    all 99 stencil candidates of the 4-parameter model under cpfit + smooth."""
    from misti_amd.engine import Engine
    bands, pulses, D, flags, x0, P = WIDE_MODELS[name]
    inp = grid()
    x, splits, rows = wide_points(name)
    e = Engine(inp.times, inp.lambdas, bands, pulses, n_param=D, **flags)
    driver_comparison(name, e, D, False, x, splits, rows, None, table)


# ---- 4. more points than one scan run --------------------------------------------------------------------------------------------------
def test_slots_of_600_points_with_boundary_points_among_them(table):
    """one_band_cpfit (D = 1, M = 3), 600 points, every seventh a rate of 0.0 under a purely relative step: curv_slots_kernel gives
    each thread a run of 3 points with live and boundary points mixed inside it.  Boundary points: MISTI_CURV_BOUNDARY and NaN
    throughout.  Every other point: bit for bit the same point computed in calls of 200 points, where a run is one point - a wrong
    run boundary hands a point the spectra of a neighbour, whose rate differs."""
    e, D, split, x0, unfolded = model_engine("one_band_cpfit")
    P = 600
    x, splits, rows, _ = points_of("one_band_cpfit", P, np.random.default_rng(13))
    boundary = np.arange(P) % 7 == 3
    x[boundary] = 0.0
    assert len(np.unique(x[~boundary])) == (~boundary).sum()
    with e:
        whole = e.curvature(x, splits, rows, table, abs_step=0.0)
        parts = [e.curvature(x[a:a + 200], splits[a:a + 200], rows[a:a + 200], table, abs_step=0.0) for a in range(0, P, 200)]
    assert (whole.status[boundary] == 7).all() and (whole.status[~boundary] == 0).all()
    for k in FIELDS:
        got, ref = getattr(whole, k), np.concatenate([getattr(p, k) for p in parts])
        if k != "status":
            assert np.isnan(got[boundary]).all() and np.isfinite(got[~boundary]).all(), k
        assert same_bits(got[~boundary], ref[~boundary]), k
    assert len(np.unique(whole.llh0[~boundary])) > 0.9 * (~boundary).sum()
