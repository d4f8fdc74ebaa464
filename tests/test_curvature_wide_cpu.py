"""The NumPy curvature rule (optimize.curvature_from_spectra, curvature_contract) against analytic derivatives at D = 4, 5, 8 and 16,
the part that needs no GPU: class logs that are exact quadratics of the parameters (tests/curvature_wide.py), whose central
differences are exact whatever the steps.  The device is held to the same values under the same floor in
tests/test_gpu_curvature_wide.py; this module is the condition that the reference alone stays inside it - and it is where a slip
in the rule's own pair order, which the kernel shares by construction, would show."""
import numpy as np
import pytest

import curvature_wide as cw

WIDTHS = (4, 5, 8, 16)


@pytest.mark.parametrize("unfolded", [False, True], ids=["folded", "unfolded"])
@pytest.mark.parametrize("D", WIDTHS)
def test_rule_equals_the_analytic_derivatives_of_quadratic_class_logs(D, unfolded):
    from misti_amd.optimize import curvature_contract, curvature_from_spectra
    case = cw.quadratic_case(D, unfolded, 300 + 10 * D + unfolded)
    rng = np.random.default_rng(7)
    table = cw.counts(rng, 6)
    rows = rng.integers(0, 6, size=case["x"].shape[0]).astype(np.int32)
    dlog, d2log, pst = curvature_from_spectra(case["jafs"], None, case["h"], unfolded)
    grad, hess = curvature_contract(dlog, d2log, table, rows, unfolded)
    assert (pst == 0).all()
    want = cw.analytic(case, table, rows, unfolded)
    tol = cw.floors(case["jafs"], case["h"], unfolded, table, rows)
    print("D = %d: stencil |L| from %.3g to %.3g" % (D, np.abs(case["L"]).min(), np.abs(case["L"]).max()))
    for name, got in (("dlog", dlog), ("d2log", d2log), ("grad", grad), ("hess", hess)):
        worst = cw.worst_ratio(got, want[name], tol[name])
        print("rule against analytic", name, D, "unfolded" if unfolded else "folded", "largest error / floor = %.3g" % worst)
        assert np.isfinite(got).all() and worst <= 1.0, (name, D, unfolded, worst)
    # the analytic values are not within the floor of zero, nor of each other across a transposition of the pair order: a wrong
    # pair rank or a mirrored store would be far outside
    assert (np.abs(want["d2log"][..., :case["K"]]) > 1e3 * tol["d2log"][..., :case["K"]]).mean() > 0.9
    if not unfolded:
        assert (dlog[..., 4:] == 0).all() and (d2log[..., 4:] == 0).all()


def test_some_stencil_log_is_below_one():
    """The max(|L|, 1) of the floor is exercised: among the cases above there are stencil logs below 1 in magnitude."""
    assert any(np.abs(cw.quadratic_case(D, u, 300 + 10 * D + u)["L"]).min() < 1.0 for D in WIDTHS for u in (False, True))
