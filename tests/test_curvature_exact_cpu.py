"""The curvature rule against exact derivatives of the model's own spectrum, the part that needs no GPU
(tests/golden/golden_curvature_exact.json.gz, made by tests/golden/make_curvature_exact.py; bounds in tests/curvature_exact.py).

 1. The fixture is what it says: its stencils are optimize.curvature_stencil's bit for bit, it covers the cases the GPU test relies
    on, and its exact standard errors are those optimize's own functions give from its exact derivatives.
 2. TRUNCATION: the rule applied in 50-digit arithmetic ("the exact stencil") against the derivative itself - the error falls
    monotonically down the ladder of relative steps for every output.
 3. The float64 rule (optimize.curvature_from_spectra / curvature_contract) fed the exact spectra rounded to double meets the bound
    the device is held to (tests/test_gpu_curvature_exact.py).
 4. What the default step costs is printed, not asserted (lines `curvature_exact truncation ...`; profiles/curvature_exact.txt)."""
import numpy as np
import pytest

import curvature_exact as cx

FX = cx.load()
POINTS = cx.points(FX)
IDS = ["%s-%s" % (m["name"], p["name"]) for m, p in POINTS]
OUTPUTS = ("dlog", "d2log", "grad", "hess")


def _stencil_strings(p, s, unfolded):
    """The exact stencil of one step as decimal strings, grad and hess (row 0 of the point's table) included."""
    return dict(dlog=s["dlog"], d2log=s["d2log"], grad=cx.exact_contract(s["dlog"], p["table"][0], unfolded),
                hess=cx.exact_contract(s["d2log"], p["table"][0], unfolded))


def test_fixture_is_the_rule_s_stencil_and_covers_the_cases():
    from misti_amd.optimize import curvature_size, curvature_stencil
    kinds = set()
    for m in FX["models"]:
        assert 4 <= len(m["lh"]) <= 6
        for p in m["points"]:
            two_pop = int(p["split"]) + (1 if p["split"] % 1 else 0)
            assert 1 <= two_pop <= 3 and len(p["x"]) == m["n_param"]
            if p["boundary"]:
                _, _, b = curvature_stencil(p["x"], cx.DEFAULT_STEP, p["abs_step"])
                assert b.all() and "steps" not in p
                kinds.add("boundary")
                continue
            for s in p["steps"]:
                pts, h, b = curvature_stencil(p["x"], s["rel_step"], p["abs_step"])
                assert not b.any() and np.array_equal(pts[0], np.array(s["stencil"])) and np.array_equal(h[0], np.array(s["h"]))
                assert len(s["jafs"]) == curvature_size(m["n_param"])
                if "q" in s:
                    assert s["q"][0] <= FX["q_switch"] < max(s["q"][1:])
                    kinds.add("straddle")
            if p["abs_step"] == 0:
                assert p["tiny_rate"] or [s["rel_step"] for s in p["steps"]] in (list(cx.LADDER), [1e-1, 1e-2, 1e-3, 1e-4])
            else:
                lo = np.array(p["steps"][0]["stencil"])[:, 0].min()
                assert 0 < lo < 1e-3 * p["steps"][0]["h"][0]           # one step from the boundary: x - h slightly above 0
                kinds.add("one_step_inside")
            kinds.add("unfolded" if m["unfolded"] else "folded")
            kinds |= {"D3_pulse"} if m["n_param"] == 3 and m["pulses"] else set()
            kinds |= {"ancient"} if m["sample_date"] >= 1 else set()
            kinds |= {"fractional"} if p["split"] % 1 else set()
            kinds |= {"tiny"} if min(p["x"]) == 1e-6 and p["tiny_rate"] else set()
    assert kinds == {"boundary", "straddle", "one_step_inside", "unfolded", "folded", "D3_pulse", "ancient", "fractional", "tiny"}


@pytest.mark.parametrize("mp_", POINTS, ids=IDS)
def test_exact_standard_errors_are_those_of_the_project_s_functions(mp_):
    """The fixture's standard errors were formed in 80-digit arithmetic from the definitions; optimize's functions, given the exact
    derivatives rounded to double, must give them to cond(H) x a few ulps."""
    m, p = mp_
    ex = p["exact"]
    H, A = cx.arr(ex["hess"]), cx.pad7(cx.arr(ex["dlog"]))
    obs, sand = cx.standard_errors(H, A, np.array(p["table"], dtype=np.float64), m["unfolded"])
    room = 64 * np.finfo(float).eps * np.linalg.cond(H)
    assert cx.rel_diff(obs, cx.arr(ex["se_observed"])) <= room and cx.rel_diff(sand, cx.arr(ex["se_sandwich"])) <= room
    # and the Hessian is one: negative definite, so the point has standard errors at all
    assert (np.linalg.eigvalsh(H) < 0).all()


@pytest.mark.parametrize("mp_", POINTS, ids=IDS)
def test_truncation_falls_monotonically_down_the_ladder(mp_):
    """Every entry of every output, strictly, at every step: in exact arithmetic the rule has nothing but truncation, c2 h^2 + c4 h^4.
    That holds because the step is the realised one (optimize.curvature_stencil: x + h and x - h are exact doubles).  With the nominal
    step max(rel |x|, abs) the rounding of x +- h leaves ulp(x) |dL| / h^2 in a second difference, which grows as h falls - e.g. 2e-6
    |dL| at x = 0.5, rel_step 1e-5 - and this test is what found it."""
    m, p = mp_
    exact = _stencil_strings(p, p["exact"], m["unfolded"])
    errs = {k: [] for k in OUTPUTS}
    for s in p["steps"]:
        got = _stencil_strings(p, s, m["unfolded"])
        for k in OUTPUTS:
            errs[k].append(np.abs(cx.exact_diff(got[k], exact[k])))
    for k in OUTPUTS:
        for a, b in zip(errs[k], errs[k][1:]):
            assert (b < a).all(), (m["name"], p["name"], k, a, b)


@pytest.mark.parametrize("mp_", POINTS, ids=IDS)
def test_float64_rule_on_rounded_exact_spectra_meets_the_derived_bound(mp_):
    from misti_amd.optimize import curvature_contract, curvature_from_spectra
    m, p = mp_
    unf = m["unfolded"]
    table = np.array(p["table"], dtype=np.float64)
    for s in p["steps"]:
        jafs, h = cx.arr(s["jafs"]), np.array(s["h"])
        dlog, d2log, st = curvature_from_spectra(jafs[None], None, h[None], unf)
        grad, hess = curvature_contract(dlog, d2log, table, [0], unf)
        want = _stencil_strings(p, s, unf)
        b = cx.bounds(jafs, h, unf, table[0])
        assert st[0] == 0
        for k, got in (("dlog", dlog[0]), ("d2log", d2log[0]), ("grad", grad[0]), ("hess", hess[0])):
            w = cx.arr(want[k])
            w = cx.pad7(w) if k in ("dlog", "d2log") else w
            err = np.abs(got - w)
            assert (err <= b[k]).all(), (m["name"], p["name"], s["rel_step"], k, float((err / b[k])[b[k] > 0].max()))


def test_report_the_truncation_of_the_default_step():
    """Not an assertion: what DESIGN.md section 4 called unmeasured.  Per point, the error of the exact stencil at rel_step 1e-2
    against the exact derivative - largest over the entries, relative to the largest exact entry - and the relative error it causes
    in every standard error; then, per ladder step, the same for the Hessian and the standard errors."""
    for m, p in POINTS:
        unf = m["unfolded"]
        table = np.array(p["table"], dtype=np.float64)
        exact = _stencil_strings(p, p["exact"], unf)
        se_obs, se_sand = cx.arr(p["exact"]["se_observed"]), cx.arr(p["exact"]["se_sandwich"])
        for s in p["steps"]:
            got = _stencil_strings(p, s, unf)
            rel = {k: float(np.abs(cx.exact_diff(got[k], exact[k])).max() / np.abs(cx.arr(exact[k])).max()) for k in OUTPUTS}
            obs, sand = cx.standard_errors(cx.arr(got["hess"]), cx.pad7(cx.arr(s["dlog"])), table, unf)
            print("curvature_exact truncation %-16s %-15s rel_step %-7g%s dlog %.2e d2log %.2e grad %.2e hess %.2e  se_observed %.2e se_sandwich %.2e"
                  % (m["name"], p["name"], s["rel_step"], " (default)" if s["rel_step"] == cx.DEFAULT_STEP else "          ",
                     rel["dlog"], rel["d2log"], rel["grad"], rel["hess"], cx.rel_diff(obs, se_obs), cx.rel_diff(sand, se_sand)))
