"""The curvature rule as stated in NumPy (optimize.curvature_stencil, curvature_from_spectra, curvature_contract), the covariances
built on it (observed_covariance, sandwich_covariance, standard_errors), the header's two entries and the `--se` refusals.  No GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the stencil -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 3])
def test_stencil_order_and_count(D):
    from misti_amd.optimize import curvature_size, curvature_stencil
    x = np.array([[0.5, 2.0, 8.0][:D], [1.0, 3.0, 0.25][:D]])
    pts, h, boundary = curvature_stencil(x, 1e-2, 0.0)
    M = 1 + 2 * D * D
    assert curvature_size(D) == M and pts.shape == (2, M, D) and h.shape == (2, D) and not boundary.any()
    assert same_bits(h, (x + 1e-2 * np.abs(x)) - x) and (np.abs(h - 1e-2 * x) <= np.spacing(x) / 2).all()
    assert same_bits(pts[:, 1, 0] - x[:, 0], h[:, 0]) and same_bits(x[:, 0] - pts[:, 2, 0], h[:, 0])     # the realised step, exactly
    for p in range(2):
        want = [list(x[p])]
        for i in range(D):
            for s in (+1, -1):
                v = list(x[p])
                v[i] = x[p, i] + h[p, i] if s > 0 else x[p, i] - h[p, i]
                want.append(v)
        for i in range(D):
            for j in range(i + 1, D):
                for si, sj in ((+1, +1), (+1, -1), (-1, +1), (-1, -1)):
                    v = list(x[p])
                    v[i] = x[p, i] + h[p, i] if si > 0 else x[p, i] - h[p, i]
                    v[j] = x[p, j] + h[p, j] if sj > 0 else x[p, j] - h[p, j]
                    want.append(v)
        assert len(want) == M and same_bits(pts[p], np.array(want))
    # the absolute step wins where it is the larger one; a single point may come as a vector
    pts1, h1, b1 = curvature_stencil(x[0], 1e-2, 0.01)
    assert pts1.shape == (1, M, D) and same_bits(h1[0], (x[0] + np.maximum(1e-2 * x[0], 0.01)) - x[0]) and not b1[0]


def test_stencil_boundary_rule():
    from misti_amd.optimize import curvature_stencil
    h0 = 1e-3
    x = np.array([[0.0, 1.0],           # a rate fitted to 0: x - h < 0
                  [h0 / 2, 1.0],        # inside the step: x - h < 0
                  [h0, 1.0],            # x - h == 0: a two-sided stencil that touches 0
                  [1.0, 1.0]])
    pts, h, boundary = curvature_stencil(x, 0.0, h0)
    assert list(boundary) == [True, True, False, False] and (h[:3, 0] == h0).all() and (np.abs(h - h0) <= np.spacing(x) / 2).all()
    assert pts[2, 2, 0] == 0.0
    # under a purely relative step a rate of 0 has no step at all: a boundary point as well; any other positive rate has a stencil
    _, h, boundary = curvature_stencil(x, 1e-2, 0.0)
    assert list(boundary) == [True, False, False, False] and h[0, 0] == 0.0
    _, _, boundary = curvature_stencil([[-0.1, 1.0]], 1e-2, 0.0)
    assert boundary[0]
    for rel, ab in ((0.0, 0.0), (-1e-2, 1e-3), (1e-2, -1.0), (np.nan, 0.0), (np.inf, 0.0), (1e-2, np.inf)):
        with pytest.raises(ValueError):
            curvature_stencil(x, rel, ab)
    with pytest.raises(ValueError):
        curvature_stencil([[np.nan, 1.0]], 1e-2, 0.0)


# ---- the rule on an analytic spectrum --------------------------------------------------------------------------------------------------
class Softmax:
    """S(theta) = softmax(a + B theta + theta^T C theta) over 7 classes, with the closed-form derivatives of log S_k (unfolded) or of
    the logs of the folded class values."""

    def __init__(self, D, seed):
        rng = np.random.default_rng(seed)
        self.D = D
        self.a = rng.normal(size=7)
        self.B = rng.normal(size=(7, D))
        C = rng.normal(size=(7, D, D)) * 0.5
        self.C = C + np.swapaxes(C, 1, 2)

    def spectrum(self, th):
        z = self.a + self.B @ th + np.einsum("i,kij,j->k", th, self.C, th)
        e = np.exp(z - z.max())
        return e / e.sum()

    def derivs(self, th, unfolded):
        """dlog[D][K], d2log[D][D][K] of the logs of the class values."""
        S = self.spectrum(th)
        dz = self.B + 2 * np.einsum("kij,j->ki", self.C, th)             # [7][D]
        d2z = 2 * self.C                                                 # [7][D][D]
        mean = S @ dz
        dS = S[:, None] * (dz - mean)                                    # [7][D]
        d2mean = np.einsum("ki,kj->ij", dS, dz) + np.einsum("k,kij->ij", S, d2z)
        d2S = dS[:, :, None] * (dz - mean)[:, None, :] + S[:, None, None] * (d2z - d2mean)
        fold = np.eye(7) if unfolded else np.array([[1, 0, 0, 0, 0, 0, 1], [0, 1, 0, 0, 0, 1, 0], [0, 0, 1, 0, 1, 0, 0], [0, 0, 0, 1, 0, 0, 0]], dtype=float)
        V, dV, d2V = fold @ S, fold @ dS, np.einsum("ck,kij->cij", fold, d2S)
        dlog = dV / V[:, None]
        d2log = d2V / V[:, None, None] - dlog[:, :, None] * dlog[:, None, :]
        return dlog.T, np.moveaxis(d2log, 0, -1)


@pytest.mark.parametrize("unfolded", [False, True], ids=["folded", "unfolded"])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_rule_is_second_order_on_an_analytic_spectrum(D, unfolded):
    """The error against the closed form shrinks by 4 +- 25 % when h halves.  Step sizes are chosen so that truncation dominates
    rounding, and that is checked here: the rounding of a second difference is at most ~ 4 ulp(|L|) / h^2, and the observed error at
    the smaller step must be 100 times that."""
    from misti_amd.optimize import curvature_from_spectra, curvature_stencil
    model = Softmax(D, 5 + D)
    theta = np.full(D, 0.7) + 0.1 * np.arange(D)
    K = 7 if unfolded else 4
    want1, want2 = model.derivs(theta, unfolded)
    errs = []
    for step in (2e-2, 1e-2):
        pts, h, boundary = curvature_stencil(theta, step, 0.0)
        jafs = np.array([[model.spectrum(t) for t in pts[0]]])
        dlog, d2log, status = curvature_from_spectra(jafs, None, h, unfolded)
        assert status[0] == 0 and not boundary[0]
        assert same_bits(d2log, np.swapaxes(d2log, 1, 2))                  # the Hessian is bitwise symmetric
        if not unfolded:
            assert (dlog[..., 4:] == 0).all() and (d2log[..., 4:] == 0).all()
        errs.append((np.abs(dlog[0, :, :K] - want1), np.abs(d2log[0, :, :, :K] - want2), h[0]))
    (e1a, e2a, ha), (e1b, e2b, hb) = errs
    L = np.abs(np.log(jafs)).max()
    rounding1 = 4 * np.finfo(float).eps * L / hb.min()
    rounding2 = 8 * np.finfo(float).eps * L / hb.min() ** 2
    assert (e1b > 100 * rounding1).all() and (e2b > 100 * rounding2).all(), "truncation must dominate rounding at these steps"
    r1, r2 = e1a / e1b, e2a / e2b
    print("error ratios when h halves: dlog %.3f ... %.3f, d2log %.3f ... %.3f" % (r1.min(), r1.max(), r2.min(), r2.max()))
    assert (np.abs(r1 - 4) <= 1).all() and (np.abs(r2 - 4) <= 1).all()


def test_a_failed_candidate_poisons_only_its_point_with_the_first_status():
    from misti_amd.optimize import curvature_contract, curvature_from_spectra, curvature_size
    rng = np.random.default_rng(3)
    D, P = 2, 5
    M = curvature_size(D)
    jafs = rng.random((P, M, 7)) + 0.05
    h = np.full((P, D), 1e-2)
    clean = curvature_from_spectra(jafs, None, h, False)
    status = np.zeros((P, M), dtype=np.int32)
    status[1, 7], status[1, 3] = 2, 6                  # the first in stencil order: candidate 3
    bad = jafs.copy()
    bad[2, 4, 3] = 0.0                                 # a class value of 0: MISTI_NUMERIC
    bad[3, 5, 1] = np.nan
    status[3, 8] = 4                                   # ... behind the NaN of candidate 5: still NUMERIC
    bad[4, 0, 0], bad[4, 0, 6] = -1.0, 0.5             # a folded class value that is negative
    dlog, d2log, pst = curvature_from_spectra(bad, status, h, False)
    assert list(pst) == [0, 6, 5, 5, 5] and list(clean[2]) == [0] * P
    assert np.isnan(dlog[1:]).all() and np.isnan(d2log[1:]).all()
    assert same_bits(dlog[0], clean[0][0]) and same_bits(d2log[0], clean[1][0])
    # unfolded, class 0 and 6 stand alone: 0.5 is fine, -1 is not
    assert list(curvature_from_spectra(bad[4:], None, h[4:], True)[2]) == [5]
    table = np.zeros((3, 8))
    table[:, 1:] = rng.integers(1, 1000, size=(3, 7))
    grad, hess = curvature_contract(dlog, d2log, table, [0, 1, 2, 0, 1], False)
    assert np.isnan(grad[1:]).all() and np.isnan(hess[1:]).all() and np.isfinite(grad[0]).all() and np.isfinite(hess[0]).all()
    assert same_bits(hess, np.swapaxes(hess, 1, 2))


# ---- covariances -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unfolded", [False, True], ids=["folded", "unfolded"])
def test_score_covariance_is_the_covariance_of_explicit_scores(unfolded):
    from misti_amd.optimize import class_counts, sandwich_covariance, score_covariance
    rng = np.random.default_rng(17)
    P, D, R = 3, 2, 12
    dlog = rng.normal(size=(P, D, 7))
    if not unfolded:
        dlog[..., 4:] = 0.0
    table = np.zeros((R, 8))
    table[:, 1:] = rng.integers(1000, 60000, size=(R, 7))
    table[:, 0] = table[:, 1:].sum(axis=1)
    got = score_covariance(dlog, table, unfolded=unfolded)
    f = class_counts(table[1:], unfolded)
    for p in range(P):
        scores = f @ dlog[p].T                                           # [R - 1][D]: the score of every bootstrap row
        want = np.atleast_2d(np.cov(scores, rowvar=False, ddof=1))
        scale = np.abs(f).sum(axis=1).max() ** 2 * np.abs(dlog[p]).max() ** 2
        assert np.abs(got[p] - want).max() <= 64 * np.finfo(float).eps * scale
    # the sandwich with H = -I is the score covariance itself; a singular or NaN Hessian gives NaN for that point alone
    H = np.tile(-np.eye(D), (P, 1, 1))
    H[1] = [[1.0, 2.0], [2.0, 4.0]]
    H[2, 0, 0] = np.nan
    sw = sandwich_covariance(H, dlog, table, unfolded=unfolded)
    assert np.allclose(sw[0], got[0], rtol=1e-13, atol=0) and np.isnan(sw[2]).all()
    assert np.isnan(sw[1]).all() or np.abs(sw[1]).max() > 1e20            # (LAPACK may return a huge inverse for an exactly singular H)
    with pytest.raises(ValueError):
        score_covariance(dlog, table[:2], unfolded=unfolded)


def test_observed_covariance_flags_an_indefinite_hessian():
    from misti_amd.optimize import correlation, observed_covariance, standard_errors
    H = np.array([[[-4.0, 1.0], [1.0, -2.0]],          # a maximum
                  [[-4.0, 0.0], [0.0, 2.0]],           # a saddle
                  [[-4.0, 2.0], [2.0, -1.0]],          # a flat direction: -H singular
                  [[np.nan, 0.0], [0.0, -1.0]]])
    r = observed_covariance(H)
    assert list(r["ok"]) == [True, False, False, False]
    assert np.allclose(r["cov"][0], np.linalg.inv(-H[0])) and np.isnan(r["cov"][1:]).all()
    w = np.linalg.eigvalsh(-H[0])
    assert r["cond"][0] == pytest.approx(w[-1] / w[0]) and np.isinf(r["cond"][1]) and np.isinf(r["cond"][2]) and np.isnan(r["cond"][3])
    se = standard_errors(r["cov"])
    assert np.allclose(se[0], np.sqrt(np.diag(np.linalg.inv(-H[0])))) and np.isnan(se[1:]).all()
    c = correlation(r["cov"][0])
    assert np.allclose(np.diag(c), 1.0) and c[0, 1] == pytest.approx(1 / np.sqrt(8))
    one = observed_covariance(H[0])                    # a single matrix
    assert one["cov"].shape == (1, 2, 2) and one["ok"][0]
    assert np.isnan(standard_errors(np.array([[-1.0]]))).all()


# ---- the header and the binding ------------------------------------------------------------------------------------------------------
def test_header_keeps_abi_6_and_declares_the_two_entries():
    from misti_amd import _lib
    text = open(os.path.join(ROOT, "include", "misti_hip.h")).read()
    assert re.search(r"^#define MISTI_ABI_VERSION 6$", text, flags=re.M) and _lib.ABI_VERSION == 6
    assert re.search(r"^#define MISTI_CURV_BOUNDARY 7\b", text, flags=re.M) and _lib.CURV_BOUNDARY == 7
    for name, n_args in (("misti_curvature_assemble_dev", 13), ("misti_curvature", 17)):
        m = re.search(r"^int %s\(([^;]*)\);" % name, text, flags=re.M)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_lib.SYMBOLS[name][1]), name
    api = open(os.path.join(ROOT, "misti_amd", "csrc", "misti_curv.cpp")).read()
    assert "int misti_curvature(" in api and "int misti_curvature_assemble_dev(" in api


# ---- the command line: --se refusals ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra, word", [
    (["--grid-solve", "--grid-st", "18", "20", "--se", "--gpus", "2"], "--gpus"),
    (["--grid-solve", "--grid-st", "18", "20", "--se", "--devices", "0,1"], "--devices"),
    (["--fit-st", "--grid-st", "18", "20", "--se"], "--fit-st"),
    (["--grid-solve", "--grid-st", "18", "20", "--hops", "2", "--se"], "--hops"),
    (["--grid-st", "18", "20", "--se"], "--grid-solve"),
    (["--grid-st", "18", "20", "--top", "2", "--se"], "--grid-solve"),
    (["--grid-solve", "--grid-st", "18", "20", "--se-step", "1e-3"], "--se"),
    (["--grid-solve", "--grid-st", "18", "20", "--se", "--se-step", "0"], "--se-step"),
    (["--grid-solve", "--grid-st", "18", "20", "--se", "--se-step", "nan"], "--se-step"),
    (["--se", "--sweep", "t", "3", "4"], "--sweep"),
])
def test_se_refusals(extra, word, capsys):
    """Refused before any file is read or the GPU is touched: the input files do not exist."""
    from misti_amd import cli
    rc = cli.main(["no1.psmc", "no2.psmc", "no.sfs", "20", "-mi", "1", "2", "20", "0.1", "1"] + extra)
    err = capsys.readouterr().err
    assert rc == 2 and "--se" in err and word in err, err


def test_se_needs_an_optimised_parameter(capsys):
    from misti_amd import cli
    rc = cli.main(["no1.psmc", "no2.psmc", "no.sfs", "20", "-mi", "1", "2", "20", "0.1", "0", "--se"])
    assert rc == 2 and "optimised parameter" in capsys.readouterr().err
    assert cli.se_error(cli.build_parser().parse_args(["a", "b", "c", "20", "-mi", "1", "2", "20", "0.1", "1", "--se"])) is None
    assert cli.se_error(cli.build_parser().parse_args(["a", "b", "c", "20", "-mi", "1", "2", "20", "0.1", "1", "--grid-solve", "--all-bs", "--se",
                                                       "--se-step", "5e-3"])) is None
