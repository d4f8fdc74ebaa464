"""What the CPU and the GPU test of the curvature against exact derivatives share (tests/golden/golden_curvature_exact.json.gz, made by
tests/golden/make_curvature_exact.py): the fixture's reader, the DERIVED bound of a difference quotient of class logs whose spectra
are only as good as tests/test_gpu_exact_spectrum.py holds them, and the standard errors with their first-order perturbation bound.

The bound.  test_gpu_exact_spectrum.py holds every normalised class of the device to |dS_c| <= RTOL S_c + ATOL sum(S).  A class the
likelihood distinguishes is the sum of n_k raw classes (folded 2, 2, 2, 1; unfolded 1 each), so its log is off by at most

    e_k = (RTOL S_k + n_k ATOL sum(S)) / S_k

and a difference quotient of such logs by the sum of the e of its terms over its denominator:

    dL/dx_i       (e(+i) + e(-i)) / 2 h_i
    d2L/dx_i^2    (e(+i) + 2 e(0) + e(-i)) / h_i^2
    d2L/dx_i dx_j (e(++) + e(+-) + e(-+) + e(--)) / 4 h_i h_j

to which the rounding floor of tests/test_gpu_curvature.py is added (FLOOR_ULPS EPS sum |terms|: the device's log and the
quotient's own operations).  grad and hess take the same bound contracted with the absolute class counts of the row.  Nothing here is
fitted to what a device returns."""
import decimal
import gzip
import json
import os

import numpy as np

from parity import EPS, FLOOR_ULPS
from test_gpu_exact_spectrum import ATOL, RTOL

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_curvature_exact.json.gz")
LADDER = (1e-1, 3e-2, 1e-2, 1e-3, 1e-4, 1e-5)
DEFAULT_STEP = 1e-2
SE_BOUND_APPLIES = 0.1          # the perturbation bound is first order: applied only where it is below this


def load():
    with gzip.open(FIXTURE, "rt") as f:
        return json.load(f)


def arr(v):
    """Nested lists of decimal strings (or numbers) as float64, each string correctly rounded."""
    return np.array(v, dtype=object).astype(np.float64)


def pad7(a):
    """Class axis (the last) padded with zeros to 7, as the device lays folded outputs out."""
    a = np.asarray(a, dtype=np.float64)
    out = np.zeros(a.shape[:-1] + (7,))
    out[..., :a.shape[-1]] = a
    return out


def log_error(jafs, unfolded):
    """e_k of every class of the spectra ``jafs[...][7]`` (the exact ones, rounded): ``[...][K]``."""
    from misti_amd.optimize import _class_values
    jafs = np.asarray(jafs, dtype=np.float64)
    S = _class_values(jafs, unfolded)
    n = np.ones(7) if unfolded else np.array([2.0, 2.0, 2.0, 1.0])
    return (RTOL * S + n * ATOL * jafs.sum(axis=-1, keepdims=True)) / S


def _quotients(t, h):
    """The three quotients' sums of per-candidate terms ``t[M][K]`` (all taken with a plus sign): ``(first[D][7], second[D][D][7])``."""
    h = np.asarray(h, dtype=np.float64)
    D = h.shape[0]
    K = t.shape[-1]
    first, second = np.zeros((D, 7)), np.zeros((D, D, 7))
    q = 0
    for i in range(D):
        first[i, :K] = (t[1 + 2 * i] + t[2 + 2 * i]) / (2 * h[i])
        second[i, i, :K] = (t[1 + 2 * i] + 2 * t[0] + t[2 + 2 * i]) / (h[i] * h[i])
        for j in range(i + 1, D):
            c = 1 + 2 * D + 4 * q
            second[i, j, :K] = second[j, i, :K] = t[c:c + 4].sum(axis=0) / (4 * h[i] * h[j])
            q += 1
    return first, second


def bounds(jafs, h, unfolded, row=None):
    """The derived bound plus the rounding floor for one point: ``jafs[M][7]`` the exact spectra of its stencil, ``h[D]``.
    dict(dlog[D][7], d2log[D][D][7], derived_d2log (without the floor)) and, with the point's ``row[8]``, grad[D] and hess[D][D]."""
    from misti_amd.optimize import _class_values, class_counts
    jafs = np.asarray(jafs, dtype=np.float64)
    e1, e2 = _quotients(log_error(jafs, unfolded), h)
    f1, f2 = _quotients(np.abs(np.log(_class_values(jafs, unfolded))), h)
    out = dict(dlog=e1 + FLOOR_ULPS * EPS * f1, d2log=e2 + FLOOR_ULPS * EPS * f2, derived_d2log=e2)
    if row is not None:
        f = np.abs(class_counts(np.asarray(row, dtype=np.float64).reshape(1, 8), unfolded)[0])
        out["grad"] = out["dlog"] @ f
        out["hess"] = out["d2log"] @ f
    return out


def se_bound(hess, d_hess):
    """First-order bound on the relative change of the inverse of ``hess`` under a perturbation within ``d_hess`` entry by entry:
    cond(H) |dH| / |H| (spectral norms; that of the perturbation is bounded by the Frobenius norm of the entry bounds)."""
    s = np.linalg.svd(np.asarray(hess, dtype=np.float64), compute_uv=False)
    return float(s[0] / s[-1] * np.linalg.norm(d_hess) / s[0])


def standard_errors(hess, dlog, table, unfolded):
    """(observed, sandwich) standard errors ``[D]`` of one point from its Hessian, its class-log derivatives ``dlog[D][7]`` and its
    count table (row 0 the data, the others the replicates): misti_amd.optimize's own functions."""
    from misti_amd import optimize as opt
    obs = opt.standard_errors(opt.observed_covariance(hess)["cov"][0])
    sand = opt.standard_errors(opt.sandwich_covariance(hess, dlog, table, unfolded=unfolded)[0])
    return obs, sand


def rel_diff(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def points(fx, with_boundary=False):
    """(model, point) pairs of the fixture; boundary points (no stencil, nothing but a status to hold) only on request."""
    return [(m, p) for m in fx["models"] for p in m["points"] if with_boundary or not p["boundary"]]


# ---- decimal strings: differences and contractions without a rounding of the operands ---------------------------------------------------
def _walk(f, *nested):
    if isinstance(nested[0], str):
        return f(*nested)
    return [_walk(f, *sub) for sub in zip(*nested)]


def exact_diff(a, b):
    """``a - b`` of two equally nested lists of decimal strings, formed in 60-digit decimal arithmetic and rounded once: float64."""
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        return np.array(_walk(lambda u, v: float(decimal.Decimal(u) - decimal.Decimal(v)), a, b), dtype=np.float64)


def exact_contract(d, row, unfolded):
    """``sum_k f_k d[...][k]`` with the class counts ``f`` of ``row[8]`` (integers) over nested decimal strings whose innermost lists
    run over the classes; decimal strings of one nesting level less."""
    from misti_amd.optimize import class_counts
    f = [decimal.Decimal(int(v)) for v in class_counts(np.asarray(row, dtype=np.float64).reshape(1, 8), unfolded)[0]]

    def go(v):
        if isinstance(v[0], str):
            return str(sum(fk * decimal.Decimal(s) for fk, s in zip(f, v)))
        return [go(s) for s in v]
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        return go(d)
