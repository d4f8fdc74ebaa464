"""An analytic reference for the curvature rule at any width (tests/test_curvature_wide_cpu.py, tests/test_gpu_curvature_wide.py).

The NumPy rule (optimize.curvature_from_spectra) is worded after the kernel, operation for operation, so a slip both share - a pair
rank, a stencil index - is invisible to a comparison of the two.  Here the class logs are EXACT QUADRATICS of the parameters,

    L_k(x) = 1/2 x^T A_k x + b_k^T x + c_k          A_k symmetric,

whose central differences over optimize.curvature_stencil's points are A_k x + b_k and A_k exactly, whatever the steps (the stencil's
abscissae x +- h are exact doubles).  The spectra are J[..., k] = exp(L_k) evaluated in numpy.longdouble and rounded to double, so
what separates the rule - or the device - from the analytic values is the rounding of exp and of log alone.

The tolerance is the floor of tests/test_gpu_curvature.py (rule()): FLOOR_ULPS x EPS x the sum of the absolute elementary terms of an
output, with every |L| replaced by max(|L|, 1): rounding exp(L) to a double moves log S by up to an ulp of 1, not of |L|, when
|L| < 1.  (The contraction's own roundings, at most 7 EPS sum_k f_k |d_k|, are far inside it: a first derivative is at most 3 and
its terms are at least 1 / h >= 50, a second derivative is below 1 and its terms are at least 4 / h^2.)"""
import numpy as np

from parity import EPS, FLOOR_ULPS

LD = np.longdouble
REL_STEP = 1e-2


def quadratic_case(D, unfolded, seed, P=5):
    """P points with x in [0.05, 2], their stencil, the spectra of the quadratic class logs (K = 7 unfolded; K = 4 folded with
    classes 4 to 6 at 0.0, so that the folded class values are J_0 ... J_3 themselves) and the analytic derivatives, rounded to
    double from longdouble.  A_k = (U + U^T) / 2D and b_k = U / sqrt(D) with U uniform in [-1, 1] keep |L| of order 1 ... 10 at
    every width; c_k in [-6, -1]."""
    from misti_amd.optimize import curvature_size, curvature_stencil
    assert np.finfo(LD).eps <= 2.0 ** -63, "the reference needs a long double wider than the double it is rounded to"
    rng = np.random.default_rng(seed)
    K = 7 if unfolded else 4
    U = rng.uniform(-1.0, 1.0, size=(K, D, D))
    A = ((U + U.transpose(0, 2, 1)) / (2.0 * D)).astype(LD)
    b = (rng.uniform(-1.0, 1.0, size=(K, D)) / np.sqrt(D)).astype(LD)
    c = rng.uniform(-6.0, -1.0, size=K).astype(LD)
    x = rng.uniform(0.05, 2.0, size=(P, D))
    pts, h, boundary = curvature_stencil(x, REL_STEP, 0.0)
    assert not boundary.any() and pts.shape == (P, curvature_size(D), D)
    z = pts.astype(LD)
    L = 0.5 * np.einsum("pmi,kij,pmj->pmk", z, A, z) + np.einsum("pmi,ki->pmk", z, b) + c
    jafs = np.zeros(pts.shape[:2] + (7,))
    jafs[..., :K] = np.exp(L).astype(np.float64)
    dlog = np.zeros((P, D, 7), dtype=LD)
    d2log = np.zeros((P, D, D, 7), dtype=LD)
    dlog[..., :K] = np.einsum("kij,pj->pik", A, x.astype(LD)) + b.T
    d2log[..., :K] = A.transpose(1, 2, 0)
    return dict(x=x, h=h, jafs=jafs, L=L.astype(np.float64), dlog=dlog, d2log=d2log, K=K)


def analytic(case, table, rows, unfolded):
    """The four outputs from the analytic derivatives (the contraction in longdouble), rounded to double."""
    from misti_amd.optimize import class_counts
    f = class_counts(table, unfolded)[rows].astype(LD)
    return dict(dlog=case["dlog"].astype(np.float64), d2log=case["d2log"].astype(np.float64),
                grad=np.einsum("pk,pik->pi", f, case["dlog"]).astype(np.float64),
                hess=np.einsum("pk,pijk->pij", f, case["d2log"]).astype(np.float64))


def floors(jafs, h, unfolded, table, rows):
    """rule()'s floor per output with max(|L|, 1) in the place of every |L|."""
    from misti_amd.optimize import _class_values, class_counts
    P, D = h.shape
    aL = np.zeros(jafs.shape)
    cv = np.maximum(np.abs(np.log(_class_values(jafs, unfolded))), 1.0)
    aL[..., :cv.shape[-1]] = cv
    t1, t2 = np.zeros((P, D, 7)), np.zeros((P, D, D, 7))
    q = 0
    for i in range(D):
        hi = h[:, i, None]
        t1[:, i] = (aL[:, 1 + 2 * i] + aL[:, 2 + 2 * i]) / (2 * hi)
        t2[:, i, i] = (aL[:, 1 + 2 * i] + 2 * aL[:, 0] + aL[:, 2 + 2 * i]) / (hi * hi)
        for j in range(i + 1, D):
            c = 1 + 2 * D + 4 * q
            t2[:, i, j] = t2[:, j, i] = aL[:, c:c + 4].sum(axis=1) / (4 * hi * h[:, j, None])
            q += 1
    f = np.abs(class_counts(table, unfolded)[rows])
    return dict(dlog=FLOOR_ULPS * EPS * t1, d2log=FLOOR_ULPS * EPS * t2,
                grad=FLOOR_ULPS * EPS * np.einsum("pk,pik->pi", f, t1), hess=FLOOR_ULPS * EPS * np.einsum("pk,pijk->pij", f, t2))


def counts(rng, R):
    rows = np.zeros((R, 8))
    rows[:, 1:] = rng.integers(0, 50000, size=(R, 7))
    rows[:, 0] = rows[:, 1:].sum(axis=1)
    return rows


def worst_ratio(got, want, tol):
    """Largest |got - want| / tol (an error where the floor is 0 - the folded entries 4 to 6 - is infinite)."""
    err = np.abs(got - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))))
