// The least-squares solver of the lambda correction: rcp64 / sqrt64, the 3 x 3 solves, the Jacobi SVD, the trust-region steps of
// SciPy's trf (unbounded for the pair chain, bounded for the post-split refits) and the bookkeeping of one evaluated trial.
// Reached one problem per lane by misti_lsq_probe (lsq_probe_kernel), and by every chain kernel; restated by tests/lsq_rule.py and
// held against 50 digits by tests/test_lsq_probe_cpu.py and test_gpu_lsq_probe.py.
#pragma once
#include <math.h>
#include <stdint.h>

#include "misti_device.h"
#include "misti_wave.h"

namespace misti {

// Reciprocal / square root for the solver's bookkeeping: hardware seed + Newton steps, ~1 ulp,
// a third of the instructions of the correctly rounded forms (no denormal/overflow scaling:
// every operand here is a normal-range quantity or the result is tested for finiteness anyway).
__device__ __forceinline__ double rcp64(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    r = fma(fma(-x, r, 1.0), r, r);
    return r;
}
__device__ __forceinline__ double sqrt64(double x) {
    // straight-line: the solver's bookkeeping is one dependent instruction stream, every branch costs it a handful of
    // scalar instructions.  rsq(0) = inf and rsq(inf) = 0 make the Newton steps NaN: those two inputs are passed through;
    // negative and NaN inputs give NaN by themselves (rsq), as sqrt() does.
    double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = 0.5 * y;
    double r = fma(-h, g, 0.5);
    g = fma(g, r, g); h = fma(h, r, h);
    r = fma(-h, g, 0.5);
    g = fma(g, r, g); h = fma(h, r, h);
    double d = fma(-g, g, x);
    const double s = fma(d, h, g);
    return (x == 0.0 || x == INFINITY) ? x : s;
}

// 3x3 inverse times vector (for the default-fit residual, CorrectLambda.py:99-107)
__device__ __forceinline__ void solve3(const double M[3][3], const double b[3], double x[3]) {
    double c00 = M[1][1] * M[2][2] - M[1][2] * M[2][1];
    double c01 = M[1][2] * M[2][0] - M[1][0] * M[2][2];
    double c02 = M[1][0] * M[2][1] - M[1][1] * M[2][0];
    double det = M[0][0] * c00 + M[0][1] * c01 + M[0][2] * c02;
    double id = 1.0 / det;
    double c10 = M[0][2] * M[2][1] - M[0][1] * M[2][2];
    double c11 = M[0][0] * M[2][2] - M[0][2] * M[2][0];
    double c12 = M[0][1] * M[2][0] - M[0][0] * M[2][1];
    double c20 = M[0][1] * M[1][2] - M[0][2] * M[1][1];
    double c21 = M[0][2] * M[1][0] - M[0][0] * M[1][2];
    double c22 = M[0][0] * M[1][1] - M[0][1] * M[1][0];
    x[0] = (c00 * b[0] + c10 * b[1] + c20 * b[2]) * id;
    x[1] = (c01 * b[0] + c11 * b[1] + c21 * b[2]) * id;
    x[2] = (c02 * b[0] + c12 * b[1] + c22 * b[2]) * id;
}

// 3x3 solve by Gaussian elimination with partial pivoting (the order of LAPACK's getrf/getrs, which is what
// scipy.linalg.inv does): unlike the cofactor form it never multiplies a structurally zero entry into a live one, so a
// component of the solution that does not depend on some matrix entry mathematically does not depend on it bitwise
// either - the reference's finite-difference Jacobian has exact zeros there and so must ours.
__device__ __forceinline__ void solve3_ge(const double Min[3][3], const double b[3], double x[3]) {
    double A[3][3], r[3];
    for (int i = 0; i < 3; ++i) { r[i] = b[i]; for (int j = 0; j < 3; ++j) A[i][j] = Min[i][j]; }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        // pivot: largest magnitude in column c at or below the diagonal (first one on ties, as idamax)
        int pv = c;
#pragma unroll
        for (int i = c + 1; i < 3; ++i) if (fabs(A[i][c]) > fabs(A[pv][c])) pv = i;
#pragma unroll
        for (int i = c + 1; i < 3; ++i) {
            if (i == pv) {                                   // swap rows c and pv (selects: pv is data)
                for (int j = 0; j < 3; ++j) { const double t = A[c][j]; A[c][j] = A[i][j]; A[i][j] = t; }
                const double t = r[c]; r[c] = r[i]; r[i] = t;
            }
        }
        const double piv = 1.0 / A[c][c];                    // getf2 scales the column by the reciprocal of the pivot
#pragma unroll
        for (int i = c + 1; i < 3; ++i) {
            const double l = A[i][c] * piv;
            for (int j = c + 1; j < 3; ++j) A[i][j] = A[i][j] - l * A[c][j];
            r[i] = r[i] - l * r[c];
        }
    }
    x[2] = r[2] / A[2][2];
    x[1] = (r[1] - A[1][2] * x[2]) / A[1][1];
    x[0] = ((r[0] - A[0][1] * x[1]) - A[0][2] * x[2]) / A[0][0];
}

__device__ __forceinline__ void mat3_mul(const double X[3][3], const double Y[3][3], double Z[3][3]) {
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Z[r][c] = (X[r][0] * Y[0][c] + X[r][1] * Y[1][c]) + X[r][2] * Y[2][c];
}
__device__ __forceinline__ void mat3_vec(const double X[3][3], const double v[3], double o[3]) {
    for (int r = 0; r < 3; ++r) o[r] = (X[r][0] * v[0] + X[r][1] * v[1]) + X[r][2] * v[2];
}
// X = A^-1 B for a 3 x 3 right-hand side: Gaussian elimination with partial pivoting (rows swapped by selects: the pivot is data)
__device__ __forceinline__ void mat3_solve(const double Ain[3][3], const double Bin[3][3], double X[3][3]) {
    double A[3][3], R[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { A[i][j] = Ain[i][j]; R[i][j] = Bin[i][j]; }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        int pv = c;
#pragma unroll
        for (int i = c + 1; i < 3; ++i) if (fabs(A[i][c]) > fabs(A[pv][c])) pv = i;
#pragma unroll
        for (int i = c + 1; i < 3; ++i) {
            const bool sw = i == pv;
            for (int j = 0; j < 3; ++j) {
                const double a = A[c][j], b = A[i][j]; A[c][j] = sw ? b : a; A[i][j] = sw ? a : b;
                const double u = R[c][j], v = R[i][j]; R[c][j] = sw ? v : u; R[i][j] = sw ? u : v;
            }
        }
        const double piv = rcp64(A[c][c]);                    // getf2 scales the column by the reciprocal of the pivot
#pragma unroll
        for (int i = c + 1; i < 3; ++i) {
            const double l = A[i][c] * piv;
            for (int j = c + 1; j < 3; ++j) A[i][j] = A[i][j] - l * A[c][j];
            for (int j = 0; j < 3; ++j) R[i][j] = R[i][j] - l * R[c][j];
        }
    }
    // back substitution with the reciprocals of the diagonal (an fp64 division is ~40 instructions, and there would be nine)
    const double r0 = rcp64(A[0][0]), r1 = rcp64(A[1][1]), r2 = rcp64(A[2][2]);
    for (int j = 0; j < 3; ++j) {
        X[2][j] = R[2][j] * r2;
        X[1][j] = (R[1][j] - A[1][2] * X[2][j]) * r1;
        X[0][j] = ((R[0][j] - A[0][1] * X[1][j]) - A[0][2] * X[2][j]) * r0;
    }
}

// ------------------------------------------------------- least squares -------
// SciPy's trust-region-reflective solver for the 2x2 systems of the
// lambda-correction, restated so that the ITERATION SEQUENCE matches
// scipy.optimize.least_squares(method='trf', x_scale=1, loss='linear',
// tr_solver='exact', jac='2-point', ftol=1e-8, xtol=gtol=1e-10, max_nfev=100*n)
// as called at CorrectLambda.py:85,260,303,305 (SciPy 1.15.3:
// optimize/_lsq/trf.py trf_no_bounds :401-560 / trf_bounds :205-400,
// common.py solve_lsq_trust_region :57, update_tr_radius :222, check_termination
// :705, CL_scaling_vector :467; _numdiff.py _compute_absolute_step :146).
// The reference's results are defined by where that iteration stops (SURVEY.md
// section 7, hard part 1), not by the exact root.
constexpr double LSQ_EPS = 2.220446049250313e-16;
constexpr double LSQ_FTOL = 1e-8, LSQ_XTOL = 1e-10, LSQ_GTOL = 1e-10;
constexpr double SQRT_EPS = 1.4901161193847656e-08;

// thin SVD of an m x 2 matrix (m = 2 or 4) by one one-sided Jacobi rotation
struct Svd2 {
    double s[2];        // singular values, descending
    double V[2][2];     // V[:, i] = right singular vector i  (V[r][i])
    double uf[2];       // U^T f
};
template <int MROWS>
__device__ __forceinline__ Svd2 svd_mx2(const double A[MROWS][2], const double f[MROWS]) {
    double al = 0, be = 0, ga = 0;
    for (int r = 0; r < MROWS; ++r) { al += A[r][0] * A[r][0]; be += A[r][1] * A[r][1]; ga += A[r][0] * A[r][1]; }
    double c = 1.0, sn = 0.0;
    if (ga != 0.0) {
        double zeta = (be - al) * rcp64(2.0 * ga);
        const double den = fabs(zeta) + sqrt64(1.0 + zeta * zeta);
        double t = copysign(1.0, zeta) * rcp64(den);
        t = den < INFINITY ? t : copysign(0.0, zeta);      // zeta^2 overflowed (|zeta| > 1.3e154): rcp64(inf) is NaN, the tangent is 0
        c = rcp64(sqrt64(1.0 + t * t));
        sn = c * t;
    }
    double n1 = 0, n2 = 0, f1 = 0, f2 = 0;
    for (int r = 0; r < MROWS; ++r) {
        double a1 = c * A[r][0] - sn * A[r][1];
        double a2 = sn * A[r][0] + c * A[r][1];
        n1 += a1 * a1; n2 += a2 * a2; f1 += a1 * f[r]; f2 += a2 * f[r];
    }
    Svd2 o;
    double s1 = sqrt64(n1), s2 = sqrt64(n2);
    double v1[2] = {c, -sn}, v2[2] = {sn, c};
    double u1 = s1 > 0 ? f1 * rcp64(s1) : 0.0, u2 = s2 > 0 ? f2 * rcp64(s2) : 0.0;
    if (s1 >= s2) { o.s[0] = s1; o.s[1] = s2; o.V[0][0] = v1[0]; o.V[1][0] = v1[1]; o.V[0][1] = v2[0]; o.V[1][1] = v2[1]; o.uf[0] = u1; o.uf[1] = u2; }
    else          { o.s[0] = s2; o.s[1] = s1; o.V[0][0] = v2[0]; o.V[1][0] = v2[1]; o.V[0][1] = v1[0]; o.V[1][1] = v1[1]; o.uf[0] = u2; o.uf[1] = u1; }
    return o;
}

// common.py solve_lsq_trust_region :57-166 (n = 2)
__device__ __forceinline__ void solve_tr(const Svd2& d, int m, double Delta, double& alpha, double p[2]) {
    double suf0 = d.s[0] * d.uf[0], suf1 = d.s[1] * d.uf[1];
    bool full_rank = (m >= 2) && (d.s[1] > LSQ_EPS * m * d.s[0]);
    if (full_rank) {
        double a = d.uf[0] * rcp64(d.s[0]), b = d.uf[1] * rcp64(d.s[1]);
        p[0] = -(d.V[0][0] * a + d.V[0][1] * b);
        p[1] = -(d.V[1][0] * a + d.V[1][1] * b);
        if (p[0] * p[0] + p[1] * p[1] <= Delta * Delta) { alpha = 0.0; return; }
    }
    const double rDelta = rcp64(Delta);
    double alpha_upper = sqrt64(suf0 * suf0 + suf1 * suf1) * rDelta;
    double s0s = d.s[0] * d.s[0], s1s = d.s[1] * d.s[1];
    auto phi_fn = [&](double al, double& phi, double& dphi) {
        double r0 = rcp64(s0s + al), r1 = rcp64(s1s + al);
        double a = suf0 * r0, b = suf1 * r1;
        double pn = sqrt64(a * a + b * b);
        phi = pn - Delta;
        dphi = -(a * a * r0 + b * b * r1) * rcp64(pn);
    };
    double alpha_lower = 0.0;
    if (full_rank) { double ph, dp; phi_fn(0.0, ph, dp); alpha_lower = -ph * rcp64(dp); }
    double al = alpha;
    if (!full_rank && al == 0.0) al = fmax(0.001 * alpha_upper, sqrt64(alpha_lower * alpha_upper));
    for (int it = 0; it < 10; ++it) {
        if (al < alpha_lower || al > alpha_upper) al = fmax(0.001 * alpha_upper, sqrt64(alpha_lower * alpha_upper));
        double ph, dp; phi_fn(al, ph, dp);
        if (ph < 0) alpha_upper = al;
        double ratio = ph * rcp64(dp);
        alpha_lower = fmax(alpha_lower, al - ratio);
        al -= (ph + Delta) * ratio * rDelta;
        if (fabs(ph) < 0.01 * Delta) break;
    }
    double a = suf0 * rcp64(s0s + al), b = suf1 * rcp64(s1s + al);
    p[0] = -(d.V[0][0] * a + d.V[0][1] * b);
    p[1] = -(d.V[1][0] * a + d.V[1][1] * b);
    double sc = Delta * rcp64(sqrt64(p[0] * p[0] + p[1] * p[1]));
    p[0] *= sc; p[1] *= sc;
    alpha = al;
}

// common.py update_tr_radius :222-245
__device__ __forceinline__ double update_radius(double Delta, double actual, double predicted, double step_norm, bool bound_hit, double& ratio) {
    if (predicted > 0) ratio = actual / predicted;
    else if (predicted == 0 && actual == 0) ratio = 1.0;
    else ratio = 0.0;
    if (ratio < 0.25) Delta = 0.25 * step_norm;
    else if (ratio > 0.75 && bound_hit) Delta *= 2.0;
    return Delta;
}
// common.py check_termination :705-717 (0 = continue)
__device__ __forceinline__ int check_term(double dF, double F, double dx, double xn, double ratio) {
    bool f_ok = dF < LSQ_FTOL * F && ratio > 0.25;
    bool x_ok = dx < LSQ_XTOL * (LSQ_XTOL + xn);
    return (f_ok && x_ok) ? 4 : f_ok ? 2 : x_ok ? 3 : 0;
}
// _numdiff._compute_absolute_step :173-178 (rel_step=None, '2-point')
__device__ __forceinline__ double fd_step(double x) { return SQRT_EPS * (x >= 0 ? 1.0 : -1.0) * fmax(1.0, fabs(x)); }

// ---- bounded variant (trf_bounds, trf.py:205-400) for N = 1, 2 unknowns, lower bound
// lb on every variable, no upper bound (CorrectLambda.py:82-86, :253-260).  The
// residual functor is evaluated per lane (no cross-lane traffic), so different
// lanes may run different problems (post-split refits: one interval per lane).
template <int N> struct SvdN { double s[N]; double V[N][N]; double uf[N]; };

__device__ __forceinline__ SvdN<1> svd_aug(const double A[2][1], const double f[2]) {
    SvdN<1> o;
    double nn = A[0][0] * A[0][0] + A[1][0] * A[1][0];
    o.s[0] = sqrt(nn);
    o.V[0][0] = 1.0;
    o.uf[0] = o.s[0] > 0 ? (A[0][0] * f[0] + A[1][0] * f[1]) / o.s[0] : 0.0;
    return o;
}
__device__ __forceinline__ SvdN<2> svd_aug(const double A[4][2], const double f[4]) {
    Svd2 t = svd_mx2<4>(A, f);
    SvdN<2> o;
    for (int i = 0; i < 2; ++i) { o.s[i] = t.s[i]; o.uf[i] = t.uf[i]; for (int r = 0; r < 2; ++r) o.V[r][i] = t.V[r][i]; }
    return o;
}

template <int N> __device__ __forceinline__ double vnorm(const double v[N]) {
    double a = 0; for (int i = 0; i < N; ++i) a += v[i] * v[i]; return sqrt(a);
}

// common.py solve_lsq_trust_region :57-166, general n
template <int N> __device__ __forceinline__ void solve_tr_n(const SvdN<N>& d, int m, double Delta, double& alpha, double p[N]) {
    double suf[N];
    for (int i = 0; i < N; ++i) suf[i] = d.s[i] * d.uf[i];
    bool full_rank = (m >= N) && (d.s[N - 1] > LSQ_EPS * m * d.s[0]);
    if (full_rank) {
        for (int r = 0; r < N; ++r) { double a = 0; for (int i = 0; i < N; ++i) a += d.V[r][i] * (d.uf[i] / d.s[i]); p[r] = -a; }
        if (vnorm<N>(p) <= Delta) { alpha = 0.0; return; }
    }
    double alpha_upper = vnorm<N>(suf) / Delta;
    auto phi_fn = [&](double al, double& phi, double& dphi) {
        double q[N], acc = 0;
        for (int i = 0; i < N; ++i) { double e = d.s[i] * d.s[i] + al; q[i] = suf[i] / e; acc += suf[i] * suf[i] / (e * e * e); }
        double pn = vnorm<N>(q);
        phi = pn - Delta; dphi = -acc / pn;
    };
    double alpha_lower = 0.0;
    if (full_rank) { double ph, dp; phi_fn(0.0, ph, dp); alpha_lower = -ph / dp; }
    double al = alpha;
    if (!full_rank && al == 0.0) al = fmax(0.001 * alpha_upper, sqrt(alpha_lower * alpha_upper));
    for (int it = 0; it < 10; ++it) {
        if (al < alpha_lower || al > alpha_upper) al = fmax(0.001 * alpha_upper, sqrt(alpha_lower * alpha_upper));
        double ph, dp; phi_fn(al, ph, dp);
        if (ph < 0) alpha_upper = al;
        double ratio = ph / dp;
        alpha_lower = fmax(alpha_lower, al - ratio);
        al -= (ph + Delta) * ratio / Delta;
        if (fabs(ph) < 0.01 * Delta) break;
    }
    for (int r = 0; r < N; ++r) { double a = 0; for (int i = 0; i < N; ++i) a += d.V[r][i] * (suf[i] / (d.s[i] * d.s[i] + al)); p[r] = -a; }
    double sc = Delta / vnorm<N>(p);
    for (int r = 0; r < N; ++r) p[r] *= sc;
    alpha = al;
}

// common.py step_size_to_bound :372-398 with ub = +inf
template <int N> __device__ __forceinline__ double step_to_bound(const double x[N], const double s[N], double lb, int hits[N]) {
    double steps[N], mn = INFINITY;
    for (int i = 0; i < N; ++i) {
        steps[i] = INFINITY;
        if (s[i] != 0) steps[i] = fmax((lb - x[i]) / s[i], s[i] > 0 ? INFINITY : -INFINITY);
        mn = fmin(mn, steps[i]);
    }
    for (int i = 0; i < N; ++i) hits[i] = (steps[i] == mn) ? (s[i] > 0 ? 1 : (s[i] < 0 ? -1 : 0)) : 0;
    return mn;
}
// common.py evaluate_quadratic :325-361 / build_quadratic_1d :248-299 / minimize_quadratic_1d :302-322
template <int N> __device__ __forceinline__ double eval_quad(const double Jh[N][N], const double gh[N], const double s[N], const double diag[N]) {
    double q = 0, l = 0;
    for (int r = 0; r < N; ++r) { double js = 0; for (int c = 0; c < N; ++c) js += Jh[r][c] * s[c]; q += js * js; }
    for (int i = 0; i < N; ++i) { q += s[i] * diag[i] * s[i]; l += s[i] * gh[i]; }
    return 0.5 * q + l;
}
template <int N> __device__ __forceinline__ void build_quad(const double Jh[N][N], const double gh[N], const double s[N], const double diag[N],
                                                            const double* s0, double& a, double& b, double& c) {
    double v[N];
    a = 0; b = 0; c = 0;
    for (int r = 0; r < N; ++r) { v[r] = 0; for (int k = 0; k < N; ++k) v[r] += Jh[r][k] * s[k]; a += v[r] * v[r]; }
    for (int i = 0; i < N; ++i) { a += s[i] * diag[i] * s[i]; b += gh[i] * s[i]; }
    a *= 0.5;
    if (s0) {
        double uu = 0;
        for (int r = 0; r < N; ++r) { double u = 0; for (int k = 0; k < N; ++k) u += Jh[r][k] * s0[k]; b += u * v[r]; uu += u * u; }
        c = 0.5 * uu;
        for (int i = 0; i < N; ++i) { c += gh[i] * s0[i]; b += s0[i] * diag[i] * s[i]; }
        for (int i = 0; i < N; ++i) c += 0.5 * s0[i] * diag[i] * s0[i];
    }
}
__device__ __forceinline__ double min_quad(double a, double b, double lo, double hi, double c, double& y) {
    double t = lo; y = lo * (a * lo + b) + c;
    double yh = hi * (a * hi + b) + c;
    if (yh < y) { y = yh; t = hi; }
    if (a != 0) { double e = -0.5 * b / a; if (lo < e && e < hi) { double ye = e * (a * e + b) + c; if (ye < y) { y = ye; t = e; } } }
    return t;
}
// trf.py select_step :128-203
template <int N> __device__ __forceinline__ double select_step(const double x[N], const double Jh[N][N], const double diag[N], const double gh[N],
                                                              double p[N], double ph[N], const double d[N], double Delta, double lb, double theta,
                                                              double step[N], double steph[N]) {
    bool inb = true;
    for (int i = 0; i < N; ++i) inb = inb && (x[i] + p[i] >= lb);
    if (inb) { for (int i = 0; i < N; ++i) { step[i] = p[i]; steph[i] = ph[i]; } return -eval_quad<N>(Jh, gh, ph, diag); }
    int hits[N];
    double pstride = step_to_bound<N>(x, p, lb, hits);
    double rh[N], r[N], xb[N];
    for (int i = 0; i < N; ++i) { rh[i] = hits[i] != 0 ? -ph[i] : ph[i]; r[i] = d[i] * rh[i]; }
    for (int i = 0; i < N; ++i) { p[i] *= pstride; ph[i] *= pstride; xb[i] = x[i] + p[i]; }
    double to_tr;
    {   // intersect_trust_region(p_h, r_h, Delta), common.py:17-54: positive root
        double a = 0, b = 0, c = -Delta * Delta;
        for (int i = 0; i < N; ++i) { a += rh[i] * rh[i]; b += ph[i] * rh[i]; c += ph[i] * ph[i]; }
        double dd = sqrt(b * b - a * c);
        double q = -(b + copysign(dd, b));
        double t1 = q / a, t2 = c / q;
        to_tr = fmax(t1, t2);
    }
    int h2[N];
    double to_bound = step_to_bound<N>(xb, r, lb, h2);
    double rs = fmin(to_bound, to_tr), rl, ru;
    if (rs > 0) { rl = (1 - theta) * pstride / rs; ru = (rs == to_bound) ? theta * to_bound : to_tr; }
    else { rl = 0; ru = -1; }
    double rval = INFINITY;
    if (rl <= ru) {
        double a, b, c;
        build_quad<N>(Jh, gh, rh, diag, ph, a, b, c);
        double t = min_quad(a, b, rl, ru, c, rval);
        for (int i = 0; i < N; ++i) { rh[i] = rh[i] * t + ph[i]; r[i] = rh[i] * d[i]; }
    }
    for (int i = 0; i < N; ++i) { p[i] *= theta; ph[i] *= theta; }
    double pval = eval_quad<N>(Jh, gh, ph, diag);
    double agh[N], ag[N];
    for (int i = 0; i < N; ++i) { agh[i] = -gh[i]; ag[i] = d[i] * agh[i]; }
    double to_tr2 = Delta / vnorm<N>(agh);
    double to_b2 = step_to_bound<N>(x, ag, lb, h2);
    double ags = to_b2 < to_tr2 ? theta * to_b2 : to_tr2;
    double a, b, c, agval;
    build_quad<N>(Jh, gh, agh, diag, nullptr, a, b, c);
    ags = min_quad(a, b, 0.0, ags, 0.0, agval);
    for (int i = 0; i < N; ++i) { agh[i] *= ags; ag[i] *= ags; }
    if (pval < rval && pval < agval) { for (int i = 0; i < N; ++i) { step[i] = p[i]; steph[i] = ph[i]; } return -pval; }
    if (rval < pval && rval < agval) { for (int i = 0; i < N; ++i) { step[i] = r[i]; steph[i] = rh[i]; } return -rval; }
    for (int i = 0; i < N; ++i) { step[i] = ag[i]; steph[i] = agh[i]; }
    return -agval;
}

// fun(x, f): N residuals of N unknowns.  x is updated in place.
// Returns the solver word (nfev | SciPy status << 16 | kind 2 << 20, see include/misti_hip.h).
template <int N, class Fun> __device__ __forceinline__ int32_t trf_bounded(Fun fun, double x[N], double lb) {
    auto eval = [&](const double xx[N], double f[N], double J[N][N]) {
        fun(xx, f);
        for (int j = 0; j < N; ++j) {
            double h = fd_step(xx[j]);
            if (xx[j] + h < lb) h = -h;                       // _adjust_scheme_to_bounds, 1-sided
            double x1[N], f1[N];
            for (int i = 0; i < N; ++i) x1[i] = xx[i];
            x1[j] = xx[j] + h;
            double dx = x1[j] - xx[j];
            fun(x1, f1);
            for (int r = 0; r < N; ++r) J[r][j] = (f1[r] - f[r]) / dx;
        }
    };
    for (int i = 0; i < N; ++i) {                              // make_strictly_feasible(x0), least_squares.py:828
        double th = 1e-10 * fmax(1.0, fabs(lb));
        if (x[i] - lb <= th) x[i] = lb + th;
    }
    double f[N], J[N][N], g[N];
    eval(x, f, J);
    int nfev = 1;
    const int max_nfev = 100 * N;
    double cost = 0;
    for (int i = 0; i < N; ++i) cost += f[i] * f[i];
    cost *= 0.5;
    auto grad = [&]() { for (int c = 0; c < N; ++c) { g[c] = 0; for (int r = 0; r < N; ++r) g[c] += J[r][c] * f[r]; } };
    grad();
    double v[N], dv[N];
    auto CL = [&]() { for (int i = 0; i < N; ++i) { if (g[i] > 0) { v[i] = x[i] - lb; dv[i] = 1.0; } else { v[i] = 1.0; dv[i] = 0.0; } } };
    CL();
    double Delta;
    { double t[N]; for (int i = 0; i < N; ++i) t[i] = x[i] / sqrt(v[i]); Delta = vnorm<N>(t); if (Delta == 0) Delta = 1.0; }
    double alpha = 0.0;
    int term = 0;
    for (;;) {
        CL();
        double g_norm = 0;
        for (int i = 0; i < N; ++i) g_norm = fmax(g_norm, fabs(g[i] * v[i]));
        if (g_norm < LSQ_GTOL) term = 1;
        if (term != 0 || nfev >= max_nfev) break;
        if (!(g_norm < INFINITY)) break;
        double d[N], diag[N], gh[N], Jh[N][N], A[2 * N][N], fa[2 * N];
        for (int i = 0; i < N; ++i) { d[i] = sqrt(v[i]); diag[i] = g[i] * dv[i]; gh[i] = d[i] * g[i]; }
        for (int r = 0; r < N; ++r) { fa[r] = f[r]; fa[N + r] = 0.0; for (int c = 0; c < N; ++c) { Jh[r][c] = J[r][c] * d[c]; A[r][c] = Jh[r][c]; A[N + r][c] = (r == c) ? sqrt(diag[r]) : 0.0; } }
        SvdN<N> sv = svd_aug(A, fa);
        double theta = fmax(0.995, 1.0 - g_norm);
        double actual = -1.0;
        double xn[N], fn[N], Jn[N][N], cost_new = cost;
        while (actual <= 0 && nfev < max_nfev) {
            double ph[N], p[N], step[N], steph[N];
            solve_tr_n<N>(sv, N, Delta, alpha, ph);
            for (int i = 0; i < N; ++i) p[i] = d[i] * ph[i];
            double predicted = select_step<N>(x, Jh, diag, gh, p, ph, d, Delta, lb, theta, step, steph);
            for (int i = 0; i < N; ++i) { xn[i] = x[i] + step[i]; if (xn[i] <= lb) xn[i] = nextafter(lb, INFINITY); }   // make_strictly_feasible(rstep=0)
            eval(xn, fn, Jn);
            ++nfev;
            double shn = vnorm<N>(steph);
            bool fin = true;
            for (int i = 0; i < N; ++i) fin = fin && isfinite(fn[i]);
            if (!fin) { Delta = 0.25 * shn; continue; }
            cost_new = 0;
            for (int i = 0; i < N; ++i) cost_new += fn[i] * fn[i];
            cost_new *= 0.5;
            actual = cost - cost_new;
            double ratio;
            double Delta_new = update_radius(Delta, actual, predicted, shn, shn > 0.95 * Delta, ratio);
            term = check_term(actual, cost, vnorm<N>(step), vnorm<N>(x), ratio);
            if (term != 0) break;
            alpha *= Delta / Delta_new;
            Delta = Delta_new;
        }
        if (actual > 0) {
            for (int i = 0; i < N; ++i) { x[i] = xn[i]; f[i] = fn[i]; for (int c = 0; c < N; ++c) J[i][c] = Jn[i][c]; }
            cost = cost_new;
            grad();
        }
    }
    return solver_word(nfev, term, 2);
}

// Residuals and forward-difference Jacobian at a point from the six residuals evaluated there (base point, first rate
// stepped, second rate stepped; both genomes).
__device__ __forceinline__ void collect_core(double x0, double x1, double fb0, double fb1, double fa0, double fa1, double fc0, double fc1,
                                             double f[2], double J[2][2], bool& finite) {
    const double h0 = fd_step(x0), h1 = fd_step(x1);
    const double xa = x0 + h0, xb = x1 + h1;
    const double dx0 = xa - x0, dx1 = xb - x1;      // recomputed as exactly representable (_numdiff.py)
    const double r0 = rcp64(dx0), r1 = rcp64(dx1);
    f[0] = fb0; f[1] = fb1;
    J[0][0] = (fa0 - fb0) * r0; J[1][0] = (fa1 - fb1) * r0;
    J[0][1] = (fc0 - fb0) * r1; J[1][1] = (fc1 - fb1) * r1;
    finite = isfinite(fb0) && isfinite(fb1);
}
// ... at the point xe from the six lanes base .. base + 5 that evaluated it (wave- or group-uniform result)
template <int GROUP>
__device__ __forceinline__ void pair_collect(double res, const double xe[2], int base, double f[2], double J[2][2], bool& finite) {
    const double fb0 = gbcast<GROUP>(res, base + 0), fb1 = gbcast<GROUP>(res, base + 1);
    const double fa0 = gbcast<GROUP>(res, base + 2), fa1 = gbcast<GROUP>(res, base + 3);
    const double fc0 = gbcast<GROUP>(res, base + 4), fc1 = gbcast<GROUP>(res, base + 5);
    collect_core(xe[0], xe[1], fb0, fb1, fa0, fa1, fc0, fc1, f, J, finite);
}
// ... in every slot at once: each lane gets the result of ITS slot (lanes sbase .. sbase + 5) at its slot's point
__device__ __forceinline__ void slot_collect(double res, double x0, double x1, int sbase, double f[2], double J[2][2], bool& finite) {
    const double fb0 = __shfl(res, sbase + 0, 64), fb1 = __shfl(res, sbase + 1, 64);
    const double fa0 = __shfl(res, sbase + 2, 64), fa1 = __shfl(res, sbase + 3, 64);
    const double fc0 = __shfl(res, sbase + 4, 64), fc1 = __shfl(res, sbase + 5, 64);
    collect_core(x0, x1, fb0, fb1, fa0, fa1, fc0, fc1, f, J, finite);
}

// Trust-region bookkeeping of one evaluated trial of trf_no_bounds (trf.py:488-521; update_tr_radius,
// common.py:222-245; check_termination, common.py:705-717).  Straight-line (selects, no branches): run with
// wave-uniform operands by the serial consume loop and with one hypothesis per slot by the tree consume of
// correct_body - the same expressions, so the same bits.
__device__ __forceinline__ void tr_update(bool finite, const double p[2], const double x[2], double cost, double cost_new, double predicted,
                                          double& Delta, double& dq, int& term, bool& accept) {
    const double sn2 = p[0] * p[0] + p[1] * p[1];
    dq = 0.25 * sqrt64(sn2);                                         // radius after a poor or non-finite step
    const double actual = cost - cost_new;
    const double rq = actual * rcp64(predicted);
    const double ratio = predicted > 0 ? rq : ((predicted == 0 && actual == 0) ? 1.0 : 0.0);
    const double Delta_new = ratio < 0.25 ? dq                       // update_tr_radius
                             : ((ratio > 0.75 && sn2 > 0.9025 * Delta * Delta) ? 2.0 * Delta : Delta);
    const bool f_ok = actual < LSQ_FTOL * cost && ratio > 0.25;      // check_termination
    const double lim = LSQ_XTOL * (LSQ_XTOL + sqrt64(x[0] * x[0] + x[1] * x[1]));
    const bool x_ok = sn2 < lim * lim;
    term = !finite ? 0 : ((f_ok && x_ok) ? 4 : f_ok ? 2 : x_ok ? 3 : 0);
    Delta = !finite ? dq : (term == 0 ? Delta_new : Delta);
    accept = finite && actual > 0;
}
// predicted reduction -(0.5 |J p|^2 + p . g) of a step (evaluate_quadratic, common.py:276)
__device__ __forceinline__ double predicted_of(const double J[2][2], const double p[2], const double g[2]) {
    const double Js0 = J[0][0] * p[0] + J[0][1] * p[1], Js1 = J[1][0] * p[0] + J[1][1] * p[1];
    return -(0.5 * (Js0 * Js0 + Js1 * Js1) + (p[0] * g[0] + p[1] * g[1]));
}

// Next trial step of trf_no_bounds (trf.py:469-486): Gauss-Newton step when the Jacobian has
// full rank and the step lies in the trust region (solve_lsq_trust_region, common.py:116-125),
// otherwise the regularised step from the SVD.  Returns the predicted reduction.
template <int GROUP>
__device__ __forceinline__ double next_step(const double J[2][2], const double f[2], const double g[2], double Delta, double& alpha,
                                            double p[2], int& lm, int& axis) {
    const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    const double F = (J[0][0] * J[0][0] + J[0][1] * J[0][1]) + (J[1][0] * J[1][0] + J[1][1] * J[1][1]);
    // A structurally decoupled rate (Jacobian column exactly zero, see pair_expv): J has rank one,
    // solve_lsq_trust_region takes its regularised branch and ALWAYS rescales the step to the
    // trust radius (common.py:160-164), so the step is (0, -sign(g1) Delta) whatever alpha the
    // secular iteration ends with - and alpha is only a starting guess for the next call.
    const bool z0 = J[0][0] == 0.0 && J[1][0] == 0.0, z1 = J[0][1] == 0.0 && J[1][1] == 0.0;
    const bool rank1 = z0 != z1;
    const int k = z0 ? 1 : 0;
    axis = rank1 ? k : -1;
    const double gk = z0 ? g[1] : g[0];
    const double pk = gk > 0 ? -Delta : Delta;
    // Gauss-Newton step (computed unconditionally - straight-line code - and used when J certainly has full rank and the
    // step lies inside the trust region): s_max^2 <= F <= 2 s_max^2 and s_min = |det| / s_max, so full rank
    // (s_min > 2 eps s_max) is certain if |det| > 2 eps F
    const double rd = rcp64(det);
    const double p0 = -(J[1][1] * f[0] - J[0][1] * f[1]) * rd;
    const double p1 = -(J[0][0] * f[1] - J[1][0] * f[0]) * rd;
    const bool gn = !rank1 && fabs(det) > 2.0 * LSQ_EPS * 2.0 * F && p0 * p0 + p1 * p1 <= Delta * Delta;
    if (uni<GROUP>(rank1 || gn)) {
        p[0] = rank1 ? (z0 ? 0.0 : pk) : p0;
        p[1] = rank1 ? (z0 ? pk : 0.0) : p1;
        alpha = 0.0;
    } else {
        // the decomposition is recomputed on every regularised step (rejected steps repeat it for the same J, f: ~50 such
        // steps per chain) rather than carried through the solver loop: 16 registers of loop-carried state less
        const Svd2 d = svd_mx2<2>(J, f);
        solve_tr(d, 2, Delta, alpha, p);
        lm += 1;
    }
    return predicted_of(J, p, g);
}

}  // namespace misti
