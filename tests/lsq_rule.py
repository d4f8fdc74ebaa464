"""The solver's linear algebra (the "least squares" unit, misti_amd/csrc/misti_lsq.h) restated in Python,
operation for operation: the counterpart of tests/pair_branches.py for misti_lsq_probe.

Every function takes a KIT of arithmetic as its first argument.  With F64 the operations are numpy's float64 - correctly rounded
`/` and `sqrt` where the device has rcp64 / sqrt64, and no fma where the device contracts - and the result is the RESTATEMENT.  With
MP (mpmath, tests/golden/make_lsq_probe.py only) the same statements run in 80-digit arithmetic: one Jacobi rotation diagonalises a
2 x 2 Gram matrix exactly, so that run is the EXACT decomposition, and the trust-region iteration under it is SciPy's
solve_lsq_trust_region replayed without rounding.  A kit records every comparison a function makes (name, relative gap, outcome):
the fixture's conditions are margins on those gaps.

run(kit, kind, row) maps a problem row of the probe to its result row (the layouts of include/misti_hip.h), scipy_row() does the same
through SciPy's own functions, discrete() reads the discrete outcome off a result row and figures() measures a result row against the
fixture's exact answers in the issue's units.  figures() needs no mpmath: the regularised step at the alpha a result row carries is
-(A^T A + alpha I)^-1 A^T f, rational in the inputs, and is evaluated with fractions.Fraction."""
import math
from fractions import Fraction

import numpy as np

EPS = 2.220446049250313e-16
FTOL, XTOL = 1e-8, 1e-10
KINDS = {"SCALAR": 0, "SVD2": 1, "SVD4": 2, "STEP": 3, "STEPN": 4, "SELECT": 5, "UPDATE": 6, "SOLVE3": 7}
LSQ_IN, LSQ_OUT = 20, 16
# Bound of rcp64 / sqrt64 in ulps of the correctly rounded result (derivation: tests/test_gpu_lsq_probe.py)
SCALAR_ULPS = 0.5 + 2.0 ** -20
DEVICE_FACTOR = 4.0


def _gap(a, b):
    """Relative distance of the two sides of a comparison, in the arithmetic they come in; a side that is not finite: inf."""
    if a == b:
        return 0.0
    try:
        g = float(abs(a - b) / max(abs(a), abs(b)))
    except ZeroDivisionError:
        return math.inf
    return g if g == g else math.inf


class F64:
    """float64, IEEE: x / 0 is inf, 0 / 0 is NaN, fmax / fmin drop a NaN as C's do."""
    name = "f64"

    def __init__(self):
        self.trace = []

    num = staticmethod(np.float64)
    inf = np.float64(np.inf)
    sqrt = staticmethod(np.sqrt)
    fabs = staticmethod(np.abs)
    copysign = staticmethod(np.copysign)
    fmax = staticmethod(np.fmax)
    fmin = staticmethod(np.fmin)

    @staticmethod
    def div(a, b):
        return np.float64(a) / np.float64(b)

    def rcp(self, x):
        return np.float64(1.0) / np.float64(x)

    @staticmethod
    def isfinite(x):
        return bool(np.isfinite(x))

    def cmp(self, name, a, op, b):
        r = bool({"<": a < b, "<=": a <= b, ">": a > b, ">=": a >= b, "==": a == b, "!=": a != b}[op])
        self.trace.append((name, _gap(a, b), r))
        return r

    def note(self, name, a, b, outcome):
        """A comparison decided elsewhere (on a difference, say), with the two sides its margin is measured between."""
        self.trace.append((name, _gap(a, b), outcome))
        return outcome


class MP(F64):
    """mpmath at 80 digits with the same conventions (mpmath has no signed zero: copysign(1, 0) is 1, as for +0)."""
    name = "mp"

    def __init__(self):
        import mpmath
        self.mp = mpmath.mp.clone()
        self.mp.dps = 80
        self.trace = []
        self.inf = self.mp.inf

    def num(self, x):
        return self.mp.mpf(float(x)) if not isinstance(x, self.mp.mpf) else x

    def sqrt(self, x):
        x = self.num(x)
        return self.mp.nan if (x < 0 or self.mp.isnan(x)) else self.mp.sqrt(x)

    def fabs(self, x):
        return abs(self.num(x))

    def copysign(self, x, y):
        return abs(x) if y >= 0 else -abs(x)

    def fmax(self, a, b):
        a, b = self.num(a), self.num(b)
        return b if self.mp.isnan(a) else a if self.mp.isnan(b) else max(a, b)

    def fmin(self, a, b):
        a, b = self.num(a), self.num(b)
        return b if self.mp.isnan(a) else a if self.mp.isnan(b) else min(a, b)

    def div(self, a, b):
        a, b = self.num(a), self.num(b)
        if b == 0:
            return self.mp.nan if (a == 0 or self.mp.isnan(a)) else (self.mp.inf if a > 0 else -self.mp.inf)
        return a / b

    def rcp(self, x):
        return self.div(1, x)

    def isfinite(self, x):
        return bool(self.mp.isfinite(x))


def live(trace):
    """The comparisons of a trace whose outcome can reach a result: the sign of phi in the iteration that converges only moves
    alpha_upper, which nothing reads afterwards (and phi is 0 to rounding there when the secular equation has one term)."""
    return [t for i, t in enumerate(trace) if not (t[0] == "phi<0" and i + 1 < len(trace) and trace[i + 1][0] == "converged" and trace[i + 1][2])]


# ------------------------------------------------------------------ the restated functions
def svd_mx2(K, A, f):
    """svd_mx2<MROWS>: thin SVD of an m x 2 matrix by one one-sided Jacobi rotation.  Returns s[2], V[2][2], uf[2]."""
    z = K.num(0.0)
    al, be, ga = z, z, z
    for r in range(len(A)):
        al = al + A[r][0] * A[r][0]
        be = be + A[r][1] * A[r][1]
        ga = ga + A[r][0] * A[r][1]
    c, sn = K.num(1.0), z
    if K.cmp("ga!=0", ga, "!=", z):
        zeta = (be - al) * K.rcp(2.0 * ga)
        sg = K.copysign(K.num(1.0), zeta)
        if K.name == "mp" and zeta == 0:                 # (be - al) is +0 there and zeta carries the sign of ga: float64 has it, mpmath not
            sg = K.copysign(K.num(1.0), ga)
        t = sg * K.rcp(K.fabs(zeta) + K.sqrt(1.0 + zeta * zeta))
        c = K.rcp(K.sqrt(1.0 + t * t))
        sn = c * t
    n1, n2, f1, f2 = z, z, z, z
    for r in range(len(A)):
        a1 = c * A[r][0] - sn * A[r][1]
        a2 = sn * A[r][0] + c * A[r][1]
        n1 = n1 + a1 * a1
        n2 = n2 + a2 * a2
        f1 = f1 + a1 * f[r]
        f2 = f2 + a2 * f[r]
    s1, s2 = K.sqrt(n1), K.sqrt(n2)
    u1 = f1 * K.rcp(s1) if s1 > 0 else z
    u2 = f2 * K.rcp(s2) if s2 > 0 else z
    if K.cmp("s1>=s2", s1, ">=", s2):
        return [s1, s2], [[c, sn], [-sn, c]], [u1, u2]
    return [s2, s1], [[sn, c], [c, -sn]], [u2, u1]


def svd_aug1(K, A, f):
    """svd_aug for N = 1 (a 2 x 1 column): real sqrt and / on the device."""
    nn = A[0] * A[0] + A[1] * A[1]
    s = K.sqrt(nn)
    uf = K.div(A[0] * f[0] + A[1] * f[1], s) if s > 0 else K.num(0.0)
    return [s], [[K.num(1.0)]], [uf]


def solve_tr(K, d, m, Delta, alpha):
    """solve_tr (n = 2, the chain kernels' form: reciprocals, squared norms).  Returns p, alpha, iterations (-1: Gauss-Newton)."""
    s, V, uf = d
    suf0, suf1 = s[0] * uf[0], s[1] * uf[1]
    full_rank = m >= 2 and K.cmp("rank", s[1], ">", EPS * m * s[0])
    if full_rank:
        a, b = uf[0] * K.rcp(s[0]), uf[1] * K.rcp(s[1])
        p = [-(V[0][0] * a + V[0][1] * b), -(V[1][0] * a + V[1][1] * b)]
        if K.cmp("inside", p[0] * p[0] + p[1] * p[1], "<=", Delta * Delta):
            return p, K.num(0.0), -1
    rDelta = K.rcp(Delta)
    alpha_upper = K.sqrt(suf0 * suf0 + suf1 * suf1) * rDelta
    s0s, s1s = s[0] * s[0], s[1] * s[1]

    def phi_fn(al):
        r0, r1 = K.rcp(s0s + al), K.rcp(s1s + al)
        a, b = suf0 * r0, suf1 * r1
        pn = K.sqrt(a * a + b * b)
        return pn - Delta, -(a * a * r0 + b * b * r1) * K.rcp(pn)

    alpha_lower = K.num(0.0)
    if full_rank:
        ph, dp = phi_fn(K.num(0.0))
        alpha_lower = -ph * K.rcp(dp)
    al = K.num(alpha)
    if not full_rank and al == 0.0:
        al = K.fmax(0.001 * alpha_upper, K.sqrt(alpha_lower * alpha_upper))
    iters = 0
    for it in range(10):
        iters = it + 1
        if K.cmp("below", al, "<", alpha_lower) or K.cmp("above", al, ">", alpha_upper):
            al = K.fmax(0.001 * alpha_upper, K.sqrt(alpha_lower * alpha_upper))
        ph, dp = phi_fn(al)
        if K.note("phi<0", ph + Delta, Delta, bool(ph < 0)):
            alpha_upper = al
        ratio = ph * K.rcp(dp)
        alpha_lower = K.fmax(alpha_lower, al - ratio)
        al = al - (ph + Delta) * ratio * rDelta
        if K.cmp("converged", K.fabs(ph), "<", 0.01 * Delta):
            break
    a, b = suf0 * K.rcp(s0s + al), suf1 * K.rcp(s1s + al)
    p = [-(V[0][0] * a + V[0][1] * b), -(V[1][0] * a + V[1][1] * b)]
    sc = Delta * K.rcp(K.sqrt(p[0] * p[0] + p[1] * p[1]))
    return [p[0] * sc, p[1] * sc], al, iters


def vnorm(K, v):
    a = K.num(0.0)
    for x in v:
        a = a + x * x
    return K.sqrt(a)


def solve_tr_n(K, N, d, m, Delta, alpha):
    """solve_tr_n<N> (the bounded solver's form: SciPy's expressions, real divisions)."""
    s, V, uf = d
    suf = [s[i] * uf[i] for i in range(N)]
    full_rank = m >= N and K.cmp("rank", s[N - 1], ">", EPS * m * s[0])
    if full_rank:
        p = []
        for r in range(N):
            a = K.num(0.0)
            for i in range(N):
                a = a + V[r][i] * K.div(uf[i], s[i])
            p.append(-a)
        if K.cmp("inside", vnorm(K, p), "<=", Delta):
            return p, K.num(0.0), -1
    alpha_upper = K.div(vnorm(K, suf), Delta)

    def phi_fn(al):
        q, acc = [], K.num(0.0)
        for i in range(N):
            e = s[i] * s[i] + al
            q.append(K.div(suf[i], e))
            acc = acc + K.div(suf[i] * suf[i], e * e * e)
        pn = vnorm(K, q)
        return pn - Delta, K.div(-acc, pn)

    alpha_lower = K.num(0.0)
    if full_rank:
        ph, dp = phi_fn(K.num(0.0))
        alpha_lower = K.div(-ph, dp)
    al = K.num(alpha)
    if not full_rank and al == 0.0:
        al = K.fmax(0.001 * alpha_upper, K.sqrt(alpha_lower * alpha_upper))
    iters = 0
    for it in range(10):
        iters = it + 1
        if K.cmp("below", al, "<", alpha_lower) or K.cmp("above", al, ">", alpha_upper):
            al = K.fmax(0.001 * alpha_upper, K.sqrt(alpha_lower * alpha_upper))
        ph, dp = phi_fn(al)
        if K.note("phi<0", ph + Delta, Delta, bool(ph < 0)):
            alpha_upper = al
        ratio = K.div(ph, dp)
        alpha_lower = K.fmax(alpha_lower, al - ratio)
        al = al - K.div((ph + Delta) * ratio, Delta)
        if K.cmp("converged", K.fabs(ph), "<", 0.01 * Delta):
            break
    p = []
    for r in range(N):
        a = K.num(0.0)
        for i in range(N):
            a = a + V[r][i] * K.div(suf[i], s[i] * s[i] + al)
        p.append(-a)
    sc = K.div(Delta, vnorm(K, p))
    return [x * sc for x in p], al, iters


def next_step(K, J, f, Delta, alpha):
    """next_step with g = J^T f as correct_body forms it.  Returns p, alpha, predicted, lm increment, axis, iterations."""
    g = [J[0][0] * f[0] + J[1][0] * f[1], J[0][1] * f[0] + J[1][1] * f[1]]
    det = J[0][0] * J[1][1] - J[0][1] * J[1][0]
    F = (J[0][0] * J[0][0] + J[0][1] * J[0][1]) + (J[1][0] * J[1][0] + J[1][1] * J[1][1])
    z0 = J[0][0] == 0.0 and J[1][0] == 0.0
    z1 = J[0][1] == 0.0 and J[1][1] == 0.0
    rank1 = z0 != z1
    axis = (1 if z0 else 0) if rank1 else -1
    gk = g[1] if z0 else g[0]
    pk = -Delta if gk > 0 else Delta
    rd = K.rcp(det)
    p0 = -(J[1][1] * f[0] - J[0][1] * f[1]) * rd
    p1 = -(J[0][0] * f[1] - J[1][0] * f[0]) * rd
    iters, lm = -1, 0
    gn = (not rank1) and K.cmp("det", K.fabs(det), ">", 2.0 * EPS * 2.0 * F) and K.cmp("inside", p0 * p0 + p1 * p1, "<=", Delta * Delta)
    if rank1 or gn:
        p = [(K.num(0.0) if z0 else pk), (pk if z0 else K.num(0.0))] if rank1 else [p0, p1]
        alpha = K.num(0.0)
    else:
        p, alpha, iters = solve_tr(K, svd_mx2(K, J, f), 2, Delta, alpha)
        lm = 1
    Js0 = J[0][0] * p[0] + J[0][1] * p[1]
    Js1 = J[1][0] * p[0] + J[1][1] * p[1]
    predicted = -(0.5 * (Js0 * Js0 + Js1 * Js1) + (p[0] * g[0] + p[1] * g[1]))
    return p, alpha, predicted, lm, axis, iters


def step_to_bound(K, N, x, s, lb):
    steps, mn = [], K.inf
    for i in range(N):
        st = K.inf
        if s[i] != 0:
            st = K.fmax(K.div(lb - x[i], s[i]), K.inf if s[i] > 0 else -K.inf)
        steps.append(st)
        mn = K.fmin(mn, st)
    if N == 2 and K.isfinite(steps[0]) and K.isfinite(steps[1]):
        K.cmp("hits", steps[0], "==", steps[1])
    hits = [((1 if s[i] > 0 else -1 if s[i] < 0 else 0) if steps[i] == mn else 0) for i in range(N)]
    return mn, hits


def eval_quad(K, N, Jh, gh, s, diag):
    q, l = K.num(0.0), K.num(0.0)
    for r in range(N):
        js = K.num(0.0)
        for c in range(N):
            js = js + Jh[r][c] * s[c]
        q = q + js * js
    for i in range(N):
        q = q + s[i] * diag[i] * s[i]
        l = l + s[i] * gh[i]
    return 0.5 * q + l


def build_quad(K, N, Jh, gh, s, diag, s0):
    z = K.num(0.0)
    a, b, c, v = z, z, z, []
    for r in range(N):
        vr = z
        for k in range(N):
            vr = vr + Jh[r][k] * s[k]
        v.append(vr)
        a = a + vr * vr
    for i in range(N):
        a = a + s[i] * diag[i] * s[i]
        b = b + gh[i] * s[i]
    a = a * 0.5
    if s0 is not None:
        uu = z
        for r in range(N):
            u = z
            for k in range(N):
                u = u + Jh[r][k] * s0[k]
            b = b + u * v[r]
            uu = uu + u * u
        c = 0.5 * uu
        for i in range(N):
            c = c + gh[i] * s0[i]
            b = b + s0[i] * diag[i] * s[i]
        for i in range(N):
            c = c + 0.5 * s0[i] * diag[i] * s0[i]
    return a, b, c


def min_quad(K, a, b, lo, hi, c):
    t, y = lo, lo * (a * lo + b) + c
    yh = hi * (a * hi + b) + c
    if K.cmp("quad_hi", yh, "<", y):
        y, t = yh, hi
    if a != 0:
        e = K.div(-0.5 * b, a)
        if K.cmp("quad_lo<e", lo, "<", e) and K.cmp("quad_e<hi", e, "<", hi):
            ye = e * (a * e + b) + c
            if K.cmp("quad_e", ye, "<", y):
                y, t = ye, e
    return t, y


def select_step(K, N, x, Jh, diag, gh, p, ph, d, Delta, lb, theta):
    """select_step<N>.  Returns step, steph, predicted, path ("inside", "scaled", "reflected", "gradient"), and the three candidates."""
    p, ph = list(p), list(ph)
    if all(K.cmp("inb%d" % i, x[i] + p[i], ">=", lb) for i in range(N)):
        return p, ph, -eval_quad(K, N, Jh, gh, ph, diag), "inside", None
    pstride, hits = step_to_bound(K, N, x, p, lb)
    rh = [-ph[i] if hits[i] != 0 else ph[i] for i in range(N)]
    r = [d[i] * rh[i] for i in range(N)]
    p = [v * pstride for v in p]
    ph = [v * pstride for v in ph]
    xb = [x[i] + p[i] for i in range(N)]
    a, b, c = K.num(0.0), K.num(0.0), -Delta * Delta
    for i in range(N):
        a = a + rh[i] * rh[i]
        b = b + ph[i] * rh[i]
        c = c + ph[i] * ph[i]
    dd = K.sqrt(b * b - a * c)
    q = -(b + K.copysign(dd, b))
    to_tr = K.fmax(K.div(q, a), K.div(c, q))
    to_bound, _ = step_to_bound(K, N, xb, r, lb)
    rs = K.fmin(to_bound, to_tr)
    if K.cmp("rs>0", rs, ">", K.num(0.0)):
        rl = K.div((1 - theta) * pstride, rs)
        ru = theta * to_bound if K.note("rs==to_bound", to_bound, to_tr, bool(rs == to_bound)) else to_tr   # fmin drops a NaN to_tr
    else:
        rl, ru = K.num(0.0), K.num(-1.0)
    rval = K.inf
    if K.cmp("rl<=ru", rl, "<=", ru):
        qa, qb, qc = build_quad(K, N, Jh, gh, rh, diag, ph)
        t, rval = min_quad(K, qa, qb, rl, ru, qc)
        rh = [rh[i] * t + ph[i] for i in range(N)]
        r = [rh[i] * d[i] for i in range(N)]
    p = [v * theta for v in p]
    ph = [v * theta for v in ph]
    pval = eval_quad(K, N, Jh, gh, ph, diag)
    agh = [-gh[i] for i in range(N)]
    ag = [d[i] * agh[i] for i in range(N)]
    to_tr2 = K.div(Delta, vnorm(K, agh))
    to_b2, _ = step_to_bound(K, N, x, ag, lb)
    ags = theta * to_b2 if K.cmp("ag_bound", to_b2, "<", to_tr2) else to_tr2
    qa, qb, qc = build_quad(K, N, Jh, gh, agh, diag, None)
    ags, agval = min_quad(K, qa, qb, K.num(0.0), ags, K.num(0.0))
    agh = [v * ags for v in agh]
    ag = [v * ags for v in ag]
    cand = {"scaled": (p, ph, -pval), "reflected": (r, rh, -rval), "gradient": (ag, agh, -agval)}
    c1 = K.cmp("p<r", pval, "<", rval)
    c2 = K.cmp("p<ag", pval, "<", agval)
    c3 = K.cmp("r<ag", rval, "<", agval)
    path = "scaled" if (c1 and c2) else "reflected" if ((K.cmp("r<p", rval, "<", pval)) and c3) else "gradient"
    return cand[path][0], cand[path][1], cand[path][2], path, cand


def tr_update(K, finite, p, x, cost, cost_new, predicted, Delta):
    """tr_update.  Returns Delta, dq, term, accept, and the case of the new radius ("quartered", "doubled", "kept")."""
    sn2 = p[0] * p[0] + p[1] * p[1]
    dq = 0.25 * K.sqrt(sn2)
    actual = cost - cost_new
    rq = actual * K.rcp(predicted)
    zero = K.num(0.0)
    if K.cmp("predicted>0", predicted, ">", zero):
        ratio = rq
    else:
        ratio = K.num(1.0) if (predicted == 0 and actual == 0) else zero
    if K.cmp("ratio<0.25", ratio, "<", 0.25):
        Delta_new, case = dq, "quartered"
    elif K.cmp("ratio>0.75", ratio, ">", 0.75) and K.cmp("bound_hit", sn2, ">", 0.9025 * Delta * Delta):
        Delta_new, case = 2.0 * Delta, "doubled"
    else:
        Delta_new, case = Delta, "kept"
    f_ok = K.cmp("ftol", actual, "<", FTOL * cost) and K.cmp("ratio>0.25", ratio, ">", 0.25)
    lim = XTOL * (XTOL + K.sqrt(x[0] * x[0] + x[1] * x[1]))
    x_ok = K.cmp("xtol", sn2, "<", lim * lim)
    term = 0 if not finite else (4 if (f_ok and x_ok) else 2 if f_ok else 3 if x_ok else 0)
    if not finite:
        Delta_out, case = dq, "quartered"
    elif term == 0:
        Delta_out = Delta_new
    else:
        Delta_out, case = Delta, "kept"
    accept = bool(finite) and K.cmp("accept", actual, ">", zero)
    return Delta_out, dq, term, accept, case


def solve3(K, M, b):
    c00 = M[1][1] * M[2][2] - M[1][2] * M[2][1]
    c01 = M[1][2] * M[2][0] - M[1][0] * M[2][2]
    c02 = M[1][0] * M[2][1] - M[1][1] * M[2][0]
    det = M[0][0] * c00 + M[0][1] * c01 + M[0][2] * c02
    idet = K.div(1.0, det)
    c10 = M[0][2] * M[2][1] - M[0][1] * M[2][2]
    c11 = M[0][0] * M[2][2] - M[0][2] * M[2][0]
    c12 = M[0][1] * M[2][0] - M[0][0] * M[2][1]
    c20 = M[0][1] * M[1][2] - M[0][2] * M[1][1]
    c21 = M[0][2] * M[1][0] - M[0][0] * M[1][2]
    c22 = M[0][0] * M[1][1] - M[0][1] * M[1][0]
    return [(c00 * b[0] + c10 * b[1] + c20 * b[2]) * idet, (c01 * b[0] + c11 * b[1] + c21 * b[2]) * idet, (c02 * b[0] + c12 * b[1] + c22 * b[2]) * idet]


def _eliminate(K, A, R):
    """Gaussian elimination with partial pivoting (the first of equal pivots, as idamax) on A with right-hand sides R[3][k]."""
    swaps = []
    for c in range(2):
        pv = c
        for i in range(c + 1, 3):
            if K.cmp("pivot%d" % c, K.fabs(A[i][c]), ">", K.fabs(A[pv][c])):
                pv = i
        swaps.append(pv != c)
        if pv != c:
            A[c], A[pv] = A[pv], A[c]
            R[c], R[pv] = R[pv], R[c]
        piv = K.rcp(A[c][c])
        for i in range(c + 1, 3):
            l = A[i][c] * piv
            for j in range(c + 1, 3):
                A[i][j] = A[i][j] - l * A[c][j]
            for j in range(len(R[i])):
                R[i][j] = R[i][j] - l * R[c][j]
    return swaps


def solve3_ge(K, M, b):
    A = [[K.num(v) for v in row] for row in M]
    R = [[K.num(v)] for v in b]
    swaps = _eliminate(K, A, R)
    x2 = K.div(R[2][0], A[2][2])
    x1 = K.div(R[1][0] - A[1][2] * x2, A[1][1])
    x0 = K.div((R[0][0] - A[0][1] * x1) - A[0][2] * x2, A[0][0])
    return [x0, x1, x2], swaps


def mat3_inverse(K, M):
    """mat3_solve(M, I): back substitution with the reciprocals of the diagonal."""
    A = [[K.num(v) for v in row] for row in M]
    R = [[K.num(1.0 if i == j else 0.0) for j in range(3)] for i in range(3)]
    _eliminate(K, A, R)
    r0, r1, r2 = K.rcp(A[0][0]), K.rcp(A[1][1]), K.rcp(A[2][2])
    X = [[None] * 3 for _ in range(3)]
    for j in range(3):
        X[2][j] = R[2][j] * r2
        X[1][j] = (R[1][j] - A[1][2] * X[2][j]) * r1
        X[0][j] = ((R[0][j] - A[0][1] * X[1][j]) - A[0][2] * X[2][j]) * r0
    return X


# ------------------------------------------------------------------ rows of the probe
def _mat(K, row, r, c, at=0):
    return [[K.num(row[at + i * c + j]) for j in range(c)] for i in range(r)]


def _vec(K, row, n, at):
    return [K.num(row[at + i]) for i in range(n)]


def _full(row):
    r = [0.0] * LSQ_IN
    r[:len(row)] = [float(v) for v in row]
    return r


def run(K, kind, row):
    """One problem row through the restated functions: (result row of LSQ_OUT entries, info for the fixture)."""
    with np.errstate(all="ignore"):
        return _run(K, kind, row)


def _run(K, kind, row):
    q = _full(row)
    z = K.num(0.0)
    out = [z] * LSQ_OUT
    info = {}
    if kind == "SCALAR":
        x = K.num(q[0])
        out[0], out[1] = K.rcp(x), K.sqrt(x)
    elif kind in ("SVD2", "SVD4"):
        if kind == "SVD4" and int(q[12]) == 1:
            s, V, uf = svd_aug1(K, [K.num(q[0]), K.num(q[2])], _vec(K, q, 2, 8))
            out[0], out[2], out[6] = s[0], V[0][0], uf[0]
        else:
            A, f = (_mat(K, q, 2, 2), _vec(K, q, 2, 4)) if kind == "SVD2" else (_mat(K, q, 4, 2), _vec(K, q, 4, 8))
            s, V, uf = svd_mx2(K, A, f)
            out[0:8] = [s[0], s[1], V[0][0], V[0][1], V[1][0], V[1][1], uf[0], uf[1]]
    elif kind == "STEP":
        p, alpha, predicted, lm, axis, iters = next_step(K, _mat(K, q, 2, 2), _vec(K, q, 2, 4), K.num(q[6]), K.num(q[7]))
        out[0:6] = [p[0], p[1], alpha, predicted, K.num(lm), K.num(axis)]
        info["iters"] = iters
    elif kind == "STEPN":
        N = int(q[12])
        if N == 1:
            d = svd_aug1(K, [K.num(q[0]), K.num(q[2])], _vec(K, q, 2, 8))
        else:
            d = svd_mx2(K, _mat(K, q, 4, 2), _vec(K, q, 4, 8))
        p, alpha, iters = solve_tr_n(K, N, d, N, K.num(q[13]), K.num(q[14]))
        out[0:N] = p
        out[2] = alpha
        info["iters"] = iters
    elif kind == "SELECT":
        N = int(q[19])
        pick = lambda at: [K.num(q[at + i]) for i in range(N)]
        Jh = [[K.num(q[2])]] if N == 1 else _mat(K, q, 2, 2, 2)
        step, steph, pred, path, cand = select_step(K, N, pick(0), Jh, pick(6), pick(8), pick(10), pick(12), pick(14), K.num(q[16]), K.num(q[17]), K.num(q[18]))
        out[0:N] = step
        out[2:2 + N] = steph
        out[4] = pred
        info["path"] = path
        if cand:
            info["cand"] = {k: [float(v) for v in c[0]] for k, c in cand.items()}
    elif kind == "UPDATE":
        D, dq, term, accept, case = tr_update(K, q[0] != 0.0, _vec(K, q, 2, 1), _vec(K, q, 2, 3), K.num(q[5]), K.num(q[6]), K.num(q[7]), K.num(q[8]))
        out[0:4] = [D, dq, K.num(term), K.num(1.0 if accept else 0.0)]
        info["case"] = case
    elif kind == "SOLVE3":
        M, b = _mat(K, q, 3, 3), _vec(K, q, 3, 9)
        x = solve3(K, M, b)
        y, swaps = solve3_ge(K, M, b)
        X = mat3_inverse(K, M)
        out[0:3], out[3:6] = x, y
        out[6:15] = [X[i][j] for i in range(3) for j in range(3)]
        info["swaps"] = swaps
    else:
        raise KeyError(kind)
    return [float(v) for v in out], info


def scipy_row(kind, row):
    """The same result row from NumPy's / SciPy's own functions (float64, LAPACK), with the iteration count where SciPy has one."""
    from scipy import linalg
    from scipy.optimize._lsq import common, trf
    q = np.array(_full(row))
    out = np.zeros(LSQ_OUT)
    info = {}
    with np.errstate(all="ignore"):
        if kind == "SCALAR":
            out[0], out[1] = 1.0 / q[0], np.sqrt(q[0])
        elif kind in ("SVD2", "SVD4", "STEP", "STEPN"):
            N = 2 if kind in ("SVD2", "STEP") else int(q[12])
            if kind in ("SVD2", "STEP"):
                A, f = q[0:4].reshape(2, 2), q[4:6]
            elif N == 1:
                A, f = q[[0, 2]].reshape(2, 1), q[8:10]
            else:
                A, f = q[0:8].reshape(4, 2), q[8:12]
            if not np.isfinite(A).all():
                return None, info
            U, s, Vt = np.linalg.svd(A, full_matrices=False)
            V, uf = Vt.T, U.T @ f
            if kind in ("SVD2", "SVD4"):
                out[0:N] = s
                for r in range(N):
                    for i in range(N):
                        out[2 + 2 * r + i] = V[r][i]
                out[6:6 + N] = uf
            else:
                Delta, alpha = (q[6], q[7]) if kind == "STEP" else (q[13], q[14])
                p, alpha, n_iter = common.solve_lsq_trust_region(N, N, uf, s, V, Delta, initial_alpha=alpha)
                out[0:N] = p
                out[2] = alpha
                info["iters"] = -1 if (n_iter == 0 and alpha == 0.0) else int(n_iter)
                if kind == "STEP":
                    out[3] = -common.evaluate_quadratic(A, A.T @ f, p)
                    out[4] = out[5] = np.nan
        elif kind == "SELECT":
            N = int(q[19])
            pick = lambda at: q[at:at + N].copy()
            Jh = q[2:3].reshape(1, 1) if N == 1 else q[2:6].reshape(2, 2)
            try:
                step, steph, pred = trf.select_step(pick(0), Jh.copy(), pick(6), pick(8), pick(10), pick(12), pick(14), q[16], np.full(N, q[17]), np.full(N, np.inf), q[18])
            except ValueError:                               # SciPy refuses a step outside its region; the device function has a value there
                return None, info
            out[0:N], out[2:2 + N], out[4] = step, steph, pred
        elif kind == "UPDATE":
            finite, p, x, cost, cost_new, predicted, Delta = q[0] != 0, q[1:3], q[3:5], q[5], q[6], q[7], q[8]
            sn = np.linalg.norm(p)
            if not finite:
                out[0:4] = [0.25 * sn, 0.25 * sn, 0.0, 0.0]
            else:
                actual = cost - cost_new
                Dn, ratio = common.update_tr_radius(Delta, actual, predicted, sn, sn > 0.95 * Delta)
                term = common.check_termination(actual, cost, sn, np.linalg.norm(x), ratio, FTOL, XTOL)
                out[0:4] = [Delta if term else Dn, 0.25 * sn, float(term or 0), float(actual > 0)]
        elif kind == "SOLVE3":
            M, b = q[0:9].reshape(3, 3), q[9:12]
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                x = linalg.solve(M, b)
                out[0:3] = out[3:6] = x
                out[6:15] = linalg.inv(M).ravel()
    return [float(v) for v in out], info


# ------------------------------------------------------------------ discrete outcomes and figures of a result row
def discrete(kind, prob, row):
    """The discrete outcome a result row shows, in the form the fixture stores it under "disc"."""
    q = _full(prob["in"])
    if kind == "STEP":
        return {"lm": int(row[4]) if row[4] == row[4] else None, "axis": int(row[5]) if row[5] == row[5] else None, "alpha0": bool(row[2] == 0.0)}
    if kind == "STEPN":
        return {"alpha0": bool(row[2] == 0.0)}
    if kind == "SELECT":
        N = int(q[19])
        cand = prob["ex"].get("cand")
        if not cand:
            return {"path": "inside"}
        dist = {k: max(abs(row[i] - c[i]) for i in range(N)) for k, c in cand.items()}
        return {"path": min(sorted(dist), key=lambda k: dist[k])}
    if kind == "UPDATE":
        D = q[8]
        case = "kept" if row[0] == D else "doubled" if row[0] == 2.0 * D else "quartered"
        return {"term": int(row[2]), "accept": int(row[3]), "case": case}
    return {}


def _rel(err, scale):
    return 0.0 if err == 0.0 else err / scale if scale > 0.0 else math.inf


def _unit(err, kappa):
    """A relative error in units of eps kappa; no correct digit (relative error 1) is the most a figure says."""
    if err != err:
        return math.inf
    return min(err, 1.0) / (EPS * max(kappa, 1.0))


def exact_reg_step(A, f, alpha, Delta):
    """-(A^T A + alpha I)^-1 A^T f for an m x 2 matrix, exactly (Fraction): (the step rescaled to Delta, |unscaled step| / Delta)."""
    A = [[Fraction(float(v)) for v in r] for r in A]
    f = [Fraction(float(v)) for v in f]
    al = Fraction(float(alpha))
    a = sum(r[0] * r[0] for r in A) + al
    b = sum(r[0] * r[1] for r in A)
    c = sum(r[1] * r[1] for r in A) + al
    g0 = sum(r[0] * v for r, v in zip(A, f))
    g1 = sum(r[1] * v for r, v in zip(A, f))
    det = a * c - b * b
    p0, p1 = -(c * g0 - b * g1) / det, -(a * g1 - b * g0) / det
    n2 = p0 * p0 + p1 * p1
    if n2 == 0:
        return [math.nan, math.nan], math.nan
    D = Fraction(float(Delta))
    sc = lambda p: math.copysign(float(Delta) * math.sqrt(float(p * p / n2)), float(p)) if p != 0 else 0.0
    return [sc(p0), sc(p1)], math.sqrt(float(n2 / (D * D)))


def _vec_err(a, b):
    n = max(abs(v) for v in b)
    return _rel(max(abs(x - y) for x, y in zip(a, b)), n)


def figures(kind, prob, row):
    """{class: figure} of a result row against the exact answers of the fixture; a class is "<first tag>[:<part>]".  STEP and STEPN
    rows are measured at their OWN alpha (exact_reg_step); "phi" is ||p(alpha)| / Delta - 1|, not in eps units."""
    q, ex, tag = _full(prob["in"]), prob["ex"], prob["t"][0]
    row = [float(v) for v in row]
    fig = {}
    if kind == "SCALAR":
        for i, name in ((0, "rcp"), (1, "sqrt")):
            r, resid = ex[name]
            if not (math.isfinite(r) and r != 0.0 and math.isfinite(row[i])):
                fig[name] = 0.0 if (row[i] == r or (row[i] != row[i] and r != r)) else math.inf
            else:
                fig[name] = abs((row[i] - r) / (math.ulp(r)) - resid)
        return fig
    if kind in ("SVD2", "SVD4"):
        N = 2 if kind == "SVD2" else int(q[12])
        s = ex["row"][0:N]
        kappa = s[0] / s[-1] if s[-1] > 0 else 1.0
        fn = max(abs(v) for v in (q[4:6] if kind == "SVD2" else q[8:8 + 2 * N])) or 1.0
        e = max(_rel(abs(row[i] - s[i]), s[i]) for i in range(N))
        if "equal_sv" in prob["t"]:                      # V is not unique: the Gauss-Newton vector V (uf / s) is
            gn = lambda r: [sum(r[2 + 2 * k + i] * r[6 + i] / r[i] for i in range(N)) for k in range(N)]
            e = max(e, _vec_err(gn(row), gn(ex["row"])))
        else:
            for i in range(N):
                if s[i] == 0.0 and N == 2 and s[0] == 0.0:
                    continue
                sg = math.copysign(1.0, sum(row[2 + 2 * k + i] * ex["row"][2 + 2 * k + i] for k in range(N)))
                e = max(e, max(abs(sg * row[2 + 2 * k + i] - ex["row"][2 + 2 * k + i]) for k in range(N)))
                e = max(e, abs(sg * row[6 + i] - ex["row"][6 + i]) / fn)
        fig[tag] = _unit(e if all(v == v for v in row[0:8]) else math.nan, kappa)
        return fig
    if kind in ("STEP", "STEPN"):
        N = 2 if kind == "STEP" else int(q[12])
        A, f = ([q[0:2], q[2:4]], q[4:6]) if kind == "STEP" else ([q[0:2], q[2:4], q[4:6], q[6:8]], q[8:12])
        Delta = q[6] if kind == "STEP" else q[13]
        s, alpha = ex["s"], row[2]
        if kind == "STEP" and row[5] >= 0:               # rank one: exactly (0, -+Delta)
            fig[tag] = 0.0 if row[0:2] == ex["row"][0:2] and alpha == 0.0 else math.inf
        elif "nan" in prob["t"]:
            fig[tag] = 0.0 if all(v != v for v in row[0:N]) else math.inf
        elif alpha == 0.0:
            fig[tag] = _unit(_vec_err(row[0:N], ex["gn"]), s[0] / s[-1] if s[-1] > 0 else 1.0)
        elif N == 1:
            want = -math.copysign(Delta, ex["uf0"])
            fig[tag] = _unit(abs(row[0] - want) / Delta, 1.0)
        else:
            p, ratio = exact_reg_step(A, f, alpha, Delta)
            kappa = math.sqrt((s[0] * s[0] + alpha) / (s[1] * s[1] + alpha)) if alpha > 0 else math.inf
            fig[tag] = _unit(_vec_err(row[0:2], p), kappa)
            fig[tag + ":phi"] = abs(ratio - 1.0)
        if kind == "STEP" and "nan" not in prob["t"] and all(math.isfinite(v) for v in row[0:4]):
            J = [[Fraction(v) for v in r] for r in A]
            ff, p = [Fraction(v) for v in f], [Fraction(v) for v in row[0:2]]
            g = [J[0][0] * ff[0] + J[1][0] * ff[1], J[0][1] * ff[0] + J[1][1] * ff[1]]
            Js = [J[0][0] * p[0] + J[0][1] * p[1], J[1][0] * p[0] + J[1][1] * p[1]]
            quad, lin = (Js[0] * Js[0] + Js[1] * Js[1]) / 2, [p[0] * g[0], p[1] * g[1]]
            exact, scale = -(quad + lin[0] + lin[1]), float(quad + abs(lin[0]) + abs(lin[1]))
            fig[tag + ":pred"] = _unit(_rel(abs(float(Fraction(row[3]) - exact)), scale), 1.0)
        return fig
    if kind == "SELECT":
        N = int(q[19])
        e = max(_vec_err(row[0:N], ex["row"][0:N]), _vec_err(row[2:2 + N], ex["row"][2:2 + N]))
        fig[tag] = _unit(e, 1.0)
        fig[tag + ":pred"] = _unit(_rel(abs(row[4] - ex["row"][4]), ex["pred_scale"]), 1.0)
        return fig
    if kind == "UPDATE":
        fig[tag] = _unit(max(_rel(abs(row[1] - ex["row"][1]), abs(ex["row"][1])), _rel(abs(row[0] - ex["row"][0]), abs(ex["row"][0]))), 1.0)
        return fig
    if kind == "SOLVE3":
        k1 = ex["cond1"]
        fig[tag + ":cof"] = _unit(_vec_err(row[0:3], ex["row"][0:3]), k1)
        fig[tag + ":ge"] = _unit(_vec_err(row[3:6], ex["row"][3:6]), k1)
        fig[tag + ":inv"] = _unit(_vec_err(row[6:15], ex["row"][6:15]), k1)
        return fig
    raise KeyError(kind)


def worst(kind, problems, rows):
    """Worst figure per class over a kind's problems; rows may hold None (SciPy has no answer)."""
    w = {}
    for p, r in zip(problems, rows):
        if r is None:
            continue
        for k, v in figures(kind, p, r).items():
            w[k] = max(w.get(k, 0.0), v)
    return w
