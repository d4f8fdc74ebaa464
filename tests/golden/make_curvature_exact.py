#!/usr/bin/env python3
"""Generate tests/golden/golden_curvature_exact.json.gz: derivatives of the class logs L_k = log S_k of small models in exact arithmetic.

    python tests/golden/make_curvature_exact.py            # (re)write the fixture
    python tests/golden/make_curvature_exact.py --check    # regenerate and compare with the committed fixture

Deterministic, CPU only, does not use the reference.  Every model is one of the exact-spectrum engine (trueEPS, cpfit: the rates of
the two-population intervals are the inputs, so the spectrum is a smooth function of the parameters - the two migration rates, and
with D = 3 a pulse strength) and every spectrum comes from tests/exact_spectrum.py.  Per model: the C-ABI inputs of
misti_amd.engine.Engine.  Per point: split, x, abs_step, and

  steps[]   per rel_step of the ladder: h and the stencil of optimize.curvature_stencil (the device's candidates bit for bit), the
            exact spectrum (7 classes) and the exact class logs L_k at every stencil candidate, and the rule of
            optimize.curvature_from_spectra applied to those logs in 50-digit arithmetic: "the exact stencil" dlog, d2log
  exact     the derivatives themselves - central differences at h_i = 1e-20 max(|x_i|, 1) with 80 working digits (truncation
            ~1e-40 relative; repeated at 1e-18 and asserted to agree to 1e-30) - and grad, hess, the observed and the sandwich
            standard errors they give against the point's table, all in that arithmetic
  table     1 + 16 rows of counts (row 0 plays the data): optimize.parametric_rows at the centre's spectrum, 1e6 sites, fixed seed

A boundary point (x_i - h_i < 0: MISTI_CURV_BOUNDARY) has none of these.  `correction[]` is the part through the lambda-correction
(cpfit, corrected rates) for three of the points - see "Part B" below: the exact derivatives with the rates the 100-digit root of the
cpfit system, and per ladder step the float64 oracle's spectra and its own errors against them (`--correction-only` remakes this part
on top of the committed smooth part; the result is the full generation's).  The generator asserts what the tests rely on: the
q-straddling point has its centre on the series side (q <= 96) and a +h candidate on the contour side at every ladder step; at
rel_step >= 1e-3 the derived bound of tests/curvature_exact.py is below 1e-3 of max |d2L| for every point but the one with a rate
of 1e-6; at rel_step 1e-2 and 1e-3 the standard-error bound applies (< 0.1) to every point but that one.
Values are 50-digit strings, doubles are written by repr."""
import argparse
import copy
import gzip
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import mpmath as mp                      # noqa: E402
import numpy as np                       # noqa: E402
import exact_spectrum as ex              # noqa: E402
import curvature_exact as cx             # noqa: E402
from make_exact_spectrum import MIG, Q_SWITCH, hit_q     # noqa: E402
from misti_amd import optimize as opt    # noqa: E402

OUT = cx.FIXTURE
DIGITS = 50
DPS_STENCIL, DPS_EXACT = 50, 80
H_EXACT, H_PROOF = "1e-20", "1e-18"
AGREE = "1e-30"
N_SITES, N_BOOT, SEED = 10 ** 6, 16, 20261019
BOUNDARY_ABS_STEP = 1e-3

T4, LH4 = [0.5, 0.8, 1.0], [[1.0, 1.4], [0.8, 0.6], [1.0, 1.0], [0.9, 0.9]]
T5, LH5 = [0.4, 0.7, 1.1, 0.9], [[1.2, 0.8], [0.9, 1.1], [1.0, 1.0], [0.7, 0.7], [1.3, 1.3]]


def model(name, times, lh, bands, points, pulses=(), n_param=2, sample_date=0, unfolded=False):
    return dict(name=name, times=[float(t) for t in times], lh=[[float(a), float(b)] for a, b in lh], bands=[list(b) for b in bands],
                pulses=[list(p) for p in pulses], n_param=n_param, sample_date=sample_date, unfolded=unfolded, points=points)


def point(name, split, x, ladder=cx.LADDER, abs_step=0.0, boundary=False, tiny=False):
    return dict(name=name, split=float(split), x=[float(v) for v in x], abs_step=float(abs_step), boundary=boundary, tiny_rate=tiny,
                ladder=[float(r) for r in ladder])


def models():
    out = []
    # the near-boundary pair: under a relative step alone x - h = x (1 - rel_step) never leaves the positive side, so the pair takes an
    # absolute step that wins (h = 1e-3 at the default rel_step): x_0 - h is 1e-7 above 0 at one point and 1e-7 below at the other
    out.append(model("two_way_folded", T4, LH4, MIG,
                     [point("interior", 2, (0.2, 0.5)),
                      point("rate_1e-6", 2, (1e-6, 0.5), tiny=True),
                      point("one_step_inside", 2, (BOUNDARY_ABS_STEP + 1e-7, 0.5), ladder=(cx.DEFAULT_STEP,), abs_step=BOUNDARY_ABS_STEP),
                      point("one_step_outside", 2, (BOUNDARY_ABS_STEP - 1e-7, 0.5), ladder=(cx.DEFAULT_STEP,), abs_step=BOUNDARY_ABS_STEP,
                            boundary=True)]))
    out.append(model("two_way_unfolded", T4, LH4, MIG, [point("interior", 2, (0.2, 0.5))], unfolded=True))
    # D = 3, M = 19: the costliest model keeps four steps of the ladder.  Unfolded, and rates of this size, because the pulse strength
    # is nearly collinear with the rate of the same direction otherwise (condition number of the Hessian ~1e3 against 26 here)
    out.append(model("pulse_d3", T5, LH5, MIG, [point("pulse", 2, (1.0, 0.5, 0.5), ladder=(1e-1, 1e-2, 1e-3, 1e-4))],
                     pulses=[(0, 1, 0.0, 2)], n_param=3, unfolded=True))
    out.append(model("ancient_sd1", T5, LH5, [(0, 1, -1, 0.0, 0), (1, 1, -1, 0.0, 1)], [point("ancient", 2, (0.3, 0.6))], sample_date=1))
    out.append(model("fractional", T4, LH4, MIG, [point("split_1.5", 1.5, (0.4, 0.2))]))
    # the centre exactly ON the switch (q = 96 is the series' side: q <= Q_SWITCH), so that +h_0 of any size is on the contour's
    m0, m1 = 2.0, 1.0
    la, T = hit_q(Q_SWITCH, m0, m1)
    out.append(model("straddle_q96", [T, 0.5, 0.7], [[la, la], [1.0, 1.25], [0.8, 0.8], [0.9, 0.9]], MIG, [point("straddle", 1, (m0, m1))]))
    return out


# ---- one spectrum = one job ------------------------------------------------------------------------------------------------------------
def _s(v):
    return mp.nstr(v, DIGITS, min_fixed=1, max_fixed=0)


def _with_params(m, split, x0, params):
    """The oracle model of the point (its rates and grid: they do not depend on the parameters under trueEPS) with the mpf
    `params` in the place of the doubles."""
    om = copy.copy(ex.oracle_model(m, split, x0))
    s = om.splitT
    om.mi = [[mp.mpf(0), mp.mpf(0)] for _ in range(om.numT)]
    om.pu = [[mp.mpf(0), mp.mpf(0)] for _ in range(om.numT)]
    val = lambda v, p: params[p] if p >= 0 else mp.mpf(float(v))
    for pop, start, end, v, p in m["bands"]:
        for it in range(start, s if end == -1 else end):
            om.mi[it][pop] = val(v, p)
    for pop, t, v, p in m["pulses"]:
        om.pu[t][pop] = val(v, p)
    return om


_memo = {}
_interval = ex.interval


def _interval_memo(M, x, T):
    # an interval that no parameter reaches (before the sample date) is the same for every candidate of a worker
    bits = lambda v: mp.mpf(v)._mpf_
    key = (mp.mp.dps, tuple(bits(v) for v in M), tuple(bits(v) for v in x), None if T is None else bits(T))
    if key not in _memo:
        if len(_memo) > 64:
            _memo.clear()
        _memo[key] = _interval(M, x, T)
    return _memo[key]


def spectrum_job(job):
    m, split, x0, params, dps = job
    with mp.workdps(dps):
        # a stencil candidate comes as the hexadecimal form of its double and is taken at exactly that value (a decimal repr is
        # another number: half an ulp of the abscissa, which a second difference divides by h^2)
        exact = lambda v: mp.mpf(float.fromhex(v)) if "x" in v else mp.mpf(v)
        J = ex.spectrum(_with_params(m, split, x0, [exact(v) for v in params]), dps, interval=_interval_memo)
        return [mp.nstr(v, dps, min_fixed=1, max_fixed=0) for v in J]


def _key(m, p, params, dps):
    shape = json.dumps([m["times"], m["lh"], m["bands"], m["pulses"], m["sample_date"], p["split"]])
    return (shape, tuple(params), dps)


# ---- the rule in mpmath ----------------------------------------------------------------------------------------------------------------
def mp_stencil(x, h):
    """optimize.curvature_stencil's layout for one point, in mpf."""
    D = len(x)
    pts = [list(x)]
    for i in range(D):
        for s in (1, -1):
            v = list(x)
            v[i] = x[i] + s * h[i]
            pts.append(v)
    for i in range(D):
        for j in range(i + 1, D):
            for si, sj in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                v = list(x)
                v[i], v[j] = x[i] + si * h[i], x[j] + sj * h[j]
                pts.append(v)
    return pts


def mp_classes(J, unfolded):
    return list(J) if unfolded else [J[0] + J[6], J[1] + J[5], J[2] + J[4], J[3]]


def mp_rule(L, h):
    """optimize.curvature_from_spectra's three quotients on logs L[M][K] in mpf: (dlog[D][K], d2log[D][D][K])."""
    D, K = len(h), len(L[0])
    d1 = [[(L[1 + 2 * i][k] - L[2 + 2 * i][k]) / (2 * h[i]) for k in range(K)] for i in range(D)]
    d2 = [[None] * D for _ in range(D)]
    q = 0
    for i in range(D):
        d2[i][i] = [(L[1 + 2 * i][k] - 2 * L[0][k] + L[2 + 2 * i][k]) / (h[i] * h[i]) for k in range(K)]
        for j in range(i + 1, D):
            c = 1 + 2 * D + 4 * q
            d2[i][j] = d2[j][i] = [(L[c][k] - L[c + 1][k] - L[c + 2][k] + L[c + 3][k]) / (4 * h[i] * h[j]) for k in range(K)]
            q += 1
    return d1, d2


def mp_errors(d1, d2, table, unfolded):
    """grad, hess of row 0 and the observed / sandwich standard errors over rows 1.., as optimize's functions define them, in mpf."""
    D, K = len(d1), len(d1[0])
    f = [[mp.mpf(v) for v in mp_classes(r[1:], unfolded)] for r in table]
    grad = [mp.fsum(f[0][k] * d1[i][k] for k in range(K)) for i in range(D)]
    H = mp.matrix(D, D)
    for i in range(D):
        for j in range(D):
            H[i, j] = mp.fsum(f[0][k] * d2[i][j][k] for k in range(K))
    boot = f[1:]
    n = len(boot)
    mean = [mp.fsum(b[k] for b in boot) / n for k in range(K)]
    Cm = mp.matrix(K, K)
    for a in range(K):
        for b in range(K):
            Cm[a, b] = mp.fsum((r[a] - mean[a]) * (r[b] - mean[b]) for r in boot) / (n - 1)
    A = mp.matrix(D, K)
    for i in range(D):
        for k in range(K):
            A[i, k] = d1[i][k]
    Hi = mp.inverse(H)
    obs = mp.inverse(-H)
    sand = Hi * (A * Cm * A.T) * Hi.T
    return grad, H, [mp.sqrt(obs[i, i]) for i in range(D)], [mp.sqrt(sand[i, i]) for i in range(D)]


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------
def _exact_h(x, scale):
    return [mp.mpf(scale) * max(abs(mp.mpf(v)), 1) for v in x]


def plan(ms):
    """Every spectrum the fixture needs, once: {key: job}."""
    jobs = {}
    for m in ms:
        for p in m["points"]:
            if p["boundary"]:
                continue
            for rel in p["ladder"]:
                pts, _, boundary = opt.curvature_stencil(p["x"], rel, p["abs_step"])
                assert not boundary.any(), (m["name"], p["name"], rel)
                for c in pts[0]:
                    par = tuple(float(v).hex() for v in c)
                    jobs.setdefault(_key(m, p, par, DPS_STENCIL), (m, p["split"], p["x"], par, DPS_STENCIL))
            with mp.workdps(DPS_EXACT):
                x = [mp.mpf(v) for v in p["x"]]
                for scale in (H_EXACT, H_PROOF):
                    for c in mp_stencil(x, _exact_h(p["x"], scale)):
                        par = tuple(mp.nstr(v, DPS_EXACT, min_fixed=1, max_fixed=0) for v in c)
                        jobs.setdefault(_key(m, p, par, DPS_EXACT), (m, p["split"], p["x"], par, DPS_EXACT))
    return jobs


def _logs(spectra, unfolded):
    return [[mp.log(v) for v in mp_classes(J, unfolded)] for J in spectra]


def _max_q(m, p, params):
    om = ex.oracle_model(m, p["split"], [float(v) for v in params])
    return max(ex.device_q(om, t) for t in range(min(om.splitT, om.numT - 1)))


def assemble(ms, got):
    spec = lambda m, p, par, dps: [mp.mpf(v) for v in got[_key(m, p, par, dps)]]
    for pi, (m, p) in enumerate((m, p) for m in ms for p in m["points"]):
        unf = m["unfolded"]
        ladder = p.pop("ladder")
        if p["boundary"]:
            _, _, boundary = opt.curvature_stencil(p["x"], cx.DEFAULT_STEP, p["abs_step"])
            assert boundary.all()
            continue
        # -- the exact derivatives, and the proof of their step
        with mp.workdps(DPS_EXACT):
            x = [mp.mpf(v) for v in p["x"]]
            ders = []
            for scale in (H_EXACT, H_PROOF):
                h = _exact_h(p["x"], scale)
                pars = [tuple(mp.nstr(v, DPS_EXACT, min_fixed=1, max_fixed=0) for v in c) for c in mp_stencil(x, h)]
                ders.append(mp_rule(_logs([spec(m, p, par, DPS_EXACT) for par in pars], unf), h))
            (d1, d2), (e1, e2) = ders
            D, K = len(d1), len(d1[0])
            agree = mp.mpf(AGREE)
            for i in range(D):
                for k in range(K):
                    assert abs(d1[i][k] - e1[i][k]) <= agree * max(1, abs(d1[i][k])), (m["name"], p["name"], "dlog", i, k)
                    for j in range(D):
                        assert abs(d2[i][j][k] - e2[i][j][k]) <= agree * max(1, abs(d2[i][j][k])), (m["name"], p["name"], "d2log", i, j, k)
            centre = spec(m, p, tuple(mp.nstr(v, DPS_EXACT, min_fixed=1, max_fixed=0) for v in x), DPS_EXACT)
            rows, st = opt.parametric_rows(np.array([float(v) for v in centre]), 1 + N_BOOT, N_SITES, float(N_SITES), seed=SEED + pi)
            assert (st == 0).all()
            table = [[int(v) for v in r] for r in rows]
            grad, H, se_obs, se_sand = mp_errors(d1, d2, table, unf)
            p["table"] = table
            p["exact"] = dict(dlog=[[_s(v) for v in r] for r in d1], d2log=[[[_s(v) for v in r] for r in rr] for rr in d2],
                              grad=[_s(v) for v in grad], hess=[[_s(H[i, j]) for j in range(D)] for i in range(D)],
                              se_observed=[_s(v) for v in se_obs], se_sandwich=[_s(v) for v in se_sand])
            max_d2 = max(abs(float(d2[i][j][k])) for i in range(D) for j in range(D) for k in range(K))
            hess_exact = np.array([[float(H[i, j]) for j in range(D)] for i in range(D)])
        # -- the ladder
        p["steps"] = []
        for rel in ladder:
            pts, h, _ = opt.curvature_stencil(p["x"], rel, p["abs_step"])
            with mp.workdps(DPS_STENCIL):
                spectra = [spec(m, p, tuple(float(v).hex() for v in c), DPS_STENCIL) for c in pts[0]]
                L = _logs(spectra, unf)
                s1, s2 = mp_rule(L, [mp.mpf(float(v)) for v in h[0]])
                p["steps"].append(dict(rel_step=rel, h=[float(v) for v in h[0]], stencil=[[float(v) for v in c] for c in pts[0]],
                                       jafs=[[_s(v) for v in J] for J in spectra], logs=[[_s(v) for v in r] for r in L],
                                       dlog=[[_s(v) for v in r] for r in s1], d2log=[[[_s(v) for v in r] for r in rr] for rr in s2]))
            # what the tests rely on
            b = cx.bounds(np.array([[float(v) for v in J] for J in spectra]), h[0], unf, table[0])
            if not p["tiny_rate"]:
                if rel >= 1e-3:
                    assert b["derived_d2log"].max() < 1e-3 * max_d2, (m["name"], p["name"], rel, b["derived_d2log"].max(), max_d2)
                if rel in (1e-2, 1e-3):
                    assert cx.se_bound(hess_exact, b["hess"]) < cx.SE_BOUND_APPLIES, (m["name"], p["name"], rel)
            if m["name"].startswith("straddle"):
                qs = [_max_q(m, p, c) for c in pts[0]]
                assert qs[0] <= Q_SWITCH and qs[1] > Q_SWITCH, (rel, qs[:3])
                p["steps"][-1]["q"] = qs
    return dict(dps_stencil=DPS_STENCIL, dps_exact=DPS_EXACT, digits=DIGITS, h_exact=H_EXACT, q_switch=Q_SWITCH, n_sites=N_SITES,
                models=ms)


# ---- Part B: through the lambda-correction (cpfit, corrected rates) -------------------------------------------------------------------
# S(theta) is now the spectrum taken with the ROOT of the cpfit system per two-population interval (oracle/misti_oracle.py,
# _PairChain._residual_cp: the pair chain's probability of no coalescence, from either start, equals that of the input rates) and the
# closed forms after the split.  The exact reference is that root to DPS_ROOT digits; the oracle (SciPy's least_squares, float64) is
# measured against it over the same stencils, and its own error is what the GPU test scales (tests/test_gpu_curvature_exact.py).
CORRECTION = (("two_way_folded", "interior"), ("pulse_d3", "pulse"), ("ancient_sd1", "ancient"))
DPS_ROOT = 100
ROOT_TOL, ROOT_RESIDUAL, ROOT_NEAR_ORACLE = "1e-90", "1e-40", 1e-6
QUALIFIES = 0.1                  # a step is held only where the oracle's own error is below this fraction of the exact value
PREC, NORM_EPS = 1e-10, 0.02     # solve_lambda_system's two thresholds: neither branch may be near (asserted)


def _oracle_corrected(m, split, params):
    """ex.oracle_model with the lambda-correction switched on (trueEPS off): the project's float64 oracle."""
    from oracle.misti_oracle import OracleModel
    s = int(split) + (1 if split % 1 else 0)
    val = lambda v, p: float(params[p]) if p >= 0 else float(v)
    mi = [(pop + 1, start, s if end == -1 else end, val(v, p), 0) for pop, start, end, v, p in m["bands"]]
    pu = [(pop + 1, t, val(v, p), 0) for pop, t, v, p in m["pulses"]]
    om = OracleModel(m["times"], m["lh"], [0] * 8, split, mi, pu, trueEPS=False, cpfit=True, unfolded=m["unfolded"],
                     sampleDate=m["sample_date"])
    om.map_parameters([])
    if not om.correct_lambdas():
        raise ValueError("rate correction failed")
    return om


def _oracle_spectrum(m, split, params):
    om = _oracle_corrected(m, split, params)
    om.jaf_spectrum()
    J = np.array(om.JAFS)
    return J / J.sum()


def _pair_matrix(l, mu):
    return mp.matrix([[-2 * mu[0] - l[0], 0, mu[1]], [0, -2 * mu[1] - l[1], mu[0]], [2 * mu[0], 2 * mu[1], -mu[0] - mu[1]]])


def _pair_pulse(p0, pu):
    rate = pu[0] + pu[1]
    if not rate > 0:
        return p0
    a = 0 if pu[0] > 0 else 1
    b = 1 - a
    out = []
    for k in (0, 1):
        n = [None, None, None]
        n[a] = p0[k][a] * (1 - rate) ** 2
        n[b] = p0[k][a] * rate ** 2 + p0[k][b] + p0[k][2] * rate
        n[2] = p0[k][a] * 2 * (1 - rate) * rate + p0[k][2] * (1 - rate)
        out.append(n)
    return out


def mp_corrected(m, split, x0, params, start):
    """OracleModel.correct_lambdas (cpfit, no smoothing) in mpf at the working precision: the model of _with_params with `lc` the
    root of every two-population interval's cpfit system (mp.findroot from `start`, the oracle's rates) and the closed forms after
    the split.  Returns (model, largest residual)."""
    om = _with_params(m, split, x0, params)
    f = lambda v: mp.mpf(float(v))
    p0 = [[mp.mpf(1), mp.mpf(0), mp.mpf(0)], [mp.mpf(0), mp.mpf(1), mp.mpf(0)]]
    lc, worst = [None] * om.numT, mp.mpf(0)
    for t in range(om.splitT):
        p0 = _pair_pulse(p0, om.pu[t])
        mu, T, lh = om.mi[t], f(om.times[t]), [f(om.lh[t][0]), f(om.lh[t][1])]
        s = [mp.fsum(p0[0]), mp.fsum(p0[1])]
        if mu[0] + mu[1] < PREC:
            assert mu[0] + mu[1] == 0, "a migration rate between 0 and solve_lambda_system's threshold"
            A1, A2, A3, A4 = p0[0][0] / s[0], p0[0][1] / s[0], p0[1][0] / s[1], p0[1][1] / s[1]
            C1, C2 = p0[0][2] / s[0], p0[1][2] / s[1]
            Dt = A1 * A4 - A2 * A3
            X1, X2 = mp.exp(-lh[0] * T) - C1, mp.exp(-lh[1] * T) - C2
            a, b = (A4 * X1 - A2 * X2) / Dt, (-A3 * X1 + A1 * X2) / Dt
            assert a > 0 and b > 0
            l = [-mp.log(a) / T, -mp.log(b) / T]
            p0 = [[p0[k][0] * mp.exp(-l[0] * T), p0[k][1] * mp.exp(-l[1] * T), p0[k][2]] for k in (0, 1)]
        else:
            norm = lambda v: mp.sqrt(mp.fsum(c * c for c in v))
            assert norm([p0[0][i] - p0[1][i] for i in range(3)]) > 2 * NORM_EPS * min(norm(p0[0]), norm(p0[1])), "near the mean-rate branch"
            tgt = [mp.exp(-lh[k] * T) * s[k] for k in (0, 1)]
            P = [mp.matrix(p0[0]), mp.matrix(p0[1])]

            def res(a, b):
                E = mp.expm(_pair_matrix([a, b], mu) * T)
                return [mp.fsum(E * P[k]) - tgt[k] for k in (0, 1)]
            r = mp.findroot(res, (f(start[t][0]), f(start[t][1])), tol=mp.mpf(ROOT_TOL), maxsteps=60)
            l = [r[0], r[1]]
            worst = max([worst] + [abs(v) for v in res(*l)])
            E = mp.expm(_pair_matrix(l, mu) * T)
            p0 = [list(E * P[0]), list(E * P[1])]
        assert l[0] > 0 and l[1] > 0
        lc[t] = l
    nc = [mp.fsum(p0[0]), mp.fsum(p0[1])]                            # a probability, used as a log below (the reference's :353-354)
    for t in range(om.splitT, om.numT - 1):
        T = f(om.times[t])
        pnc = (mp.exp(-T * f(om.lh[t][0])) + mp.exp(nc[1] - nc[0] - T * f(om.lh[t][1]))) / (1 + mp.exp(nc[1] - nc[0]))
        lam = -mp.log(pnc) / T
        lc[t] = [lam, lam]
        nc = [nc[0] - T * lam, nc[1] - T * lam]
    t = om.numT - 1
    pr0, pr1 = mp.exp(nc[0]), mp.exp(nc[1])
    lam = (pr0 + pr1) / (pr0 / f(om.lh[t][0]) + pr1 / f(om.lh[t][1]))
    lc[t] = [lam, lam]
    om.lc = lc
    return om, worst


def correction_job(job):
    m, split, x0, params, start = job
    with mp.workdps(DPS_ROOT):
        om, worst = mp_corrected(m, split, x0, [mp.mpf(v) for v in params], start)
        J = ex.spectrum(om, DPS_ROOT, interval=_interval_memo)
        fmt = lambda v: mp.nstr(v, DPS_ROOT, min_fixed=1, max_fixed=0)
        return dict(jafs=[fmt(v) for v in J], lc=[[fmt(a), fmt(b)] for a, b in om.lc[:om.splitT]], residual=fmt(worst))


def _find(ms, model, point):
    m = next(m for m in ms if m["name"] == model)
    return m, next(p for p in m["points"] if p["name"] == point)


def plan_correction(ms):
    jobs = {}
    for model, point in CORRECTION:
        m, p = _find(ms, model, point)
        start = [[float(a), float(b)] for a, b in _oracle_corrected(m, p["split"], p["x"]).lc]
        with mp.workdps(DPS_ROOT):
            x = [mp.mpf(v) for v in p["x"]]
            for scale in (H_EXACT, H_PROOF):
                for c in mp_stencil(x, _exact_h(p["x"], scale)):
                    par = tuple(mp.nstr(v, DPS_ROOT, min_fixed=1, max_fixed=0) for v in c)
                    jobs.setdefault((model, point, par), (m, p["split"], p["x"], par, start))
    return jobs


def assemble_correction(ms, got):
    out = []
    for model, point in CORRECTION:
        m, p = _find(ms, model, point)
        unf = m["unfolded"]
        with mp.workdps(DPS_ROOT):
            x = [mp.mpf(v) for v in p["x"]]
            ders = []
            for scale in (H_EXACT, H_PROOF):
                h = _exact_h(p["x"], scale)
                pars = [tuple(mp.nstr(v, DPS_ROOT, min_fixed=1, max_fixed=0) for v in c) for c in mp_stencil(x, h)]
                rs = [got[(model, point, par)] for par in pars]
                assert all(mp.mpf(r["residual"]) < mp.mpf(ROOT_RESIDUAL) for r in rs), (model, "residual of the root")
                ders.append(mp_rule(_logs([[mp.mpf(v) for v in r["jafs"]] for r in rs], unf), h))
            (d1, d2), (e1, e2) = ders
            D, K = len(d1), len(d1[0])
            agree = mp.mpf(AGREE)
            for i in range(D):
                for k in range(K):
                    assert abs(d1[i][k] - e1[i][k]) <= agree * max(1, abs(d1[i][k])), (model, "dlog", i, k)
                    for j in range(D):
                        assert abs(d2[i][j][k] - e2[i][j][k]) <= agree * max(1, abs(d2[i][j][k])), (model, "d2log", i, j, k)
            centre = got[(model, point, tuple(mp.nstr(v, DPS_ROOT, min_fixed=1, max_fixed=0) for v in x))]
            # a point where the reference did not converge never enters the fixture
            oracle_lc = _oracle_corrected(m, p["split"], p["x"]).lc
            for t, (a, b) in enumerate(centre["lc"]):
                for got_l, want_l in ((mp.mpf(a), oracle_lc[t][0]), (mp.mpf(b), oracle_lc[t][1])):
                    assert abs(got_l - want_l) <= ROOT_NEAR_ORACLE * abs(got_l), (model, t, "the oracle's rate is not near the root")
            X1 = np.array([[float(v) for v in r] for r in d1])
            X2 = np.array([[[float(v) for v in r] for r in rr] for rr in d2])
        steps = []
        for rel in [s["rel_step"] for s in p["steps"]]:
            pts, h, _ = opt.curvature_stencil(p["x"], rel, p["abs_step"])
            J = np.array([_oracle_spectrum(m, p["split"], c) for c in pts[0]])
            o1, o2, st = opt.curvature_from_spectra(J[None], None, h, unf)
            assert st[0] == 0
            err1, err2 = np.abs(o1[0][:, :K] - X1), np.abs(o2[0][:, :, :K] - X2)
            ok1, ok2 = err1 < QUALIFIES * np.abs(X1), err2 < QUALIFIES * np.abs(X2)
            if rel == cx.DEFAULT_STEP:
                # (were this to fail, the finding belongs in DESIGN.md: the reference itself has no Hessian at its default step)
                assert ok1.all() and ok2.all(), (model, "the oracle does not qualify at the default step", err1 / np.abs(X1), err2 / np.abs(X2))
            steps.append(dict(rel_step=rel, oracle_jafs=[[float(v) for v in r] for r in J], oracle_err_dlog=err1.tolist(),
                              oracle_err_d2log=err2.tolist(), qualifies_dlog=ok1.tolist(), qualifies_d2log=ok2.tolist()))
        out.append(dict(model=model, point=point, lc=centre["lc"], residual=centre["residual"],
                        exact=dict(dlog=[[_s(v) for v in r] for r in d1], d2log=[[[_s(v) for v in r] for r in rr] for rr in d2]), steps=steps))
    return out


def generate(workers, keep_smooth=False):
    ms = models()
    with ProcessPoolExecutor(workers) as pool:
        if keep_smooth:
            fx = cx.load()                                               # the committed smooth part; only "correction" is made anew
        else:
            jobs = plan(ms)
            keys = sorted(jobs, key=lambda k: (-k[2], k[0], k[1]))       # the 80-digit ones first: they take longest
            fx = assemble(ms, dict(zip(keys, pool.map(spectrum_job, [jobs[k] for k in keys], chunksize=1))))
        jobs = plan_correction(fx["models"])
        keys = sorted(jobs)
        fx["correction"] = assemble_correction(fx["models"], dict(zip(keys, pool.map(correction_job, [jobs[k] for k in keys], chunksize=1))))
    return fx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="regenerate and compare with the committed fixture")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--correction-only", action="store_true",
                    help="keep the smooth part of the committed fixture and regenerate the part through the lambda-correction")
    a = ap.parse_args()
    fx = generate(a.j, a.correction_only)
    text = json.dumps(fx, separators=(",", ":")) + "\n"
    n = sum(len(m["points"]) for m in fx["models"])
    if a.check:
        with gzip.open(OUT, "rt") as f:
            old = f.read()
        if old != text:
            print("golden_curvature_exact.json.gz differs from a fresh generation")
            return 1
        print("golden_curvature_exact.json.gz reproduced (%d models, %d points)" % (len(fx["models"]), n))
        return 0
    with open(OUT, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
        f.write(text.encode())
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", n, "points")
    return 0


if __name__ == "__main__":
    sys.exit(main())
