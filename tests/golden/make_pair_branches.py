#!/usr/bin/env python3
"""Generate tests/golden/golden_pair_branches.json.gz and golden_pair_residuals.json.gz: the pair-chain residual of the lambda correction
(pair_eval -> pair_expv / pair_reduced, misti_kernels.hip) in 50-digit arithmetic, branch by branch.

    python tests/golden/make_pair_branches.py            # (re)write both fixtures
    python tests/golden/make_pair_branches.py --check    # regenerate and compare with the committed fixtures

Deterministic, CPU only, does not use the reference.  The branch of every interval / problem is the device's, restated in
tests/pair_branches.py; the coverage the fixtures promise is asserted here (pair_branches.coverage_forward, coverage_residuals) and again by
the tests that read them.

golden_pair_branches.json.gz - models for Engine.forward_rates (numT = 6, cpfit, split 5, the two migration rates as parameters): per
model times, lh and candidates; per candidate its parameters, per interval the branch, nbmax and tags, and the exact pair states
(the `pr` rows 1..5 of the forward map) propagated from the unit vectors at 50 digits.

golden_pair_residuals.json.gz - problems of misti_pair_residuals: the ten inputs, the rates the lane really evaluates (fd_step repeated
in float64), branch and regime, and the exact w = e^M P and residual; for the default fit the exact expected coalescence time, the
exact pnc, and per regime of the formula branch the largest relative error of the reference's own formula (SciPy expm and inv in
float64: the arithmetic of oracle.misti_oracle.CorrectLambda._residual_ect) against 50 digits at these very points.
Doubles are written by repr (round-trip exact); the files are gzip streams without a time stamp, so a regeneration is the same bytes."""
import argparse
import gzip
import json
import math
import os
import sys
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mpmath as mp                      # noqa: E402
import numpy as np                       # noqa: E402
import pair_branches as pb               # noqa: E402

OUT_FWD = os.path.join(HERE, "golden_pair_branches.json.gz")
OUT_RES = os.path.join(HERE, "golden_pair_residuals.json.gz")
DPS = 50
NUMT = 6


# ---- exact arithmetic ----------------------------------------------------------------------------------------------------
def _matrix(l0, l1, mu0, mu1):
    a, b, x, y = mp.mpf(mu0), mp.mpf(mu1), mp.mpf(l0), mp.mpf(l1)
    return mp.matrix([[-2 * a - x, 0, b], [0, -2 * b - y, a], [2 * a, 2 * b, -a - b]])


def exact_chain(job):
    """pr rows 1..5 of the forward map for one candidate: both genomes through the five intervals."""
    times, lh, mu0, mu1 = job
    with mp.workdps(DPS):
        v = [mp.matrix([1, 0, 0]), mp.matrix([0, 1, 0])]
        rows = []
        for t in range(NUMT - 1):
            E = mp.expm(_matrix(lh[t][0], lh[t][1], mu0, mu1) * mp.mpf(times[t]))
            v = [E * v[0], E * v[1]]
            rows.append([float(v[j & 1][j >> 1]) for j in range(6)])
        return rows


def exact_residual(job):
    """w = e^M P, and the default fit's pnc and ect, at the rates the lane evaluates."""
    cpfit, mu0, mu1, P, tgt, l0, l1 = job
    with mp.workdps(DPS):
        M = _matrix(l0, l1, mu0, mu1)
        Pv = mp.matrix([mp.mpf(x) for x in P])
        if cpfit:
            w = mp.expm(M) * Pv
            return dict(w=[float(x) for x in w], res=float(w[0] + w[1] + w[2] - mp.mpf(tgt)))
        # phi functions from one augmented exponential: exp([[M, pn, 0], [0, 0, 1], [0, 0, 0]]) = [[e^M, phi1 pn, phi2 pn], ...],
        # phi1 = int_0^1 e^{(1-s)M} ds, phi2 = int_0^1 e^{(1-s)M} s ds, so int_0^1 u e^{uM} pn du = (phi1 - phi2) pn: no inverse
        s = Pv[0] + Pv[1] + Pv[2]
        pn = Pv / s
        A = mp.zeros(5, 5)
        for i in range(3):
            for j in range(3):
                A[i, j] = M[i, j]
            A[i, 3] = pn[i]
        A[3, 4] = 1
        E = mp.expm(A)
        wn = [sum(E[i, j] * pn[j] for j in range(3)) for i in range(3)]
        vint = [E[i, 3] - E[i, 4] for i in range(3)]
        pnc = wn[0] + wn[1] + wn[2]
        ect = (mp.mpf(l0) * vint[0] + mp.mpf(l1) * vint[1]) / (1 - pnc)
        # cross-check where the power series converges fast: sum_k M^k pn / (k! (k + 2))
        if max(abs(M[i, i]) for i in range(3)) < 2:
            term, acc = pn, pn / 2
            for k in range(1, 80):
                term = M * term / k
                acc = acc + term / (k + 2)
            assert max(abs(acc[i] - vint[i]) for i in range(3)) < mp.mpf(10) ** -40
        return dict(w=[float(x * s) for x in wn], ect=float(ect), pnc=float(pnc), one_minus_pnc=float(1 - pnc),
                    res=float(ect - mp.mpf(tgt)), ect_hi=mp.nstr(ect, 30))


def reference_formula_ect(mu0, mu1, P, l0, l1):
    """The reference's formula for the expected coalescence time in float64 (T = 1), operation for operation as
    oracle.misti_oracle.CorrectLambda._residual_ect states it."""
    from scipy import linalg
    M = np.array([[-2 * mu0 - l0, 0, mu1], [0, -2 * mu1 - l1, mu0], [2 * mu0, 2 * mu1, -mu0 - mu1]])
    MET = linalg.expm(M)
    Minv = linalg.inv(M)
    pn = [v / sum(P) for v in P]
    vec1 = np.dot(MET - np.identity(3), pn)
    vec1 = np.dot(Minv, np.dot(Minv, vec1))
    vec2 = np.dot(MET, pn)
    pnc = sum(vec2)
    vec2 = np.dot(1.0, np.dot(Minv, vec2))
    vec = vec2 - vec1
    return float((l0 * vec[0] + l1 * vec[1]) / (1 - pnc))


# ---- part A: models of the forward map ---------------------------------------------------------------------------------------
def _solve_mu(target_nb, l0, l1, T, kind, ratio):
    """(mu0, mu1) of direction `kind` whose interval has nbmax ~ target_nb: the larger exit rate is 2 mu + l of the migrating side."""
    if kind == "one0":                     # mu1 == 0: cascade which = 1
        return max((target_nb / T - l0) / 2.0, 0.0), 0.0
    if kind == "one1":
        return 0.0, max((target_nb / T - l1) / 2.0, 0.0)
    m = max((target_nb / T - l0) / 2.0, 0.0)
    return m, m * ratio                    # two-way, mu1 = ratio * mu0 <= mu0 (l0 >= l1 in these models)


def forward_models():
    rng = np.random.default_rng(20240611)
    kinds = ("one0", "one1", "two")
    models = []
    # -- A: tiny coalescence rates: every norm class is reached through the migration rates alone
    times = [1.0, 1.003, 0.997, 1.0015, 0.9985]
    lh = [[1.5e-4, 1.2e-4], [2.0e-4, 0.7e-4], [1.0e-4, 1.0e-4], [1.7e-4, 1.1e-4], [0.9e-4, 0.8e-4], [1.0, 1.0]]
    targets = []
    for e in pb.TAYLOR_EDGES:
        targets += [0.5 * e * f for f in (1 - 6e-3, 1 - 1e-3, 1 - 1e-9, 1 + 1e-9, 1 + 1e-3, 1 + 6e-3)]
    targets += [0.002, 0.01, 0.04, 0.09, 0.2, 0.4, 0.8]                         # class interiors
    targets += [1.5, 2.0, 3.0, 4.0, 5.0, 5.5, 5.92, 5.97, 5.995, 6.0 * (1 - 1e-9)]   # uniformisation
    targets += [6.0 * (1 + 1e-9), 6.004, 6.02, 6.1, 7.0, 9.0, 12.0, 15.9]        # just above 6; stiff through mu alone (mu T in [3.05, 8])
    cands = []
    for i, nb in enumerate(targets):
        for kind in (kinds if nb > 5.9 else (kinds[i % 3],)):
            cands.append(_solve_mu(nb, lh[0][0], lh[0][1], times[0], kind, 0.37))
    models.append(dict(name="tiny_rates", times=times, lh=lh, cands=cands))
    # -- B: ordinary coalescence rates (rate x length 0.05 ... 0.9), the upper classes and the uniformisation range
    times = [0.5, 0.75, 0.6, 0.9, 0.4]
    lh = [[0.11, 0.10], [0.30, 0.21], [0.70, 0.33], [1.00, 0.52], [0.64, 0.41], [1.0, 1.0]]
    targets = []
    for e in pb.TAYLOR_EDGES[3:]:
        targets += [0.5 * e * f for f in (1 - 4e-3, 1 - 1e-9, 1 + 1e-9, 1 + 4e-3)]
    targets += [0.07, 0.1, 0.2, 0.35, 0.7, 1.3, 1.8, 2.5, 3.5, 4.5, 5.91, 5.96, 5.99, 6.0 * (1 - 1e-9), 6.0 * (1 + 1e-9), 6.003, 6.03, 6.2, 8.0]
    cands = []
    for i, nb in enumerate(targets):
        for kind in (kinds if nb > 5.9 else (kinds[i % 3], "two")):
            cands.append(_solve_mu(nb, lh[0][0], lh[0][1], times[0], kind, 0.61))
    models.append(dict(name="ordinary_rates", times=times, lh=lh, cands=cands))
    # -- C, D: one rate of every interval has run away (rate x length 6 ... 3e5), the other is ordinary, so the states stay far
    # above the double range; interval 3 of C (4 of D) is dyadic: c == a exactly with mu = 0.25
    for name, flip in (("runaway_a", 0), ("runaway_b", 1)):
        times, lh = [], []
        for t in range(NUMT - 1):
            T = float(10 ** rng.uniform(-0.7, 0.3))
            big = float(10 ** rng.uniform(1.5, 5.3))
            big = min(big, 3e5 / T)
            small = float(rng.uniform(0.3, 3.0))
            times.append(T)
            lh.append([big, small] if (t + flip) % 2 == 0 else [small, big])
        times[2], lh[2] = 1.5, ([2e5, 0.9] if flip == 0 else [1.1, 2e5])          # rate x length 3e5
        times[3], lh[3] = 0.5, ([100.0, 100.5] if flip == 0 else [64.5, 64.0])    # 2 mu T + l_S T == l_K T at mu = 0.25
        lh.append([1.0, 1.0])
        cands = []
        for i in range(24):                                                      # one-way, both directions
            mu = float(10 ** rng.uniform(-4, 0.6))
            cands.append((mu, 0.0) if i % 2 == 0 else (0.0, mu))
        cands += [(0.25, 0.0), (0.0, 0.25)]                                       # c == a exactly in the dyadic interval
        for t in range(NUMT - 1):                                                 # c ~ b: the entered state's rate within 1e-6 of "one in each"
            for d in (3e-7, -8e-7, 1e-12):
                cands.append((lh[t][1] * (1 + d), 0.0))
                cands.append((0.0, lh[t][0] * (1 + d)))
        cands += [(0.0, 0.0)] * 1                                                 # no migration at all, stiff rates
        for i in range(16):                                                      # two-way neighbours in the same waves (pair_eigen)
            cands.append((float(10 ** rng.uniform(-4, 0.6)), float(10 ** rng.uniform(-4, 0.6))))
        models.append(dict(name=name, times=times, lh=lh, cands=cands))
    return models


def label_forward(m):
    out = []
    for mu0, mu1 in m["cands"]:
        ivs = []
        for t in range(NUMT - 1):
            l0, l1 = m["lh"][t]
            a0, a1, b0, b1, q = pb.forward_interval(l0, l1, mu0, mu1, m["times"][t])
            br = pb.branch(b0, b1, q)
            iv = dict(branch=br, nbmax=q, rate_x_length=max(a0, a1))
            if br.startswith("cascade"):
                which = int(br[-1])
                a, c, b = (2 * b0 + a0, 2 * b1 + a1, b0 + b1) if which == 1 else (2 * b1 + a1, 2 * b0 + a0, b0 + b1)
                tags = []
                if b > 0 and c != b and abs(c - b) <= 1e-6 * b:
                    tags.append("c_near_b")
                if c == a:
                    tags.append("c_eq_a")
                if 3.05 <= max(b0, b1) <= 8 and max(a0, a1) < 0.2 * m["times"][t] and max(l0, l1) < 0.2:
                    tags.append("stiff_by_mu")
                if t == 0:
                    tags.append("unit_left")          # genome `which - 1` enters as the unit vector of the state that is left
                if b0 == 0.0 and b1 == 0.0:
                    tags.append("no_migration")
                iv["tags"] = tags
            ivs.append(iv)
        out.append(dict(params=[mu0, mu1], intervals=ivs))
    return out


# ---- part B: problems of the residual probe ----------------------------------------------------------------------------------
def _prob(cpfit, mu0, mu1, P, tgt, x0, x1, role, red, regime):
    return dict(cpfit=int(cpfit), mu0=float(mu0), mu1=float(mu1), P=[float(v) for v in P], tgt=float(tgt), x0=float(x0), x1=float(x1),
                role=int(role), red=int(red), regime=regime)


def _rates_for(rng, nb, kind):
    """(mu0, mu1, x0, x1) with max(2 mu0 + x0, 2 mu1 + x1, mu0 + mu1) ~ nb, the share of migration random."""
    share = float(rng.uniform(0.05, 0.6))
    mu = 0.5 * nb * share
    x0 = nb - 2 * mu
    x1 = x0 * float(rng.uniform(0.2, 0.95))
    if kind == "one0":
        return mu, 0.0, x0, x1
    if kind == "one1":
        return 0.0, mu, x1, x0
    return mu, mu * float(rng.uniform(0.1, 0.9)), x0, x1


def _target_in_branch(i, rng):
    """An nbmax inside Taylor class i (i = 0..6) or the uniformisation range (7), away from the edges by more than the fd step moves it."""
    if i == 7:
        return float(rng.uniform(1.05, 5.9))
    lo = 0.5 * pb.TAYLOR_EDGES[i - 1] if i else 0.0
    return float(rng.uniform(lo + 0.1 * (0.5 * pb.TAYLOR_EDGES[i] - lo), 0.95 * 0.5 * pb.TAYLOR_EDGES[i]))


def residual_problems():
    rng = np.random.default_rng(20240612)
    out = []
    vec = lambda: [float(v) for v in rng.dirichlet([1.0, 1.0, 1.0]) * 10 ** rng.uniform(-3, 0)]
    kinds = ("one0", "one1", "two")
    # -- cpfit: every branch of the forward map again through pair_eval; the first point of 8 branches under all six roles
    six = 0
    for i in range(8):
        for j in range(4):
            mu0, mu1, x0, x1 = _rates_for(rng, _target_in_branch(i, rng), kinds[(i + j) % 3])
            P = vec()
            tgt = math.exp(-x0 * 0.9) * sum(P)
            roles = range(6) if j == 0 else [int(rng.integers(0, 6))]
            six += j == 0
            for r in roles:
                out.append(_prob(1, mu0, mu1, P, tgt, x0, x1, r, 0, "cpfit_branch"))
    for kind in kinds:                                                          # the closed forms: cascade1, cascade2, eigen
        for j in range(5):
            big = float(10 ** rng.uniform(1.0, 5.4))
            mu = float(10 ** rng.uniform(-3, 0.5))
            x0, x1 = (big, float(rng.uniform(0.3, 3))) if j % 2 == 0 else (float(rng.uniform(0.3, 3)), big)
            mu0, mu1 = (mu, 0.0) if kind == "one0" else (0.0, mu) if kind == "one1" else (mu, mu * float(rng.uniform(0.01, 1)))
            P = vec()
            tgt = math.exp(-1.3) * sum(P)
            roles = range(6) if j == 0 else [int(rng.integers(0, 6))]
            for r in roles:
                out.append(_prob(1, mu0, mu1, P, tgt, x0, x1, r, 0, "cpfit_branch"))
    # -- pair_reduced: red = 1 (mu1 == 0, state 0 empty) and 2, exit rate 1 ... 3e5; |a - c| == 0 exactly and ~ 1e-9
    for j in range(20):
        red = 1 + j % 2
        dk = float(10 ** rng.uniform(0, 5.47)) if j < 16 else 3e5 if j < 18 else 1.0
        mu = float(10 ** rng.uniform(-3, 0.5))
        P = vec()
        if j in (4, 5):
            mu = dk                                   # role 0: dk = x == mu = d2 exactly
        if j in (6, 7):
            mu = dk * (1 + 1e-9)
        other = float(10 ** rng.uniform(-1, 5))       # the rate that is not read
        role = 0 if j in (4, 5, 6, 7) else int(rng.integers(0, 6))
        tgt = math.exp(-0.7) * (P[1] + P[2])
        if red == 1:
            out.append(_prob(1, mu, 0.0, [0.0, P[1], P[2]], tgt, other, dk, role, 1, "reduced"))
        else:
            out.append(_prob(1, 0.0, mu, [P[0], 0.0, P[2]], tgt, dk, other, role, 2, "reduced"))
    # -- a negative trial rate of small size (the neg term of nbmax)
    for j in range(4):
        mu0, mu1, x0, x1 = _rates_for(rng, float(rng.uniform(0.05, 3.0)), kinds[j % 3])
        P = vec()
        x0, x1 = (-x0 * 0.01, x1) if j % 2 == 0 else (x0, -x1 * 0.02)
        out.append(_prob(1, mu0, mu1, P, 0.9 * sum(P), x0, x1, int(rng.integers(0, 6)), 0, "negative_rate"))
    # -- default fit, series branch: every Taylor class, nbmax down to 1e-5
    for i in range(7):
        for j in range(7):
            nb = _target_in_branch(i, rng)
            if i == 0 and j < 4:
                nb = (1e-5, 3e-5, 1e-4, 1e-3)[j]
            mu0, mu1, x0, x1 = _rates_for(rng, nb, kinds[(i + j) % 3])
            out.append(_prob(0, mu0, mu1, vec(), 0.0, x0, x1, int(rng.integers(0, 6)), 0, "ect_series"))
    # -- default fit, formula branch
    for j in range(9):
        mu0, mu1, x0, x1 = _rates_for(rng, float(rng.uniform(1.05, 5.9)), kinds[j % 3])
        out.append(_prob(0, mu0, mu1, vec(), 0.0, x0, x1, int(rng.integers(0, 6)), 0, "ect_formula_uniformisation"))
    for j in range(9):
        big, mu = float(10 ** rng.uniform(1.0, 3.0)), float(10 ** rng.uniform(-2, 0.5))
        x0, x1 = (big, float(rng.uniform(0.3, 3))) if j % 2 == 0 else (float(rng.uniform(0.3, 3)), big)
        out.append(_prob(0, mu if j % 4 < 2 else 0.0, 0.0 if j % 4 < 2 else mu, vec(), 0.0, x0, x1, int(rng.integers(0, 6)), 0, "ect_formula_one_way_stiff"))
    for j in range(9):
        big, mu = float(10 ** rng.uniform(1.0, 3.0)), float(10 ** rng.uniform(-2, 0.5))
        x0, x1 = (big, float(rng.uniform(0.3, 3))) if j % 2 == 0 else (float(rng.uniform(0.3, 3)), big)
        out.append(_prob(0, mu, mu * float(rng.uniform(0.05, 1)), vec(), 0.0, x0, x1, int(rng.integers(0, 6)), 0, "ect_formula_two_way_stiff"))
    for j in range(9):
        big, mu = float(10 ** rng.uniform(3.0, 5.0)), 1e-3 * float(rng.uniform(0.5, 2))
        x0, x1 = (big, float(rng.uniform(0.3, 3))) if j % 2 == 0 else (float(rng.uniform(0.3, 3)), big)
        out.append(_prob(0, mu, mu * float(rng.uniform(0.5, 1.5)), vec(), 0.0, x0, x1, int(rng.integers(0, 6)), 0, "ect_formula_runaway"))
    return out


# points whose residual and state must come back NaN: (x0, x1) as text, JSON has no spelling for them
NAN_POINTS = [dict(cpfit=1, mu0=0.3, mu1=0.1, P=[0.2, 0.3, 0.1], tgt=0.5, x0="inf", x1="1.0", role=0, red=0),
              dict(cpfit=1, mu0=0.3, mu1=0.0, P=[0.0, 0.3, 0.1], tgt=0.3, x0="1.0", x1="nan", role=3, red=1),
              dict(cpfit=1, mu0=0.3, mu1=0.1, P=[0.2, 0.3, 0.1], tgt=0.5, x0="1e300", x1="1.0", role=2, red=0),
              dict(cpfit=1, mu0=0.0, mu1=0.2, P=[0.2, 0.0, 0.1], tgt=0.2, x0="2.0", x1="-1e300", role=5, red=2),
              dict(cpfit=0, mu0=0.3, mu1=0.1, P=[0.2, 0.3, 0.1], tgt=0.0, x0="nan", x1="1.0", role=0, red=0),
              dict(cpfit=0, mu0=0.3, mu1=0.1, P=[0.2, 0.3, 0.1], tgt=0.0, x0="0.5", x1="1e300", role=4, red=0)]


def label_residual(p):
    l0, l1, q, neg, ok = pb.eval_point(p["mu0"], p["mu1"], p["x0"], p["x1"], p["role"])
    p.update(l0=l0, l1=l1, q=q, neg=neg, nbmax=q + neg)
    p["branch"] = "reduced%d" % p["red"] if p["red"] else pb.branch(p["mu0"], p["mu1"], q + neg)
    if p["red"]:
        p["exit_rate"] = l1 if p["red"] == 1 else l0
        p["gap"] = abs(p["exit_rate"] - (p["mu0"] + p["mu1"]))
    return p


# ---- drivers ---------------------------------------------------------------------------------------------------------------------
def generate(workers):
    models = forward_models()
    with ProcessPoolExecutor(workers) as pool:
        fwd = []
        for m in models:
            cands = label_forward(m)
            exact = list(pool.map(exact_chain, [(m["times"], m["lh"], c["params"][0], c["params"][1]) for c in cands], chunksize=4))
            for c, e in zip(cands, exact):
                c["exact"] = e
            fwd.append(dict(name=m["name"], times=m["times"], lh=m["lh"], candidates=cands))
        probs = [label_residual(p) for p in residual_problems()]
        exact = list(pool.map(exact_residual, [(p["cpfit"], p["mu0"], p["mu1"], p["P"], p["tgt"], p["l0"], p["l1"]) for p in probs], chunksize=4))
    ref = {}
    for p, e in zip(probs, exact):
        hi = e.pop("ect_hi", None)
        p["exact"] = e
        if p["regime"].startswith("ect_formula"):
            f = reference_formula_ect(p["mu0"], p["mu1"], p["P"], p["l0"], p["l1"])
            with mp.workdps(DPS):
                rel = float(abs((mp.mpf(f) - mp.mpf(hi)) / mp.mpf(hi)))
            p["reference_formula_relative_error"] = rel
            r = ref.setdefault(p["regime"], dict(worst_relative_error=0.0, points=0))
            r["worst_relative_error"] = max(r["worst_relative_error"], rel)
            r["points"] += 1
    fx_fwd = dict(dps=DPS, numT=NUMT, bound=pb.W_BOUND, norm_floor=pb.NORM_FLOOR, models=fwd)
    fx_res = dict(dps=DPS, bound=pb.W_BOUND, problems=probs, nan_points=NAN_POINTS, reference_formula=ref)
    n_iv = pb.coverage_forward(fx_fwd)
    n_pr = pb.coverage_residuals(fx_res)
    return fx_fwd, fx_res, n_iv, n_pr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="regenerate and compare with the committed fixtures")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    fx_fwd, fx_res, n_iv, n_pr = generate(a.j)
    rc = 0
    for path, fx in ((OUT_FWD, fx_fwd), (OUT_RES, fx_res)):
        text = json.dumps(fx, indent=None, separators=(",", ":")) + "\n"
        if a.check:
            with gzip.open(path, "rt") as f:
                same = f.read() == text
            print(os.path.basename(path), "reproduced" if same else "differs from a fresh generation")
            rc |= not same
        else:
            with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
                f.write(text.encode())
            print("wrote", path, os.path.getsize(path), "bytes (%d of JSON)" % len(text))
    print("%d live intervals, %d problems; reference formula: %s" % (n_iv, n_pr, json.dumps(fx_res["reference_formula"])))
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
