#!/usr/bin/env python3
"""Generate tests/golden/golden_lsq_probe.json.gz: the problems of misti_lsq_probe (the solver's linear algebra, one problem per
lane), their exact answers, SciPy's float64 answers and the answers of the float64 restatement (tests/lsq_rule.py).

    python tests/golden/make_lsq_probe.py            # writes the fixture (mpmath 1.3.0, SciPy 1.15.3; fixed seeds)
    python tests/golden/make_lsq_probe.py --check    # re-asserts the fixture's conditions on the stored file

Per problem: "t" tags (the first is the class its figure is kept under, the rest name the branches and edges it reaches), "in" the
input row (exact doubles), "ex" the exact answers - the restated functions run in 80-digit arithmetic (one Jacobi rotation is the
exact SVD of an m x 2 matrix, and the secular iteration under it is SciPy's, without rounding), rounded to double on the way out -
"rule" the restatement's result row, "sp" SciPy's (null where SciPy has no answer), "disc" the expected discrete outcome, "seq" the
outcomes of all comparisons of the 80-digit run, "mg" the smallest relative gap of those comparisons and "need" the margin asked.

CONDITIONS (asserted here, by --check and by tests/test_lsq_probe_cpu.py): every comparison of the 80-digit run has a relative gap
above "need" = min(0.1, max(1e-6, 64 eps kappa)) - except the hand-made exact ties, named "tie:<comparison>" in the tags, which are
decided exactly - and the restatement takes the same side in every one of them.  A drawn problem that misses this is drawn again; the
share a kind loses is printed, stored in the header and stays below 5 %.

The header holds, per kind and class, the worst figure (units of eps kappa, tests/lsq_rule.figures) of SciPy and of the restatement
and their ratio; the device is held to lsq_rule.DEVICE_FACTOR x the restatement's."""
import gzip
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lsq_rule as R

OUT = os.path.join(HERE, "golden_lsq_probe.json.gz")
MAX_LOSS = 0.05
USED_IN = {"SCALAR": 1, "SVD2": 6, "SVD4": 13, "STEP": 8, "STEPN": 15, "SELECT": 20, "UPDATE": 9, "SOLVE3": 12}
USED_OUT = {"SCALAR": 2, "SVD2": 8, "SVD4": 8, "STEP": 6, "STEPN": 3, "SELECT": 5, "UPDATE": 4, "SOLVE3": 15}


def band(kappa):
    return "k4" if kappa < 1e4 else "k8" if kappa < 1e8 else "k12" if kappa < 1e12 else "k15"


def need_of(kappa):
    return min(0.1, max(1e-6, 64 * R.EPS * kappa))


def rot(th):
    return np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])


def with_kappa(rng, rows, kappa, scale=1.0):
    """rows x 2 matrix with singular values scale (1, 1 / kappa)."""
    Q, _ = np.linalg.qr(rng.standard_normal((rows, 2)))
    return scale * (Q * np.array([1.0, 1.0 / kappa])) @ rot(rng.uniform(0, 2 * math.pi)).T


# ------------------------------------------------------------------ one problem: run, check, store
def exact_of(kind, row, tags):
    """(ex, mp info, trace) of the 80-digit run."""
    M = R.MP()
    out, info = R.run(M, kind, row)
    ex = {"row": out[:USED_OUT[kind]]}
    q = R._full(row)
    if kind == "SCALAR":
        x, ex = M.num(q[0]), {}
        for name, v in (("rcp", M.rcp(x)), ("sqrt", M.sqrt(x))):
            r = float(v)
            if q[0] == 0.0:                                  # mpmath has no signed zero
                r = math.copysign(r, q[0])
            resid = float((v - M.num(r)) / M.num(math.ulp(r))) if (math.isfinite(r) and r != 0.0) else 0.0
            ex[name] = [r, float("%.9g" % resid)]
    elif kind in ("STEP", "STEPN"):
        N = 2 if kind == "STEP" else int(q[12])
        if N == 2:
            A, f = (R._mat(M, q, 2, 2), R._vec(M, q, 2, 4)) if kind == "STEP" else (R._mat(M, q, 4, 2), R._vec(M, q, 4, 8))
            s, V, uf = R.svd_mx2(R.MP(), A, f)
            ex["s"] = [float(s[0]), float(s[1])]
            if s[1] > 0:
                ex["gn"] = [float(-(V[r][0] * uf[0] / s[0] + V[r][1] * uf[1] / s[1])) for r in range(2)]
        else:
            s, V, uf = R.svd_aug1(R.MP(), [M.num(q[0]), M.num(q[2])], R._vec(M, q, 2, 8))
            ex["s"] = [float(s[0])]
            ex["uf0"] = float(uf[0])
            if s[0] > 0:
                ex["gn"] = [float(-uf[0] / s[0])]
        ex["iters"] = info["iters"]
    elif kind == "SELECT":
        if info.get("cand"):
            ex["cand"] = info["cand"]
        ex["path"] = info["path"]
        N = int(q[19])
        # scale of the predicted reduction: the terms of the quadratic at the exact step
        sh = out[2:2 + N]
        Jh = [[q[2]]] if N == 1 else [[q[2], q[3]], [q[4], q[5]]]
        ex["pred_scale"] = sum(0.5 * sum(Jh[r][c] * sh[c] for c in range(N)) ** 2 for r in range(N)) + sum(abs(sh[i] * q[6 + i] * sh[i]) * 0.5 + abs(sh[i] * q[8 + i]) for i in range(N))
    elif kind == "UPDATE":
        ex["case"] = info["case"]
    elif kind == "SOLVE3":
        mp = M.mp
        Mx = mp.matrix(3, 3)
        for i in range(3):
            for j in range(3):
                Mx[i, j] = M.num(q[3 * i + j])
        inv = mp.inverse(Mx)
        n1 = lambda X: max(sum(abs(X[i, j]) for i in range(3)) for j in range(3))
        ex["cond1"] = float(n1(Mx) * n1(inv))
        xs = inv * mp.matrix([M.num(v) for v in q[9:12]])
        for i in range(3):                                   # the 80-digit run against mpmath's own inverse
            assert abs(xs[i] - M.num(out[3 + i])) <= 1e-12 * max(abs(v) for v in xs) or not math.isfinite(out[3 + i]), (row, out)
        ex["swaps"] = info["swaps"]
    return ex, info, M.trace


def kappa_of(kind, ex):
    if kind in ("SVD2", "SVD4"):
        s = [v for v in ex["row"][0:2]]
        return s[0] / s[1] if s[1] > 0 else 1.0
    if kind in ("STEP", "STEPN"):
        s = ex["s"]
        return s[0] / s[-1] if s[-1] > 0 else 1.0
    return 1.0


def make(kind, row, tags):
    """The fixture's record of a problem, or None if it misses the conditions."""
    row = [float(v) for v in row[:USED_IN[kind]]]
    K = R.F64()
    rule, rinfo = R.run(K, kind, row)
    ex, minfo, mtrace = exact_of(kind, row, tags)
    mtrace, ktrace = R.live(mtrace), R.live(K.trace)
    ties = {t[4:] for t in tags if t.startswith("tie:")}
    need = need_of(kappa_of(kind, ex))
    # the pivots of the first column compare entries of the input: nothing is rounded, any gap decides
    # (and those of the second column of a pair-chain generator, whose entry above is an exact zero: M[2][1] - l * 0)
    unrounded = ("pivot0", "pivot1") if "generator" in tags else ("pivot0",)
    gaps = [g for (n, g, o) in mtrace if n not in ties and not (n in unrounded and g > 0)]
    mg = min(gaps) if gaps else 1.0
    seq = "".join("1" if o else "0" for (_, _, o) in mtrace)
    if [(n, o) for (n, _, o) in ktrace] != [(n, o) for (n, _, o) in mtrace] or not mg > need:
        return None
    if kind in ("STEP", "STEPN") and rinfo["iters"] != minfo["iters"]:
        return None
    prob = {"t": list(tags), "in": row, "ex": ex, "rule": rule[:USED_OUT[kind]], "seq": seq, "mg": float("%.3g" % mg) if mg < 1 else 1.0, "need": need}
    sp, sinfo = R.scipy_row(kind, row)
    prob["sp"] = sp[:USED_OUT[kind]] if sp is not None else None
    if sinfo.get("iters") is not None:
        prob["sp_iters"] = sinfo["iters"]
    prob["disc"] = R.discrete(kind, prob, rule)
    return prob


class Kind:
    def __init__(self, name):
        self.name, self.problems, self.drawn, self.lost, self.lost_edges = name, [], 0, 0, 0

    def hand(self, row, tags):
        p = make(self.name, row, tags)
        assert p is not None, (self.name, tags, row)
        self.problems.append(p)
        return p

    def draw(self, fn, n, tagger):
        """n problems from fn() -> (row, tags); tagger(prob) adds the tags that depend on the outcome.  A miss is drawn again."""
        got = 0
        while got < n:
            row, tags = fn()
            self.drawn += 1
            p = make(self.name, row, tags)
            if p is None:
                self.lost += 1
                assert self.lost <= 0.5 * self.drawn + 20, (self.name, "too many problems without margin")
                continue
            tagger(p)
            self.problems.append(p)
            got += 1


# ------------------------------------------------------------------ the kinds
def scalar(rng):
    k = Kind("SCALAR")
    ulp = math.ulp
    xs = [(2.0 ** e, "pow2") for e in range(-1021, 1024)]
    for b in (1.0, 2.0, 4.0):
        xs += [(b, "near_pow2"), (b + ulp(b), "near_pow2"), (b - ulp(b) / 2, "near_pow2")]
    for n in rng.integers(2, 1 << 26, 300):
        sq = float(n) * float(n)
        xs += [(sq, "square"), (sq + ulp(sq), "square"), (sq - ulp(sq), "square")]
    xs += [(float(2.0 ** e), "random") for e in rng.uniform(-510, 510, 2000)]
    xs += [(v, "special") for v in (2.0 ** -1022, 1000 * 5e-324, sys.float_info.max, 0.0, -0.0, math.inf, -math.inf, -1.0, math.nan)]
    for x, tag in xs:
        inr = 2.0 ** -510 <= x <= 2.0 ** 510
        k.hand([x], [tag, "in_range" if inr else "recorded" if (x > 0 and math.isfinite(x)) else "edge"])
    return k


def svd_tags(p):
    p["t"].append("swap" if p["seq"][-1] == "0" else "no_swap")


def svd2(rng):
    k = Kind("SVD2")

    def gen():
        kap = 10 ** rng.uniform(0, 15)
        sc = 10 ** rng.uniform(-150, 150) if rng.random() < 0.2 and kap < 1e3 else 10 ** rng.uniform(-3, 3)
        A = with_kappa(rng, 2, kap, sc)
        f = rng.standard_normal(2) * 10 ** rng.uniform(-3, 3)
        return list(A.ravel()) + list(f), [band(kap)] + (["scale_extreme"] if not 1e-100 < sc < 1e100 else [])
    k.draw(gen, 420, svd_tags)
    e = 2.0 ** -30
    k.hand([3.0, 0.0, 0.0, 2.0, 1.0, 1.0], ["ga0", "no_swap", "tie:ga!=0"])
    k.hand([0.0, 2.0, 3.0, 0.0, 1.0, -1.0], ["ga0", "no_swap", "tie:ga!=0"])
    k.hand([2.0, 0.0, 0.0, 3.0, 1.0, 0.5], ["ga0", "swap", "tie:ga!=0"])
    k.hand([1.0, 2.0, -2.0, 1.0, 0.5, 0.25], ["ga0", "equal_sv", "tie:ga!=0", "tie:s1>=s2"])
    k.hand([1.0, 1.0, 1.0, -1.0, 0.5, 0.25], ["ga0", "equal_sv", "tie:ga!=0", "tie:s1>=s2"])
    k.hand([2.0, 1.0, 1.0, 2.0, 0.5, 0.25], ["al_eq_be", "zeta0"])
    k.hand([2.0, -1.0, -1.0, 2.0, 0.5, 0.25], ["al_eq_be", "zeta0"])
    k.hand([2.0, 1.0, 1.0, 2.0 + e, 0.5, 0.25], ["zeta_tiny"])
    k.hand([2.0, 1.0, 1.0, 2.0 - e, 0.5, 0.25], ["zeta_tiny"])
    k.hand([1.0, e, 0.0, 1e3, 0.5, 0.25], ["zeta_huge"])
    k.hand([1e3, e, 0.0, 1.0, 0.5, 0.25], ["zeta_huge"])
    k.hand([1.0, 1e-160, 0.0, 1e3, 0.5, 0.25], ["zeta_huge", "zeta_beyond"])
    k.hand([0.0, 3.0, 0.0, 4.0, 1.0, 2.0], ["zero_col", "tie:ga!=0"])
    k.hand([3.0, 0.0, -4.0, 0.0, 1.0, 2.0], ["zero_col", "tie:ga!=0"])
    k.hand([0.0, 0.0, 0.0, 0.0, 1.0, 2.0], ["both_zero", "tie:ga!=0", "tie:s1>=s2"])
    return k


def aug_matrix(rng, N, zero_diag):
    """The augmented matrix trf_bounded builds: J_h above diag(sqrt(diag)), and (f, 0)."""
    kap = 10 ** rng.uniform(0, 12)
    d = np.sqrt(10 ** rng.uniform(-6, 1, N))
    diag = np.array([0.0 if (zero_diag or rng.random() < 0.3) else 10 ** rng.uniform(-8, 2) for _ in range(N)])
    f = rng.standard_normal(N) * 10 ** rng.uniform(-3, 1)
    if N == 1:
        Jh = np.array([[rng.standard_normal() * 10 ** rng.uniform(-3, 3)]])
        return [Jh[0][0], 0.0, math.sqrt(diag[0]), 0.0, 0, 0, 0, 0, f[0], 0.0, 0, 0, 1.0], kap, Jh, diag, f, d
    Jh = with_kappa(rng, 2, kap, 10 ** rng.uniform(-2, 2)) * d
    A = np.vstack([Jh, np.diag(np.sqrt(diag))])
    return list(A.ravel()) + [f[0], f[1], 0.0, 0.0, 2.0], kap, Jh, diag, f, d


def svd4(rng):
    k = Kind("SVD4")

    def gen():
        kap = 10 ** rng.uniform(0, 15)
        sc = 10 ** rng.uniform(-150, 150) if rng.random() < 0.2 and kap < 1e3 else 10 ** rng.uniform(-3, 3)
        A = with_kappa(rng, 4, kap, sc)
        return list(A.ravel()) + list(rng.standard_normal(4)) + [2.0], [band(kap)] + (["scale_extreme"] if not 1e-100 < sc < 1e100 else [])

    def gen_aug(zero):
        def g():
            row, kap, *_ = aug_matrix(rng, 2, zero)
            return row, ["aug", "aug_diag0" if zero else "aug_diag"]
        return g

    def gen_n1():
        row, *_ = aug_matrix(rng, 1, rng.random() < 0.3)
        return row, ["n1"] + (["aug_diag0"] if row[2] == 0.0 else [])
    k.draw(gen, 260, svd_tags)
    k.draw(gen_aug(False), 120, svd_tags)
    k.draw(gen_aug(True), 40, svd_tags)
    k.draw(gen_n1, 40, lambda p: None)
    k.hand([3.0, 0.0, 0.0, 2.0, 1.0, 0.0, 0.0, 0.5, 1.0, 1.0, 0.0, 0.0, 2.0], ["ga0", "aug", "tie:ga!=0"])
    k.hand([1.0, 2.0, -2.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.5, 0.25, 0.0, 0.0, 2.0], ["ga0", "equal_sv", "tie:ga!=0", "tie:s1>=s2"])
    k.hand([0.0, 3.0, 0.0, 4.0, 0.0, 0.0, 0.0, 1.0, 1.0, 2.0, 0.0, 0.0, 2.0], ["zero_col", "tie:ga!=0"])
    k.hand([0.0] * 8 + [1.0, 2.0, 0.0, 0.0, 2.0], ["both_zero", "tie:ga!=0", "tie:s1>=s2"])
    k.hand([0.0] * 8 + [1.0, 0.0, 0.0, 0.0, 1.0], ["n1_zero"])
    return k


def step_tags(kind):
    def tag(p):
        it = p["ex"]["iters"]
        q = R._full(p["in"])
        alpha_in = q[7] if kind == "STEP" else q[14]
        p["t"][0] = ("gn_" if it < 0 else "reg_") + p["t"][0]
        p["t"].append("iters%d" % it if it > 0 else "gauss_newton")
        p["t"].append("alpha_in0" if alpha_in == 0.0 else "carried")
        if alpha_in != 0.0 and it > 0:                           # where the carried alpha lies in the first bracket
            K = R.F64()
            R.run(K, kind, p["in"])
            first = {}
            for n, _, o in K.trace:
                if n in ("below", "above") and n not in first:
                    first[n] = o
            p["t"].append("carried_below" if first.get("below") else "carried_above" if first.get("above") else "carried_inside")
    return tag


def slow_problem(rng, quota):
    """A 2 x 2 problem whose secular iteration SciPy ends after a count that `quota` still wants: a carried alpha that is already
    right (one iteration), or f along the small singular direction and a radius far inside (7 ... 10)."""
    from scipy.optimize._lsq import common
    for _ in range(400000):
        kap = 10 ** rng.uniform(0, 12)
        J = with_kappa(rng, 2, kap, 1.0)
        U, s, Vt = np.linalg.svd(J)
        f = U @ np.array([10 ** rng.uniform(-12, 0), 1.0]) if rng.random() < 0.7 else rng.standard_normal(2)
        Delta = np.linalg.norm(np.linalg.solve(J, -f)) * 10 ** rng.uniform(-14, -0.01)
        a0 = np.linalg.norm(J.T @ f) / Delta
        alpha = 0.0 if rng.random() < 0.5 else a0 * 10 ** rng.uniform(-12, 2)
        _, al, n = common.solve_lsq_trust_region(2, 2, U.T @ f, s, Vt.T, Delta, initial_alpha=alpha)
        if rng.random() < 0.02:
            alpha, n = al * (1 + rng.uniform(-0.01, 0.01)), 1
        if quota.get(n, 0) > 0:
            return J, f, Delta, alpha, kap
    raise AssertionError(("no more slow problems", quota))


def draw_slow(k, rng, kind, quota, row_of):
    def gen():
        J, f, Delta, alpha, kap = slow_problem(rng, quota)
        return row_of(J, f, Delta, alpha), [band(kap), "screened"]

    def tag(p):
        step_tags(kind)(p)
        it = p["ex"]["iters"]
        if quota.get(it, 0) > 0:
            quota[it] -= 1
    while any(v > 0 for v in quota.values()):
        k.draw(gen, 1, tag)


def step(rng):
    k = Kind("STEP")

    def gen():
        kap = 10 ** rng.uniform(0, 12)
        sc = 10 ** rng.uniform(-20, 20) if rng.random() < 0.2 else 10 ** rng.uniform(-2, 2)
        J = with_kappa(rng, 2, kap, sc)
        f = rng.standard_normal(2) * 10 ** rng.uniform(-3, 1)
        gn = np.linalg.solve(J, -f)
        Delta = np.linalg.norm(gn) * 10 ** (rng.uniform(0.01, 1) if rng.random() < 0.25 else rng.uniform(-4, -0.01))
        alpha = 0.0
        tags = [band(kap)] + (["scaled"] if not 1e-2 <= sc <= 1e2 else [])
        if rng.random() < 0.45:
            a0 = np.linalg.norm(J.T @ f) / Delta                   # the upper end of the bracket
            u = rng.choice([-6, -1, 1.5])
            alpha = a0 * 10 ** (u + rng.uniform(-1, 1))
        return list(J.ravel()) + list(f) + [Delta, alpha], tags
    k.draw(gen, 560, step_tags("STEP"))

    # the rare ones, screened by SciPy's own iteration count, then held to the same conditions
    draw_slow(k, rng, "STEP", {1: 6, 7: 4, 8: 3, 9: 2, 10: 2}, lambda J, f, Delta, alpha: list(J.ravel()) + list(f) + [Delta, alpha])
    # rank one: a structurally zero column, both axes, both signs of the gradient
    for col in (0, 1):
        for sg in (1.0, -1.0):
            J = [[0.0, 0.0], [0.0, 0.0]]
            J[0][1 - col], J[1][1 - col] = 0.75, -1.5
            f = [sg * 0.5, -sg * 0.25]
            p = k.hand([J[0][0], J[0][1], J[1][0], J[1][1]] + f + [0.125, 3.0], ["rank1", "axis%d" % (1 - col), "g_pos" if sg > 0 else "g_neg"])
            assert p["rule"][col] == 0.0 and abs(p["rule"][1 - col]) == 0.125 and p["rule"][2] == 0.0 and p["rule"][5] == 1 - col
            assert (p["rule"][1 - col] < 0) == (sg > 0)
    k.hand([0.0, 0.0, 0.0, 0.0, 0.5, 0.25, 0.125, 0.0], ["both_zero", "nan", "tie:det", "tie:ga!=0", "tie:s1>=s2", "tie:rank", "tie:below", "tie:above"])
    # exactly on the region: p = (3, 4) / 8, Delta = 5 / 8
    p = k.hand([2.0, 0.0, 0.0, 4.0, -0.75, -2.0, 0.625, 0.0], ["gn_on_region", "tie:inside", "gauss_newton"])
    assert p["rule"][0:3] == [0.375, 0.5, 0.0]
    # exactly singular, consistent and not: the !full_rank start, with and without a carried alpha
    for alpha in (0.0, 0.3):
        k.hand([1.0, 2.0, 2.0, 4.0, 0.5, 0.25, 0.01, alpha], ["singular", "not_full_rank", "tie:det", "alpha_in0" if alpha == 0 else "carried"])
        k.hand([3.0, -1.5, 1.0, -0.5, 0.5, -0.125, 0.01, alpha], ["singular", "not_full_rank", "tie:det", "alpha_in0" if alpha == 0 else "carried"])
    # |det| on both sides of 2 eps 2 F, full rank by SciPy's test on one of them
    for kap, tag in ((2e14, "det_above"), (4e15, "det_below")):
        for th in (0.3, 1.1, 2.0):
            J = (rot(th) * np.array([1.0, 1.0 / kap])) @ rot(0.7).T
            for Delta in (1e-3, 1e30):
                # at kappa ~ 1 / eps the restatement's own singular values are rounding noise: an edge on which it does not take the
                # exact run's side of every comparison has no expected outcome and is counted (header: "edges_without_margin")
                p = make("STEP", list(J.ravel()) + [0.5, 0.25, Delta, 0.0], [tag])
                if p is None:
                    k.lost_edges += 1
                else:
                    k.problems.append(p)
    return k


def stepn(rng):
    k = Kind("STEPN")

    def gen(N):
        def g():
            row, kap, Jh, diag, f, d = aug_matrix(rng, N, rng.random() < 0.3)
            A = np.array(row[0:8]).reshape(4, 2)[:, :N] if N == 2 else np.array([[row[0]], [row[2]]])
            fa = np.array(row[8:8 + 2 * N])
            gn = np.linalg.lstsq(A, -fa, rcond=None)[0]
            Delta = np.linalg.norm(gn) * 10 ** (rng.uniform(0.01, 1) if rng.random() < 0.25 else rng.uniform(-4, -0.01))
            alpha = 0.0
            if rng.random() < 0.45:
                alpha = np.linalg.norm(A.T @ fa) / Delta * 10 ** (rng.choice([-6, -1, 1.5]) + rng.uniform(-1, 1))
            return row + [Delta, alpha], [("n1" if N == 1 else band(kap))]
        return g
    k.draw(gen(2), 360, step_tags("STEPN"))
    k.draw(gen(1), 60, step_tags("STEPN"))
    k.hand([0.0] * 8 + [1.0, 0.0, 0.0, 0.0, 1.0, 0.5, 0.0], ["n1_zero", "nan", "tie:rank", "tie:below", "tie:above"])
    k.hand([1.0, 2.0, 2.0, 4.0, 0.0, 0.0, 0.0, 0.0, 0.5, 0.25, 0.0, 0.0, 2.0, 0.01, 0.0], ["singular", "not_full_rank"])
    # the rare ones for N = 2 (J above a zero block: diag = 0, as trf_bounded builds it where no gradient component is positive)
    draw_slow(k, rng, "STEPN", {1: 4, 7: 3, 8: 2, 9: 2, 10: 2},
              lambda J, f, Delta, alpha: list(J.ravel()) + [0.0] * 4 + list(f) + [0.0, 0.0, 2.0, Delta, alpha])
    # exactly on the region: p_h = (3, 4) / 8, Delta = 5 / 8; and both columns zero
    p = k.hand([2.0, 0.0, 0.0, 4.0, 0.0, 0.0, 0.0, 0.0, -0.75, -2.0, 0.0, 0.0, 2.0, 0.625, 0.0], ["gn_on_region", "tie:ga!=0", "tie:inside", "gauss_newton"])
    assert p["rule"] == [0.375, 0.5, 0.0]
    k.hand([0.0] * 8 + [0.5, 0.25, 0.0, 0.0, 2.0, 0.125, 0.0], ["both_zero", "nan", "tie:ga!=0", "tie:s1>=s2", "tie:rank", "tie:below", "tie:above"])
    return k


def select(rng):
    from scipy.optimize._lsq import common
    k = Kind("SELECT")
    # most random problems stay inside the bounds: drawn until each path has its share (the path by the restatement, before the
    # conditions are looked at)
    quota = {"inside": 100, "reflected": 150, "gradient": 130, "scaled": 24}

    def gen():
        while True:
            row, tags = draw_one()
            path = R.run(R.F64(), "SELECT", row)[1]["path"]
            if quota[path] > 0 or not any(quota.values()):
                return row, tags

    def draw_one():
        N = 1 if rng.random() < 0.3 else 2
        lb = 0.0 if rng.random() < 0.5 else 1e-10
        x = lb + 10 ** rng.uniform(-4, 1, N)
        J = with_kappa(rng, 2, 10 ** rng.uniform(0, 4), 10 ** rng.uniform(-1, 1))[:N, :N] if N == 2 else np.array([[rng.standard_normal()]])
        f = rng.standard_normal(N) * 10 ** rng.uniform(-2, 1)
        g = J.T @ f
        v = np.where(g > 0, x - lb, 1.0)
        dv = np.where(g > 0, 1.0, 0.0)
        d, diag = np.sqrt(v), g * dv
        gh, Jh = d * g, J * d
        A = np.vstack([Jh, np.diag(np.sqrt(diag))])
        U, s, Vt = np.linalg.svd(A, full_matrices=False)
        Delta = np.linalg.norm(x / np.sqrt(v)) * 10 ** rng.uniform(-2, 1)
        ph, _, _ = common.solve_lsq_trust_region(N, N, U.T @ np.concatenate([f, np.zeros(N)]), s, Vt.T, Delta)
        theta = max(0.995, 1 - np.max(np.abs(g * v)))
        tags = ["n%d" % N, "lb0" if lb == 0 else "lb1e-10"]
        if rng.random() < 0.15:                                  # a radius smaller than the step it is given: no reflected step
            Delta = Delta * 10 ** rng.uniform(-2, -0.5)
            tags.append("shrunk_radius")
        row = np.zeros(20)
        row[0:N], row[6:6 + N], row[8:8 + N], row[10:10 + N], row[12:12 + N], row[14:14 + N] = x, diag, gh, d * ph, ph, d
        row[2:2 + N * N] = Jh.ravel()
        row[16:20] = [Delta, lb, theta, N]
        return list(row), tags

    def tag(p):
        p["t"].insert(0, p["ex"]["path"])
        K = R.F64()
        R.run(K, "SELECT", p["in"])
        tr = dict((n, o) for n, _, o in K.trace)
        if tr.get("rs>0") is False:
            p["t"].append("rs<=0")
        if "rs==to_bound" in tr:
            p["t"].append("rs_bound" if tr["rs==to_bound"] else "rs_region")
        if p["t"][0] == "scaled" and p["sp"] is not None:
            p["t"].append("scaled_scipy")                        # a scaled step that SciPy's select_step answers too
        quota[p["t"][0]] = max(0, quota[p["t"][0]] - 1)
    k.draw(gen, sum(quota.values()), tag)
    h = lambda row, tags: k.hand(row, tags)
    # a == 0 in min_quad: no curvature at all (J_h = 0, diag = 0)
    h([1.0, 1.0, 0, 0, 0, 0, 0, 0, 0.5, 0.25, -2.0, -0.5, -2.0, -0.5, 1.0, 1.0, 3.0, 0.0, 0.995, 2.0], ["a0", "n2", "tie:quad_e"])
    # a component of the step that is 0, and a tie in hits (both components reach the bound together)
    h([1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0, 0, 0.5, 0.25, -2.0, 0.0, -2.0, 0.0, 1.0, 1.0, 3.0, 0.0, 0.995, 2.0], ["step_zero", "n2"])
    h([1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0, 0, 0.5, 0.3, -2.0, -2.0, -2.0, -2.0, 1.0, 1.0, 3.0, 0.0, 0.995, 2.0], ["hits_tie", "n2", "tie:hits"])
    for p in k.problems[-3:]:
        p["t"].insert(0, p["ex"]["path"])
    return k


def update(rng):
    k = Kind("UPDATE")

    def gen():
        cost = 10 ** rng.uniform(-6, 2)
        Delta = 10 ** rng.uniform(-3, 1)
        xn = 10 ** rng.uniform(-2, 2)
        x = rot(rng.uniform(0, 6.3)) @ [xn, 0.0]
        mode = rng.integers(0, 6)
        pn = Delta * rng.choice([0.3, 0.9, 0.97, 1.0])
        ratio = rng.choice([-0.5, 0.1, 0.2, 0.3, 0.5, 0.7, 0.8, 1.0, 1.3])
        predicted = cost * 10 ** rng.uniform(-4, -0.3)
        if mode == 1:                                            # ftol: a tiny reduction
            predicted = cost * 10 ** rng.uniform(-12, -9)
        if mode == 2:                                            # xtol: a tiny step
            pn = 1e-10 * xn * 10 ** rng.uniform(-2, -0.5)
        if mode == 3:                                            # both
            predicted, pn = cost * 10 ** rng.uniform(-12, -9), 1e-10 * xn * 10 ** rng.uniform(-2, -0.5)
        p = rot(rng.uniform(0, 6.3)) @ [pn, 0.0]
        cost_new = cost - ratio * predicted
        tags, finite = [], 1.0
        if mode == 4:
            predicted = -predicted
            tags.append("predicted_neg")
        if mode == 5 and rng.random() < 0.5:
            finite, cost_new = 0.0, math.inf
            tags.append("nonfinite")
        return [finite, p[0], p[1], x[0], x[1], cost, cost_new, predicted, Delta], tags

    def tag(p):
        d = p["disc"]
        p["t"].insert(0, "term%d_%s" % (d["term"], d["case"]))
        p["t"].append("accept" if d["accept"] else "reject")
        q = p["in"]
        if q[0]:
            K = R.F64()
            R.run(K, "UPDATE", q)
            for n, _, o in K.trace:
                if n in ("ratio<0.25", "ratio>0.75", "bound_hit"):
                    p["t"].append(n + ("" if o else ":no"))
    k.draw(gen, 320, tag)
    p = k.hand([1.0, 0.3, 0.4, 1.0, 2.0, 0.5, 0.5, 0.0, 1.0], ["pred0_actual0", "tie:predicted>0", "tie:accept", "tie:ftol"])
    tag(p)
    p = k.hand([1.0, 0.3, 0.4, 1.0, 2.0, 0.5, 0.25, 0.0, 1.0], ["pred0", "tie:predicted>0"])
    tag(p)
    return k


def solve3(rng):
    k = Kind("SOLVE3")

    def gen_matrix(m0, m1, l0, l1):
        return [-2 * m0 - l0, 0.0, m1, 0.0, -2 * m1 - l1, m0, 2 * m0, 2 * m1, -m0 - m1]

    def gen():
        m0, m1, l0, l1 = 10 ** rng.uniform(-8, 4, 4)
        tags = ["generator"]
        u = rng.random()
        if u < 0.2:
            m1 = 0.0
            tags.append("mu1_0")
        elif u < 0.4:
            m0 = 0.0
            tags.append("mu0_0")
        return gen_matrix(m0, m1, l0, l1) + list(rng.uniform(0.05, 1, 3)), tags

    def gen_dense():
        kap = 10 ** rng.uniform(0, 12)
        Q1, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        Q2, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        Mx = (Q1 * np.array([1.0, kap ** -0.5, 1.0 / kap])) @ Q2.T * 10 ** rng.uniform(-3, 3)
        return list(Mx.ravel()) + list(rng.standard_normal(3)), ["dense_" + band(kap)]

    def tag(p):
        sw = p["ex"]["swaps"]
        p["t"].append("swaps%d%d" % (sw[0], sw[1]))
    k.draw(gen, 220, tag)
    k.draw(gen_dense, 200, tag)
    # structural zeros: pairs of generators that differ in an entry a component does not depend on ("pair": the partner,
    # "same": the outputs that must then agree bit for bit)
    for _ in range(20):
        m, l0, l1, l1b = 10 ** rng.uniform(-3, 3, 4)
        b = list(rng.uniform(0.05, 1, 3))
        for which in (0, 1):
            rows = [gen_matrix(m, 0.0, l0, l1), gen_matrix(m, 0.0, l0, l1b)] if which == 0 else [gen_matrix(0.0, m, l1, l0), gen_matrix(0.0, m, l1b, l0)]
            same = [3, 6, 7, 8] if which == 0 else [4, 9, 10, 11]
            n = len(k.problems)
            for j, r in enumerate(rows):
                p = k.hand(r + b, ["generator", "mu1_0" if which == 0 else "mu0_0", "structural_pair"])
                tag(p)
                p["pair"], p["same"] = n + 1 - j, same
            a, c = k.problems[n]["rule"], k.problems[n + 1]["rule"]
            assert all(a[i] == c[i] for i in same) and any(a[i] != c[i] for i in range(3, 15)), (a, c)
    tag(k.hand([2.0, 1.0, 0.0, -2.0, 3.0, 1.0, 1.0, 4.0, 5.0, 1.0, 2.0, 3.0], ["pivot_tie", "tie:pivot0", "tie:pivot1"]))
    tag(k.hand([1.0, 2.0, 3.0, 1.0, 3.0, 1.0, -1.0, 1.0, 4.0, 1.0, 2.0, 3.0], ["pivot_tie", "tie:pivot0", "tie:pivot1"]))
    p = k.hand([1.0, 2.0, 3.0, 2.0, 1.0, 1.0, 4.0, 1.0, 5.0, 1.0, 2.0, 3.0], ["two_swaps"])
    tag(p)
    assert p["ex"]["swaps"] == [True, True], p["ex"]
    return k


BUILDERS = [scalar, svd2, svd4, step, stepn, select, update, solve3]
# what the fixture promises, by tag
COVERAGE = {
    "SCALAR": ["pow2", "near_pow2", "square", "random", "special", "in_range", "recorded", "edge"],
    "SVD2": ["k4", "k8", "k12", "k15", "scale_extreme", "ga0", "al_eq_be", "zeta_tiny", "zeta_huge", "zero_col", "both_zero", "swap", "no_swap", "equal_sv"],
    "SVD4": ["k4", "k8", "k12", "k15", "scale_extreme", "ga0", "zero_col", "both_zero", "swap", "no_swap", "equal_sv", "aug", "aug_diag0", "aug_diag", "n1", "n1_zero"],
    "STEP": ["gn_k4", "gn_k8", "gn_k12", "reg_k4", "reg_k8", "reg_k12", "gn_on_region", "det_above", "det_below", "rank1", "axis0", "axis1", "g_pos", "g_neg",
             "both_zero", "alpha_in0", "carried", "carried_below", "carried_inside", "carried_above", "not_full_rank", "scaled"] + ["iters%d" % i for i in range(1, 11)],
    "STEPN": ["gn_k4", "gn_k8", "gn_k12", "reg_k4", "reg_k8", "reg_k12", "gn_n1", "reg_n1", "n1_zero", "alpha_in0", "carried", "not_full_rank", "gn_on_region",
              "both_zero", "carried_below", "carried_inside", "carried_above"] + ["iters%d" % i for i in range(1, 11)],
    "SELECT": ["inside", "scaled", "reflected", "gradient", "rs<=0", "rs_bound", "rs_region", "scaled_scipy", "a0", "step_zero", "hits_tie", "n1", "n2", "lb0", "lb1e-10"],
    "UPDATE": ["ratio<0.25", "ratio<0.25:no", "ratio>0.75", "ratio>0.75:no", "bound_hit", "bound_hit:no", "pred0_actual0", "predicted_neg", "nonfinite",
               "accept", "reject", "term0_quartered", "term0_doubled", "term0_kept", "term2_kept", "term3_kept", "term4_kept"],
    "SOLVE3": ["generator", "mu1_0", "mu0_0", "dense_k4", "dense_k8", "dense_k12", "pivot_tie", "two_swaps", "structural_pair", "swaps00", "swaps10", "swaps01", "swaps11"],
}


def check(fx):
    """The fixture's conditions, from the stored file alone (tests/test_lsq_probe_cpu.py re-runs the restatement on top)."""
    for kind, ps in fx["kinds"].items():
        tags = {t for p in ps for t in p["t"]}
        missing = [t for t in COVERAGE[kind] if t not in tags]
        assert not missing, (kind, "no problem reaches", missing)
        for p in ps:
            assert p["mg"] > p["need"], (kind, p)
            assert len(p["in"]) == USED_IN[kind] and len(p["rule"]) == USED_OUT[kind]
        assert fx["header"]["lost"][kind] <= MAX_LOSS, (kind, fx["header"]["lost"][kind])
    return True


def main():
    if "--check" in sys.argv:
        with gzip.open(OUT, "rt") as f:
            fx = json.load(f)
        check(fx)
        print("conditions hold: " + ", ".join("%s %d" % (k, len(v)) for k, v in fx["kinds"].items()))
        return
    fx = {"header": {"units": "relative error / (eps kappa), see tests/lsq_rule.figures", "device_factor": R.DEVICE_FACTOR, "scalar_ulps": R.SCALAR_ULPS,
                     "lost": {}, "edges_without_margin": {}, "worst": {}}, "kinds": {}}
    for i, b in enumerate(BUILDERS):
        k = b(np.random.default_rng(20261019 + i))
        fx["kinds"][k.name] = k.problems
        fx["header"]["lost"][k.name] = k.lost / max(k.drawn, 1)
        fx["header"]["edges_without_margin"][k.name] = k.lost_edges
        w_rule = R.worst(k.name, k.problems, [p["rule"] for p in k.problems])
        w_sp = R.worst(k.name, k.problems, [p["sp"] for p in k.problems])
        fx["header"]["worst"][k.name] = {c: {"rule": w_rule[c], "scipy": w_sp.get(c), "ratio": (w_rule[c] / w_sp[c]) if w_sp.get(c) else None} for c in sorted(w_rule)}
        print("%-7s %5d problems, %4d of %5d drawn without margin (%.2f %%)%s" % (k.name, len(k.problems), k.lost, k.drawn, 100.0 * k.lost / max(k.drawn, 1),
                                                                                  ", %d hand-made edges without margin" % k.lost_edges if k.lost_edges else ""))
        for c, v in fx["header"]["worst"][k.name].items():
            print("        %-28s restatement %-10.4g scipy %-10s ratio %s" % (c, v["rule"], "%.4g" % v["scipy"] if v["scipy"] is not None else "-", "%.3g" % v["ratio"] if v["ratio"] else "-"))
    check(fx)
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps(fx, separators=(",", ":")).encode())
    print("wrote %s: %d bytes" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) < (1 << 20)


if __name__ == "__main__":
    main()
