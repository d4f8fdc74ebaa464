"""The branch choice of the pair-chain residual (pair_eval -> pair_expv / pair_reduced, misti_pair.h) restated in plain float64
Python, and float64 restatements of its cascade, Taylor and uniformisation forms: what tests/golden/make_pair_branches.py labels
the fixtures with, and what tests/test_pair_branches_cpu.py holds to the same bounds as the device.  Every product that decides a
branch is exact or a single rounding in both places (2 * x is exact), so the labels are the device's branches to the bit."""
import math

EPS = 2.220446049250313e-16
SQRT_EPS = 1.4901161193847656e-08                   # fd_step: 2^-26
TAYLOR_EDGES = (0.01, 0.04, 0.12, 0.25, 0.5, 1.0, 2.0)     # classes of nn = 2 nbmax
TAYLOR_DEGREES = (8, 10, 12, 14, 17, 21, 27)
SERIES_MAX = 6.0                                    # uniformisation up to this nbmax, the closed forms above it
W_BOUND = 2e-13                                     # of the largest component of the exact result (the bound pair_eigen is held to)
NORM_FLOOR = 1e-280                                 # intervals whose exact result is smaller are skipped
BRANCHES = tuple("taylor%d" % i for i in range(7)) + ("series", "cascade1", "cascade2", "eigen")


def fd_step(x):
    return SQRT_EPS * (1.0 if x >= 0 else -1.0) * max(1.0, abs(x))


def branch(mu0, mu1, nbmax):
    """The form pair_expv takes for migration rates (mu0, mu1) and the bound nbmax = q + neg."""
    if not nbmax < 1e300:
        return "guard"
    if nbmax > SERIES_MAX:
        return "cascade1" if mu1 == 0.0 else "cascade2" if mu0 == 0.0 else "eigen"
    nn = 2.0 * nbmax
    if nn <= 2.0:
        for i, e in enumerate(TAYLOR_EDGES):
            if nn <= e:
                return "taylor%d" % i
    return "series"


def forward_interval(l0, l1, mu0, mu1, T):
    """forward_kernel's arguments of pair_expv for one interval: (a0, a1, b0, b1, q)."""
    a0, a1, b0, b1 = l0 * T, l1 * T, mu0 * T, mu1 * T
    return a0, a1, b0, b1, max(max(2.0 * b0 + a0, 2.0 * b1 + a1), b0 + b1)


def _fmax(a, b):                                    # fmax: a NaN loses
    if a != a:
        return b
    if b != b:
        return a
    return max(a, b)


def _fmin(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return min(a, b)


def eval_point(mu0, mu1, x0, x1, role):
    """pair_eval's set-up: the rates (l0, l1) this role evaluates, q, neg and ok."""
    xa, xb = x0 + fd_step(x0), x1 + fd_step(x1)
    e = int(role) >> 1
    l0 = xa if e == 1 else x0
    l1 = xb if e == 2 else x1
    ok = math.isfinite(x0) and math.isfinite(x1)
    m0, m1 = _fmax(x0, xa), _fmax(x1, xb)
    q = _fmax(_fmax(2.0 * mu0 + m0, 2.0 * mu1 + m1), _fmax(mu0 + mu1, 0.0))
    neg = _fmax(0.0, _fmax(-_fmin(x0, xa), -_fmin(x1, xb)))
    return l0, l1, q, neg, ok


# ---- float64 restatements ------------------------------------------------------------------------------------------------
def _dd_exp(x, y):
    g = abs(x - y)
    return math.exp(-min(x, y)) * (1.0 if g == 0.0 else -math.expm1(-g) / g)


def cascade64(which, l0, l1, mu0, mu1, v):
    mu = mu0 if which == 1 else mu1
    a = 2.0 * mu0 + l0 if which == 1 else 2.0 * mu1 + l1
    c = 2.0 * mu1 + l1 if which == 1 else 2.0 * mu0 + l0
    b = mu0 + mu1
    vS, vK, v2 = (v[0], v[1], v[2]) if which == 1 else (v[1], v[0], v[2])
    s0, s1, s2 = sorted((a, b, c))
    gap = s2 - s0
    D3 = (_dd_exp(s0, s1) - _dd_exp(s1, s2)) / gap if gap > 0.0 else 0.5 * math.exp(-s0)
    wS = math.exp(-a) * vS
    w2 = math.exp(-b) * v2 + (2.0 * mu) * _dd_exp(a, b) * vS
    wK = math.exp(-c) * vK + mu * _dd_exp(b, c) * v2 + (2.0 * mu * mu) * D3 * vS
    return [wS, wK, w2] if which == 1 else [wK, wS, w2]


def reduced64(which, l0, l1, mu0, mu1, v):
    dk = 2.0 * mu1 + l1 if which == 1 else 2.0 * mu0 + l0
    d2 = mu0 + mu1
    mu = mu0 if which == 1 else mu1
    vk = v[1] if which == 1 else v[0]
    a, c = -dk, -d2
    ax = abs(a - c)
    phi = math.exp(max(a, c)) * (1.0 if ax == 0.0 else -math.expm1(-ax) / ax)
    wk = math.exp(a) * vk + mu * phi * v[2]
    w2 = math.exp(c) * v[2]
    return [0.0, wk, w2] if which == 1 else [wk, 0.0, w2]


def taylor64(K, l0, l1, mu0, mu1, v):
    """(exp(M) v, int_0^1 u exp(u M) v du) by K terms of the series."""
    d0, d1, d2 = 2.0 * mu0 + l0, 2.0 * mu1 + l1, mu0 + mu1
    p = list(v)
    a = list(v)
    b = [0.5 * x for x in v]
    for k in range(1, K + 1):
        inv = 1.0 / k
        p = [(mu1 * p[2] - d0 * p[0]) * inv, (mu0 * p[2] - d1 * p[1]) * inv, ((2.0 * mu0 * p[0] + 2.0 * mu1 * p[1]) - d2 * p[2]) * inv]
        a = [a[i] + p[i] for i in range(3)]
        b = [b[i] + p[i] / (k + 2) for i in range(3)]
    return a, b


def uniform64(l0, l1, mu0, mu1, v, q, nbmax):
    d0, d1, d2 = 2.0 * mu0 + l0, 2.0 * mu1 + l1, mu0 + mu1
    n00, n11, n22 = q - d0, q - d1, q - d2
    eq = math.exp(-q)
    p = [eq * x for x in v]
    a = list(p)
    b = 1.0
    for k in range(1, 200):
        inv = 1.0 / k
        p = [(n00 * p[0] + mu1 * p[2]) * inv, (n11 * p[1] + mu0 * p[2]) * inv, (2.0 * mu0 * p[0] + 2.0 * mu1 * p[1] + n22 * p[2]) * inv]
        a = [a[i] + p[i] for i in range(3)]
        b *= nbmax * inv
        if b < 1e-19 and k > nbmax:
            break
    return a


def expv64(l0, l1, mu0, mu1, v, q, neg):
    """pair_expv in float64 for the branches restated here (None for pair_eigen and the guard)."""
    nb = q + neg
    br = branch(mu0, mu1, nb)
    if br.startswith("cascade"):
        return cascade64(int(br[-1]), l0, l1, mu0, mu1, v)
    if br.startswith("taylor"):
        return taylor64(TAYLOR_DEGREES[int(br[-1])], l0, l1, mu0, mu1, v)[0]
    if br == "series":
        return uniform64(l0, l1, mu0, mu1, v, q, nb)
    return None


def ect_floor(ect, pnc):
    """The default fit's series form divides by 1 - pnc, a difference from one of a sum rounded near one: its own floor."""
    from parity import FLOOR_ULPS
    return FLOOR_ULPS * EPS * abs(ect) * (1.0 + 1.0 / (1.0 - pnc))


# ---- what the fixtures promise to cover: asserted by the generator and again by the tests that read them ----
def coverage_forward(fx):
    """The coverage the forward-map fixture promises (the issue's part A); intervals whose exact result is below NORM_FLOOR do not count."""
    ivs = []
    for m in fx["models"]:
        for c in m["candidates"]:
            for t, iv in enumerate(c["intervals"]):
                if max(abs(x) for x in c["exact"][t]) >= NORM_FLOOR:
                    ivs.append((iv, c["params"]))
    n = lambda f: sum(1 for iv, p in ivs if f(iv, p))
    for i, e in enumerate(TAYLOR_EDGES):
        assert n(lambda iv, p: iv["branch"] == "taylor%d" % i) >= 8, i
        assert n(lambda iv, p: 0.99 * e <= 2 * iv["nbmax"] <= e) >= 2, e
        assert n(lambda iv, p: e < 2 * iv["nbmax"] <= 1.01 * e) >= 2, e
    assert n(lambda iv, p: iv["branch"] == "series") >= 16
    assert n(lambda iv, p: iv["branch"] == "series" and 5.9 < iv["nbmax"] <= 6.0) >= 4
    assert n(lambda iv, p: 6.0 < iv["nbmax"] <= 6.06 and iv["branch"].startswith("cascade")) >= 4
    assert n(lambda iv, p: 6.0 < iv["nbmax"] <= 6.06 and iv["branch"] == "eigen") >= 4
    for w in (1, 2):
        mine = lambda iv, p, w=w: iv["branch"] == "cascade%d" % w
        assert n(mine) >= 40, w
        assert max(iv["rate_x_length"] for iv, p in ivs if mine(iv, p)) >= 2.9e5
        for tag in ("c_near_b", "c_eq_a", "stiff_by_mu", "unit_left"):
            assert n(lambda iv, p: mine(iv, p) and tag in iv["tags"]) >= 1, (w, tag)
    assert n(lambda iv, p: "no_migration" in iv.get("tags", ()) and iv["rate_x_length"] > 6) >= 1
    for m in fx["models"]:
        assert len(m["candidates"]) >= 64, m["name"]          # full waves for the lane-independence test
    return len(ivs)


LN_DBL_MIN = math.log(2.2250738585072014e-308)       # masses above it are normal doubles


def forward_bound(t, ratio, x):
    """The bound on x_t = seen rate x length of interval t (tests/test_gpu_exact_forward.py): pair_expv is held to W_BOUND of the largest
    component of its result, the state that enters interval t carries the errors of the t intervals before it, and x = -log(nc / before)
    turns a relative error of nc into an absolute one of x - so (t + 1) W_BOUND max|v| / nc - plus the roundings of the logarithm, the
    division by T and the products rate x length.  `ratio` is max|v_exact| / nc_exact."""
    return (t + 1) * W_BOUND * ratio + 8 * EPS * max(1.0, x)


def coverage_exact_forward(fx):
    """The regimes tests/golden/golden_exact_forward.json.gz promises to reach: conditions on the inputs and their labels alone.
    Returns the number of intervals per branch."""
    regs = {r["name"]: r for r in fx["regimes"]}
    assert set(regs) == {"branches", "tiny", "no_migration", "decay", "pulses", "hold_mu", "fractional", "statuses"}, sorted(regs)
    per_branch = {}
    for r in fx["regimes"]:
        for m in r["models"]:
            assert 6 <= len(m["lh"]) <= 12 and len(m["times"]) == len(m["lh"]) - 1 and len(m["candidates"]) <= 65, m["name"]
            for c in m["candidates"]:
                assert sorted(c["exact"]) == [str(h) for h in m["hold"]]
                for e in c["exact"].values():
                    for br in e.get("branch", ()):
                        per_branch[br] = per_branch.get(br, 0) + 1
    # -- every branch, through models
    for br in BRANCHES:
        assert per_branch.get(br, 0) >= 8, (br, per_branch)
    walk = regs["branches"]["models"][0]
    assert len(walk["candidates"]) == 65
    walks = lambda b: b[0] == "taylor0" and len(set(b) & set(BRANCHES[:7])) >= 5 and "series" in b and b[-1] in BRANCHES[8:]
    assert sum(1 for c in walk["candidates"] if walks(c["exact"]["0"]["branch"])) >= 3          # one per direction of migration
    stiff, one_way = 0.0, set()
    for m in regs["branches"]["models"]:
        for c in m["candidates"]:
            for t, br in enumerate(c["exact"]["0"]["branch"]):
                if br == "eigen":
                    stiff = max(stiff, max(m["lh"][t]) * m["times"][t])
                if br.startswith("cascade") and max(c["params"]) > 0:
                    one_way.add(br)
    assert stiff >= 2e5, stiff
    assert one_way == {"cascade1", "cascade2"}, one_way
    # -- tiny intervals: every decade, at the chain's start and in a mixed state, with and without migration
    decades = set()
    for m in regs["tiny"]["models"]:
        d = m["decade"]
        for c in m["candidates"]:
            e = c["exact"]["0"]
            for t in (0, 2, 3):
                assert all(0.2 * 10.0 ** -d <= x <= 1.5 * 10.0 ** -d for x in e["x"][t]), (m["name"], c["params"], t, e["x"][t])
                decades.add((d, "no_migration" in c["tags"], t == 0))
            assert c["params"] == [0.0, 0.0] if "no_migration" in c["tags"] else max(c["params"]) > 0
            mixed = e["pr"][2]                                   # the state the tiny interval 2 starts from
            assert "no_migration" in c["tags"] or max(mixed[4], mixed[5]) > 1e-3, (m["name"], mixed)
    assert decades == {(d, nm, st) for d in range(2, 13) for nm in (False, True) for st in (False, True)}
    # -- no migration at all
    nm = regs["no_migration"]["models"][0]
    assert not nm["bands"] and not nm["pulses"] and len(nm["candidates"]) >= 8
    # -- decaying mass
    reached, past, skew = set(), 0, 0.0
    for m in regs["decay"]["models"]:
        lowest = min(v for c in m["candidates"] for row in c["exact"]["0"]["ln_nc"] for v in row)
        for c in m["candidates"]:
            e = c["exact"]["0"]
            cum = [sum(row[k] for row in e["x"]) for k in (0, 1)]
            for target in (50, 300, 700):
                if max(cum) >= target and lowest > LN_DBL_MIN:
                    reached.add(target)
            past += max(cum) > 745
            for row in e["pr"][1:]:
                for k in (0, 1):
                    comp = [abs(row[j]) for j in (k, 2 + k, 4 + k) if row[j] != 0.0]
                    if lowest > LN_DBL_MIN and comp:
                        skew = max(skew, max(comp) / min(comp))
    assert reached == {50, 300, 700}, reached
    assert past == 2, past
    assert skew >= 1e200, skew
    # -- pulses
    seen = set()
    for m in regs["pulses"]["models"]:
        assert [p[1] for p in m["pulses"]] == [0, 2, 3, 5] and all(c["split"] == 6.0 for c in m["candidates"])
        pops = {p[0] for p in m["pulses"]}
        for c in m["candidates"]:
            for rate in ("rate_1e-12", "rate_0.5", "rate_1-2^-53"):
                for where in ("first_interval", "last_before_split", "consecutive"):
                    if rate in c["tags"] and where in c["tags"]:
                        seen |= {(p, rate, where) for p in pops}
            if "rate_0" in c["tags"]:
                assert not any(c["params"])
                seen |= {(p, "rate_0", "") for p in pops}
    assert len(seen) == 2 * (9 + 1), sorted(seen)
    # -- hold_mu
    for m in regs["hold_mu"]["models"]:
        numT = len(m["lh"])
        assert m["hold"] == [0, 1] and [c["split"] for c in m["candidates"]] == [float(s) for s in range(1, numT + 1)]
        last = m["candidates"][-1]["exact"]
        assert all(last[h]["status"] == 3 and last[h]["n_eval"] == numT - 1 for h in ("0", "1")), m["name"]
    by_name = {m["name"]: m for m in regs["hold_mu"]["models"]}
    for name in ("fixed_ends", "end_at_split"):
        for pop in (0, 1):
            assert len({b[3] for b in by_name[name]["bands"] if b[0] == pop}) == 3
    assert sum(1 for b in by_name["end_at_split"]["bands"] if b[2] == -1) == 2 and all(b[2] != -1 for b in by_name["fixed_ends"]["bands"])
    assert all(c["exact"]["0"]["status"] in (0, 3) for c in by_name["fixed_ends"]["candidates"])
    assert {c["exact"]["1"]["status"] for c in by_name["end_at_split"]["candidates"]} == {0, 3, 4}
    assert all(b[1] == 0 and b[2] == -1 for b in by_name["constant"]["bands"])
    # -- fractional splits
    fr = regs["fractional"]["models"][0]
    numT = len(fr["lh"])
    assert fr["hold"] == [0, 1]
    assert {(int(c["split"]), c["split"] - int(c["split"])) for c in fr["candidates"]} == {(s, f) for s in (0, 3, numT - 2) for f in (2.0 ** -20, 0.5, 1 - 2.0 ** -20)}
    for c in fr["candidates"]:
        e = c["exact"]["0"]
        assert e["status"] == 0 and e["n_eval"] == int(c["split"]) + 1 and e["model_rows"][-1] == fr["lh"][-1], c["split"]
    # -- statuses
    st = {tag: c["exact"]["0"]["status"] for c in regs["statuses"]["models"][0]["candidates"] for tag in c["tags"]}
    assert st == dict(split_0=0, ok=0, negative_parameter=1, split_below_0=4, split_above_numT=4, split_at_numT=3, fraction_of_the_last=4,
                      fraction_before_the_band=0), st
    return per_branch


def coverage_residuals(fx):
    """The coverage the probe's fixture promises (the issue's part B)."""
    ps = fx["problems"]
    n = lambda f: sum(1 for p in ps if f(p))
    cp = [p for p in ps if p["cpfit"] and not p["red"]]
    for br in BRANCHES:
        pts = {(p["mu0"], p["mu1"], p["x0"], p["x1"]) for p in cp if p["branch"] == br}
        assert len(pts) >= 4, (br, len(pts))
    by_point = {}
    for p in cp:
        by_point.setdefault((p["mu0"], p["mu1"], p["x0"], p["x1"], tuple(p["P"])), set()).add(p["role"])
    assert sum(1 for r in by_point.values() if r == set(range(6))) >= 8
    red = [p for p in ps if p["red"]]
    assert len(red) >= 16 and {p["red"] for p in red} == {1, 2}
    assert min(p["exit_rate"] for p in red) <= 1.0 + 1e-6 and max(p["exit_rate"] for p in red) >= 2.9e5
    assert any(p["gap"] == 0.0 for p in red) and any(0 < p["gap"] <= 3e-9 * p["exit_rate"] for p in red)
    assert n(lambda p: p["regime"] == "negative_rate" and p["neg"] > 0 and p["neg"] < 0.1) >= 4
    for i in range(7):
        assert n(lambda p: not p["cpfit"] and p["regime"] == "ect_series" and p["branch"] == "taylor%d" % i) >= 6, i
    assert min(p["nbmax"] for p in ps if p["regime"] == "ect_series") <= 1.1e-5
    want = dict(ect_formula_uniformisation=("series",), ect_formula_one_way_stiff=("cascade1", "cascade2"), ect_formula_two_way_stiff=("eigen",),
                ect_formula_runaway=("eigen",))
    for regime, brs in want.items():
        assert n(lambda p: p["regime"] == regime and p["branch"] in brs) >= 8, regime
        assert n(lambda p: p["regime"] == regime and p["branch"] not in brs) == 0, regime
        assert fx["reference_formula"][regime]["worst_relative_error"] > 0
    assert n(lambda p: p["regime"] == "ect_formula_runaway" and 1e3 <= max(p["l0"], p["l1"]) <= 1.01e5 and 4e-4 <= p["mu0"] <= 2.1e-3) >= 8
    nanp = fx["nan_points"]
    assert any(not math.isfinite(float(p["x0"])) or not math.isfinite(float(p["x1"])) for p in nanp)
    assert any(max(abs(float(p["x0"])), abs(float(p["x1"]))) >= 1e300 and math.isfinite(float(p["x0"])) and math.isfinite(float(p["x1"])) for p in nanp)
    return len(ps)
