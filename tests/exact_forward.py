"""The forward map (CoalescentRates, MigrationInference.py:542-564, with CoalRates, CorrectLambda.py:112-122) in 50-digit arithmetic.

A restatement of ``OracleModel.coalescent_rates`` that takes the oracle's structure - the pair chain's generator pattern
(``_PairChain._matrix``), the pulse operator (``_pulse_pairs``), how a fractional split inserts its interval
(``OracleModel.__init__``) - and nothing of its floating-point arithmetic: the generator and the pulse operator are integer tables
here (tests/test_exact_forward_cpu.py holds them against the oracle's functions), every double is taken at its exact value, and the
exponential is ``mp.expm`` of the 3 x 3 generator x T with no special case for a migration rate of zero.

The model is given as the C ABI takes it (include/misti_hip.h): ``bands`` of ``(pop, start, end, value, param)`` with ``end == -1``
meaning the candidate's split index, ``pulses`` of ``(pop, time, value, param)``, indices on the candidate's own grid.  The two
lengths of the interval that a fractional split cuts are the doubles ``frac * T`` and ``T - frac * T`` - as the oracle and the
device form them - and exact from there on.

``hold_mu`` has the header's meaning: every interval sees the migration rates of the candidate's last two-population interval.
That is interval ``split - 1``; for a split at ``numT`` (status MISTI_INF_COAL: the last interval has no length and is not
evaluated) it is the last interval that is evaluated, ``numT - 2`` - the device's own rule, the reference has no value there.
"""
import math

import mpmath as mp

DPS = 50
OK, NEG_PARAM, INF_COAL, BAD_STRUCTURE = 0, 1, 3, 4

# M[i][j] = sum of coef * rate over (l0, l1, mu0, mu1); column = source state (both in 0, both in 1, one in each)
GENERATOR = {(0, 0): (-1, 0, -2, 0), (0, 2): (0, 0, 0, 1),
             (1, 1): (0, -1, 0, -2), (1, 2): (0, 0, 1, 0),
             (2, 0): (0, 0, 2, 0), (2, 1): (0, 0, 0, 2), (2, 2): (0, 0, -1, -1)}
# pulse of rate r out of population a (b = 1 - a): (dst, src, power of 1 - r, power of r, factor) over the roles (a, b, 2)
PULSE = (("a", "a", 2, 0, 1), ("b", "a", 0, 2, 1), ("b", "b", 0, 0, 1), ("b", "2", 0, 1, 1), ("2", "a", 1, 1, 2), ("2", "2", 1, 0, 1))


def generator(l0, l1, mu0, mu1):
    r = (mp.mpf(l0), mp.mpf(l1), mp.mpf(mu0), mp.mpf(mu1))
    M = mp.matrix(3, 3)
    for (i, j), co in GENERATOR.items():
        M[i, j] = sum(c * x for c, x in zip(co, r))
    return M


def pulse(v, pu0, pu1):
    """The pulse operator on one pair-state vector (three mpf); no pulse unless pu0 + pu1 > 0."""
    r = mp.mpf(pu0) + mp.mpf(pu1)
    if not r > 0:
        return list(v)
    a = 0 if pu0 > 0 else 1
    idx = {"a": a, "b": 1 - a, "2": 2}
    out = [mp.mpf(0)] * 3
    for dst, src, ns, nm, f in PULSE:
        out[idx[dst]] = out[idx[dst]] + f * (1 - r) ** ns * r ** nm * v[idx[src]]
    return out


class Grid:
    """A candidate's view of the model's grid and its status, by the header's rules (setup_candidate, misti_model.h)."""

    def __init__(self, times, lh, bands, split_time, params, sample_date=0):
        numT0 = len(lh)
        self.times, self.lh, self.src = [float(t) for t in times], [list(map(float, r)) for r in lh], list(range(numT0))
        self.numT, self.ins, self.status = numT0, -1, OK
        st = float(split_time)
        if not st >= 0 or not st >= sample_date or math.floor(st) > numT0:
            self.status, self.split = BAD_STRUCTURE, 0
            return
        s = int(math.floor(st))
        frac = st - s
        self.split = s
        if frac != 0.0:
            if s > numT0 - 2:
                self.status = BAD_STRUCTURE
                return
            t1 = frac * self.times[s]                       # two float64 roundings, as the oracle and the device form them
            t2 = self.times[s] - t1
            self.times[s:s + 1] = [t1, t2]
            self.lh.insert(s + 1, list(self.lh[s]))
            self.src = [t if t <= s else t - 1 for t in range(numT0 + 1)]
            self.ins, self.split, self.numT = s, s + 1, numT0 + 1
        for b, (pop, start, end, _, _) in enumerate(bands):
            if end < -1 or end > numT0 + 1:
                self.status = BAD_STRUCTURE
            eb = self.split if end < 0 else end
            if start < sample_date or eb <= start:
                self.status = BAD_STRUCTURE
            for pop_c, sc, ec, _, _ in bands[:b]:
                ec = self.split if ec < 0 else ec
                if pop_c == pop and start < ec and sc < eb:
                    self.status = BAD_STRUCTURE
        if self.status == OK and any(p < 0 for p in params):
            self.status = NEG_PARAM
        if self.status == OK and self.split >= self.numT:
            self.status = INF_COAL
        self.n_eval = min(self.split, self.numT - 1)        # intervals below the split that have a length

    def model_rows(self):
        """Rows n_eval .. numT0 of the device's lh output: the model's own rates, row numT0 used by a fractional split only."""
        numT0 = len(self.src) if self.ins < 0 else len(self.src) - 1
        return [list(self.lh[t]) if t < self.numT else [0.0, 0.0] for t in range(self.n_eval, numT0 + 1)]


def _value(value, param, params):
    return float(params[param]) if param >= 0 else float(value)


def migration(bands, params, split, t):
    mu = [0.0, 0.0]
    for pop, start, end, value, param in bands:
        if start <= t < (split if end < 0 else end):
            mu[pop] = _value(value, param, params)
    return mu


def pulse_rates(pulses, params, t):
    pu = [0.0, 0.0]
    for pop, time, value, param in pulses:
        if t == time:
            pu[pop] = _value(value, param, params)
    return pu


def exact_forward(times, lh, bands, pulses, split_time, params=(), hold_mu=False, sample_date=0):
    """One candidate.  Returns dict(status, numT, split, ins, n_eval, model_rows) and, where the status is OK or INF_COAL, per
    evaluated interval t < n_eval: T[t] (the double), mu[t] (the rates the interval sees), x[t][k] = -log(nc / before) and
    rate[t][k] = x / T (mpf), nc[t][k], v[t][k] (three mpf: the pair state of genome k after the interval), and row0[k] (the
    state after the first interval's pulse).  The `pr` layout of misti_forward_rates is pr[6 (t + 1) + j] = v[t][j & 1][j >> 1]."""
    bands, pulses, params = [tuple(b) for b in bands], [tuple(p) for p in pulses], [float(p) for p in params]
    g = Grid(times, lh, bands, split_time, params, sample_date)
    out = dict(status=g.status, numT=g.numT, split=g.split, ins=g.ins)
    if g.status not in (OK, INF_COAL):
        return out
    out.update(n_eval=g.n_eval, model_rows=g.model_rows(), T=[], mu=[], x=[], rate=[], nc=[], v=[], lh=[])
    with mp.workdps(DPS):
        p = [[mp.mpf(1), mp.mpf(0), mp.mpf(0)], [mp.mpf(0), mp.mpf(1), mp.mpf(0)]]
        out["row0"] = [list(p[0]), list(p[1])]
        held = migration(bands, params, g.split, min(g.split, g.numT - 1) - 1) if g.split >= 1 else [0.0, 0.0]
        for t in range(g.n_eval):
            pu = pulse_rates(pulses, params, t)
            p = [pulse(p[k], pu[0], pu[1]) for k in (0, 1)]
            if t == 0:
                out["row0"] = [list(p[0]), list(p[1])]
            mu = held if hold_mu else migration(bands, params, g.split, t)
            T = g.times[t]
            E = mp.expm(generator(g.lh[t][0], g.lh[t][1], mu[0], mu[1]) * mp.mpf(T))
            xs, ncs, vs = [], [], []
            for k in (0, 1):
                before = p[k][0] + p[k][1] + p[k][2]
                w = E * mp.matrix(p[k])
                p[k] = [w[0], w[1], w[2]]
                nc = w[0] + w[1] + w[2]
                xs.append(-mp.log(nc / before))
                ncs.append(nc)
                vs.append(list(p[k]))
            out["T"].append(T)
            out["mu"].append(list(mu))
            out["lh"].append(list(g.lh[t]))
            out["x"].append(xs)
            out["rate"].append([x / mp.mpf(T) for x in xs])
            out["nc"].append(ncs)
            out["v"].append(vs)
    return out
