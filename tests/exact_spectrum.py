"""The expected joint allele-frequency spectrum (JAFSpectrum, MigrationInference.py:467-506) in 50-digit arithmetic.

A restatement of ``OracleModel.jaf_spectrum`` that takes the oracle's constant structure (``TWO_POP`` / ``ONE_POP``: generator
patterns, pulse operator, ancient-sample map, collapse ranges and spectrum weights) and nothing of its floating-point
arithmetic.  Each finite interval's end state and occupation integral come from ONE exponential of the augmented matrix

    [[M T, x T],        exp(.) = [[e^{M T}, int_0^T e^{M s} ds x],
     [  0,   0]]                  [     0,                     1]]

so a generator with migration switched off (stationary states, singular M) needs no deletion and no inverse; the last,
infinite interval is -M^-1 x (with two populations and mu0 + mu1 = 0 there is no such integral: InfiniteCoalescence).

Input: an ``oracle.misti_oracle.OracleModel`` built with ``trueEPS=True`` on which ``map_parameters`` and ``correct_lambdas``
have run, so that ``lc`` holds the rates the spectrum is taken with.  Its ``numT``, ``splitT`` (a fractional split's interval
already inserted), ``sampleDate``, ``mi``, ``pu``, ``lc`` and ``times`` are read; doubles are taken at their exact values, and an
mpf in their place as it is (tests/golden/make_curvature_exact.py differentiates the spectrum with steps no double can hold).
"""
import mpmath as mp

from oracle.misti_oracle import ONE_POP, TWO_POP

DPS = 50


class InfiniteCoalescence(ValueError):
    """Two populations in the last interval without migration (:475-476): no finite spectrum."""


def _generator_two(la, mu):
    # the two-population generator from its four rate patterns (column = source state)
    A, B = TWO_POP.A, TWO_POP.B
    N = TWO_POP.N
    M = mp.matrix(N, N)
    for i in range(N):
        for j in range(N):
            v = la[0] * int(A[0][i, j]) + la[1] * int(A[1][i, j]) + mu[0] * int(B[0][i, j]) + mu[1] * int(B[1][i, j])
            if v:
                M[i, j] = v
    return M


def _generator_one(la):
    M = mp.matrix(ONE_POP.N, ONE_POP.N)
    for i in range(ONE_POP.N):
        for j in range(ONE_POP.N):
            if ONE_POP.A[i, j]:
                M[i, j] = la * int(ONE_POP.A[i, j])
    return M


def _pulse(x, r, pop1):
    out = mp.matrix(TWO_POP.N, 1)
    for dst, src, ns, nm in TWO_POP.pulse[pop1]:
        out[dst] += (1 - r) ** ns * r ** nm * x[src]
    return out


def _ancient(x):
    out = mp.matrix(TWO_POP.N, 1)
    for i in range(TWO_POP.N):
        for j in range(TWO_POP.N):
            if TWO_POP.ancient[i, j]:
                out[i] += int(TWO_POP.ancient[i, j]) * x[j]
    return out


def interval(M, x, T):
    """(e^{M T} x, int_0^T e^{M s} x ds) from one exponential of the augmented matrix; T = None: the infinite interval."""
    n = M.rows
    if T is None:
        return mp.matrix(n, 1), -mp.lu_solve(M, x)
    A = mp.matrix(n + 1, n + 1)
    for i in range(n):
        for j in range(n):
            A[i, j] = M[i, j] * T
        A[i, n] = x[i] * T
    E = mp.expm(A)
    P1 = mp.matrix(n, 1)
    integ = mp.matrix(n, 1)
    for i in range(n):
        P1[i] = mp.fsum(E[i, j] * x[j] for j in range(n))
        integ[i] = E[i, n]
    return P1, integ


def raw_spectrum(om, dps=DPS, interval=interval):
    """The seven unnormalised classes of the expected spectrum (mpf), JAFSpectrum :467-506.  `interval`: a stand-in for the
    function of that name (a generator that meets the same interval many times passes a memoising one)."""
    with mp.workdps(dps):
        f = lambda v: v if isinstance(v, mp.mpf) else mp.mpf(float(v))    # an mpf passes as it is (make_curvature_exact.py)
        N = TWO_POP.N
        split, numT, sd = om.splitT, om.numT, om.sampleDate
        x = mp.matrix(N, 1)
        x[2] = 1
        jafs = [mp.mpf(0)] * 7
        for it in range(numT):
            two = it < split
            if two:
                mu = [f(om.mi[it][0]), f(om.mi[it][1])]
                if it == numT - 1 and mu[0] + mu[1] == 0:
                    raise InfiniteCoalescence("two populations in the last interval without migration")
            if it == sd:
                x = _ancient(x)
            pr = f(om.pu[it][0]) + f(om.pu[it][1])
            if two and pr > 0:
                x = _pulse(x, pr, 0 if om.pu[it][0] > 0 else 1)
            if it == split:
                c = mp.matrix(ONE_POP.N, 1)
                for k, (a, b) in enumerate(TWO_POP.collapse):
                    c[k] = mp.fsum(x[i] for i in range(a, b))
                x = c
            if two:
                M = _generator_two([f(om.lc[it][0]), f(om.lc[it][1])], mu)
                w = TWO_POP.jaf
            else:
                M = _generator_one(f(om.lc[it][0]))
                w = ONE_POP.jaf
            T = f(om.times[it]) if it < numT - 1 else None
            x, integ = interval(M, x, T)
            for c in range(7 if it >= sd else 2):
                jafs[c] += mp.fsum(int(w[i, c]) * integ[i] for i in range(M.rows) if w[i, c])
        return jafs


def spectrum(om, dps=DPS, interval=interval):
    """The normalised spectrum (7 mpf), as JAFSLikelihood normalises it (:583-584)."""
    with mp.workdps(dps):
        raw = raw_spectrum(om, dps, interval)
        tot = mp.fsum(raw)
        return [v / tot for v in raw]


def oracle_model(model, split, params):
    """The OracleModel of one fixture candidate (tests/golden/golden_exact_spectrum.json): bands and pulses in the C-ABI form
    of misti_amd.engine.Engine - (pop 0/1, start, end, value, param), end == -1 meaning the candidate's split index, param >= 0
    selecting params[param] - resolved into fixed -mi / -pu options; true rates (trueEPS), the closed-form single-population
    rates after the split (cpfit); map_parameters and correct_lambdas have run."""
    from oracle.misti_oracle import OracleModel
    s = int(split) + (1 if split % 1 else 0)
    val = lambda v, p: float(params[p]) if p >= 0 else float(v)
    mi = [(pop + 1, start, s if end == -1 else end, val(v, p), 0) for pop, start, end, v, p in model["bands"]]
    pu = [(pop + 1, t, val(v, p), 0) for pop, t, v, p in model["pulses"]]
    om = OracleModel(model["times"], model["lh"], [0] * 8, split, mi, pu, trueEPS=True, cpfit=True,
                     unfolded=model["unfolded"], sampleDate=model["sample_date"])
    om.map_parameters([])
    try:
        ok = om.correct_lambdas()
    except ZeroDivisionError:
        # past S = 745 the weights of the last interval's mean (:372-376) underflow and the reference divides 0 by 0; with
        # equal rates the mean is that rate for any weights (the device forms the weights' ratio and gets it)
        l0, l1 = om.lh[-1]
        if l0 != l1:
            raise
        om.lc[-1] = [l0, l0]
        ok = True
    if not ok:
        raise ValueError("rate correction failed")
    return om


def device_q(om, t):
    """q = (largest exit rate) x (interval length) of two-population interval t, as twopop_interval forms it."""
    la0, la1 = om.lc[t]
    mu0, mu1 = om.mi[t]
    return om.times[t] * max(6 * la0 + 4 * mu0, 6 * la1 + 4 * mu1, 3 * la0 + 3 * mu0 + mu1, 3 * la1 + 3 * mu1 + mu0,
                             la0 + la1 + 2 * mu0 + 2 * mu1)


def llk(J, row, unfolded, dps=DPS):
    """Composite log-likelihood of one JSFS row of 8 (SetJAFS :217-227 and :600-609) at the spectrum J (mpf)."""
    with mp.workdps(dps):
        d = [mp.mpf(float(v)) for v in row[1:]]
        if unfolded:
            cnt, cls = d, list(J)
        else:
            cnt = [d[0] + d[6], d[1] + d[5], d[2] + d[4], d[3]]
            cls = [J[0] + J[6], J[1] + J[5], J[2] + J[4], J[3]]
        out = mp.loggamma(mp.fsum(d) + 1)
        for n, p in zip(cnt, cls):
            out -= mp.loggamma(n + 1)
            if n:
                out += n * mp.log(p)
        return out
