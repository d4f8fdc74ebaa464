#!/usr/bin/env python3
"""Generate tests/golden/golden_exact_spectrum.json: the expected spectrum of small models in 50-digit arithmetic.

    python tests/golden/make_exact_spectrum.py            # (re)write the fixture
    python tests/golden/make_exact_spectrum.py --check    # regenerate and compare with the committed fixture

Deterministic, CPU only, does not use the reference: the models are listed below and every value comes from
tests/exact_spectrum.py (the oracle supplies only the constant structure and, with trueEPS, the rates).  Plain data per
model: the C-ABI inputs of misti_amd.engine.Engine (times, lh, bands, pulses, n_param, sample_date, unfolded; always trueEPS
and cpfit), the JSFS rows, and per candidate its split time, parameter vector, the rates lc, the largest q of its
two-population intervals, the status the device reports, and the exact normalised spectrum and llk per row as 40-digit
strings (status "inf_coal": no finite spectrum).
Doubles are written by repr (round-trip exact).
"""
import argparse
import json
import math
import os
import sys
from concurrent.futures import ProcessPoolExecutor
from fractions import Fraction

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mpmath as mp                      # noqa: E402
import exact_spectrum as ex              # noqa: E402

OUT = os.path.join(HERE, "golden_exact_spectrum.json")
DIGITS = 40
Q_SWITCH = 96.0

ROWS = [[0, 9000, 4000, 6000, 3000, 700, 1500, 200],
        [0, 120, 45, 80, 33, 10, 21, 5],
        [0, 500, 0, 300, 0, 0, 90, 17]]                        # zero classes
ROWS9 = ROWS + [[0, 1e6, 3e5, 5e5, 2e5, 4e4, 1e5, 1e4],
                [0, 1, 0, 0, 0, 0, 0, 0],
                [0, 0, 7, 0, 3, 0, 0, 0],
                [0, 2500, 800, 0, 700, 90, 300, 0],
                [0, 40, 12, 25, 9, 3, 7, 1],
                [0, 0, 0, 0, 11, 0, 0, 0]]                     # 9 rows: the llk kernel instead of the inline epilogue


def _rd(x):
    return float(Fraction(x))              # correct rounding of an exact rational


def _q_both(la, mu0, mu1, T):
    """q as the device forms it, with and without contraction of the products into fused multiply-adds."""
    F = Fraction
    plain = lambda a, b: _rd(F(_rd(F(a[0]) * F(a[1]))) + F(_rd(F(b[0]) * F(b[1]))))
    fused = lambda a, b: _rd(F(a[0]) * F(a[1]) + F(_rd(F(b[0]) * F(b[1]))))
    out = []
    for op in (plain, fused):
        r40 = op((6, la), (4, mu0))
        r04 = op((6, la), (4, mu1))
        r31 = _rd(F(op((3, la), (3, mu0))) + F(mu1))
        r13 = _rd(F(op((3, la), (3, mu1))) + F(mu0))
        r22 = _rd(F(_rd(F(_rd(F(la) + F(la))) + F(_rd(2 * F(mu0))))) + F(_rd(2 * F(mu1))))
        out.append(_rd(F(T) * F(max(r40, r04, r31, r13, r22))))
    return out


def hit_q(target, mu0, mu1):
    """(la, T) with la0 = la1 = la whose q is `target` to the bit however the device rounds."""
    base = (target - 4 * max(mu0, mu1)) / 6
    Ts = [1.0]
    for _ in range(8):
        Ts.append(math.nextafter(Ts[-1], 2.0))
    for T in Ts:
        la0 = base / T
        for s in (1, -1):
            la = la0
            for _ in range(64):
                if _q_both(la, mu0, mu1, T) == [target, target]:
                    return la, T
                la = math.nextafter(la, s * math.inf)
    raise RuntimeError("no exact q for %r" % target)


def model(name, regime, times, lh, bands, cands, pulses=(), n_param=0, sample_date=0, unfolded=False, rows=ROWS):
    return dict(name=name, regime=regime, times=[float(t) for t in times], lh=[[float(a), float(b)] for a, b in lh],
                bands=[list(b) for b in bands], pulses=[list(p) for p in pulses], n_param=n_param, sample_date=sample_date,
                unfolded=unfolded, rows=[[float(v) for v in r] for r in rows],
                candidates=[dict(split=float(s), params=[float(v) for v in p]) for s, p in cands])


MIG = [(0, 0, -1, 0.0, 0), (1, 0, -1, 0.0, 1)]                # both directions from the present to the split, rates as params 0, 1


def models():
    out = []
    # -- the switch between the series and the contour: one two-population interval, then two single-population ones
    mig = {"mu0": (0.0, 0.0), "oneway": (0.25, 0.0), "weak2way": (2.0 ** -6, 2.0 ** -6)}
    for q in (95.99, 96.0, math.nextafter(96.0, math.inf), 97.0, 150.0, 1e3, 1e5, 1e6):
        for tag, (m0, m1) in mig.items():
            la, T = hit_q(q, m0, m1)
            out.append(model("switch_q%r_%s" % (q, tag), "switch", [T, 0.5], [[la, la], [1.0, 1.25], [0.8, 0.8]], MIG,
                             [(1, (m0, m1))], n_param=2))
    # -- strong two-way migration (mu T >= 8) with ordinary rates
    for mu in (8.0, 12.0, 25.0, 100.0):
        out.append(model("strong_mu%g" % mu, "strong_migration", [1.0, 0.5], [[1.0, 1.0], [1.0, 1.0], [0.8, 0.8]], MIG,
                         [(1, (mu, mu)) for _ in range(1)], n_param=2))
        for la in (5.0, 20.0):
            out.append(model("strong_mu%g_la%g" % (mu, la), "strong_migration", [1.0, 0.5], [[la, la * 0.75], [1.0, 1.0], [0.8, 0.8]],
                             MIG, [(1, (mu, mu * 0.5))], n_param=2))
    # -- tiny q: an interval far shorter than every rate's scale
    for q in (1e-10, 1e-6, 1e-3):
        out.append(model("tiny_q%g" % q, "tiny_q", [q / 8, 0.7], [[1.0, 1.0], [1.0, 1.5], [0.9, 0.9]], MIG,
                         [(1, (0.5, 0.5)), (1, (0.0, 0.0))], n_param=2))
    # -- pulses, both directions, at interval 0 and at the last two-population interval; the strength is param 2
    for pop in (0, 1):
        for at in (0, 2):
            out.append(model("pulse_pop%d_at%d" % (pop, at), "pulse", [0.4, 0.7, 1.1, 0.9],
                             [[1.2, 0.8], [0.9, 1.1], [1.0, 1.0], [0.7, 0.7], [1.3, 1.3]], MIG,
                             [(3, (0.3, 0.1, pr)) for pr in (1e-12, 0.5, 1 - 1e-12, 1.0)],
                             pulses=[(pop, at, 0.0, 2)], n_param=3))
    # -- an ancient sample at interval 1 and at split - 1 (migration starts at the sample date)
    for sd in (1, 3):
        out.append(model("ancient_sd%d" % sd, "ancient_sample", [0.4, 0.7, 1.1, 0.9], [[1.2, 0.8], [0.9, 1.1], [1.0, 1.0], [0.7, 0.7], [1.3, 1.3]],
                         [(0, sd, -1, 0.0, 0), (1, sd, -1, 0.0, 1)], [(4, (0.3, 0.6)), (4, (0.0, 0.0))], n_param=2, sample_date=sd))
    # -- split times: integer and fractional, the first interval, numT - 1, numT (two populations in the infinite interval)
    out.append(model("splits", "split", [0.4, 0.7, 1.1, 0.9], [[1.2, 0.8], [0.9, 1.1], [1.0, 1.0], [0.7, 0.7], [1.3, 1.3]], MIG,
                     [(s, (0.4, 0.2)) for s in (1, 2, 2.25, 2.999, 4, 5)] + [(5, (0.0, 0.0)), (2.25, (0.0, 0.0))], n_param=2))
    # -- after the split: more than 64 and 128 intervals (the prefix sum over several wave chunks), e^-S below the double range,
    # an interval of 1e-12 (expm1)
    for n in (70, 140):
        times = [0.6, 0.9] + [0.05 + 0.01 * (i % 7) for i in range(n - 3)]
        lh = [[1.1, 0.9], [1.0, 1.2]] + [[0.5 + 0.1 * (i % 5), 0.5 + 0.1 * (i % 5)] for i in range(n - 2)]
        out.append(model("post_n%d" % n, "post_split", times, lh, MIG, [(2, (0.3, 0.2)), (1, (0.3, 0.2))], n_param=2))
    times = [0.6, 0.9, 1e-12, 0.5] + [2.0] * 100
    lh = [[1.1, 0.9], [1.0, 1.2], [3.0, 3.0], [1.0, 1.0]] + [[4.0, 4.0]] * 101
    out.append(model("post_deep", "post_split", times, lh, MIG, [(2, (0.3, 0.2))], n_param=2))
    # -- replicates: folded and unfolded, 9 rows (the test also evaluates the first 8)
    for unf in (False, True):
        out.append(model("rows_%s" % ("unfolded" if unf else "folded"), "replicates", [0.5, 0.8, 1.0], [[1.0, 1.4], [0.8, 0.6], [1.0, 1.0], [0.9, 0.9]],
                       MIG, [(2, (0.2, 0.5)), (1, (1.5, 0.0))], n_param=2, unfolded=unf, rows=ROWS9))
    return out


def _s(v):
    return mp.nstr(v, DIGITS, min_fixed=1, max_fixed=0)


def solve(job):
    m, ci = job
    c = m["candidates"][ci]
    om = ex.oracle_model(m, c["split"], c["params"])
    # the device's contract: two populations in the last interval (split == numT) is MISTI_INF_COAL even where migration makes
    # the reference's spectrum finite (include/misti_hip.h)
    out = dict(device_status="inf_coal" if om.splitT >= om.numT else "ok",
               lc=[[float(a), float(b)] for a, b in om.lc],
               q=max([ex.device_q(om, t) for t in range(min(om.splitT, om.numT - 1))] + [0.0]))
    try:
        J = ex.spectrum(om)
    except ex.InfiniteCoalescence:
        out["status"] = "inf_coal"
        return out
    with mp.workdps(ex.DPS):
        out["status"] = "ok"
        out["jafs"] = [_s(v) for v in J]
        out["llk"] = [_s(ex.llk(J, r, m["unfolded"])) for r in m["rows"]]
    return out


def generate(workers):
    ms = models()
    jobs = [(m, i) for m in ms for i in range(len(m["candidates"]))]
    with ProcessPoolExecutor(workers) as pool:
        res = list(pool.map(solve, jobs))
    for (m, i), r in zip(jobs, res):
        m["candidates"][i].update(r)
    return dict(dps=ex.DPS, digits=DIGITS, q_switch=Q_SWITCH, models=ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="regenerate and compare with the committed fixture")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    fx = generate(a.j)
    text = json.dumps(fx, indent=1) + "\n"
    if a.check:
        with open(OUT) as f:
            old = f.read()
        if old != text:
            print("golden_exact_spectrum.json differs from a fresh generation")
            return 1
        print("golden_exact_spectrum.json reproduced (%d models, %d candidates)"
              % (len(fx["models"]), sum(len(m["candidates"]) for m in fx["models"])))
        return 0
    with open(OUT, "w") as f:
        f.write(text)
    print("wrote", OUT, len(text), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
