#!/usr/bin/env python3
"""Generate tests/golden/golden_exact_forward.json.gz: the forward map (forward_kernel behind misti_forward_rates) in 50-digit
arithmetic (tests/exact_forward.py), regime by regime.

    python tests/golden/make_exact_forward.py            # (re)write the fixture
    python tests/golden/make_exact_forward.py --check    # regenerate, compare with the committed fixture, assert its coverage

Deterministic, CPU only, does not use the reference.  Every regime is a list of small models (numT 6 ... 12, two populations) for
misti_amd.engine.Engine(times, lh, bands, pulses, n_param, true_eps=True) with at most 65 candidates (split, params) each.  Per
candidate and setting of hold_mu ("0" / "1") the record holds the status by the header's rules and, per interval below the split:
the branch pair_expv takes there (pair_branches.branch of pair_branches.forward_interval), the interval's length T as the device
forms it, the exact x = -log(nc / before) of both genomes (the seen rate is x / T), ratio = the largest exact state over nc (the
factor of the bound), ln_nc = log(nc) (where the masses stand in the double range), the exact `pr` rows 0 ... n_eval, and the rows
of the `lh` output from n_eval on (the model's own rates, row numT as a fractional split leaves it).
Doubles are written by repr (round-trip exact); the file is a gzip stream without a time stamp, so a regeneration is the same bytes."""
import argparse
import gzip
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import mpmath as mp                      # noqa: E402
import exact_forward as xf               # noqa: E402
import pair_branches as pb               # noqa: E402

OUT = os.path.join(HERE, "golden_exact_forward.json.gz")
ONE_MINUS = 1.0 - 2.0 ** -53
FRACTIONS = (2.0 ** -20, 0.5, 1.0 - 2.0 ** -20)


def _sig(x, digits=7):
    return float("%.*e" % (digits - 1, float(x)))


# ---- one candidate at 50 digits ------------------------------------------------------------------------------------------
def exact_record(job):
    times, lh, bands, pulses, split, params, hold = job
    e = xf.exact_forward(times, lh, bands, pulses, split, params, hold_mu=bool(hold))
    rec = dict(status=e["status"])
    if e["status"] not in (xf.OK, xf.INF_COAL):
        return rec
    with mp.workdps(xf.DPS):
        n = e["n_eval"]
        rec.update(n_eval=n, T=e["T"], model_rows=e["model_rows"], branch=[], x=[], ratio=[], ln_nc=[])
        rec["pr"] = [[float(e["row0"][j & 1][j >> 1]) for j in range(6)]]
        for t in range(n):
            (l0, l1), (mu0, mu1) = e["lh"][t], e["mu"][t]
            a0, a1, b0, b1, q = pb.forward_interval(l0, l1, mu0, mu1, e["T"][t])
            rec["branch"].append(pb.branch(b0, b1, q))
            rec["x"].append([float(x) for x in e["x"][t]])
            rec["ratio"].append([_sig(max(abs(c) for c in e["v"][t][k]) / e["nc"][t][k]) for k in (0, 1)])
            rec["ln_nc"].append([_sig(mp.log(e["nc"][t][k])) for k in (0, 1)])
            rec["pr"].append([float(e["v"][t][j & 1][j >> 1]) for j in range(6)])
    return rec


# ---- the regimes -----------------------------------------------------------------------------------------------------------
def _two_way_bands():
    return [(0, 0, -1, 0.0, 0), (1, 0, -1, 0.0, 1)]            # both rates are parameters, up to the split


def _geometric(first, ratio, n):
    return [first * ratio ** t for t in range(n)]


def _model(name, times, lh, bands, pulses, n_param, cands, hold=(0,)):
    return dict(name=name, times=[float(t) for t in times], lh=[[float(a), float(b)] for a, b in lh], bands=[list(b) for b in bands],
                pulses=[list(p) for p in pulses], n_param=n_param, hold=list(hold),
                candidates=[dict(split=float(s), params=[float(v) for v in p], tags=list(tags)) for s, p, tags in cands])


def regime_branches():
    """One candidate walks from taylor0 to the closed forms over 11 intervals whose lengths grow geometrically; the scale of the
    migration rates shifts the walk.  65 candidates: the full wave and one more of the shape test."""
    numT = 12
    times = _geometric(2e-3, 2.6, numT - 1)
    lh = [[0.9 + 0.05 * (t % 3), 0.6 + 0.07 * (t % 4)] for t in range(numT)]
    cands = []
    for i in range(21):
        mu = 0.02 * 1.45 ** i                                  # 0.02 ... 34
        cands.append((numT - 1, (mu, 0.37 * mu), ("two_way",)))
        cands.append((numT - 1, (mu, 0.0), ("one_way_0",)))
        cands.append((numT - 1, (0.0, 0.8 * mu), ("one_way_1",)))
    cands += [(numT - 1, (0.0, 0.0), ("no_migration",)), (numT - 1, (1.0, 1.0), ("two_way",))]
    walk = _model("walk", times, lh, _two_way_bands(), [], 2, cands)
    # a runaway rate in the population that is left, so that the masses stay in the double range: rate x length 15 ... 2e5
    stiff = []
    for name, pop in (("stiff_0", 0), ("stiff_1", 1)):
        times = [0.5, 1.25, 1.0, 0.8, 0.4]
        big = [30.0, 1e3, 2e5, 4e4, 250.0]
        small = [0.7, 1.1, 0.4, 0.9, 1.3, 1.0]
        lh = [([b, s] if pop == 0 else [s, b]) for b, s in zip(big + [1.0], small)]
        cands = []
        for mu in (1e-3, 0.03, 0.4, 2.5):
            cands.append((5, (mu, 0.6 * mu), ("two_way",)))
            cands.append((5, (0.2 * mu, mu), ("two_way",)))
            cands.append((5, (mu, 0.0) if pop == 0 else (0.0, mu), ("one_way_%d" % pop,)))
        stiff.append(_model(name, times, lh, _two_way_bands(), [], 2, cands))
    return dict(name="branches", models=[walk] + stiff)


def regime_tiny():
    """Interval 0 (the chain's start: unit vectors), and intervals 2 and 3 (after an ordinary interval: mixed states) have rate x
    length of one decade, 1e-2 ... 1e-12; with and without migration."""
    models = []
    for d in range(2, 13):
        tiny = 10.0 ** -d
        times = [tiny, 0.9, tiny, 0.5 * tiny, 0.7]
        lh = [[1.0, 0.8], [0.9, 1.2], [1.0, 0.8], [1.6, 2.0], [1.1, 0.7], [1.0, 1.0]]
        cands = [(5, (0.0, 0.0), ("no_migration",)), (5, (0.7, 0.4), ("two_way",)), (5, (1.3, 0.0), ("one_way_0",)), (5, (0.0, 0.9), ("one_way_1",))]
        m = _model("tiny_1e-%02d" % d, times, lh, _two_way_bands(), [], 2, cands)
        m["decade"] = d
        models.append(m)
    return dict(name="tiny", models=models)


def regime_no_migration():
    """No band at all: the exact seen rate of genome k is the model's own rate of population k."""
    numT = 8
    times = [1e-6, 0.01, 0.3, 1.0, 2.5, 7.0, 20.0]
    lh = [[1.0, 2.0], [0.5, 0.3], [1.7, 0.9], [0.8, 1.5], [1.2, 0.25], [0.6, 0.9], [0.35, 0.45], [1.0, 1.0]]
    cands = [(s, (), ("no_migration",)) for s in range(1, numT + 1)] + [(2.5, (), ("no_migration",)), (6.25, (), ("no_migration",))]
    return dict(name="no_migration", models=[_model("no_bands", times, lh, [], [], 0, cands)])


def regime_decay():
    """Chains whose cumulated rate x length reaches 50, 300 and 700 within the double range, components hundreds of orders apart
    within one state, and two candidates past e^-745."""
    numT = 12
    shape = [0.6, 0.8, 1.0, 1.3, 0.7, 1.1, 0.9, 1.2, 1.0, 0.75, 1.15]                  # sums to 10.5
    models = []
    for name, total in (("decay_50", 50.25), ("decay_300", 301.5), ("decay_700", 703.5), ("decay_past_745", 808.5)):
        times = [total / 10.5 * s / 1.25 for s in shape]
        lh = [[1.25, 1.25]] * numT
        # without migration, and with migration out of one population only (the genome of the other stays where it is), the sum
        # of rate x length is `total` for a genome; with migration both ways a genome's pair spends time apart and decays less
        cands = [(numT - 1, (0.0, 0.0), ("no_migration", "full_decay")), (numT - 1, (0.3, 0.0), ("one_way_0", "full_decay")),
                 (numT - 1, (0.0, 0.02), ("one_way_1", "full_decay")), (numT - 1, (40.0, 25.0), ("two_way",)), (numT - 1, (0.2, 0.1), ("two_way",))]
        if name == "decay_past_745":
            cands = cands[:2]
        models.append(_model(name, times, lh, _two_way_bands(), [], 2, cands))
    times = [65.0 * s / 1.0 for s in shape]
    lh = [[1.0, 0.004 + 0.001 * (t % 3)] for t in range(numT)]
    cands = [(numT - 1, (1e-3, 1e-3), ("two_way", "skew")), (numT - 1, (1e-2, 0.0), ("one_way_0", "skew")), (numT - 1, (0.0, 1e-2), ("one_way_1", "skew")),
             (numT - 1, (0.0, 0.0), ("no_migration", "skew"))]
    models.append(_model("decay_skew", times, lh, _two_way_bands(), [], 2, cands))
    return dict(name="decay", models=models)


def regime_pulses():
    """Pulses at intervals 0, 2, 3 and 5 (the last before the split at 6), each with its own parameter: a candidate switches them on
    with the rates 1e-12, 0.5 and 1 - 2^-53 (0: no pulse); out of population 0, out of population 1, and alternating."""
    numT = 8
    times = [0.1, 0.25, 0.4, 0.3, 0.6, 0.8, 1.0]
    lh = [[1.0, 1.4], [0.7, 0.9], [1.2, 0.8], [0.9, 1.1], [0.6, 1.3], [1.1, 0.7], [0.9, 0.9], [1.0, 1.0]]
    bands = [(0, 0, -1, 0.35, -1), (1, 0, -1, 0.15, -1)]
    models = []
    for name, pops in (("pulses_pop0", (0, 0, 0, 0)), ("pulses_pop1", (1, 1, 1, 1)), ("pulses_mixed", (1, 0, 1, 0))):
        pulses = [(pop, t, 0.0, i) for i, (pop, t) in enumerate(zip(pops, (0, 2, 3, 5)))]
        cands = [(6, (0.0, 0.0, 0.0, 0.0), ("rate_0",))]
        for r, tag in ((1e-12, "rate_1e-12"), (0.5, "rate_0.5"), (ONE_MINUS, "rate_1-2^-53")):
            cands.append((6, (r, 0.0, 0.0, 0.0), (tag, "first_interval")))
            cands.append((6, (0.0, 0.0, 0.0, r), (tag, "last_before_split")))
            cands.append((6, (0.0, r, r, 0.0), (tag, "consecutive")))
        cands.append((6, (0.5, 1e-12, ONE_MINUS, 0.25), ("all_four",)))
        models.append(_model(name, times, lh, bands, pulses, 4, cands))
    return dict(name="pulses", models=models)


HOLD_TIMES = [0.2, 0.35, 0.5, 0.3, 0.7, 0.45, 0.9]
HOLD_LH = [[1.0, 1.3], [0.8, 0.6], [1.1, 0.9], [0.7, 1.2], [1.4, 0.8], [0.9, 1.0], [0.6, 0.75], [1.0, 1.0]]


def _hold_bands(last_end):
    return [(0, 0, 2, 0.3, -1), (0, 2, 4, 0.8, -1), (0, 4, last_end, 0.15, -1), (1, 0, 3, 0.5, -1), (1, 3, 5, 0.05, -1), (1, 5, last_end, 1.1, -1)]


def regime_hold_mu():
    """Three bands of different rates in each direction, splits at every boundary 1 ... numT, hold_mu 0 and 1.  `fixed_ends`: every
    split is a valid structure.  `end_at_split`: the last band of each direction ends at the split (end == -1), which SetModel's rule
    start < end refuses for the splits at or below its start - those candidates carry the status.  `constant`: one rate per
    direction up to the split, where hold_mu = 1 is hold_mu = 0 bit for bit."""
    numT = 8
    splits = [(s, (), ("split_%d" % s,)) for s in range(1, numT + 1)]
    return dict(name="hold_mu", models=[
        _model("fixed_ends", HOLD_TIMES, HOLD_LH, _hold_bands(numT), [], 0, splits, hold=(0, 1)),
        _model("end_at_split", HOLD_TIMES, HOLD_LH, _hold_bands(-1), [], 0, splits, hold=(0, 1)),
        _model("constant", HOLD_TIMES, HOLD_LH, [(0, 0, -1, 0.4, -1), (1, 0, -1, 0.25, -1)], [], 0, splits, hold=(0, 1))])


def regime_fractional():
    """Fractions 2^-20, 0.5 and 1 - 2^-20 of the first interval, a middle one and the last that has a length; the bands are indices
    on the candidate's grid (one interval more), hold_mu 0 and 1."""
    numT = 8
    cands = [(s + f, (), ("interval_%d" % s, "fraction_%d" % i)) for s in (0, 3, numT - 2) for i, f in enumerate(FRACTIONS)]
    return dict(name="fractional", models=[_model("fractional", HOLD_TIMES, HOLD_LH, _hold_bands(numT + 1), [], 0, cands, hold=(0, 1))])


def regime_statuses():
    numT = 8
    cands = [(0.0, (0.3,), ("split_0",)), (5.0, (0.3,), ("ok",)), (5.0, (-0.1,), ("negative_parameter",)), (-1.0, (0.3,), ("split_below_0",)),
             (float(numT + 1), (0.3,), ("split_above_numT",)), (float(numT), (0.3,), ("split_at_numT",)), (numT - 0.5, (0.3,), ("fraction_of_the_last",)),
             (0.5, (0.3,), ("fraction_before_the_band",))]
    return dict(name="statuses", models=[_model("statuses", HOLD_TIMES, HOLD_LH, [(0, 1, 5, 0.3, 0)], [], 1, cands, hold=(0, 1))])


def regimes():
    return [regime_branches(), regime_tiny(), regime_no_migration(), regime_decay(), regime_pulses(), regime_hold_mu(), regime_fractional(),
            regime_statuses()]


# ---- drivers ---------------------------------------------------------------------------------------------------------------------
def generate(workers):
    regs = regimes()
    jobs, slots = [], []
    for r in regs:
        for m in r["models"]:
            for c in m["candidates"]:
                c["exact"] = {}
                for h in m["hold"]:
                    jobs.append((m["times"], m["lh"], m["bands"], m["pulses"], c["split"], c["params"], h))
                    slots.append((c, str(h)))
    with ProcessPoolExecutor(workers) as pool:
        for (c, h), rec in zip(slots, pool.map(exact_record, jobs, chunksize=4)):
            c["exact"][h] = rec
    fx = dict(dps=xf.DPS, w_bound=pb.W_BOUND, regimes=regs)
    return fx, pb.coverage_exact_forward(fx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="regenerate, compare with the committed fixture and assert its coverage")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    fx, counts = generate(a.j)
    text = json.dumps(fx, indent=None, separators=(",", ":")) + "\n"
    rc = 0
    if a.check:
        with gzip.open(OUT, "rt") as f:
            same = f.read() == text
        print(os.path.basename(OUT), "reproduced" if same else "differs from a fresh generation")
        rc = int(not same)
    else:
        with open(OUT, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
            f.write(text.encode())
        print("wrote", OUT, os.path.getsize(OUT), "bytes (%d of JSON)" % len(text))
    print(json.dumps(counts))
    return rc


if __name__ == "__main__":
    sys.exit(main())
