#!/usr/bin/env python3
"""Generate ``golden_pulse_sweep.json`` by RUNNING THE REFERENCE: the GNU-parallel recipe with a pulse in the place of a band,

    parallel ./MiSTI.py g1.psmc g2.psmc sim.jafs {st} -uf -mi 1 4 {st} 0.2 0 -pu 1 10 0.05 0 -pu 2 {t} {f} 0 ::: st 20 20.5 ::: t ... ::: f ...

one reference run per (fit, st, t, f) grid point.  Runs only where the reference is installed (it never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_pulse_sweep.py            # writes the fixture
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_pulse_sweep.py --check    # the conditions on the fixture, from the file alone

The case-running and perturbation helpers are make_golden.py's (``case``: the reference's values and its own spread under the 2^-48
input perturbations, 3 or 9 kinds); the one-ulp-in-expm runs are internal_noise.py's, stored in the record itself
(``internal_spread``, ``internal_fail``, ``internal_runs``, ``internal_llh``).  Records are those of golden_sweep.json, with a
``sweep`` entry naming st, the pulse times and the fractions.

The grid: numT = 32 (``misti_amd.synth``), one fixed band ending at the split, one fixed pulse at interval 10 - a time the sweep
never takes - and the swept pulse ``-pu 2 {t} {f} 0`` with t in 3, 7, 12, 16, 20 and f in 0.1, 0.35, at the integer split 20 and the
fractional split 20.5, under --cpfit and the default fit: 40 cases.  t = 20 is the shortened interval of the fractional split
(applied) and the split index of the integer one (valid, never applied: the reference's loops run over t < splitT).

The conditions (``--check``; chosen so that the reference alone meets them, before any device result exists): at least 24 cases with
a finite llh, at least 8 per fit."""
import json
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden_pulse_sweep.json")
TIMES = (3, 7, 12, 16, 20)
FRACTIONS = (0.1, 0.35)
SPLITS = (20, 20.5)
FIXED_PULSE = [1, 10, 0.05, 0]
MIN_FINITE, MIN_FINITE_PER_FIT = 24, 8


def cases():
    import make_golden as mg                     # the reference, synth, parity: its imports
    import internal_noise as noise
    inp = mg.synth.psmc_pair(16, 17)
    st0 = 20
    true_mi = [[1, 4, st0, 0.2, 0]]
    true_pu = [FIXED_PULSE, [2, 12, 0.1, 0]]
    t32, lh32, _ = mg.synth.self_consistent(inp, st0, true_mi, true_pu)
    truth = mg.case("tmp", t32, lh32, [1] * 8, st0, true_mi, true_pu, trueEPS=True, cpfit=True, unfolded=True)
    sfs = mg.synth.counts_from_spectrum(truth["out"]["JAFS"])
    out = []
    for cp in (True, False):
        for st in SPLITS:
            end = int(st) + (1 if st % 1 else 0)
            for t in TIMES:
                for fi, f in enumerate(FRACTIONS):
                    mi = [[1, 4, end, 0.2, 0]]
                    pu = [list(FIXED_PULSE), [2, t, f, 0]]
                    kw = dict(smooth=True, unfolded=True)
                    if cp:
                        kw["cpfit"] = True
                    c = mg.case("pu_%s_st%g_t%d_f%d" % ("cp" if cp else "df", st, t, fi), t32, lh32, sfs, st, mi, pu, **kw)
                    c["out"].pop("Pr", None)
                    c["sweep"] = {"st": st, "pulse_times": [FIXED_PULSE[1], t], "fractions": [FIXED_PULSE[2], f]}
                    o = c["out"]
                    if o["llh"] is not None:
                        with warnings.catch_warnings():
                            warnings.simplefilter("ignore")
                            vals = [noise.run(c["in"], noise.NoisyLinalg(7000 + s)) for s in range(noise.RUNS)]
                        fin = [v for v in vals if v is not None]
                        o["internal_spread"] = max(abs(v - o["llh"]) / abs(o["llh"]) for v in fin) if fin else None
                        o["internal_fail"], o["internal_runs"], o["internal_llh"] = noise.RUNS - len(fin), noise.RUNS, vals
                    out.append(c)
    return out, mg.dedupe(out)


def check(d):
    """The conditions on the fixture, from its records alone."""
    finite = [c for c in d["cases"] if c["out"]["llh"] is not None]
    per_fit = {fit: sum(1 for c in finite if bool(c["in"]["kw"].get("cpfit")) == fit) for fit in (True, False)}
    assert len(finite) >= MIN_FINITE, "%d cases with a finite llh, %d needed" % (len(finite), MIN_FINITE)
    assert min(per_fit.values()) >= MIN_FINITE_PER_FIT, "finite cases per fit %r, %d needed" % (per_fit, MIN_FINITE_PER_FIT)
    for c in finite:
        o = c["out"]
        assert len(o["pert_llh"]) in (3, 9) and o["internal_runs"] == len(o["internal_llh"]) > 0, c["name"]
        assert c["sweep"]["pulse_times"] == [int(p[1]) for p in c["in"]["pu"]], c["name"]
    assert os.path.getsize(PATH) <= 200 * 1024, "the fixture is larger than the other sweep fixtures"
    return len(d["cases"]), len(finite), per_fit


def main():
    if "--check" not in sys.argv:
        sys.path.insert(0, HERE)
        cs, grids = cases()
        json.dump({"generator": "tests/golden/make_pulse_sweep.py", "scipy": "1.15.3", "numpy": "2.2.6", "grids": grids, "cases": cs}, open(PATH, "w"))
    n, n_fin, per_fit = check(json.load(open(PATH)))
    print("%d cases, %d with a finite llh (--cpfit %d, default fit %d): the fixture's conditions hold" % (n, n_fin, per_fit[True], per_fit[False]))


if __name__ == "__main__":
    main()
