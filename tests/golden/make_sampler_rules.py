#!/usr/bin/env python3
"""Generate tests/golden/golden_sampler_rules.json.gz: every array the four public sampler rules of misti_amd.optimize return
(ensemble_rule, ensemble_prior_rule, tempered_rule, tempered_prior_rule) on a handful of small seeded cases, to the bit.

    python tests/golden/make_sampler_rules.py            # (re)write the fixture
    python tests/golden/make_sampler_rules.py --check    # regenerate, compare with the committed fixture, assert its coverage

Deterministic, CPU only, the project's own code and nothing of the reference.  The rules are the oracle the device samplers are held
to (tests/test_gpu_ens.py, test_gpu_pt.py, test_gpu_prior.py); this fixture holds the oracle itself from outside, so that a rewrite of
the rules cannot move their bits unseen.  The objectives are built from + - *, comparisons and numpy.where only - as the rules' own
arithmetic is (optimize.ens_exp) -, so no libm stands behind a bit.  A float array is stored as the 64-bit patterns of its elements
(-inf and NaN survive), an integer array as it is; the file is a gzip stream without a time stamp, so a regeneration is the same
bytes.  tests/test_sampler_rules_cpu.py runs cases() again and compares."""
import argparse
import gzip
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "golden_sampler_rules.json.gz")
RULES = ("ensemble_rule", "ensemble_prior_rule", "tempered_rule", "tempered_prior_rule")


# ---- objectives: f = -llk of M points X[M][N], point m belonging to search s[m] ------------------------------------------------------
def bowl(X, s):
    """0.5 |x|^2, shifted per search: the coordinates added in increasing order."""
    X, s = np.asarray(X, dtype=np.float64), np.asarray(s, dtype=np.float64)
    f = 0.125 * s
    for k in range(X.shape[1]):
        f = f + 0.5 * (X[:, k] * X[:, k])
    return f


def holes(X, s):
    """bowl with a region that has no value (+inf: coordinate 0 above 0.75) and one that returns NaN (coordinate 0 below -0.75)."""
    X = np.asarray(X, dtype=np.float64)
    return np.where(X[:, 0] > 0.75, np.inf, np.where(X[:, 0] < -0.75, np.nan, bowl(X, s)))


def start(shape, lo, hi, seed):
    """Walkers [S]...[W][N] inside their boxes lo / hi [S][N]: a fixed coordinate (lo == hi) at lo exactly."""
    S, N = shape[0], shape[-1]
    lo, hi = np.broadcast_to(np.asarray(lo, dtype=float), (S, N)), np.broadcast_to(np.asarray(hi, dtype=float), (S, N))
    u = np.random.Generator(np.random.Philox(seed)).random(shape)
    ix = (slice(None),) + (None,) * (len(shape) - 2)
    return np.minimum(lo[ix] + u * (hi - lo)[ix], hi[ix])


BOX3 = (np.array([[-3.0, -2.0, 0.25], [-1.0, 0.5, -4.0], [-2.0, -2.0, -2.0]]),      # a box per search; search 1 holds coordinate 1 fixed
        np.array([[3.0, 2.0, 1.5], [2.0, 0.5, 4.0], [2.0, 2.0, 2.0]]))
IDS3 = [7, 2, 40]
PRIOR3 = dict(scale=np.array([1, 0, 0], dtype=np.int32), kind=np.array([0, 1, 2], dtype=np.int32),      # log | normal | exponential
              p0=np.array([0.0, 0.25, 0.5]), p1=np.array([0.0, 0.75, 0.0]))
PRIOR_PER = dict(scale=np.array([[1, 0, 0], [0, 0, 1], [0, 0, 0]], dtype=np.int32), kind=np.array([[0, 1, 2], [2, 0, 1], [1, 0, 0]], dtype=np.int32),
                 p0=np.array([[0.0, 0.25, 0.5], [1.5, 0.0, -0.5], [0.5, 0.0, 0.0]]), p1=np.array([[0.0, 0.75, 0.0], [0.0, 0.0, 1.25], [2.0, 0.0, 0.0]]))
PRIOR_FLAT = dict(scale=np.zeros(2, dtype=np.int32), kind=np.zeros(2, dtype=np.int32), p0=np.zeros(2), p1=np.zeros(2))
BOX2 = (np.array([-1.0, -1.5]), np.array([1.0, 1.5]))
BOX1 = (np.array([-1.0]), np.array([1.0]))


def plain(name, fun, shape, box, n_step, prior=False, **kw):
    args = dict(init=start(shape, box[0], box[1], len(name)), lo=box[0], hi=box[1], n_step=n_step, **kw)
    if prior is not False:
        args["prior"] = prior
    return dict(name=name, rule="ensemble_rule" if prior is False else "ensemble_prior_rule", fun=fun, args=args)


def tempered(name, fun, shape, box, ladder, n_step, prior=False, **kw):
    args = dict(init=start(shape, box[0], box[1], len(name)), lo=box[0], hi=box[1], ladder=np.asarray(ladder, dtype=float), n_step=n_step, **kw)
    if prior is not False:
        args["prior"] = prior
    return dict(name=name, rule="tempered_rule" if prior is False else "tempered_prior_rule", fun=fun, args=args)


def cases():
    """The cases: dict(name, rule, fun, args); `args` are the rule's keyword arguments behind fun_batch."""
    return [
        plain("ids_boxes_temperatures", holes, (3, 6, 3), BOX3, 7, thin=2, temperature=np.array([1.5, 0.75, 3.0]), seed=11, ids=IDS3),
        plain("wide_stretch_leaves_the_box", bowl, (2, 4, 1), BOX1, 5, a=6.0, seed=3),
        plain("two_coordinates", holes, (2, 4, 2), BOX2, 4, thin=3, temperature=0.5, seed=5, ids=[9, 1]),
        plain("no_step", bowl, (2, 4, 2), BOX2, 0, seed=1),
        plain("no_search", bowl, (0, 4, 2), BOX2, 1, seed=1),
        plain("prior_for_all", bowl, (2, 6, 3), (BOX3[0][0], BOX3[1][0]), 6, prior=PRIOR3, thin=4, temperature=np.array([1.0, 2.5]), seed=13),
        plain("prior_per_search", holes, (3, 4, 3), BOX3, 5, prior=PRIOR_PER, thin=2, seed=17, ids=IDS3),
        plain("prior_that_says_nothing", bowl, (2, 4, 2), BOX2, 4, prior=PRIOR_FLAT, seed=19),
        tempered("one_rung_per_fit", holes, (3, 1, 6, 3), BOX3, [[1.5], [0.75], [3.0]], 7, thin=2, swap_every=1, burn=1, seed=11, ids=IDS3),
        tempered("two_rungs_for_all", bowl, (2, 2, 4, 1), BOX1, [1.0, 4.0], 6, swap_every=2, a=6.0, seed=23),
        tempered("three_rungs_per_fit", holes, (3, 3, 4, 3), BOX3, [[1.0, 3.0, 9.0], [0.5, 1.0, 6.0], [2.0, 2.5, 40.0]], 7, thin=2, swap_every=1, burn=2,
                 seed=29, ids=IDS3),
        tempered("four_rungs_no_swaps", bowl, (2, 4, 4, 2), BOX2, [1.0, 2.0, 8.0, 64.0], 5, thin=2, swap_every=0, seed=31),
        tempered("four_rungs_swaps", holes, (1, 4, 6, 2), BOX2, [[0.5, 2.0, 8.0, 32.0]], 6, thin=1, swap_every=1, burn=3, seed=37, ids=[5]),
        tempered("no_step", bowl, (2, 2, 4, 2), BOX2, [1.0, 2.0], 0, burn=4, seed=1),
        tempered("no_fit", bowl, (0, 2, 4, 2), BOX2, [1.0, 2.0], 1, seed=1),
        tempered("prior_for_all", bowl, (2, 3, 4, 3), (BOX3[0][0], BOX3[1][0]), [1.0, 4.0, 16.0], 6, prior=PRIOR3, thin=4, swap_every=1, seed=41),
        tempered("prior_per_fit", holes, (3, 2, 6, 3), BOX3, [[1.0, 3.0], [0.5, 1.0], [2.0, 2.5]], 5, prior=PRIOR_PER, thin=2, swap_every=2, burn=1,
                 seed=43, ids=IDS3),
        tempered("prior_that_says_nothing", bowl, (2, 2, 4, 2), BOX2, [1.0, 3.0], 4, prior=PRIOR_FLAT, seed=47),
        tempered("one_rung_with_a_prior", bowl, (2, 1, 6, 3), (BOX3[0][0], BOX3[1][0]), [[1.0], [2.5]], 6, prior=PRIOR3, thin=4, swap_every=0, seed=13),
    ]


def run(case):
    """The case through its rule: (the rule's dict, what the objective returned on the way: dict(inf, nan) counts)."""
    from misti_amd import optimize
    saw = dict(inf=0, nan=0)

    def fun(X, s):
        f = case["fun"](X, s)
        saw["inf"] += int(np.isposinf(f).sum())
        saw["nan"] += int(np.isnan(f).sum())
        return f

    return getattr(optimize, case["rule"])(fun, **case["args"]), saw


def proposals(case):
    """Proposals the case makes, inside their box or not: searches x rungs x walkers x steps."""
    return int(np.prod(case["args"]["init"].shape[:-1])) * int(case["args"]["n_step"])


def encode(v):
    if isinstance(v, (int, np.integer)):
        return int(v)
    v = np.ascontiguousarray(v)
    if v.dtype == np.float64:
        return dict(shape=list(v.shape), bits=v.reshape(-1).view(np.uint64).tolist())
    assert v.dtype == np.int32, v.dtype
    return dict(shape=list(v.shape), ints=v.reshape(-1).tolist())


def generate():
    out = []
    for case in cases():
        r, saw = run(case)
        out.append(dict(name=case["name"], rule=case["rule"], saw=saw, out={k: encode(v) for k, v in r.items()}))
    return dict(cases=out)


def coverage(fx):
    """What the fixture promises to reach, counted on the cases and their recorded results.  Returns the counts."""
    cs = {(c["rule"], c["name"]): c for c in cases()}
    assert [(c["rule"], c["name"]) for c in fx["cases"]] == list(cs) and {c["rule"] for c in fx["cases"]} == set(RULES)
    n = dict.fromkeys(("ids", "box_per_search", "fixed", "temperature_per_search", "inf", "nan", "outside", "no_step", "no_search", "burn",
                       "ladder_per_fit", "ladder_for_all", "prior_for_all", "prior_per_search", "prior_flat", "log", "normal", "exponential",
                       "thin_left_over", "parity0", "parity1"), 0)
    W, N, L, swaps = set(), set(), set(), set()
    for rec in fx["cases"]:
        c = cs[(rec["rule"], rec["name"])]
        a = c["args"]
        S, n_step, thin = a["init"].shape[0], a["n_step"], a.get("thin", 1)
        ids = a.get("ids")
        n["ids"] += S == 3 and ids is not None and sorted(ids) != list(range(min(ids), min(ids) + 3))
        n["box_per_search"] += np.ndim(a["lo"]) == 2
        n["fixed"] += bool((np.asarray(a["lo"]) == np.asarray(a["hi"])).any())
        n["temperature_per_search"] += np.ndim(a.get("temperature", 1.0)) == 1
        n["inf"] += rec["saw"]["inf"] > 0
        n["nan"] += rec["saw"]["nan"] > 0
        n["outside"] += S > 0 and n_step > 0 and rec["out"]["n_points"] < proposals(c)
        n["no_step"] += n_step == 0
        n["no_search"] += S == 0
        n["thin_left_over"] += n_step % thin != 0
        W.add(a["init"].shape[-2])
        N.add(a["init"].shape[-1])
        if "ladder" in a:
            L.add(a["init"].shape[1])
            n["ladder_per_fit" if a["ladder"].ndim == 2 else "ladder_for_all"] += 1
            swaps.add(a.get("swap_every", 1))
            n["burn"] += a.get("burn", 0) > 0 and n_step // thin > 0
            for t in range(1, n_step + 1):
                e = a.get("swap_every", 1)
                if e >= 1 and t % e == 0 and ((t // e - 1) & 1) + 1 < a["init"].shape[1]:
                    n["parity%d" % ((t // e - 1) & 1)] += 1
        p = a.get("prior")
        if p is not None:
            says = bool(np.any(p["scale"]) or np.any(p["kind"]))
            n["prior_flat"] += not says
            n["prior_for_all"] += says and p["scale"].ndim == 1
            n["prior_per_search"] += says and p["scale"].ndim == 2
            n["log"] += bool((p["scale"] == 1).any())
            n["normal"] += bool((p["kind"] == 1).any())
            n["exponential"] += bool((p["kind"] == 2).any())
    assert all(v >= 1 for v in n.values()), n
    assert {4, 6} <= W and {1, 2, 3} <= N and {1, 2, 3, 4} <= L and {0, 1, 2} <= swaps, (W, N, L, swaps)
    # the proposal outside its box, where it was arranged: a stretch scale of 6 in the box [-1, 1]
    wide = [r for r in fx["cases"] if r["name"] == "wide_stretch_leaves_the_box"][0]
    assert wide["out"]["n_points"] < proposals(cs[("ensemble_rule", wide["name"])]) and wide["saw"] == dict(inf=0, nan=0)
    return n


def dump(fx):
    import io
    buf = io.BytesIO()
    with gzip.GzipFile(fileobj=buf, mode="wb", mtime=0, filename="") as f:
        f.write(json.dumps(fx, separators=(",", ":")).encode())
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    fx = generate()
    print(json.dumps(coverage(fx)))
    if a.check:
        with gzip.open(OUT, "rt") as f:
            assert json.load(f) == fx, "the committed fixture differs from a regeneration"
        print("the committed fixture equals a regeneration")
        return
    with open(OUT, "wb") as f:
        f.write(dump(fx))
    print("wrote %s: %d cases, %d bytes" % (OUT, len(fx["cases"]), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
