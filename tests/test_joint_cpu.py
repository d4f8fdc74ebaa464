"""Joint credible regions of coordinate pairs without a GPU: the rule (optimize.ensemble_joint_rule - what the device result is compared
against, bit for bit, in tests/test_gpu_joint.py) against a restatement that loops over the samples and walks the sorted cells, against
numpy.histogram2d away from the bin edges, the corners of the rule, the helper joint_table, the refusals misti_ens_joint_dev makes
before it looks at a context (and that the older doors keep theirs), the header against the binding and the build lists, and the
parser's `--mcmc-joint`."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT

E_ARG, E_LIMIT = -1, -4
MASSES = (0.95, 0.5, 1.0, 1e-9)
NAN, INF = float("nan"), float("inf")


def lib():
    from misti_amd import _lib
    return _lib.load()


def chain_of(xa, xb):
    """Two columns of samples as a chain [1][m][1][2]."""
    return np.stack([np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64)], axis=-1)[None, :, None, :]


def rule(xa, xb, bins, rng=None, masses=MASSES):
    from misti_amd.optimize import ensemble_joint_rule
    return ensemble_joint_rule(chain_of(xa, xb)[0], [(0, 1)], bins=bins, range=rng, masses=masses)


def brute_bin(x, lo, hi, B):
    """The bin of an inside sample by the letter, on Python floats (IEEE doubles, one rounding per operation)."""
    d = hi - lo
    scale = float(B) / d if d != 0.0 else (INF if not math.isnan(d) else NAN)
    t = (x - lo) * scale
    if not t >= 0.0:
        return 0
    if t >= float(B):
        return B - 1
    return int(t)


def brute(xa, xb, Ba, Bb, window, masses):
    """The rule by the letter: a loop over the samples; the cells sorted by count descending and the cumulative sum walked until it
    holds k samples - the count reached there is the level, and every cell of that count belongs to the region."""
    (lo_a, hi_a), (lo_b, hi_b) = window
    cnt = [[0] * Bb for _ in range(Ba)]
    for x, y in zip(xa, xb):
        x, y = float(x), float(y)
        if lo_a <= x and x <= hi_a and lo_b <= y and y <= hi_b:
            cnt[brute_bin(x, lo_a, hi_a, Ba)][brute_bin(y, lo_b, hi_b, Bb)] += 1
    inside = sum(map(sum, cnt))
    mode = (-1, -1)
    for ia in range(Ba):
        for ib in range(Bb):
            if cnt[ia][ib] > (cnt[mode[0]][mode[1]] if mode[0] >= 0 else 0):
                mode = (ia, ib)
    regions = []
    flat = sorted((c for row in cnt for c in row if c > 0), reverse=True)
    for p in masses:
        if not inside:
            regions.append((0, 0, 0))
            continue
        k = 1
        while float(k) < float(inside) * p:
            k += 1
        k = min(max(k, 1), inside)
        total = 0
        for c in flat:
            total += c
            if total >= k:
                level = c
                break
        regions.append((level, sum(1 for c in flat if c >= level), sum(c for c in flat if c >= level)))
    return cnt, inside, mode, regions


def agree(xa, xb, bins, rng=None, masses=MASSES):
    """rule() against brute() on one pair; returns the rule's result."""
    r = rule(xa, xb, bins, rng, masses)
    Ba, Bb = (bins, bins) if np.isscalar(bins) else bins
    cnt, inside, mode, regions = brute(xa, xb, Ba, Bb, r["range"][0].tolist(), masses)
    from misti_amd.optimize import joint_counts
    assert joint_counts(r, 0).tolist() == cnt
    assert r["counts"].dtype == np.int32 and r["inside"][0] == inside and r["outside"][0] == len(xa) - inside
    assert tuple(r["mode"][0]) == mode
    assert [(int(r["level"][0, i]), int(r["cells"][0, i]), int(r["held"][0, i])) for i in range(len(masses))] == regions
    return r


def test_rule_against_the_walk_and_histogram2d():
    rng = np.random.default_rng(20261021)
    xa, xb = rng.normal(0.3, 1.0, 4000), rng.normal(-1.0, 0.5, 4000)
    window = [(-1.5, 2.0), (-2.0, 0.25)]
    for Ba, Bb in ((7, 5), (32, 32), (128, 3)):
        edges = [np.linspace(lo, hi, B + 1) for (lo, hi), B in zip(window, (Ba, Bb))]
        for v, e in zip((xa, xb), edges):                      # no sample within an ulp of an interior edge: there the two may differ
            gap = np.abs(v[:, None] - e[None, 1:-1]) if e.size > 2 else np.ones((1, 1))
            assert (gap > np.spacing(np.abs(e[None, 1:-1]) if e.size > 2 else 1.0)).all()
        r = agree(xa, xb, (Ba, Bb), window)
        from misti_amd.optimize import joint_counts
        h, _, _ = np.histogram2d(xa, xb, bins=[Ba, Bb], range=window)
        assert joint_counts(r, 0).tolist() == h.astype(np.int64).tolist()
        assert 0 < r["inside"][0] < 4000                         # the window leaves samples outside
    r = agree(xa, xb, (9, 11))                                  # the ranges taken from the data: everything finite is inside
    assert r["inside"][0] == 4000 and r["range"][0].tolist() == [[xa.min(), xa.max()], [xb.min(), xb.max()]]


def test_several_searches_pairs_and_burn():
    from misti_amd.optimize import ensemble_joint_rule, joint_counts
    rng = np.random.default_rng(3)
    x = rng.standard_normal((3, 12, 4, 3))
    r = ensemble_joint_rule(x, [(0, 1), (2, 0)], bins=[(4, 5), (3, 2)], burn=2, masses=(0.9,))
    assert r["counts"].shape == (3, 26) and r["offsets"].tolist() == [0, 20, 26] and r["range"].shape == (3, 2, 2, 2)
    for s in range(3):
        for q, (a, b) in enumerate(((0, 1), (2, 0))):
            one = ensemble_joint_rule(x[s, 2:], [(a, b)], bins=[(4, 5), (3, 2)][q], masses=(0.9,))
            assert joint_counts(r, q, s).tobytes() == joint_counts(one, 0).tobytes() and r["range"][s, q].tobytes() == one["range"][0].tobytes()
            assert (r["level"][s, q], r["cells"][s, q], r["held"][s, q]) == (one["level"][0], one["cells"][0], one["held"][0])
    whole, alone = r, ensemble_joint_rule(x[2:], [(0, 1), (2, 0)], bins=[(4, 5), (3, 2)], burn=2, masses=(0.9,))
    for k in ("counts", "range", "inside", "mode", "level", "cells", "held"):
        assert whole[k][2].tobytes() == alone[k][0].tobytes()
    for bad in (dict(pairs=[(0, 0)]), dict(pairs=[(0, 3)]), dict(pairs=[(-1, 0)]), dict(pairs=[(0, 1)], bins=0), dict(pairs=[(0, 1)], bins=129),
                dict(pairs=[(0, 1)], burn=12), dict(pairs=[(0, 1)], masses=(0.0,)), dict(pairs=[(0, 1)], masses=(NAN,)), dict(pairs=[(0, 1)] * 121)):
        with pytest.raises(ValueError):
            ensemble_joint_rule(x, **bad)


def test_corners_of_the_bin():
    # hi == lo on one axis: 0 inf is NaN, bin 0
    r = agree([1.0, 1.0, 2.0], [0.0, 1.0, 0.5], (4, 4), [(1.0, 1.0), (0.0, 1.0)])
    assert r["inside"][0] == 2 and r["counts"].reshape(4, 4)[0].tolist() == [1, 0, 0, 1]
    # x == lo lands in bin 0, x == hi in the last
    r = agree([-0.3, 1.7], [1.7, -0.3], (3, 128), [(-0.3, 1.7), (-0.3, 1.7)])
    assert r["counts"].reshape(3, 128)[0, 127] == 1 and r["counts"].reshape(3, 128)[2, 0] == 1
    # either side of an interior edge: the index is monotone and moves by one at most
    for B in (3, 128):
        for lo, hi in ((0.0, 1.0), (-0.3, 1.7)):
            for i in range(1, B):
                e = lo + i * (hi - lo) / B
                xs = [np.nextafter(e, -INF), e, np.nextafter(e, INF)]
                got = [brute_bin(float(x), lo, hi, B) for x in xs]
                assert got == sorted(got) and got[0] >= i - 1 and got[2] <= i, (B, i, got)
                if B == 128 and (lo, hi) == (0.0, 1.0):        # powers of two: everything is exact
                    assert got == [i - 1, i, i]
                r = rule(xs, [0.5] * 3, (B, 1), [(lo, hi), (0.0, 1.0)], masses=())
                assert np.flatnonzero(r["counts"]).tolist() == sorted(set(got)), (B, i)


def test_corners_of_the_range():
    x, y = [0.0, 0.5, 1.0], [0.0, 0.5, 1.0]
    for window in ([(1.0, 0.0), (0.0, 1.0)], [(0.0, 1.0), (NAN, 1.0)], [(0.0, NAN), (0.0, 1.0)]):      # lo > hi, a NaN: all outside
        r = agree(x, y, (2, 2), window)
        assert r["inside"][0] == 0 and r["outside"][0] == 3 and tuple(r["mode"][0]) == (-1, -1)
        assert not r["counts"].any() and not r["level"].any() and not r["cells"].any() and not r["held"].any()
    for window in ([(-INF, INF), (0.0, 1.0)], [(-1e308, 1e308), (0.0, 1.0)], [(-INF, 1.0), (0.0, 1.0)]):   # an infinite hi - lo: bin 0
        r = agree(x, y, (4, 2), window)
        assert r["inside"][0] == 3 and r["counts"].reshape(4, 2).sum(axis=1).tolist() == [3, 0, 0, 0]
    r = agree([NAN] * 4, [NAN] * 4, (3, 3))                     # nothing finite: the canonical NaN twice
    assert r["range"].view(np.uint64).tolist() == [[[0x7ff8000000000000] * 2] * 2] and r["inside"][0] == 0 and r["outside"][0] == 4
    r = agree([NAN, 2.0, -INF, INF], [1.0, 3.0, 1.0, 1.0], (3, 3))     # the extremes are those of the FINITE samples
    assert r["range"][0].tolist() == [[2.0, 2.0], [1.0, 3.0]] and r["inside"][0] == 1
    r = agree([0.0, -0.0, 0.0], [1.0, 1.0, 1.0], (2, 2))         # -0.0 sorts before +0.0: bits copied
    assert r["range"][0, 0].view(np.uint64).tolist() == [1 << 63, 0] and r["inside"][0] == 3
    r = agree([0.25], [-4.0], (128, 127))                       # one sample
    assert r["inside"][0] == 1 and tuple(r["mode"][0]) == (0, 0) and r["level"][0].tolist() == [1] * 4 == r["cells"][0].tolist() == r["held"][0].tolist()


def test_corners_of_the_level():
    g = (np.arange(6) + 0.5) / 6.0
    xa, xb = (v.reshape(-1).repeat(5) for v in np.meshgrid(g, g, indexing="ij"))       # equal counts everywhere: the level takes every cell
    r = agree(xa, xb, (6, 6), [(0.0, 1.0), (0.0, 1.0)])
    assert set(r["counts"].tolist()) == {5} and r["level"][0].tolist() == [5] * 4 and r["cells"][0].tolist() == [36] * 4 and r["held"][0].tolist() == [180] * 4
    assert tuple(r["mode"][0]) == (0, 0)                        # ties to the lowest ia, then the lowest ib
    r = agree([0.5] * 9, [0.5] * 9, (4, 4), [(0.0, 1.0), (0.0, 1.0)])                   # all samples in one cell
    assert tuple(r["mode"][0]) == (2, 2) and r["level"][0].tolist() == [9] * 4 and r["cells"][0].tolist() == [1] * 4
    # counts 4, 3, 2, 1 in a row: mass 1 takes every non-empty cell, 1e-9 the mode alone, 0.5 (k = 5) the cells holding 4 + 3
    xa = [0.1] * 4 + [0.3] * 3 + [0.5] * 2 + [0.7]
    r = agree(xa, [0.5] * 10, (5, 1), [(0.0, 1.0), (0.0, 1.0)], masses=(1.0, 1e-9, 0.5, 0.7, 0.71))
    assert r["level"][0].tolist() == [1, 4, 3, 3, 2] and r["cells"][0].tolist() == [4, 1, 2, 2, 3] and r["held"][0].tolist() == [10, 4, 7, 7, 9]
    xa = [0.1] * 3 + [0.3] * 3 + [0.5] * 3 + [0.7]                                       # a tie at the level: all three cells are in
    r = agree(xa, [0.5] * 10, (5, 1), [(0.0, 1.0), (0.0, 1.0)], masses=(0.1, 0.4))
    assert r["level"][0].tolist() == [3, 3] and r["cells"][0].tolist() == [3, 3] and r["held"][0].tolist() == [9, 9]


def test_joint_table_on_a_hand_made_table():
    from misti_amd.optimize import joint_table, prior_spec
    counts = np.array([[0, 0, 0, 0], [0, 5, 3, 0], [0, 1, 0, 0]], dtype=np.int32)           # 3 x 4 cells on [0, 3] x [1, 5]
    r = dict(counts=counts.reshape(-1), range=np.array([[[0.0, 3.0], [1.0, 5.0]]]), inside=np.array([9], dtype=np.int32), mode=np.array([[1, 1]], dtype=np.int32),
             level=np.array([[3, 1]], dtype=np.int32), cells=np.array([[2, 3]], dtype=np.int32), held=np.array([[8, 9]], dtype=np.int32),
             pairs=np.array([[2, 0]]), bins=np.array([[3, 4]]), offsets=np.array([0, 12]), masses=np.array([0.8, 1.0]))
    (t,) = joint_table(r)
    assert t["pair"] == (2, 0) and t["window"] == ((0.0, 3.0), (1.0, 5.0)) and t["inside"] == 9 and t["mode"] == (1, 1) and t["mode_centre"] == (1.5, 2.5)
    assert t["edges"][0].tolist() == [0.0, 1.0, 2.0, 3.0] and t["edges"][1].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]
    a, b = t["regions"]
    assert (a["mass"], a["level"], a["cells"], a["held"], a["area"], a["extent"]) == (0.8, 3, 2, 8, 2 / 12, ((1.0, 2.0), (2.0, 4.0)))
    assert a["mask"].tolist() == (counts >= 3).tolist()
    assert (b["level"], b["cells"], b["held"], b["area"], b["extent"]) == (1, 3, 9, 3 / 12, ((1.0, 3.0), (2.0, 4.0)))
    assert "extent_natural" not in a and "coordinate" not in t
    (t,) = joint_table(r, prior=prior_spec(3, log=(0,)))        # coordinate 0 is the pair's SECOND axis
    assert t["coordinate"] == ("linear", "log") and t["natural_is_image"] is True
    assert t["regions"][0]["extent_natural"] == ((1.0, 2.0), (math.exp(2.0), math.exp(4.0))) and t["regions"][0]["extent"] == ((1.0, 2.0), (2.0, 4.0))
    assert t["window_natural"] == ((0.0, 3.0), (math.exp(1.0), math.exp(5.0))) and t["mode_centre_natural"] == (1.5, math.exp(2.5))
    assert (t["edges_natural"][1] == np.exp(t["edges"][1])).all() and (t["edges_natural"][0] == t["edges"][0]).all()
    (t,) = joint_table(r, prior=prior_spec(3))
    assert t["natural_is_image"] is False and t["regions"][1]["extent_natural"] == t["regions"][1]["extent"]
    empty = dict(r, counts=np.zeros(12, dtype=np.int32), inside=np.array([0], dtype=np.int32), mode=np.array([[-1, -1]], dtype=np.int32),
                 level=np.zeros((1, 2), dtype=np.int32))
    (t,) = joint_table(empty)
    assert math.isnan(t["mode_centre"][0]) and t["regions"][0]["cells"] == 0 and math.isnan(t["regions"][0]["extent"][0][0]) and not t["regions"][0]["mask"].any()
    both = joint_table({k: (np.stack([v, v]) if k in ("counts", "range", "inside", "mode", "level", "cells", "held") else v) for k, v in r.items()})
    assert len(both) == 2 and both[1][0]["regions"][0]["extent"] == ((1.0, 2.0), (2.0, 4.0))


# ---- what the ABI refuses before it looks at a context ----------------------------------------------------------------------------------
def joint(S=2, K=10, W=4, N=3, chain=1, pairs=((0, 1), (2, 0)), bins=((4, 4), (128, 1)), masses=(0.95,), null=(), **kw):
    """misti_ens_joint_dev WITHOUT a context: a descriptor that passes every check ends at "ctx is NULL"."""
    from misti_amd import _lib
    pr, bn, ms = np.asarray(pairs, dtype=np.int32), np.asarray(bins, dtype=np.int32), np.asarray(masses, dtype=np.float64)
    f = dict(size=C.sizeof(_lib.EnsJoint), burn=0, n_pair=pr.shape[0], pairs=pr.ctypes.data, bins=bn.ctypes.data, n_mass=ms.size, masses=ms.ctypes.data if ms.size else None)
    f.update(kw)
    f.update({k: None for k in null})
    j = _lib.EnsJoint(**f)
    rc = lib().misti_ens_joint_dev(None, S, K, W, N, C.c_void_p(chain) if chain else None, C.byref(j))
    return rc, lib().misti_last_error().decode()


@pytest.mark.parametrize("kw, code, word", [
    (dict(), E_ARG, "ctx is NULL"),                                                  # the descriptor passes: only the context is missing
    (dict(counts=8, range_out=8, inside=8, mode=8, level=8, cells=8, held=8, range=8), E_ARG, "ctx is NULL"),
    (dict(masses=(1.0, 1e-300, 0.5) + (0.5,) * 5), E_ARG, "ctx is NULL"),
    (dict(masses=(), counts=8, mode=8), E_ARG, "ctx is NULL"),                       # a histogram needs no mass
    (dict(pairs=[(a, b) for a in range(16) for b in range(a)], bins=[(1, 128)] * 120, N=16), E_ARG, "ctx is NULL"),
    (dict(size=8), E_ARG, "size"),
    (dict(S=-1), E_ARG, "negative number of searches"),
    (dict(W=0), E_ARG, "no walker or coordinate"),
    (dict(N=0), E_ARG, "no walker or coordinate"),
    (dict(burn=10), E_ARG, "burn must be 0 ... K - 1"),
    (dict(burn=-1), E_ARG, "burn must be 0 ... K - 1"),
    (dict(chain=0), E_ARG, "the chain is NULL"),
    (dict(W=257), E_LIMIT, "MISTI_ENS_MAX_WALKERS"),
    (dict(N=17), E_LIMIT, "MISTI_MAX_PARAMS"),
    (dict(K=2 ** 30), E_LIMIT, "INT32_MAX samples"),
    (dict(S=2 ** 31), E_LIMIT, "too many searches"),
    (dict(n_pair=0), E_ARG, "n_pair must be 1 ... 120"),
    (dict(n_pair=121), E_ARG, "n_pair must be 1 ... 120"),
    (dict(null=("pairs",)), E_ARG, "pairs / bins is NULL"),
    (dict(null=("bins",)), E_ARG, "pairs / bins is NULL"),
    (dict(pairs=((0, 1), (3, 0))), E_ARG, "outside 0 ... 2"),
    (dict(pairs=((0, -1), (2, 0))), E_ARG, "outside 0 ... 2"),
    (dict(pairs=((0, 1), (2, 2))), E_ARG, "two distinct coordinates"),
    (dict(bins=((4, 4), (0, 1))), E_ARG, "bins[1][0] = 0"),
    (dict(bins=((4, 129), (1, 1))), E_ARG, "bins[0][1] = 129"),
    (dict(n_mass=-1), E_ARG, "n_mass must be 0 ... 8"),
    (dict(n_mass=9), E_ARG, "n_mass must be 0 ... 8"),
    (dict(null=("masses",)), E_ARG, "masses is NULL"),
    (dict(masses=(0.5, 0.0)), E_ARG, "masses[1]"),
    (dict(masses=(1.0000001,)), E_ARG, "masses[0]"),
    (dict(masses=(0.5, 0.9, NAN)), E_ARG, "masses[2]"),
    (dict(masses=(), level=8), E_ARG, "n_mass == 0"),
    (dict(masses=(), cells=8), E_ARG, "n_mass == 0"),
    (dict(masses=(), held=8), E_ARG, "n_mass == 0"),
    # the header's order: of two faults the earlier one is named
    (dict(size=8, S=-1), E_ARG, "size"),
    (dict(S=-1, burn=10), E_ARG, "negative number"),
    (dict(burn=10, chain=0), E_ARG, "burn"),
    (dict(chain=0, W=257), E_ARG, "chain is NULL"),
    (dict(W=257, n_pair=0), E_LIMIT, "MISTI_ENS_MAX_WALKERS"),
    (dict(n_pair=0, null=("pairs",)), E_ARG, "n_pair"),
    (dict(pairs=((0, 0), (2, 0)), bins=((0, 4), (1, 1))), E_ARG, "distinct"),
    (dict(bins=((0, 4), (1, 1)), n_mass=9), E_ARG, "bins[0][0]"),
    (dict(n_mass=9, null=("masses",)), E_ARG, "n_mass"),
    (dict(masses=(2.0,), null=("masses",)), E_ARG, "masses is NULL"),
])
def test_joint_argument_checks(kw, code, word):
    rc, why = joint(**kw)
    assert rc == code and word in why, (rc, why)


def test_a_null_descriptor_and_the_older_doors_keep_their_texts():
    from misti_amd import _lib
    L = lib()
    why = lambda: L.misti_last_error().decode()
    assert L.misti_ens_joint_dev(None, 1, 1, 4, 2, C.c_void_p(8), None) == E_ARG and why() == "the joint descriptor is NULL"
    ens, pt, post = _lib.EnsSample(size=C.sizeof(_lib.EnsSample)), _lib.PtSample(size=C.sizeof(_lib.PtSample)), _lib.EnsPost(size=C.sizeof(_lib.EnsPost))
    small = lambda cls: cls(size=C.sizeof(cls) - 8)
    jt = _lib.EnsJoint(size=C.sizeof(_lib.EnsJoint))
    doors = [(lambda q, p: L.misti_ensemble_sample(None, q), ens, "misti_ens_t"),
             (lambda q, p: L.misti_ensemble_posterior(None, q, p), ens, "misti_ens_t"),
             (lambda q, p: L.misti_ensemble_sample_prior(None, q, p, None), ens, "misti_ens_t"),
             (lambda q, p: L.misti_tempered_sample(None, q, p), pt, "misti_pt_t"),
             (lambda q, p: L.misti_tempered_sample_prior(None, q, p, None), pt, "misti_pt_t"),
             (lambda q, p: L.misti_ensemble_sample_joint(None, q, p, None, None), ens, "misti_ens_t"),          # joint == NULL IS the older entry
             (lambda q, p: L.misti_tempered_sample_joint(None, q, p, None, None), pt, "misti_pt_t"),
             (lambda q, p: L.misti_ensemble_sample_joint(None, q, p, None, C.byref(jt)), ens, "misti_ens_t"),
             (lambda q, p: L.misti_tempered_sample_joint(None, q, p, None, C.byref(jt)), pt, "misti_pt_t")]
    for call, q, name in doors:
        assert call(None, None) == E_ARG and why() == "the sampler descriptor is NULL"
        assert call(C.byref(small(type(q))), None) == E_ARG
        assert why() == "the sampler descriptor's size is %u, this library's %s has %u bytes" % (C.sizeof(q) - 8, name, C.sizeof(q))
        # an empty descriptor of the right size: its split mode 0 is neither of the two
        assert call(C.byref(q), C.byref(post)) == E_ARG
        assert why() == "the sampler descriptor's split mode 0 is neither MISTI_SPLIT_PER_START nor MISTI_SPLIT_FITTED"
    for call, q, name in doors[1:]:
        assert call(C.byref(q), C.byref(small(_lib.EnsPost))) == E_ARG
        assert why() == "the summary descriptor's size is %u, this library's misti_ens_post_t has %u bytes" % (C.sizeof(post) - 8, C.sizeof(post))
    assert L.misti_ensemble_posterior(None, C.byref(ens), None) == E_ARG and why() == "the summary descriptor is NULL"
    for door, q in ((L.misti_ensemble_sample_joint, ens), (L.misti_tempered_sample_joint, pt)):            # the joint's size beside the others'
        assert door(None, C.byref(q), None, None, C.byref(small(_lib.EnsJoint))) == E_ARG
        assert why() == "the joint descriptor's size is %u, this library's misti_ens_joint_t has %u bytes" % (C.sizeof(jt) - 8, C.sizeof(jt))
    # misti_ens_summary_dev: its descriptor, its shapes, its masses - the words they had
    pr = np.array([0.5])
    ok = dict(size=C.sizeof(_lib.EnsPost), n_prob=1, probs=pr.ctypes.data, c=5.0)
    for args, p, text in (((1, 1, 4, 2), None, "the summary descriptor is NULL"),
                          ((-1, 1, 4, 2), _lib.EnsPost(**ok), "negative number of searches, or no walker or coordinate (S = -1, W = 4, N = 2)"),
                          ((1, 1, 4, 2), _lib.EnsPost(**dict(ok, burn=1)), "burn must be 0 ... K - 1 (got 1 for 1 kept steps)"),
                          ((1, 1, 4, 2), _lib.EnsPost(**dict(ok, n_mass=9)), "n_mass must be 0 ... 8 (got 9)"),
                          ((1, 1, 4, 2), _lib.EnsPost(**dict(ok, hpd=8)), "hpd / hpd_at given with n_mass == 0: a shortest interval needs its mass"),
                          ((1, 1, 4, 2), _lib.EnsPost(**ok), "ctx is NULL")):
        assert L.misti_ens_summary_dev(None, *args, C.c_void_p(8), None, C.byref(p) if p is not None else None) == E_ARG and why() == text


# ---- header, binding, build lists, command line -------------------------------------------------------------------------------------------
def test_header_binding_and_build_lists_agree():
    from misti_amd import _lib, build, optimize
    hdr = open(os.path.join(ROOT, "include", "misti_hip.h")).read()
    assert lib().misti_abi_version() == 6 == _lib.ABI_VERSION and "#define MISTI_ABI_VERSION 6" in hdr
    body = hdr[:hdr.index("} misti_ens_joint_t;")].rsplit("typedef struct {", 1)[1]
    names = [n for line in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", line.strip())]
    assert names == [n for n, _ in _lib.EnsJoint._fields_], names
    assert names == ["size", "burn", "n_pair", "pairs", "bins", "range", "n_mass", "masses", "counts", "range_out", "inside", "mode", "level", "cells", "held"]
    define = lambda text, name: int(re.search(r"^#define %s (\d+)" % name, text, flags=re.M).group(1))
    assert _lib.JOINT_MAX_PAIRS == define(hdr, "MISTI_JOINT_MAX_PAIRS") == 120 == 16 * 15 // 2 == optimize.JOINT_MAX_PAIRS
    assert _lib.JOINT_MAX_BINS == define(hdr, "MISTI_JOINT_MAX_BINS") == 128 == optimize.JOINT_MAX_BINS
    joint_h = open(os.path.join(ROOT, "misti_amd", "csrc", "misti_joint.h")).read()
    assert _lib.JOINT_SLAB == define(joint_h, "MISTI_JOINT_SLAB") and _lib.JOINT_SLAB >= 256
    assert _lib.JOINT_MAX_BINS ** 2 * 4 <= 64 * 1024            # the largest pair's cells fit the LDS a workgroup may have
    assert "misti_joint.hip" in build.SOURCES and "misti_joint.h" in build.HEADERS
    for name in ("misti_ens_joint_dev", "misti_ensemble_sample_joint", "misti_tempered_sample_joint"):
        assert name in _lib.SYMBOLS and re.search(r"^int %s\(misti_ctx\* ctx, " % name, hdr, flags=re.M) and hasattr(lib(), name)
    assert "optimize.ensemble_joint_rule" in hdr and "SAMPLING COORDINATE" in hdr
    # the older descriptors did not move
    assert (C.sizeof(_lib.EnsPost), C.sizeof(_lib.EnsSample), C.sizeof(_lib.PtSample), C.sizeof(_lib.Prior)) == (144, 192, 240, 40)
    assert [n for n, _ in _lib.EnsPost._fields_][-6:] == ["best_at", "n_mass", "masses", "hpd", "hpd_at", "order"]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Left out: joint two-dimensional regions" not in design and "ensemble_joint_rule" in design


BASE = ["a.psmc", "b.psmc", "d.sfs", "20"]
SOLVE = ["--grid-solve", "--grid-st", "15", "17", "-mi", "1", "4", "16", "0.2", "1", "-mi", "2", "4", "16", "0.3", "1", "--box", "0", "0.01", "5", "--box", "1", "0.01", "5"]
FIT = ["--fit-st", "-mi", "1", "4", "16", "0.2", "1", "--box", "0", "0.01", "5", "--box", "st", "10", "19"]


def test_parser_accepts_mcmc_joint():
    from misti_amd import cli
    parse = lambda args: cli.build_parser().parse_args(BASE + args)
    a = parse(SOLVE + ["--mcmc", "8", "50", "--mcmc-joint", "0", "1"])
    assert cli.mcmc_error(a) is None
    assert cli._mcmc_joint(a, 2) == dict(pairs=[(0, 1)], bins=[[32, 32]], range="box", masses=(0.95,))
    a = parse(FIT + ["--mcmc", "8", "50", "--mcmc-joint", "st", "0", "64", "--mcmc-joint", "0", "st", "--mcmc-joint-mass", "0.5", "0.9", "--mcmc-joint-out", "j.npz"])
    assert cli.mcmc_error(a) is None
    assert cli._mcmc_joint(a, 1) == dict(pairs=[(1, 0), (0, 1)], bins=[[64, 64], [32, 32]], range="box", masses=(0.5, 0.9))
    for more in (["--mcmc-post"], ["--mcmc-post", "--mcmc-hpd"], ["--mcmc-ladder", "3", "4"], ["--mcmc-log", "0"], ["--mcmc-prior", "0", "exponential", "1"],
                 ["--mcmc-post", "--mcmc-ladder", "3", "4", "--mcmc-log", "0", "st"]):
        assert cli.mcmc_error(parse(FIT + ["--mcmc", "8", "50", "--mcmc-joint", "0", "st"] + more)) is None, more
    a = parse(SOLVE + ["--mcmc", "8", "50"])
    assert a.mcmc_joint is None and cli.mcmc_error(a) is None and cli._mcmc_joint(a, 2) is None
    for args, word in ((["--mcmc-joint", "0", "1"] + SOLVE, "give --mcmc W STEPS"),
                       (["--mcmc-joint-mass", "0.5"] + SOLVE, "give --mcmc W STEPS"),
                       (["--mcmc-joint-out", "j.npz"] + SOLVE, "give --mcmc W STEPS"),
                       (["--mcmc", "8", "50", "--mcmc-joint", "0", "2"] + SOLVE, "no coordinate of this run"),
                       (["--mcmc", "8", "50", "--mcmc-joint", "0", "st"] + SOLVE, "no coordinate of this run"),
                       (["--mcmc", "8", "50", "--mcmc-joint", "1", "1"] + SOLVE, "A == B"),
                       (["--mcmc", "8", "50", "--mcmc-joint", "0"] + SOLVE, "two coordinates"),
                       (["--mcmc", "8", "50", "--mcmc-joint", "0", "1", "0"] + SOLVE, "1 ... 128"),
                       (["--mcmc", "8", "50", "--mcmc-joint", "0", "1", "129"] + SOLVE, "1 ... 128"),
                       (["--mcmc", "8", "50", "--mcmc-joint", "0", "1", "--mcmc-joint-mass", "0"] + SOLVE, "(0, 1]"),
                       (["--mcmc", "8", "50", "--mcmc-joint-mass", "0.5"] + SOLVE, "give it")):
        why = cli.mcmc_error(parse(args))
        assert why is not None and "--mcmc-joint" in why and word in why, (args, why)
    assert "--mcmc-joint A B [BINS]" in cli.__doc__ and "--mcmc-joint-mass" in cli.__doc__ and "--mcmc-joint-out" in cli.__doc__
