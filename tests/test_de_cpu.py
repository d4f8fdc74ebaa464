"""Differential evolution per search without a GPU: the stream (optimize.de_draws against NumPy's Philox at the stated blocks,
misti_de_draws - the very functions the kernels call - against de_draws), the rule on analytic objectives
(optimize.differential_evolution_rule - what the device result is compared against in tests/test_gpu_de.py), the independence of a
search from the others in its call, the argument checks misti_de_search makes before it looks at a context, and the command line's
parsing and refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

E_ARG, E_LIMIT = -1, -4
WORDS = 20                      # 4 x MISTI_DE_BLOCKS words per member and generation


def lib():
    from misti_amd import _lib
    return _lib.load()


def c_draws(seed, id_, g, m, P, N):
    r1, r2, jr, uF, u = C.c_int32(-7), C.c_int32(-7), C.c_int32(-7), C.c_double(-7.0), np.full(N, -7.0)
    rc = lib().misti_de_draws(seed, id_, g, m, P, N, C.byref(r1), C.byref(r2), C.byref(jr), C.byref(uF), u.ctypes.data_as(C.c_void_p))
    assert rc == 0, lib().misti_last_error()
    return dict(r1=r1.value, r2=r2.value, jrand=jr.value, u_F=uF.value, u=u)


# ---- the stream ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, id_", [(0, 0), (7, 3), (2 ** 64 - 1, 2 ** 40 + 5)])
def test_de_draws_are_numpys_philox_at_the_stated_blocks(seed, id_):
    """Member i of generation g owns the 5 blocks from block (g P + i) 5 on of numpy.random.Philox(key=[seed, id]) - words
    (g P + i) 20 ... of its random_raw stream from counter 0: w[0] r1, w[1] r2, w[2] jrand, w[3] F's uniform, w[4 + k] coordinate k's;
    a uniform is (raw >> 11) 2^-53, an index the high 64 bits of raw x n (Python integers here)."""
    from misti_amd.optimize import de_draws
    P, N, G = 5, 3, 4
    raw = [int(v) for v in np.random.Philox(key=np.array([seed, id_], dtype=np.uint64)).random_raw(G * P * WORDS)]
    for g in range(G):
        for i in range(P):
            w = raw[(g * P + i) * WORDS:(g * P + i + 1) * WORDS]
            d = de_draws(seed, id_, g, i, P, N)
            others = [m for m in range(P) if m != i]
            r1 = others[(w[0] * (P - 1)) >> 64]
            r2 = [m for m in others if m != r1][(w[1] * (P - 2)) >> 64]
            assert (d["r1"], d["r2"], d["jrand"]) == (r1, r2, (w[2] * N) >> 64)
            assert d["u_F"] == (w[3] >> 11) * 2.0 ** -53
            assert d["u"].tolist() == [(w[4 + k] >> 11) * 2.0 ** -53 for k in range(N)]


@pytest.mark.parametrize("P", [4, 5, 64])
@pytest.mark.parametrize("N", [1, 2, 16])
def test_the_library_draws_what_de_draws_states(P, N):
    from misti_amd.optimize import de_draws
    for g, i in ((0, 0), (0, P - 1), (1, 0), (1, 2), (7, P - 1), (1000, 3)):
        want, got = de_draws(11, 6, g, i, P, N), c_draws(11, 6, g, i, P, N)
        assert (got["r1"], got["r2"], got["jrand"], got["u_F"]) == (want["r1"], want["r2"], want["jrand"], want["u_F"]), (g, i)
        assert np.array_equal(got["u"], want["u"]) and (0 <= got["u"]).all() and (got["u"] < 1).all()


@pytest.mark.parametrize("P", [4, 5, 9])
def test_r1_r2_and_the_member_are_distinct(P):
    """P = 4 is the edge: r2 is drawn from two members.  With few members the 59 generations reach every ordered triple."""
    seen = set()
    for g in range(1, 60):
        for i in range(P):
            d = c_draws(3, 1, g, i, P, 2)
            assert len({i, d["r1"], d["r2"]}) == 3 and 0 <= d["r1"] < P and 0 <= d["r2"] < P and 0 <= d["jrand"] < 2
            seen.add((i, d["r1"], d["r2"]))
    assert P > 5 or len(seen) == P * (P - 1) * (P - 2)


def test_draws_argument_checks():
    L = lib()
    a, u = C.c_int32(), np.zeros(16)
    p = (C.byref(a), C.byref(a), C.byref(a), C.byref(C.c_double()), u.ctypes.data_as(C.c_void_p))
    assert L.misti_de_draws(0, 0, -1, 0, 4, 1, *p) == E_ARG
    assert L.misti_de_draws(0, 0, 0, 0, 3, 1, *p) == E_ARG
    assert L.misti_de_draws(0, 0, 0, 4, 4, 1, *p) == E_ARG
    assert L.misti_de_draws(0, 0, 0, 0, 4, 0, *p) == E_ARG
    assert L.misti_de_draws(0, 0, 0, 0, 4, 1, p[0], p[1], p[2], p[3], None) == E_ARG and b"NULL" in L.misti_last_error()
    assert L.misti_de_draws(0, 0, 0, 0, 257, 1, *p) == E_LIMIT and b"MISTI_DE_MAX_POP" in L.misti_last_error()
    assert L.misti_de_draws(0, 0, 0, 0, 4, 17, *p) == E_LIMIT and b"MISTI_MAX_PARAMS" in L.misti_last_error()
    assert L.misti_de_draws(0, 0, 0, 255, 256, 16, *p) == 0


# ---- the rule on analytic objectives --------------------------------------------------------------------------------------------------------
def rastrigin(X, s=None):
    X = np.asarray(X, dtype=float)
    return 10.0 * X.shape[1] + np.sum(X * X - 10.0 * np.cos(2.0 * np.pi * X), axis=1)


START, LO, HI = [3.3, -2.6], [-5.12, -5.12], [5.12, 5.12]
DE = dict(pop=20, maxiter=200, tol=1e-8, seed=1)


def test_the_rule_ends_in_the_global_basin_where_nelder_mead_does_not():
    """Rastrigin's function in [-5.12, 5.12]^2 from (3.3, -2.6): the local search ends in the basin of (3, -3), f = 17.9; the
    population search (20 members, seed 1, at most 200 generations) at the origin, f = 0."""
    from misti_amd.optimize import batched_nelder_mead, differential_evolution_rule
    nm = batched_nelder_mead(lambda X: rastrigin(X), [START])
    assert nm.converged[0] and nm.fun[0] > 17.0 and np.abs(nm.x[0]).min() > 2.5
    r = differential_evolution_rule(rastrigin, [START], LO, HI, **DE)
    assert r["status"][0] == 0 and r["nit"][0] < 200 and np.abs(r["x"][0]).max() < 1e-6 and -r["llh"][0] < 1e-10
    assert r["nfev"][0] == 20 * (r["nit"][0] + 1) == r["n_points"]
    assert r["population"].shape == (1, 20, 2) and np.array_equal(-r["population_llh"][0], rastrigin(r["population"][0]))
    assert r["llh"][0] == r["population_llh"][0].max()


def test_every_point_lies_inside_the_box_and_a_fixed_coordinate_never_moves():
    """A narrow box around a minimum on its edge makes mutants leave it all the time: each is put halfway back, none is handed on."""
    from misti_amd.optimize import differential_evolution_rule
    lo, hi = np.array([0.4, 1.25, -5.0]), np.array([0.6, 1.25, -2.9])
    seen = []

    def f(X, s):
        seen.append(np.array(X))
        return rastrigin(X)
    r = differential_evolution_rule(f, [[9.0, 0.0, -3.0], [0.5, 1.25, -9.0]], lo, hi, pop=7, maxiter=25, tol=0.0, F=(0.9, 1.9), CR=0.9, seed=4)
    X = np.concatenate(seen)
    assert X.shape == (2 * 7 * 26, 3) == (r["n_points"], 3) and (r["status"] == 2).all() and (r["nit"] == 25).all()
    assert (X >= lo).all() and (X <= hi).all() and (X[:, 1] == 1.25).all()
    assert np.array_equal(X[0], [0.6, 1.25, -3.0]) and np.array_equal(X[7], [0.5, 1.25, -5.0])        # member 0: the start, clipped
    assert (r["x"][:, 1] == 1.25).all() and (r["population"][:, :, 1] == 1.25).all()
    # generation 1 of search 0 written out in scalars from de_draws: mutant, crossover, the midpoint repair, the fixed coordinate
    from misti_amd.optimize import de_draws
    x0, f0 = seen[0][:7], rastrigin(seen[0][:7])
    b, repaired = int(np.argmin(f0)), 0
    for i in range(7):
        d = de_draws(4, 0, 1, i, 7, 3)
        F = 0.9 + d["u_F"] * (1.9 - 0.9)
        for k in range(3):
            t = x0[i][k]
            if lo[k] == hi[k]:
                t = lo[k]
            elif k == d["jrand"] or d["u"][k] < 0.9:
                v = x0[b][k] + F * (x0[d["r1"]][k] - x0[d["r2"]][k])
                t = x0[i][k] + 0.5 * (hi[k] - x0[i][k]) if v > hi[k] else x0[i][k] + 0.5 * (lo[k] - x0[i][k]) if v < lo[k] else v
                repaired += v > hi[k] or v < lo[k]
            assert seen[1][i][k] == t, (i, k)
    assert repaired >= 3


def test_an_objective_without_a_value_returns_minus_inf_with_status_2():
    from misti_amd.optimize import differential_evolution_rule
    r = differential_evolution_rule(lambda X, s: np.full(len(X), np.inf), [START], LO, HI, pop=4, maxiter=3)
    assert r["llh"][0] == -np.inf and r["status"][0] == 2 and r["nit"][0] == 3 and r["nfev"][0] == 16
    assert (r["x"][0] >= LO).all() and (r["x"][0] <= HI).all()                                       # inf <= inf replaces: member 0 has moved, inside the box
    r = differential_evolution_rule(lambda X, s: np.full(len(X), np.nan), [START], LO, HI, pop=4, maxiter=3)
    assert r["llh"][0] == -np.inf and r["status"][0] == 2


def test_a_stopped_search_submits_no_further_points():
    """Search 1 lives in a box a hair wide: its values agree at once and it stops after the initial population."""
    from misti_amd.optimize import differential_evolution_rule
    lo = np.array([LO, [1.0, 1.0]])
    hi = np.array([HI, [1.0 + 1e-9, 1.0 + 1e-9]])
    calls = []

    def f(X, s):
        calls.append(np.array(s))
        return rastrigin(X)
    r = differential_evolution_rule(f, [START, [1.0, 1.0]], lo, hi, pop=5, maxiter=6, tol=1e-6, seed=2)
    assert r["status"].tolist() == [2, 0] and r["nit"].tolist() == [6, 0] and r["nfev"].tolist() == [35, 5]
    assert r["n_points"] == 40 and all((c == 0).all() for c in calls[1:]) and len(calls) == 7


def test_a_search_is_the_same_alone_among_others_and_under_a_permutation():
    from misti_amd.optimize import differential_evolution_rule
    rng = np.random.default_rng(5)
    starts = rng.uniform(-5, 5, size=(4, 2))
    kw = dict(pop=6, maxiter=12, tol=1e-3, seed=9)
    ids = np.array([0, 1, 2, 3])
    together = differential_evolution_rule(rastrigin, starts, LO, HI, ids=ids, **kw)
    assert not np.array_equal(together["x"][0], together["x"][1])
    fields = ("x", "llh", "nit", "nfev", "status", "population", "population_llh")
    for s in range(4):
        alone = differential_evolution_rule(rastrigin, starts[s:s + 1], LO, HI, ids=ids[s:s + 1], **kw)
        for k in fields:
            assert np.array_equal(alone[k][0], together[k][s]), (s, k)
    perm = np.array([2, 0, 3, 1])
    shuffled = differential_evolution_rule(rastrigin, starts[perm], LO, HI, ids=ids[perm], **kw)
    for k in fields:
        assert np.array_equal(shuffled[k], together[k][perm]), k
    default = differential_evolution_rule(rastrigin, starts, LO, HI, **kw)                            # ids default to 0 ... S - 1
    assert all(np.array_equal(default[k], together[k]) for k in fields)


def test_the_rule_refuses_a_box_it_cannot_fill():
    from misti_amd.optimize import differential_evolution_rule
    for lo, hi in (([0.0, -np.inf], [1.0, 1.0]), ([0.0, 0.0], [1.0, np.nan]), ([2.0, 0.0], [1.0, 1.0]), ([-1e308, 0.0], [1e308, 1.0])):
        with pytest.raises(ValueError):
            differential_evolution_rule(rastrigin, [START], lo, hi)
    with pytest.raises(ValueError):
        differential_evolution_rule(rastrigin, [START], LO, HI, pop=3)


# ---- what the ABI refuses before it looks at a context ----------------------------------------------------------------------------------
def de_search(ctx=None, size=None, null=(), **kw):
    """misti_de_search WITHOUT a context: every check below comes before the context is looked at, and a descriptor that passes them
    ends at "ctx is NULL".  No output is ever written."""
    from misti_amd import _lib
    S = kw.pop("n_start", 2)
    a = dict(starts=np.zeros((max(S, 1), 2)), rows=np.zeros(max(S, 1), dtype=np.int32), jsfs=np.ones((3, 8)), box_lo=np.zeros((1, 2)),
             box_hi=np.ones((1, 2)), x=np.zeros((max(S, 1), 2)), llh=np.zeros(max(S, 1)), split_times=np.full(max(S, 1), 5.0))
    for k in list(kw):
        if k in a:
            a[k] = np.ascontiguousarray(kw.pop(k), dtype=a[k].dtype)
    f = dict(size=C.sizeof(_lib.DeSearch) if size is None else size, split=_lib.SPLIT_PER_START, n_start=S, n_rep=3, n_box=1, pop=8, maxiter=5,
             tol=0.01, atol=0.0, F_lo=0.5, F_hi=1.0, CR=0.7, seed=0)
    f.update(kw)
    q = _lib.DeSearch(**f, **{k: (None if k in null else v.ctypes.data) for k, v in a.items()})
    rc = lib().misti_de_search(ctx, C.byref(q))
    assert not a["x"].any() and not a["llh"].any()
    return rc, lib().misti_last_error().decode()


@pytest.mark.parametrize("kw, code, word", [
    (dict(), E_ARG, "ctx is NULL"),                                                 # the descriptor passes: only the context is missing
    (dict(n_start=0, n_box=0), E_ARG, "ctx is NULL"),
    (dict(size=8), E_ARG, "size"),
    (dict(split=0), E_ARG, "split mode"),
    (dict(n_start=-1), E_ARG, "negative"),
    (dict(null=("starts",)), E_ARG, "NULL"),
    (dict(null=("box_lo",)), E_ARG, "NULL"),
    (dict(null=("split_times",)), E_ARG, "split_times"),
    (dict(null=("split_times",), split=2), E_ARG, "ctx is NULL"),                   # a fitted split needs none
    (dict(n_rep=0), E_ARG, "n_rep"),
    (dict(pop=3), E_ARG, "pop"),
    (dict(pop=257), E_LIMIT, "MISTI_DE_MAX_POP"),
    (dict(maxiter=0), E_ARG, "maxiter"),
    (dict(tol=-1.0), E_ARG, "tol"),
    (dict(atol=float("nan")), E_ARG, "atol"),
    (dict(F_lo=1.0, F_hi=0.5), E_ARG, "F_lo <= F_hi"),
    (dict(F_hi=float("inf")), E_ARG, "F"),
    (dict(CR=1.5), E_ARG, "CR"),
    (dict(CR=float("nan")), E_ARG, "CR"),
    (dict(n_box=3), E_ARG, "n_box"),
    (dict(rows=[0, 3]), E_ARG, "rows[1]"),
    (dict(rows=[-1, 0]), E_ARG, "rows[0]"),
    (dict(split_times=[5.0, float("inf")]), E_ARG, "split_times[1]"),
])
def test_de_search_argument_checks(kw, code, word):
    rc, why = de_search(**kw)
    assert rc == code and word in why, (rc, why)


def test_a_null_descriptor_is_refused():
    assert lib().misti_de_search(None, None) == E_ARG and b"NULL" in lib().misti_last_error()


# ---- header, binding, command line --------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_entry_points_and_the_abi_stays_6():
    from misti_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "misti_hip.h")).read()
    assert re.search(r"^int misti_de_search\(misti_ctx\* ctx, const misti_de_t\* search\);", hdr, flags=re.M)
    assert re.search(r"^int misti_de_draws\(uint64_t seed, uint64_t id, int64_t generation, int32_t member, int32_t pop, int32_t n,", hdr, flags=re.M)
    flat = " ".join(hdr.split()).replace("* ", "")
    assert "THE PROJECT'S OWN, NOT SCIPY'S" in flat and "optimize.differential_evolution_rule" in hdr
    assert "#define MISTI_DE_MAX_POP 256" in hdr and "#define MISTI_ABI_VERSION 6" in hdr
    assert lib().misti_abi_version() == 6 and _lib.ABI_VERSION == 6
    assert {"misti_de_search", "misti_de_draws"} <= set(_lib.SYMBOLS) and (_lib.DE_MAX_POP, _lib.DE_BLOCKS) == (256, 5)
    assert "misti_de.hip" in build.SOURCES
    # the binding's record is the header's: every field, in order
    body = hdr[:hdr.index("} misti_de_t;")].rsplit("typedef struct {", 1)[1]
    names = [n for line in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", line.strip())]
    assert names == [n for n, _ in _lib.DeSearch._fields_], names


BASE = ["a.psmc", "b.psmc", "d.sfs", "20"]
SOLVE = ["--grid-solve", "--grid-st", "15", "17", "-mi", "1", "4", "16", "0.2", "1", "--box", "0", "0.01", "5"]
FIT = ["--fit-st", "--grid-st", "15", "17", "-mi", "1", "4", "16", "0.2", "1", "--box", "0", "0.01", "5", "--box", "st", "14", "18"]


def test_parser_accepts_de():
    from misti_amd import cli
    a = cli.build_parser().parse_args(BASE + SOLVE + ["--de", "8", "5", "--de-seed", "3", "--de-F", "0.4", "0.9", "--de-CR", "0.5", "--de-polish"])
    assert (a.de, a.de_seed, a.de_F, a.de_CR, a.de_polish) == ([8, 5], 3, [0.4, 0.9], 0.5, True) and cli.de_error(a) is None
    assert cli._de_options(a) == dict(pop=8, maxiter=5, F=(0.4, 0.9), CR=0.5, seed=3, polish=True)
    a = cli.build_parser().parse_args(BASE + FIT + ["--all-bs", "--de", "16", "40"])
    assert cli.de_error(a) is None and cli._de_options(a) == dict(pop=16, maxiter=40, F=(0.5, 1.0), CR=0.7, seed=0, polish=False)
    assert cli.de_error(cli.build_parser().parse_args(BASE)) is None
    assert "not SciPy's" in " ".join(cli.build_parser().format_help().split())


@pytest.mark.parametrize("args, word", [
    (["--de-seed", "3"], "give --de POP GENS"),
    (["--de-polish"], "give --de POP GENS"),
    (["--de", "3", "5"] + SOLVE, "4 ... 256"),
    (["--de", "300", "5"] + SOLVE, "4 ... 256"),
    (["--de", "8", "0"] + SOLVE, "at least 1"),
    (["--de", "8", "5"] + SOLVE + ["--hops", "3"], "--hops"),
    (["--de", "8", "5"] + SOLVE + ["--se"], "--se"),
    (["--de", "8", "5", "--grid-st", "15", "17"], "--fit-st or --grid-solve"),
    (["--de", "8", "5"] + SOLVE + ["--gpus", "2"], "one GPU"),
    (["--de", "8", "5"] + SOLVE + ["--grid-mi", "0", "0.1", "1", "3"], "--grid-mi"),
    (["--de", "8", "5"] + SOLVE + ["--de-seed", "-1"], "uint64"),
    (["--de", "8", "5"] + SOLVE + ["--de-F", "1", "0.5"], "--de-F"),
    (["--de", "8", "5"] + SOLVE + ["--de-CR", "1.5"], "--de-CR"),
    (["--de", "8", "5"] + SOLVE[:-4], "no --box 0"),
    (["--de", "8", "5"] + FIT[:-4], "no --box st"),
    (["--de", "8", "5"] + SOLVE[:-4] + ["--box", "0", "0.01", "inf"], "finite box"),
])
def test_de_error_names_the_reason(args, word):
    from misti_amd import cli
    why = cli.de_error(cli.build_parser().parse_args(BASE + args))
    assert why is not None and word in why, why


def test_refused_before_a_file_is_read(capsys):
    from misti_amd import cli
    assert cli.main(["no.psmc", "no.psmc", "no.sfs", "20", "--de", "8", "5"] + SOLVE[:-4]) == 2      # (the files do not exist)
    assert "--box" in capsys.readouterr().err
