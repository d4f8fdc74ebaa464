"""Trajectory bands without a GPU: optimize.trajectory_bands_rule against a brute-force loop, its membership edges, the rank rule of
misti_bands_rank against the rule's (i, g), the argument checks of misti_traj_bands_dev / misti_traj_bands (they run before the first
HIP call), and the header, the binding and the build lists."""
import ctypes as C
import math
import os
import re
import struct

import numpy as np
import pytest

from conftest import ROOT

E_ARG = -1
NAN = float("nan")
CANON = 0x7ff8000000000000
POISON = 1e300


def lib():
    from misti_amd import _lib
    return _lib.load()


def bits(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def key(v):
    b = bits(v)
    return (~b) & (2 ** 64 - 1) if b >> 63 else b ^ (1 << 63)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def brute(lc, split, status, probs):
    """Membership by an `if`, sorted() on the key, quantiles read as order statistics: per series (n, members, per p (i, g))."""
    G, m, T1, _ = lc.shape
    out = {}
    for g in range(G):
        for j in range(T1 - 1):
            for pop in range(2):
                mem = []
                for i in range(m):
                    v = float(lc[g, i, j, pop])
                    if status is not None and int(status[g, i]) != 0:
                        continue
                    if not (float(j) < float(split[g, i])):
                        continue
                    if v != v:
                        continue
                    mem.append(v)
                mem = sorted(mem, key=key)
                ranks = []
                for p in probs:
                    h = float(len(mem) - 1) * float(p)
                    ranks.append((int(math.floor(h)), h - math.floor(h)))
                out[g, j, pop] = (mem, ranks)
    return out


def check_against_brute(lc, split, status, probs):
    from misti_amd.optimize import trajectory_bands_rule, lsum
    r = trajectory_bands_rule(lc, split, status, probs, order=True)
    ref = brute(lc, split, status, probs)
    interpolated = exact = 0
    for (g, j, pop), (mem, ranks) in ref.items():
        n = len(mem)
        assert r["count"][g, j, pop] == n
        if n == 0:
            for k in ("mean", "lo", "hi"):
                assert bits(r[k][g, j, pop]) == CANON
            assert all(bits(q) == CANON for q in r["quant"][g, j, pop])
            continue
        assert [bits(v) for v in r["sorted"][g, j, pop, :n]] == [bits(v) for v in mem]
        assert bits(r["lo"][g, j, pop]) == bits(mem[0]) and bits(r["hi"][g, j, pop]) == bits(mem[-1])
        want = lsum(np.array(mem)) / float(n)
        assert bits(r["mean"][g, j, pop]) == (CANON if want != want else bits(want))
        for p, (i, w) in enumerate(ranks):
            got = r["quant"][g, j, pop, p]
            if w == 0.0 or i >= n - 1:
                assert bits(got) == bits(mem[min(i, n - 1)])                # EQUAL to the order statistic
                exact += 1
            else:
                with np.errstate(all="ignore"):
                    expr = np.float64(mem[i]) + np.float64(w) * (np.float64(mem[i + 1]) - np.float64(mem[i]))
                assert bits(got) == (CANON if expr != expr else bits(expr))
                if math.isfinite(mem[i]) and math.isfinite(mem[i + 1]):
                    assert mem[i] <= got <= mem[i + 1]
                interpolated += 1
    assert not np.any(r["count"] < 0)
    return r, exact, interpolated


def random_case(seed, G, m, numT):
    rng = np.random.default_rng(seed)
    lc = np.exp(rng.standard_normal((G, m, numT + 1, 2)))
    lc[:, :, numT, :] = POISON                                               # row numT is never read
    split = rng.uniform(0.0, numT + 0.5, size=(G, m))
    whole = rng.random((G, m)) < 0.4
    split[whole] = np.floor(split[whole])
    status = (rng.random((G, m)) < 0.15).astype(np.int32) * rng.integers(1, 7, size=(G, m)).astype(np.int32)
    lc[rng.random(lc.shape) < 0.02] = NAN
    lc[:, :, numT, :] = POISON
    return lc, split, status


def no_poison(r):
    for k in ("mean", "lo", "hi", "quant"):
        v = r[k][np.isfinite(r[k])]                                          # the poison is finite: neither itself nor a sum or a mean over it
        assert not np.any(np.abs(v) >= 1e290), k
    if "sorted" in r:
        assert not np.any(r["sorted"] == POISON)


@pytest.mark.parametrize("seed, G, m, numT, probs", [
    (1, 1, 1, 2, (0.5,)), (2, 2, 7, 3, (0.0, 1.0, 0.5)), (3, 1, 65, 6, (0.025, 0.5, 0.975)),
    (4, 3, 130, 5, (0.0, 1.0, 0.5, 0.025, 1.0 / 3.0, math.nextafter(1.0, 0.0), 0.25, 0.9))])
def test_rule_against_brute_force(seed, G, m, numT, probs):
    lc, split, status = random_case(seed, G, m, numT)
    r, exact, interpolated = check_against_brute(lc, split, status, probs)
    no_poison(r)
    assert exact > 0 and (m < 7 or interpolated > 0)
    r2, _, _ = check_against_brute(lc, split, None, probs)                   # status absent: every sample is OK
    assert (r2["count"] >= r["count"]).all() and ((r2["count"] > r["count"]).any() or not status.any())


def test_one_group_without_the_leading_axis():
    from misti_amd.optimize import trajectory_bands_rule
    lc, split, status = random_case(9, 1, 20, 4)
    a = trajectory_bands_rule(lc, split, status)
    b = trajectory_bands_rule(lc[0], split[0], status[0])
    assert all(same_bits(a[k][0], b[k]) for k in a)
    assert set(a) == {"count", "mean", "lo", "hi", "quant"} and a["count"].dtype == np.int32


def edge_inputs():
    """One group, numT = 4, m = 8: the membership edges, interval by interval."""
    numT, m = 4, 8
    lc = np.full((1, m, numT + 1, 2), 2.0)
    lc[0, :, :, 1] = np.arange(1.0, m + 1.0)[:, None]
    lc[0, :, numT, :] = POISON
    split = np.array([[2.0, math.nextafter(2.0, math.inf), NAN, 4.0, 4.0, 4.0, 4.0, 3.5]])
    status = np.array([[0, 0, 0, 5, 0, 0, 0, 0]], dtype=np.int32)
    lc[0, 4, 1, 0] = NAN                                                     # a NaN value: out of (j = 1, pop 0) only
    lc[0, 5, 0, 0], lc[0, 6, 0, 0] = 0.0, -0.0                               # both zeros in (j = 0, pop 0)
    lc[0, 5, 3, 1], lc[0, 6, 3, 1] = math.inf, -math.inf                     # both infinities in (j = 3, pop 1)
    return lc, split, status


def test_membership_edges():
    from misti_amd.optimize import trajectory_bands_rule
    lc, split, status = edge_inputs()
    probs = (0.0, 0.5, 1.0)
    r, _, _ = check_against_brute(lc, split, status, probs)
    no_poison(r)
    # j = 0: samples 0, 1, 4, 5, 6, 7 (2 has a NaN split, 3 a non-zero status)
    assert r["count"][0, 0].tolist() == [6, 6]
    # split == j exactly is not a member, nextafter(j, inf) is: at j = 2 sample 0 (split 2.0) is out and sample 1 in
    assert r["count"][0, 1].tolist() == [5, 6] and r["count"][0, 2].tolist() == [5, 5]
    s = trajectory_bands_rule(lc, split, status, probs, order=True)["sorted"]
    assert 1.0 not in s[0, 2, 1] and 2.0 in s[0, 2, 1]                        # pop 1 carries the sample's number + 1
    # j = 3: splits 4.0 and 3.5 only
    assert r["count"][0, 3].tolist() == [4, 4]
    # -0.0 before +0.0
    assert bits(s[0, 0, 0, 0]) == bits(-0.0) and bits(s[0, 0, 0, 1]) == bits(0.0) and bits(r["lo"][0, 0, 0]) == bits(-0.0)
    # +-inf are ordinary members: the extremes, and an interpolation between them and a mean over them is the canonical NaN
    assert r["lo"][0, 3, 1] == -math.inf and r["hi"][0, 3, 1] == math.inf and bits(r["mean"][0, 3, 1]) == CANON
    # without the status sample 3 joins
    r2 = trajectory_bands_rule(lc, split, None, probs)
    assert r2["count"][0, 0].tolist() == [7, 7] and r2["count"][0, 3].tolist() == [5, 5]


def test_empty_single_and_equal_series():
    from misti_amd.optimize import trajectory_bands_rule
    numT, m = 3, 5
    lc = np.full((2, m, numT + 1, 2), 0.75)
    lc[:, :, numT, :] = POISON
    split = np.array([[0.0, 0.0, 1.0, 0.0, -1.0], [3.0] * m])                # group 0: n = 1 at j = 0, n = 0 above; group 1: full
    r = trajectory_bands_rule(lc, split, None, (0.0, 1.0 / 3.0, 1.0))
    assert r["count"][0].tolist() == [[1, 1], [0, 0], [0, 0]] and r["count"][1].tolist() == [[m, m]] * 3
    assert all(bits(v) == bits(0.75) for k in ("mean", "lo", "hi") for v in r[k][0, 0]) and all(bits(v) == bits(0.75) for v in r["quant"][0, 0].ravel())
    for k in ("mean", "lo", "hi", "quant"):
        assert all(bits(v) == CANON for v in r[k][0, 1:].ravel()), k
        assert all(bits(v) == bits(0.75) for v in r[k][1].ravel()), k             # all values equal: every summary is that value
    no_poison(r)


def test_rule_refuses_bad_arguments():
    from misti_amd.optimize import trajectory_bands_rule
    lc, split, status = random_case(5, 1, 4, 2)
    for probs in ((), (0.5,) * 9, (1.5,), (-0.1,), (NAN,)):
        with pytest.raises(ValueError):
            trajectory_bands_rule(lc, split, status, probs)
    with pytest.raises(ValueError):
        trajectory_bands_rule(lc[0, :, :, 0], split, status)


# ---- the rank rule on the host ---------------------------------------------------------------------------------------------------------
PROBS = (0.0, 1.0, 0.5, 0.025, 1.0 / 3.0, math.nextafter(1.0, 0.0))


def test_bands_rank_equals_the_rule():
    from misti_amd.optimize import bands_rank
    L = lib()
    lo, hi, g = C.c_int64(), C.c_int64(), C.c_double()
    for n in list(range(1, 71)) + [2047, 2048, 2049]:
        for p in PROBS:
            assert L.misti_bands_rank(n, p, C.byref(lo), C.byref(hi), C.byref(g)) == 0
            h = float(n - 1) * p
            i, w = int(math.floor(h)), h - math.floor(h)
            assert bits(g.value) == bits(w), (n, p)
            if w == 0.0 or i >= n - 1:
                assert lo.value == hi.value == min(i, n - 1), (n, p)
            else:
                assert (lo.value, hi.value) == (i, i + 1), (n, p)
            assert bands_rank(n, p) == (lo.value, hi.value, g.value)
            assert 0 <= lo.value <= hi.value <= n - 1
    why = lambda: L.misti_last_error().decode()
    assert L.misti_bands_rank(0, 0.5, C.byref(lo), C.byref(hi), C.byref(g)) == E_ARG and "n must be >= 1" in why()
    for p in (-0.1, 1.0000001, NAN):
        assert L.misti_bands_rank(5, p, C.byref(lo), C.byref(hi), C.byref(g)) == E_ARG and "not in [0, 1]" in why()
    assert L.misti_bands_rank(5, 0.5, None, C.byref(hi), C.byref(g)) == E_ARG and "NULL" in why()


# ---- the argument checks: before the first HIP call, in the header's order --------------------------------------------------------------
def bands(door="dev", G=1, m=4, size=None, n_prob=None, probs=(0.5,), null=(), workspace_bytes=0, batch_limit=0, inputs=8, desc=True):
    from misti_amd import _lib
    pr = np.asarray(probs, dtype=np.float64)
    b = _lib.Bands(size=C.sizeof(_lib.Bands) if size is None else size, n_prob=pr.size if n_prob is None else n_prob,
                   probs=None if "probs" in null else pr.ctypes.data, workspace_bytes=workspace_bytes, batch_limit=batch_limit)
    at = C.c_void_p(inputs) if inputs else None
    d = C.byref(b) if desc else None
    L = lib()
    rc = L.misti_traj_bands_dev(None, G, m, at, at, None, d) if door == "dev" else L.misti_traj_bands(None, G, m, at, at, None, None, d)
    return rc, L.misti_last_error().decode()


@pytest.mark.parametrize("door", ["dev", "host"])
@pytest.mark.parametrize("kw, code, word", [
    (dict(desc=False), E_ARG, "the bands descriptor is NULL"),
    (dict(size=8), E_ARG, "the bands descriptor's size is 8, this library's misti_bands_t has"),
    (dict(n_prob=0), E_ARG, "n_prob must be 1 ... 8 (got 0)"),
    (dict(n_prob=9), E_ARG, "n_prob must be 1 ... 8 (got 9)"),
    (dict(null=("probs",)), E_ARG, "probs is NULL"),
    (dict(probs=(0.5, -0.1)), E_ARG, "probs[1] = -0.1 is not in [0, 1]"),
    (dict(probs=(1.0000001,)), E_ARG, "probs[0]"),
    (dict(probs=(0.1, 0.2, NAN)), E_ARG, "probs[2]"),
    (dict(workspace_bytes=-1), E_ARG, "must not be negative"),
    (dict(batch_limit=-1), E_ARG, "must not be negative"),
    (dict(G=-1), E_ARG, "negative number of groups, or no sample (G = -1, m = 4)"),
    (dict(m=0), E_ARG, "negative number of groups, or no sample (G = 1, m = 0)"),
    (dict(inputs=0), E_ARG, "NULL"),
    (dict(), E_ARG, "ctx is NULL"),
    (dict(G=0, inputs=0), E_ARG, "ctx is NULL"),                            # G == 0 needs no input: the next refusal is the context's
    # the header's order: of two faults the earlier one is named
    (dict(size=8, n_prob=0), E_ARG, "size"),
    (dict(n_prob=0, null=("probs",)), E_ARG, "n_prob"),
    (dict(null=("probs",), G=-1), E_ARG, "probs is NULL"),
    (dict(probs=(2.0,), workspace_bytes=-1), E_ARG, "probs[0]"),
    (dict(workspace_bytes=-1, G=-1), E_ARG, "must not be negative"),
    (dict(G=-1, inputs=0), E_ARG, "negative number of groups"),
    (dict(m=0, inputs=0), E_ARG, "no sample"),
])
def test_bands_argument_checks(door, kw, code, word):
    rc, why = bands(door, **kw)
    assert rc == code and word in why, (rc, why)


# ---- header, binding, build lists ----------------------------------------------------------------------------------------------------------
def test_header_binding_and_build_lists_agree():
    from misti_amd import _lib, build, optimize
    hdr = open(os.path.join(ROOT, "include", "misti_hip.h")).read()
    assert lib().misti_abi_version() == _lib.ABI_VERSION
    body = hdr[:hdr.index("} misti_bands_t;")].rsplit("typedef struct {", 1)[1]
    names = [n for line in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", line.strip())]
    assert names == [n for n, _ in _lib.Bands._fields_], names
    assert names == ["size", "n_prob", "probs", "count", "mean", "quant", "lo", "hi", "workspace_bytes", "batch_limit"]
    assert C.sizeof(_lib.Bands) == 72
    bands_h = open(os.path.join(ROOT, "misti_amd", "csrc", "misti_bands.h")).read()
    assert _lib.BANDS_TILE == int(re.search(r"constexpr int BANDS_TILE = (\d+);", bands_h).group(1)) == 64
    assert _lib.BANDS_TILE * (_lib.BANDS_TILE + 1) * 8 <= 64 * 1024            # the padded tile fits the LDS a workgroup may have
    assert {"misti_bands.hip", "misti_bands.cpp"} <= set(build.SOURCES) and "misti_bands.h" in build.HEADERS
    for name in ("misti_traj_bands_dev", "misti_traj_bands"):
        assert name in _lib.SYMBOLS and re.search(r"^int %s\(misti_ctx\* ctx, int64_t G, int64_t m, " % name, hdr, flags=re.M) and hasattr(lib(), name)
    assert "misti_bands_rank" in _lib.SYMBOLS and re.search(r"^int misti_bands_rank\(int64_t n, double p, ", hdr, flags=re.M)
    assert "optimize.trajectory_bands_rule" in hdr and "MigrationInference.py:89-99" in hdr and "RATES, not sizes" in hdr
    assert "RATES" in optimize.trajectory_bands_rule.__doc__
    # the older descriptors did not move
    assert (C.sizeof(_lib.EnsPost), C.sizeof(_lib.EnsSample), C.sizeof(_lib.PtSample), C.sizeof(_lib.Prior)) == (144, 192, 240, 40)


def test_table_of_one_group():
    from misti_amd.optimize import trajectory_bands_rule, trajectory_bands_table
    lc, split, status = edge_inputs()
    r = trajectory_bands_rule(lc[0], split[0], status[0], (0.1, 0.9))
    rows = trajectory_bands_table(r, [0.5, 1.0, 2.0])
    assert [row["interval"] for row in rows] == [0, 1, 2, 3] and [row["time"] for row in rows] == [0.0, 0.5, 1.0, 2.0]
    assert rows[1]["count"].tolist() == [5, 6] and same_bits(rows[3]["quant"], r["quant"][3])
    with pytest.raises(ValueError):
        trajectory_bands_table(trajectory_bands_rule(lc, split, status), [0.5, 1.0, 2.0])


# ---- the command line ------------------------------------------------------------------------------------------------------------------------
BASE = ["a.psmc", "b.psmc", "d.sfs", "20"]
SOLVE = ["--grid-solve", "--grid-st", "15", "17", "-mi", "1", "4", "16", "0.2", "1", "-mi", "2", "4", "16", "0.3", "1", "--box", "0", "0.01", "5", "--box", "1", "0.01", "5"]
FIT = ["--fit-st", "-mi", "1", "4", "16", "0.2", "1", "--box", "0", "0.01", "5", "--box", "st", "10", "19"]


def test_parser_accepts_the_bands_options():
    from misti_amd import cli
    parse = lambda args: cli.build_parser().parse_args(BASE + args)
    for mode in (SOLVE, FIT):
        for more in ([], ["--hops", "3"], ["--de", "8", "5"]):
            a = parse(mode + ["--all-bs", "--bands"] + more)
            assert cli.bands_error(a) is None and cli._probs(a.bands) == (0.025, 0.5, 0.975), more
    a = parse(FIT + ["--all-bs", "--bands", "0.1", "0.5", "0.9", "--bands-out", "b.npz"])
    assert cli.bands_error(a) is None and cli._probs(a.bands) == (0.1, 0.5, 0.9) and a.bands_out == "b.npz"
    a = parse(FIT)
    assert a.bands is None and a.mcmc_bands is None and cli.bands_error(a) is None and cli.mcmc_error(a) is None
    for more in ([], ["--mcmc-post"], ["--mcmc-ladder", "2", "4"], ["--mcmc-log", "0"], ["--mcmc-prior", "0", "exponential", "1"], ["--mcmc-out", "c.npz"]):
        a = parse(FIT + ["--mcmc", "8", "50", "--mcmc-bands"] + more)
        assert cli.mcmc_error(a) is None and cli._probs(a.mcmc_bands) == (0.025, 0.5, 0.975), more
    a = parse(SOLVE + ["--mcmc", "8", "50", "--mcmc-bands", "0.25", "0.75", "--mcmc-bands-thin", "3"])
    assert cli.mcmc_error(a) is None and cli._probs(a.mcmc_bands) == (0.25, 0.75) and a.mcmc_bands_thin == 3


def test_bands_options_without_their_mode_are_argument_errors():
    from misti_amd import cli
    parse = lambda args: cli.build_parser().parse_args(BASE + args)
    for args, word in ((["--bands-out", "b.npz", "--all-bs"] + FIT, "belongs to --bands"),
                       (["--bands"] + FIT, "needs --all-bs"),
                       (["--bands", "--all-bs", "-mi", "1", "4", "16", "0.2", "1"], "--grid-solve or --fit-st"),
                       (["--bands", "1.5", "--all-bs"] + FIT, "[0, 1]"),
                       (["--bands"] + ["0.5"] * 9 + ["--all-bs"] + FIT, "at most 8"),
                       (["--bands", "--all-bs", "--devices", "0,1"] + FIT, "one GPU")):
        why = cli.bands_error(parse(args))
        assert why is not None and "--bands" in why and word in why, (args, why)
    for args, word in ((["--mcmc-bands"] + FIT, "give --mcmc W STEPS"),
                       (["--mcmc-bands-thin", "2"] + FIT, "give --mcmc W STEPS"),
                       (["--mcmc", "8", "50", "--mcmc-bands-thin", "2"] + FIT, "give it"),
                       (["--mcmc", "8", "50", "--mcmc-bands", "-0.1"] + FIT, "[0, 1]"),
                       (["--mcmc", "8", "50", "--mcmc-bands"] + ["0.5"] * 9 + FIT, "at most 8"),
                       (["--mcmc", "8", "50", "--mcmc-bands", "--mcmc-bands-thin", "0"] + FIT, "T >= 1")):
        why = cli.mcmc_error(parse(args))
        assert why is not None and "--mcmc-bands" in why and word in why, (args, why)
    for opt in ("--bands [P ...]", "--bands-out FILE.npz", "--mcmc-bands [P ...]", "--mcmc-bands-thin T"):
        assert opt in cli.__doc__, opt
    assert "RATES, not sizes" in cli.__doc__
