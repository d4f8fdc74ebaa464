"""Trajectory bands on the device - misti_traj_bands_dev through Engine.trajectory_bands_dev - against optimize.trajectory_bands_rule, bit
for bit, on synthetic lc tensors the test uploads itself: no engine evaluation, so the shapes stay tiny.

With T = _lib.POST_SORT_TILE = 2048, m takes every value of {1, 2, 63, 64, 65, T - 1, T, T + 1, 2 T + 1, 3 T + 1} (one sample; around a
wave and the gather's tile of 64; around the sort's tile; a short last run in the first and in the second merge pass) at numT = 20, and
numT every value of {2, 20, 128, 255} at m = 65 and m = T + 1.  The issue names numT = 1 as the smallest; misti_create refuses a grid
below two intervals (test_the_smallest_grid says so), so the smallest context there is has numT = 2.  G in {1, 3}, n_prob in {1, 8}."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POISON = 1e300
OUTPUTS = ("count", "mean", "quant", "lo", "hi")
PROBS8 = (0.0, 1.0, 0.5, 0.025, 1.0 / 3.0, math.nextafter(1.0, 0.0), 0.25, 0.975)


def tile():
    from misti_amd import _lib
    return _lib.POST_SORT_TILE


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


_ENGINES = {}


@pytest.fixture(scope="module")
def engine_of():
    """A synthetic context per numT: the reduction reads numT alone."""
    from misti_amd.engine import Engine
    def get(numT):
        if numT not in _ENGINES:
            _ENGINES[numT] = Engine(np.arange(1, numT) * 0.1, np.ones((numT, 2)))
        return _ENGINES[numT]
    yield get
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def reduce_dev(eng, lc, split, status, probs, want=None, **kw):
    out = eng.trajectory_bands_dev(on_device(lc), on_device(split), None if status is None else on_device(status), probs=probs, want=want, **kw)
    eng.sync()
    return {k: v.cpu().numpy() for k, v in out.items() if k in OUTPUTS}


def assert_rule(dev, ref, names=OUTPUTS, where=""):
    for k in names:
        if not same_bits(dev[k], ref[k]):
            kind = np.int64 if dev[k].dtype == np.float64 else np.int32
            bad = np.argwhere(np.ascontiguousarray(dev[k]).view(kind) != np.ascontiguousarray(ref[k]).view(kind))
            print(where, k, "differs at", bad[:5].tolist(), "device", dev[k][tuple(bad[0])], "rule", ref[k][tuple(bad[0])])
        assert same_bits(dev[k], ref[k]), (where, k)


FLAVOURS = ("random", "dups", "signs", "sorted", "reverse", "nonfinite")


def synthetic(case, G, m, numT):
    """lc[G][m][numT + 1][2], split[G][m], status[G][m]: every group another flavour of values, splits fractional and whole mixed (some
    at 0 and below: members of nothing; some at numT and above: members of everything), a sixth of the samples failed, a few NaN values,
    row numT poisoned."""
    rng = np.random.default_rng(900 + case)
    shape = (m, numT + 1, 2)
    lcs = []
    for g in range(G):
        kind = FLAVOURS[(case + g) % len(FLAVOURS)]
        if kind == "dups":                                       # long runs of equal keys across every tile boundary and merge cut
            v = rng.choice(np.array([1.5, 0.25, 1e-3, 7.0, 0.5]), size=shape)
        elif kind == "signs":
            v = rng.choice(np.array([0.0, -0.0, 1.75, -1.75, 2.0 ** -1074, -2.0 ** -1074]), size=shape)
        elif kind in ("sorted", "reverse"):
            v = np.sort(np.exp(rng.standard_normal(shape)), axis=0)
            v = np.ascontiguousarray(v if kind == "sorted" else v[::-1])
        else:
            v = np.exp(rng.standard_normal(shape) * 3.0)
            if kind == "nonfinite":
                v[rng.random(shape) < 0.01] = np.inf
                v[rng.random(shape) < 0.01] = -np.inf
        v[rng.random(shape) < 0.01] = np.nan
        lcs.append(v)
    lc = np.stack(lcs)
    lc[:, :, numT, :] = POISON
    split = rng.uniform(-0.5, numT + 1.0, size=(G, m))
    whole = rng.random((G, m)) < 0.4
    split[whole] = np.floor(split[whole])
    split[rng.random((G, m)) < 0.25] = float(numT)               # a good share of full members, so that the high intervals are not empty
    status = (rng.random((G, m)) < 1.0 / 6.0).astype(np.int32) * rng.integers(1, 7, size=(G, m)).astype(np.int32)
    return lc, split, status


def cases():
    T = tile()
    out = []
    for i, m in enumerate((1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 3 * T + 1)):
        out.append((m, 20, (1, 3)[i % 2], (1, 8)[(i // 2) % 2]))
    for i, numT in enumerate((2, 128, 255)):
        out.append((65, numT, (3, 1)[i % 2], (8, 1)[i % 2]))
    out += [(T + 1, 2, 3, 8), (T + 1, 128, 1, 1), (T + 1, 255, 1, 8)]
    return out


CASES = cases()


def test_the_issues_sizes_are_covered():
    assert tile() == 2048
    assert {c[0] for c in CASES} == {1, 2, 63, 64, 65, 2047, 2048, 2049, 4097, 6145}
    assert {c[1] for c in CASES if c[0] == 65} == {2, 20, 128, 255} == {c[1] for c in CASES if c[0] == 2049}
    assert {c[2] for c in CASES} == {1, 3} and {c[3] for c in CASES} == {1, 8}


def test_the_smallest_grid():
    """numT = 1 of the issue's list cannot exist: the library refuses a grid below two intervals, as it always did."""
    from misti_amd import _lib
    from misti_amd.engine import Engine
    with pytest.raises(_lib.MistiError) as e:
        Engine(np.zeros(0), np.ones((1, 2)))
    assert e.value.code == -1 and "numT must be >= 2" in str(e.value)


@pytest.mark.parametrize("case", range(len(CASES)), ids=["m%d-T%d-G%d-P%d" % c for c in CASES])
def test_device_equals_the_rule(engine_of, case):
    from misti_amd.optimize import trajectory_bands_rule
    m, numT, G, P = CASES[case]
    lc, split, status = synthetic(case, G, m, numT)
    probs = PROBS8[:P] if P > 1 else (0.5,)
    ref = trajectory_bands_rule(lc, split, status, probs)
    dev = reduce_dev(engine_of(numT), lc, split, status, probs)
    assert_rule(dev, ref, where=str(CASES[case]))
    assert ref["count"].max() > 0 and (m < 64 or ref["count"].max() > m // 4)            # the case is not empty
    for k in ("mean", "quant", "lo", "hi"):
        v = dev[k][np.isfinite(dev[k])]
        assert not np.any(np.abs(v) >= 1e290), k                                             # row numT is never read


def edge_inputs():
    """tests/test_bands_cpu.py's membership edges: one group, numT = 4, m = 8."""
    numT, m = 4, 8
    lc = np.full((1, m, numT + 1, 2), 2.0)
    lc[0, :, :, 1] = np.arange(1.0, m + 1.0)[:, None]
    lc[0, :, numT, :] = POISON
    split = np.array([[2.0, math.nextafter(2.0, math.inf), np.nan, 4.0, 4.0, 4.0, 4.0, 3.5]])
    status = np.array([[0, 0, 0, 5, 0, 0, 0, 0]], dtype=np.int32)
    lc[0, 4, 1, 0] = np.nan
    lc[0, 5, 0, 0], lc[0, 6, 0, 0] = 0.0, -0.0
    lc[0, 5, 3, 1], lc[0, 6, 3, 1] = np.inf, -np.inf
    return lc, split, status


def test_membership_edges_on_the_device(engine_of):
    from misti_amd.optimize import trajectory_bands_rule
    lc, split, status = edge_inputs()
    probs = (0.0, 0.5, 1.0, 0.3)
    for st in (status, None):
        dev = reduce_dev(engine_of(4), lc, split, st, probs)
        assert_rule(dev, trajectory_bands_rule(lc, split, st, probs), where="edges")
    assert dev["count"][0].tolist() == [[7, 7], [6, 7], [6, 6], [5, 5]]                       # without the status
    dev = reduce_dev(engine_of(4), lc, split, status, probs)
    assert dev["count"][0].tolist() == [[6, 6], [5, 6], [5, 5], [4, 4]]
    assert np.signbit(dev["lo"][0, 0, 0]) and dev["lo"][0, 0, 0] == 0.0 and dev["lo"][0, 3, 1] == -np.inf and dev["hi"][0, 3, 1] == np.inf
    assert dev["mean"][0, 3, 1:].view(np.int64).tolist() == [0x7ff8000000000000]


def test_empty_series_beside_full_ones(engine_of):
    """n == 0, n == 1 and all values equal, in the same launch as full series - at a size with several sort tiles."""
    from misti_amd.optimize import trajectory_bands_rule
    numT, m, G = 20, tile() + 7, 3
    lc, split, status = synthetic(77, G, m, numT)
    split[0, :] = 5.0                                            # group 0: nothing at and above interval 5
    split[1, :] = 0.0                                            # group 1: no member anywhere
    split[1, m // 2] = 1.0                                       # ... but one sample at interval 0
    status[1, m // 2] = 0
    lc[1, m // 2, 0, :] = 0.625
    lc[2, :, 7, 0] = 3.5                                         # all values equal
    ref = trajectory_bands_rule(lc, split, status, (0.1, 0.5))
    dev = reduce_dev(engine_of(numT), lc, split, status, (0.1, 0.5))
    assert_rule(dev, ref, where="empty")
    assert not dev["count"][0, 5:].any() and dev["count"][0, :5].all() and dev["count"][1].tolist() == [[1, 1]] + [[0, 0]] * (numT - 1)
    assert np.isnan(dev["mean"][1, 1:]).all() and dev["quant"][1, 0].tolist() == [[0.625, 0.625]] * 2
    assert set(dev["quant"][2, 7, 0].tolist()) == {3.5} and dev["mean"][2, 7, 0] == 3.5


def test_ties_across_tile_boundaries(engine_of):
    """Two values only, their runs cut by every tile boundary of the gather and of the sort, and every merge cut inside a run."""
    from misti_amd.optimize import trajectory_bands_rule
    numT, m = 2, 3 * tile() + 1
    rng = np.random.default_rng(5)
    lc = rng.choice(np.array([0.5, 0.25]), size=(1, m, numT + 1, 2))
    lc[0, :, 1, 0] = 0.5
    lc[0, tile() - 1:tile() + 1, 1, 0] = 0.25                    # two small keys astride the first tile boundary
    lc[:, :, numT, :] = POISON
    split = np.full((1, m), 2.0)
    ref = trajectory_bands_rule(lc, split, None, PROBS8)
    dev = reduce_dev(engine_of(numT), lc, split, None, PROBS8)
    assert_rule(dev, ref, where="ties")
    assert dev["count"].tolist() == [[[m, m], [m, m]]] and dev["lo"][0, 1, 0] == 0.25 and dev["hi"][0, 1, 0] == 0.5


def test_each_output_alone_and_the_sentinels(engine_of):
    """Every output alone, the others NULL, equals the same output when all are computed; a guard behind each output buffer stays."""
    import ctypes as C
    import torch
    from misti_amd import _lib
    numT, m, G = 20, tile() + 1, 3
    eng = engine_of(numT)
    lc, split, status = synthetic(31, G, m, numT)
    probs = (0.025, 0.5, 0.975)
    full = reduce_dev(eng, lc, split, status, probs)
    for k in OUTPUTS:
        alone = reduce_dev(eng, lc, split, status, probs, want=(k,))
        assert set(alone) == {k} and same_bits(alone[k], full[k]), k
    # the raw entry with guarded buffers
    d_lc, d_split, d_status = on_device(lc), on_device(split), on_device(status)
    n = G * numT * 2
    sizes = dict(count=n, mean=n, quant=n * len(probs), lo=n, hi=n)
    GUARD = 64
    bufs = {}
    for k, cnt in sizes.items():
        if k == "count":
            bufs[k] = torch.full((cnt + GUARD,), -77, dtype=torch.int32, device="cuda")
        else:
            bufs[k] = torch.full((cnt + GUARD,), -7.75, dtype=torch.float64, device="cuda")
    pr = np.asarray(probs, dtype=np.float64)
    torch.cuda.synchronize()                                     # the fills ran on torch's stream, the library has its own
    b = _lib.Bands(size=C.sizeof(_lib.Bands), n_prob=pr.size, probs=pr.ctypes.data, **{k: v.data_ptr() for k, v in bufs.items()})
    _lib.check(eng._lib.misti_traj_bands_dev(eng._ctx, G, m, C.c_void_p(d_lc.data_ptr()), C.c_void_p(d_split.data_ptr()), C.c_void_p(d_status.data_ptr()), C.byref(b)))
    eng.sync()
    for k, cnt in sizes.items():
        host = bufs[k].cpu().numpy()
        assert same_bits(host[:cnt].reshape(full[k].shape), full[k]), k
        assert (host[cnt:] == (-77 if k == "count" else -7.75)).all(), k


def test_determinism_and_the_workspace_bound(engine_of):
    """Two calls give identical bits; so does a workspace that holds one group per pass."""
    numT, m, G = 20, 2 * tile() + 1, 3
    eng = engine_of(numT)
    lc, split, status = synthetic(41, G, m, numT)
    a = reduce_dev(eng, lc, split, status, PROBS8)
    b = reduce_dev(eng, lc, split, status, PROBS8)
    c = reduce_dev(eng, lc, split, status, PROBS8, workspace_bytes=1)
    for k in OUTPUTS:
        assert same_bits(a[k], b[k]) and same_bits(a[k], c[k]), k


def test_no_group_writes_nothing(engine_of):
    import torch
    eng = engine_of(20)
    out = eng.trajectory_bands_dev(torch.empty((0, 5, 21, 2), dtype=torch.float64, device="cuda"), torch.empty((0, 5), dtype=torch.float64, device="cuda"))
    eng.sync()
    assert out["count"].shape == (0, 20, 2) and out["quant"].shape == (0, 20, 2, 3)


def test_sizes_beyond_the_launch_indices_are_refused_before_any_launch(engine_of):
    """The MISTI_E_LIMIT refusals sit behind the context: dummy pointers, nothing is launched or allocated."""
    import ctypes as C
    from misti_amd import _lib
    eng = engine_of(20)
    pr = np.array([0.5])
    b = _lib.Bands(size=C.sizeof(_lib.Bands), n_prob=1, probs=pr.ctypes.data, count=8)
    at = C.c_void_p(8)
    why = lambda: eng._lib.misti_last_error().decode()
    big = (2 ** 31 - 1) // 8 + 1
    assert eng._lib.misti_traj_bands_dev(eng._ctx, 1, big, at, at, None, C.byref(b)) == -4 and "samples per group exceed INT32_MAX / 8" in why()
    assert eng._lib.misti_traj_bands_dev(eng._ctx, 3, big // 2, at, at, None, C.byref(b)) == -4 and "G x m" in why()
    assert eng._lib.misti_traj_bands(eng._ctx, 1, big, None, at, None, None, C.byref(b)) == -4 and "INT32_MAX / 8" in why()


def test_a_host_tensor_is_refused_in_python(engine_of):
    import torch
    eng = engine_of(20)
    lc, split = torch.ones((1, 4, 21, 2), dtype=torch.float64), torch.full((1, 4), 20.0, dtype=torch.float64)
    for args in ((lc, split.cuda()), (lc.cuda(), split), (lc.cuda(), split.cuda(), torch.zeros((1, 4), dtype=torch.int32))):
        with pytest.raises(ValueError, match="CUDA tensor"):
            eng.trajectory_bands_dev(*args)
