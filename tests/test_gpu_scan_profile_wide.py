"""misti_scan_profile_dev beyond 256 groups, where profile_offsets_kernel gives each of its 256 threads a RUN of ceil(n_group / 256)
groups: run lengths of 1, 2, 3 and 4 with a ragged last run and threads that have no group at all, and the limit
MISTI_SCAN_MAX_GROUPS = 65 535 (the gridDim.y of scan_profile_kernel) from the accepting side.  tests/test_gpu_scan_profile.py stops at
200 groups - one group per thread.  The reference is that module's: the table of misti_llk_dev on the same buffers, reduced by
optimize.profile_per_group; index and value bit for bit.  A run boundary that is off by one moves first[] for every group behind it,
and the groups then read their neighbours' members."""
import numpy as np
import pytest

from test_gpu_scan_profile import Buffers, check, counts, engine, same_bits, spectra

pytestmark = pytest.mark.gpu

N = 1500
GROUPS = (256, 257, 513, 1000)


def labels(rng, n, G):
    """Random labels that include -1 and G + 3: some candidates in no group, some groups empty."""
    group = rng.choice(np.concatenate([np.arange(G), [-1, G + 3]]), size=n)
    group[rng.choice(n, size=2, replace=False)] = -1, G + 3
    return group


@pytest.mark.parametrize("unfolded", [False, True], ids=["folded", "unfolded"])
def test_more_groups_than_threads_of_the_offsets_scan(unfolded):
    """test_every_shape_equals_the_reduced_table's recipe with 1 500 candidates in 256 groups (a run of 1, every thread busy), 257 (runs
    of 2, the last of them ragged, 127 threads without a group), 513 (runs of 3) and 1 000 (runs of 4; most groups hold one or two
    members and some none), for 3 and 257 replicates; a tenth of the candidates without a value."""
    rng = np.random.default_rng(61 + unfolded)
    with engine(unfolded) as e:
        for R in (3, 257):
            status = (rng.random(N) < 0.1).astype(np.int32) * 2
            buf = Buffers(e, spectra(rng, N), status, counts(rng, R))
            table = buf.table()
            assert np.isneginf(table[status != 0]).all() and np.isfinite(table[status == 0]).all()
            for G in GROUPS:
                group = labels(rng, N, G)
                assert (group == -1).any() and (group == G + 3).any()
                _, val, best = check(buf, group, G, (R, G), table)
                size = np.bincount(group[(group >= 0) & (group < G)], minlength=G)
                assert np.isneginf(val[:, size == 0]).all() and (best[:, size == 0] == -1).all()
                if G == 1000:
                    assert (size == 0).sum() > 50 and ((size == 1) | (size == 2)).sum() > G // 2


def test_runs_of_three_groups_under_every_slice_count(monkeypatch):
    """513 groups under MISTI_SCAN_SLICES (read once per context) = 1, 7 and the library's own choice: one result, the reduced table's."""
    from misti_amd.optimize import profile_per_group
    rng = np.random.default_rng(63)
    G = 513
    jafs, rows = spectra(rng, N), counts(rng, 3)
    status = (rng.random(N) < 0.1).astype(np.int32) * 2
    group = labels(rng, N, G)
    got = {}
    for slices in ("1", "7", None):
        if slices is None:
            monkeypatch.delenv("MISTI_SCAN_SLICES")
        else:
            monkeypatch.setenv("MISTI_SCAN_SLICES", slices)
        with engine() as e:
            buf = Buffers(e, jafs, status, rows)
            got[slices] = buf.profile(group, G)
            if slices == "1":
                table = buf.table()
    want_val, want = profile_per_group(table, group, G)
    for slices, (val, best) in got.items():
        assert np.array_equal(best, want) and same_bits(val, want_val), slices


def test_the_largest_number_of_groups():
    """MISTI_SCAN_MAX_GROUPS = 65 535 groups (runs of 256, the last of 255), 70 000 candidates, 2 replicates: label c % 65 535, so
    that the first 4 465 groups hold two members and the others one, but for 300 candidates at -1 - among them both members of some
    groups, which are then empty - and a tenth without a value; prof_best wanted and NULL."""
    rng = np.random.default_rng(65)
    G, n, R = 65535, 70000, 2
    group = np.arange(n) % G
    out = np.concatenate([rng.choice(n, size=290, replace=False), [7, 7 + G, 4000, 4000 + G, 65534]])
    group[out] = -1
    status = (rng.random(n) < 0.1).astype(np.int32) * 2
    with engine() as e:
        buf = Buffers(e, spectra(rng, n), status, counts(rng, R))
        table, val, best = check(buf, group, G, "limit")
        val2, best2 = buf.profile(group, G, want_best=False)
    assert same_bits(val2, val) and (best2 == -7).all()
    for g in (7, 4000, 65534):                                             # every member at -1: empty
        assert np.isneginf(val[:, g]).all() and (best[:, g] == -1).all()
    has = best >= 0
    assert has.mean() > 0.85 and (group[best[has]] == np.broadcast_to(np.arange(G), best.shape)[has]).all()
    assert (best[has] >= G).sum() > 1000                                   # second members win their share
