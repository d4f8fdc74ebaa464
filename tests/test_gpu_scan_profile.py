"""The profile likelihood per group and replicate without the likelihood table (misti_scan_profile_dev, optimize.scan_profile,
`--profile AXIS [AXIS]`).  The reference everywhere is the table itself - misti_llk_dev on the same buffers, or Engine.evaluate -
reduced on the host by optimize.profile_per_group: indices equal, values bit for bit."""
import io
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NINF = -np.inf


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def grid():
    from misti_amd import synth, io as mio
    return mio.merge_psmc(mio.read_psmc_file(io.StringIO(synth.psmc_text(16, 1, synth.THETA_1))),
                          mio.read_psmc_file(io.StringIO(synth.psmc_text(17, 2, synth.THETA_2))))


def engine(unfolded=False):
    from misti_amd.engine import Engine
    inp = grid()
    return Engine(inp.times, inp.lambdas, unfolded=unfolded)


def spectra(rng, n):
    j = rng.random((n, 7)) + 0.05
    return j / j.sum(axis=1, keepdims=True)


def counts(rng, R):
    rows = np.zeros((R, 8))
    rows[:, 1:] = rng.integers(0, 50000, size=(R, 7))
    rows[:, 0] = rows[:, 1:].sum(axis=1)
    return rows


class Buffers:
    """Hand-made spectra, statuses and rows on the device, the table misti_llk_dev makes of them and the profile of them."""

    def __init__(self, e, jafs, status, rows):
        import torch
        self.e, self.torch, self.dev = e, torch, torch.device("cuda", 0)
        self.n, self.R = jafs.shape[0], rows.shape[0]
        self.jafs = torch.as_tensor(np.ascontiguousarray(jafs, dtype=np.float64), device=self.dev)
        self.status = None if status is None else torch.as_tensor(np.ascontiguousarray(status, dtype=np.int32), device=self.dev)
        self.rows = torch.as_tensor(np.ascontiguousarray(rows, dtype=np.float64), device=self.dev)
        torch.cuda.synchronize()                      # the engine issues on its own non-blocking stream

    def ptr_status(self):
        return self.status.data_ptr() if self.status is not None else 0

    def table(self):
        out = self.torch.full((self.n, self.R), float("nan"), dtype=self.torch.float64, device=self.dev)
        self.torch.cuda.synchronize()
        self.e.llk_dev(self.n, self.jafs.data_ptr(), self.ptr_status(), self.R, self.rows.data_ptr(), out.data_ptr())
        self.e.sync()
        self.d_table = out
        return out.cpu().numpy()

    def profile(self, group, n_group, want_best=True):
        """Outputs pre-filled with sentinels, and a guard allocated right behind them: an overrun would show there."""
        t = self.torch
        d_group = t.as_tensor(np.ascontiguousarray(group, dtype=np.int32), device=self.dev)
        val = t.full((self.R, n_group), 7.0, dtype=t.float64, device=self.dev)
        guard_v = t.full((64,), 7.0, dtype=t.float64, device=self.dev)
        best = t.full((self.R, n_group), -7, dtype=t.int32, device=self.dev)
        guard_i = t.full((64,), -7, dtype=t.int32, device=self.dev)
        t.cuda.synchronize()
        self.e.scan_profile_dev(self.n, self.jafs.data_ptr(), self.ptr_status(), d_group.data_ptr(), n_group, self.R, self.rows.data_ptr(),
                                val.data_ptr(), best.data_ptr() if want_best else 0)
        self.e.sync()
        assert float(guard_v.sum().item()) == 64 * 7.0 and int(guard_i.sum().item()) == 64 * -7
        return val.cpu().numpy(), best.cpu().numpy().astype(np.int64)


def check(buf, group, n_group, tag, table=None):
    from misti_amd.optimize import profile_per_group
    table = buf.table() if table is None else table
    val, best = buf.profile(group, n_group)
    want_val, want = profile_per_group(table, group, n_group)
    assert np.array_equal(best, want), tag
    assert same_bits(val, want_val), tag
    return table, val, best


# ---- the kernel alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unfolded", [False, True], ids=["folded", "unfolded"])
def test_every_shape_equals_the_reduced_table(unfolded):
    """One replicate, odd and even widths and a workgroup boundary (256 replicates, which is also a boundary of the merge's 32-row
    tiles), the LDS chunk boundary (64 candidates), one group, a few, as many as candidates; random labels that include -1 and
    n_group + 3, so that some candidates are in no group and some groups are empty; a tenth of the candidates without a value."""
    rng = np.random.default_rng(41 + unfolded)
    with engine(unfolded) as e:
        for R in (1, 2, 255, 256, 257):
            rows = counts(rng, R)
            for n in (1, 5, 63, 64, 65, 200):
                status = (rng.random(n) < 0.1).astype(np.int32) * 2
                buf = Buffers(e, spectra(rng, n), status, rows)
                table = buf.table()
                assert np.isneginf(table[status != 0]).all() and np.isfinite(table[status == 0]).all()
                for G in sorted({1, 2, 7, n}):
                    group = rng.choice(np.concatenate([np.arange(G), [-1, G + 3]]), size=n)
                    check(buf, group, G, (R, n, G), table)
        # status NULL: every candidate has a value; prof_best NULL: only the values, and the index buffer is left alone
        buf = Buffers(e, spectra(rng, 65), None, counts(rng, 3))
        group = rng.integers(0, 4, size=65)
        table, val, best = check(buf, group, 4, "no status")
        assert np.isfinite(table).all() and (best >= 0).all()
        val2, best2 = buf.profile(group, 4, want_best=False)
        assert same_bits(val2, val) and (best2 == -7).all()


def test_group_sizes_at_the_chunk_boundary():
    """Groups of exactly 63, 64 and 65 members (one chunk less one, one chunk, one chunk and one), of 1 and of 0 members, their
    member indices interleaved so that the gather through the member list is not contiguous."""
    rng = np.random.default_rng(43)
    group = np.concatenate([np.full(63, 0), np.full(64, 1), np.full(65, 2), np.full(1, 3)])       # group 4 has no member
    rng.shuffle(group)
    n = group.size
    assert n == 193 and [int((group == g).sum()) for g in range(5)] == [63, 64, 65, 1, 0]
    status = (rng.random(n) < 0.1).astype(np.int32) * 4
    with engine() as e:
        buf = Buffers(e, spectra(rng, n), status, counts(rng, 70))
        table, val, best = check(buf, group, 5, "chunk boundary")
    assert np.isneginf(val[:, 4]).all() and (best[:, 4] == -1).all()
    lone = int(np.where(group == 3)[0][0])
    assert (best[:, 3] == (lone if status[lone] == 0 else -1)).all()


def test_the_result_does_not_move_with_the_slice_count(monkeypatch):
    """MISTI_SCAN_SLICES (read once per context) cuts every group's member list into 1, 2 and 7 slices: one result.  200 candidates
    in 3 groups of unequal size (120, 65 and 15: 15 members in 7 slices of 3 leave the last two slices of that group without a
    member), every spectrum present three times, so that ties cross groups and cuts."""
    from misti_amd.optimize import profile_per_group
    rng = np.random.default_rng(45)
    base = spectra(rng, 67)
    jafs = np.vstack([base, base, base])[:200]
    group = np.concatenate([np.full(120, 0), np.full(65, 1), np.full(15, 2)])
    rng.shuffle(group)
    status = (rng.random(200) < 0.1).astype(np.int32)
    rows = counts(rng, 257)
    got = {}
    for slices in ("1", "2", "7", None):
        if slices is None:
            monkeypatch.delenv("MISTI_SCAN_SLICES")
        else:
            monkeypatch.setenv("MISTI_SCAN_SLICES", slices)
        with engine() as e:
            buf = Buffers(e, jafs, status, rows)
            got[slices] = buf.profile(group, 3)
            if slices == "1":
                table = buf.table()
    want_val, want = profile_per_group(table, group, 3)
    for slices in ("1", "2", "7", None):
        val, best = got[slices]
        assert np.array_equal(best, want) and same_bits(val, want_val), slices


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_equal_values_go_to_the_lowest_index(order):
    """Every spectrum appears twelve times over 600 candidates (three workgroups of the scatter, whose order of arrival in the
    member lists is not defined, and several slices), in 4 groups whose labels run with the candidate index or against it: whichever
    position of its member list holds the lowest index of a tie, that index is reported."""
    rng = np.random.default_rng(47)
    n = 600
    jafs = spectra(rng, 50)[np.arange(n) % 50]
    label = np.arange(n) % 4 if order == "ascending" else (n - 1 - np.arange(n)) // 150
    with engine() as e:
        buf = Buffers(e, jafs, None, counts(rng, 33))
        table, val, best = check(buf, label, 4, order)
    for r in range(best.shape[0]):
        for g in range(4):
            members = np.where(label == g)[0]
            ties = members[table[members, r] == val[r, g]]
            assert len(ties) >= 3 and best[r, g] == ties.min(), (r, g)


def test_identity_labels_are_the_table_and_one_group_is_the_scan():
    import torch
    from misti_amd.optimize import best_k_per_replicate
    rng = np.random.default_rng(49)
    n, R = 333, 300
    status = (rng.random(n) < 0.2).astype(np.int32) * 3
    rows = counts(rng, R)
    jafs = spectra(rng, n)
    jafs[100:200] = jafs[:100]                         # ties
    with engine() as e:
        buf = Buffers(e, jafs, status, rows)
        table = buf.table()
        # every candidate its own group: the transposed table, -inf / -1 where it has no value
        val, best = buf.profile(np.arange(n), n)
        assert same_bits(val, np.ascontiguousarray(table.T))
        assert np.array_equal(best, np.where(np.isneginf(table.T), -1, np.arange(n)[None, :]))
        # one group: misti_scan_best_dev with k = 1 and misti_argmax_dev of the table
        val, best = buf.profile(np.zeros(n), 1)
        s_best = torch.empty((R, 1), dtype=torch.int32, device=buf.dev)
        s_val = torch.empty((R, 1), dtype=torch.float64, device=buf.dev)
        a_best = torch.empty(R, dtype=torch.int32, device=buf.dev)
        a_val = torch.empty(R, dtype=torch.float64, device=buf.dev)
        torch.cuda.synchronize()
        e.scan_best_dev(n, buf.jafs.data_ptr(), buf.status.data_ptr(), R, buf.rows.data_ptr(), 1, s_best.data_ptr(), s_val.data_ptr())
        e.argmax_dev(n, R, buf.d_table.data_ptr(), a_best.data_ptr(), a_val.data_ptr())
        e.sync()
    assert np.array_equal(best[:, 0], s_best.cpu().numpy()[:, 0]) and same_bits(val, s_val.cpu().numpy())
    assert np.array_equal(best[:, 0], a_best.cpu().numpy()) and same_bits(val[:, 0], a_val.cpu().numpy())
    want, want_val = best_k_per_replicate(table, 1)
    assert np.array_equal(best, want) and same_bits(val, want_val)


def test_a_group_without_a_value_is_empty():
    rng = np.random.default_rng(51)
    n, R = 130, 5
    jafs, rows = spectra(rng, n), counts(rng, R)
    group = rng.integers(0, 3, size=n)
    status = np.where(group == 1, rng.integers(1, 7, size=n), 0).astype(np.int32)      # every member of group 1 has a status 1 ... 6
    with engine() as e:
        table, val, best = check(Buffers(e, jafs, status, rows), group, 3, "status")
        assert np.isneginf(val[:, 1]).all() and (best[:, 1] == -1).all()
        assert np.isfinite(val[:, [0, 2]]).all() and (group[best[:, 0]] == 0).all() and (group[best[:, 2]] == 2).all()
        # no candidate has a value at all
        val, best = Buffers(e, jafs, np.full(n, 5, dtype=np.int32), rows).profile(group, 3)
        assert np.isneginf(val).all() and (best == -1).all()


@pytest.mark.parametrize("unfolded", [False, True], ids=["folded", "unfolded"])
def test_zero_times_minus_infinity_never_wins_a_group(unfolded):
    """A spectrum with an empty class against a row with no count in it: 0 x log 0 is NaN in the table; against a row WITH a count
    there it is -inf.  Neither wins a group, and a group of such candidates alone is empty."""
    rng = np.random.default_rng(53)
    jafs = spectra(rng, 6)
    jafs[[1, 4], 3] = 0.0                              # class 3 stands alone folded and unfolded
    rows = counts(rng, 4)
    rows[[0, 2], 4] = 0.0                              # rows 0 and 2 have no count in it
    rows[:, 0] = rows[:, 1:].sum(axis=1)
    group = np.array([0, 0, 0, 2, 1, 2])               # group 0: the NaN / -inf candidate 1 among others; group 1: candidate 4 alone
    with engine(unfolded) as e:
        table, val, best = check(Buffers(e, jafs, None, rows), group, 3, "nan")
    assert np.isnan(table[[1, 4]][:, [0, 2]]).all() and np.isneginf(table[[1, 4]][:, [1, 3]]).all()
    assert np.isneginf(val[:, 1]).all() and (best[:, 1] == -1).all()
    assert np.isin(best[:, 0], [0, 2]).all() and np.isin(best[:, 2], [3, 5]).all() and np.isfinite(val[:, [0, 2]]).all()


def test_argument_errors_and_empty_calls():
    """Every refusal comes before anything touches the device; a call without replicates writes nothing; a call without candidates -
    every pointer but the outputs NULL, on a context that has launched nothing yet - fills -inf / -1 and nothing behind it."""
    import torch
    from misti_amd._lib import MistiError
    rng = np.random.default_rng(55)
    with engine() as e:
        buf = Buffers(e, spectra(rng, 5), None, counts(rng, 3))
        d_group = torch.zeros(5, dtype=torch.int32, device=buf.dev)
        out = torch.full((3 * 4,), 7.0, dtype=torch.float64, device=buf.dev)
        out_i = torch.full((3 * 4,), -7, dtype=torch.int32, device=buf.dev)
        torch.cuda.synchronize()
        j, g, r, o, oi = buf.jafs.data_ptr(), d_group.data_ptr(), buf.rows.data_ptr(), out.data_ptr(), out_i.data_ptr()

        def code(*args):
            with pytest.raises(MistiError) as err:
                e.scan_profile_dev(*args)
            return err.value.code

        assert code(5, j, 0, g, 0, 3, r, o, oi) == -1                     # n_group 0
        assert code(5, j, 0, g, -2, 3, r, o, oi) == -1
        assert code(5, j, 0, g, 65536, 3, r, o, oi) == -4                 # beyond MISTI_SCAN_MAX_GROUPS
        assert code(5, j, 0, 0, 2, 3, r, o, oi) == -1                     # d_group NULL
        assert code(5, j, 0, g, 2, 3, r, 0, oi) == -1                     # d_prof_llk NULL
        assert code(5, 0, 0, g, 2, 3, r, o, oi) == -1                     # d_jafs NULL
        assert code(5, j, 0, g, 2, 3, 0, o, oi) == -1                     # d_jsfs NULL
        assert code(-1, j, 0, g, 2, 3, r, o, oi) == -1
        assert code(5, j, 0, g, 2, -1, r, o, oi) == -1
        assert code(2 ** 31, j, 0, g, 2, 3, r, o, oi) == -4
        e.sync()
        assert (out.cpu().numpy() == 7.0).all() and (out_i.cpu().numpy() == -7).all()      # nothing touched the device
        # no replicate: nothing is written
        e.scan_profile_dev(5, j, 0, g, 4, 0, r, o, oi)
        e.sync()
        assert (out.cpu().numpy() == 7.0).all() and (out_i.cpu().numpy() == -7).all()
        # no candidate: -inf / -1 in [n_rep][n_group], nothing behind it
        e.scan_profile_dev(0, 0, 0, 0, 3, 3, 0, o, oi)
        e.sync()
        assert np.isneginf(out.cpu().numpy()[:9]).all() and (out.cpu().numpy()[9:] == 7.0).all()
        assert (out_i.cpu().numpy()[:9] == -1).all() and (out_i.cpu().numpy()[9:] == -7).all()


# ---- through the engine -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def w3():
    from misti_amd import workloads
    from misti_amd.engine import truth_spectrum
    return workloads.config3(lambda *a: truth_spectrum(*a), n_start=24)


def test_scan_profile_equals_the_host_reduction_of_evaluate(w3):
    import random
    from misti_amd import io as mio, synth
    from misti_amd.engine import Engine
    from misti_amd.optimize import profile_per_group, scan_profile
    params = w3.params.copy()
    params[[2, 11, 23], 0] = -0.01
    params[7, 1] = -1.0
    rows = np.array(mio.bootstrap_table(synth.chunk_rows(w3.jsfs[0], 20), 8, random.Random(3)), dtype=np.float64)
    group = np.random.default_rng(57).integers(0, 5, size=24)
    with Engine(w3.times, w3.lh, **w3.engine_kwargs()) as e:
        host = e.evaluate(w3.split_time, params, rows)
        val, best, status = scan_profile(e, w3.split_time, params, rows, group, 5)
    assert (host.status[[2, 7, 11, 23]] == 1).all() and np.array_equal(status, host.status)
    want_val, want = profile_per_group(host.llk, group, 5)
    assert np.array_equal(best, want) and same_bits(val, want_val)
    assert val.shape == (rows.shape[0], 5) and not np.isin(best, [2, 7, 11, 23]).any() and (best >= 0).any()
    with Engine(w3.times, w3.lh, **w3.engine_kwargs()) as e, pytest.raises(ValueError):
        scan_profile(e, w3.split_time, params, rows, group[:5], 5)


def test_per_candidate_band_bounds_and_pulse_times(w3):
    import random
    from conftest import load_golden
    from misti_amd import io as mio, synth
    from misti_amd.engine import Engine
    from misti_amd.optimize import profile_per_group, scan_profile
    rows = np.array(mio.bootstrap_table(synth.chunk_rows(w3.jsfs[0], 20), 5, random.Random(4)), dtype=np.float64)
    n = 12
    bounds = np.array([[[4 + c % 3, -1], [10 + c % 4, 60 if c % 2 else -1]] for c in range(n)], dtype=np.int32)
    bounds[5] = [[12, 8], [10, -1]]                                    # ends before it starts: SetModel refuses it (status 4)
    split = np.array([62.0, 63.5, 64.0, 65.0] * 3)
    group = np.arange(n) % 4                                           # the profile over the split value
    with Engine(w3.times, w3.lh, **w3.engine_kwargs()) as e:
        host = e.evaluate(split, w3.params[:n], rows, band_bounds=bounds)
        val, best, status = scan_profile(e, split, w3.params[:n], rows, group, 4, band_bounds=bounds)
    want_val, want = profile_per_group(host.llk, group, 4)
    assert host.status[5] == 4 and np.array_equal(status, host.status)
    assert np.array_equal(best, want) and same_bits(val, want_val) and not (best == 5).any()
    assert len({float(v) for v in host.llk[:, 0]}) > 6                 # the bounds reach the values
    # a pulse model: the date of the second pulse per candidate
    g = load_golden("golden_pulse_sweep")[0]["in"]
    ptable = np.array(mio.bootstrap_table(synth.chunk_rows(g["sfs"], 20), 3, random.Random(3)), dtype=np.float64)
    times = np.array([[10, t] for t in (3, 5, 7, 12, 15, 20, 25)], dtype=np.int32)
    sp = np.array([20.0, 20.5, 18.0, 20.0, 20.5, 18.0, 20.0])
    par = np.tile([0.2, 0.1], (len(sp), 1))
    group = np.array([0, 1, 2, 0, 1, 2, 0])
    with Engine(g["times"], g["lambdas"], [(0, 4, -1, 0.2, 0)], [(0, 10, 0.05, -1), (1, 3, 0.0, 1)], n_param=2, cpfit=True, smooth=True,
                unfolded=True) as e:
        host = e.evaluate(sp, par, ptable, pulse_times=times)
        val, best, status = scan_profile(e, sp, par, ptable, group, 3, pulse_times=times)
    want_val, want = profile_per_group(host.llk, group, 3)
    assert np.array_equal(status, host.status) and np.array_equal(best, want) and same_bits(val, want_val)
    assert len({float(v) for v in host.llk[:, 0] if np.isfinite(v)}) > 3


# ---- the command line ---------------------------------------------------------------------------------------------------------------
LINE = re.compile(r"^bs_id = (\S+) \tsplitT = (\S+) \tparams (\S*) \tllh = (\S+) \tstatus = (\S+)$", flags=re.M)
PROFILE = re.compile(r"^bs_id = (\S+) \tprofile ([^\n]*?) \tllh = (\S+)(?: \tsplitT = (\S+) \tparams (\S*) \tstatus = (\S+))?$", flags=re.M)


def test_command_line_profile(tmp_path):
    from misti_amd.optimize import axis_groups, profile_per_group
    from test_gpu_cli import run_cli, write_inputs
    f1, f2, fj, inp, row = write_inputs(tmp_path)
    args = [f1, f2, fj, "20", "-mi", "1", "2", "20", "0.1", "1", "--cpfit", "--grid-st", "18", "21", "--grid-mi", "0", "0.001", "0.1", "6", "--all-bs",
            "--funits", str(tmp_path / "x")]
    rc, full = run_cli(args)
    assert rc == 0
    all_lines = LINE.findall(full)                                      # candidate outermost, row innermost
    n, R = 4 * 6, 5
    assert len(all_lines) == n * R
    text = np.array([l[3] for l in all_lines]).reshape(n, R)
    table = np.array([[float(t) for t in line] for line in text])
    cand = [(all_lines[c * R][1], all_lines[c * R][2]) for c in range(n)]      # the printed splitT and params of every candidate
    keep = lambda t, word: [l for l in t.splitlines() if l.startswith(word)]
    for axes, which in ((["st"], 0), (["0"], 1), (["st", "0"], (0, 1))):
        rc, out = run_cli(args + ["--profile"] + axes)
        assert rc == 0, axes
        group, G = axis_groups((4, 6), which)
        want_val, want = profile_per_group(table, group, G)
        lines = PROFILE.findall(out)
        assert len(lines) == R * G, out[-2000:]
        for i, l in enumerate(lines):                                    # row outermost, group innermost
            r, g = divmod(i, G)
            c = want[r, g]
            assert l[0] == str(r)
            if c < 0:                                                    # a group without a value: llh = -inf and no candidate
                assert l[2:] == ("-inf", "", "", ""), (axes, r, g)
                continue
            assert l[2] == text[c, r] and float(l[2]) == want_val[r, g], (axes, r, g)      # the same double prints the same text
            assert (l[3], l[4]) == cand[c] and l[5] == "0", (axes, r, g)
            member = cand[int(np.where(group == g)[0][0])]
            where = dict(w.split(" = ") for w in l[1].split(" \t"))
            assert list(where) == ["st" if a == "st" else "p" + a for a in axes]
            assert where.get("st", member[0]) == member[0] and where.get("p0", member[1]) == member[1]
        assert keep(out, "best:") == keep(full, "best:") and len(keep(out, "best:")) == 1
        assert len(keep(out, "support:")) == (R if len(axes) == 1 else 0)
        if "st" in axes:
            assert keep(out, "bootstrap:") == keep(full, "bootstrap:") and len(keep(out, "bootstrap:")) == 1
        else:
            assert keep(out, "bootstrap:") == []
        assert re.search(r"^Evaluated 24 candidates x 5 replicates in ", out, flags=re.M)
    # the support: line is profile_interval of the printed profile, with the drop given or the computed default
    from scipy import stats
    from misti_amd.optimize import profile_interval
    splits = [float(c[0]) for c in cand[::6]]
    want_val, _ = profile_per_group(table, axis_groups((4, 6), 0)[0], 4)
    for extra, drop in (([], 0.5 * stats.chi2.ppf(0.95, 1)), (["--profile-drop", "0"], 0.0), (["--profile-drop", "1e9"], 1e9)):
        rc, out = run_cli(args + ["--profile", "st"] + extra)
        iv = profile_interval(want_val, splits, drop)
        got = re.findall(r"^support: bs_id = (\d+) best st = (\S+) llh = (\S+) within (\S+) of it: st in \[(\S+), (\S+)\]$", out, flags=re.M)
        assert rc == 0 and len(got) == R, out[-1500:]
        for r, s in enumerate(got):
            assert [float(v) for v in s[1:3]] == [iv["best"][r], iv["llh"][r]] and float(s[3]) == float("%.6g" % drop)
            assert [float(v) for v in s[4:]] == [iv["lo"][r], iv["hi"][r]]
        if drop == 1e9:
            assert all(float(s[4]) == splits[0] and float(s[5]) == splits[-1] for s in got)
