"""The k best candidates per replicate without the likelihood table (misti_scan_best_dev, optimize.scan_best / scan_polish,
`--top K [--polish]`).  The reference everywhere is the table itself - misti_llk_dev on the same buffers, or Engine.evaluate -
reduced on the host by optimize.best_k_per_replicate: indices equal, values bit for bit."""
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
    """Hand-made spectra, statuses and rows on the device, the table misti_llk_dev makes of them and the scan of them."""

    def __init__(self, e, jafs, status, rows):
        import torch
        self.e, self.torch, self.dev = e, torch, torch.device("cuda", 0)
        self.n, self.R = jafs.shape[0], rows.shape[0]
        self.jafs = torch.as_tensor(np.ascontiguousarray(jafs, dtype=np.float64), device=self.dev)
        self.status = None if status is None else torch.as_tensor(np.ascontiguousarray(status, dtype=np.int32), device=self.dev)
        self.rows = torch.as_tensor(np.ascontiguousarray(rows, dtype=np.float64), device=self.dev)
        torch.cuda.synchronize()                      # the engine issues on its own non-blocking stream

    def table(self):
        out = self.torch.full((self.n, self.R), float("nan"), dtype=self.torch.float64, device=self.dev)
        self.torch.cuda.synchronize()
        self.e.llk_dev(self.n, self.jafs.data_ptr(), self.status.data_ptr() if self.status is not None else 0, self.R, self.rows.data_ptr(), out.data_ptr())
        self.e.sync()
        self.d_table = out
        return out.cpu().numpy()

    def scan(self, k, want_llk=True):
        t = self.torch
        best = t.full((self.R, k), -7, dtype=t.int32, device=self.dev)
        val = t.full((self.R, k), 7.0, dtype=t.float64, device=self.dev)
        guard = t.full((64,), 7.0, dtype=t.float64, device=self.dev)       # allocated right behind: an overrun would show here
        t.cuda.synchronize()
        self.e.scan_best_dev(self.n, self.jafs.data_ptr(), self.status.data_ptr() if self.status is not None else 0, self.R, self.rows.data_ptr(), k,
                             best.data_ptr(), val.data_ptr() if want_llk else 0)
        self.e.sync()
        assert float(guard.sum().item()) == 64 * 7.0
        return best.cpu().numpy().astype(np.int64), val.cpu().numpy()


def check(buf, ks, tag):
    from misti_amd.optimize import best_k_per_replicate
    table = buf.table()
    for k in ks:
        best, val = buf.scan(k)
        want, want_val = best_k_per_replicate(table, k)
        assert np.array_equal(best, want), (tag, k)
        assert same_bits(val, want_val), (tag, k)
    return table


# ---- the kernel alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unfolded", [False, True], ids=["folded", "unfolded"])
def test_every_shape_equals_the_reduced_table(unfolded):
    """Odd and even widths and a workgroup boundary (256 replicates), the LDS chunk boundary (64 candidates), fewer candidates than
    places, k below, at and between the compiled widths; a tenth of the candidates without a value."""
    rng = np.random.default_rng(21 + unfolded)
    with engine(unfolded) as e:
        for R in (1, 2, 3, 255, 256, 257):
            rows = counts(rng, R)
            for n in (1, 5, 63, 64, 65, 200):
                status = (rng.random(n) < 0.1).astype(np.int32) * 2
                table = check(Buffers(e, spectra(rng, n), status, rows), (1, 2, 3, 8), (R, n))
                assert np.isneginf(table[status != 0]).all() and np.isfinite(table[status == 0]).all()
        # status NULL: every candidate has a value; best_llk NULL: only the indices
        buf = Buffers(e, spectra(rng, 65), None, counts(rng, 3))
        check(buf, (2,), "no status")
        best, val = buf.scan(2, want_llk=False)
        assert (val == 7.0).all() and (best >= 0).all()


def test_the_result_does_not_move_with_the_slice_count(monkeypatch):
    """MISTI_SCAN_SLICES (read once per context) cuts 200 candidates into 1, 2 and 7 slices (200 is no multiple of 7): one result.
    Every spectrum appears three times, so that ties cross the cuts."""
    from misti_amd.optimize import best_k_per_replicate
    rng = np.random.default_rng(23)
    base = spectra(rng, 67)
    jafs = np.vstack([base, base, base])[:200]
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
            got[slices] = [buf.scan(k) for k in (1, 3, 8)]
            if slices == "1":
                table = buf.table()
    for k, (best, val) in zip((1, 3, 8), got["1"]):
        want, want_val = best_k_per_replicate(table, k)
        assert np.array_equal(best, want) and same_bits(val, want_val)
    for slices in ("2", "7", None):
        for (b1, v1), (b, v) in zip(got["1"], got[slices]):
            assert np.array_equal(b1, b) and same_bits(v1, v), slices


@pytest.mark.parametrize("order", ["same", "reversed"])
def test_equal_values_come_out_in_index_order(order):
    """Every spectrum twice - rows i and i + n/2, or the copies in reverse order: each pair is listed lower index first, and both
    of its members wherever k allows."""
    rng = np.random.default_rng(25)
    half = 70
    base = spectra(rng, half)
    jafs = np.vstack([base, base if order == "same" else base[::-1]])
    twin = (lambda c: (c + half) % (2 * half)) if order == "same" else (lambda c: 2 * half - 1 - c)
    with engine() as e:
        buf = Buffers(e, jafs, None, counts(rng, 33))
        check(buf, (1, 2, 4, 8), order)
        best, val = buf.scan(8)
    for r in range(best.shape[0]):
        for j in range(0, 8, 2):
            a, b = int(best[r, j]), int(best[r, j + 1])
            assert b == twin(a) and a < b and val[r, j] == val[r, j + 1], (r, j, a, b)
        assert (np.diff(val[r]) <= 0).all()


def test_candidates_without_a_value_are_never_listed():
    rng = np.random.default_rng(27)
    n, R = 130, 5
    jafs, rows = spectra(rng, n), counts(rng, R)
    with engine() as e:
        # statuses 1 ... 6 on a third of the candidates
        status = np.where(rng.random(n) < 0.33, rng.integers(1, 7, size=n), 0).astype(np.int32)
        best, val = Buffers(e, jafs, status, rows).scan(8)
        assert (best >= 0).all() and (status[best] == 0).all() and np.isfinite(val).all()
        check(Buffers(e, jafs, status, rows), (4,), "status")
        # only two candidates have a value, four places
        status = np.full(n, 2, dtype=np.int32)
        status[[17, 99]] = 0
        best, val = Buffers(e, jafs, status, rows).scan(4)
        assert (np.sort(best[:, :2], axis=1) == [17, 99]).all() and (best[:, 2:] == -1).all()
        assert np.isfinite(val[:, :2]).all() and np.isneginf(val[:, 2:]).all()
        check(Buffers(e, jafs, status, rows), (4,), "two values")
        # none has
        best, val = Buffers(e, jafs, np.full(n, 5, dtype=np.int32), rows).scan(3)
        assert (best == -1).all() and np.isneginf(val).all()
        # no candidate at all
        buf = Buffers(e, jafs[:0], None, rows)
        best, val = buf.scan(3)
        assert (best == -1).all() and np.isneginf(val).all()


@pytest.mark.parametrize("unfolded", [False, True], ids=["folded", "unfolded"])
def test_zero_times_minus_infinity_is_never_listed(unfolded):
    """A spectrum with an empty class against a row with no count in it: 0 x log 0 is NaN in the table, and no place of the list;
    against a row WITH a count there it is -inf, and no place either."""
    rng = np.random.default_rng(29)
    jafs = spectra(rng, 6)
    jafs[[1, 4], 3] = 0.0                              # class 3 stands alone folded and unfolded
    rows = counts(rng, 4)
    rows[[0, 2], 4] = 0.0                              # rows 0 and 2 have no count in it
    rows[:, 0] = rows[:, 1:].sum(axis=1)
    with engine(unfolded) as e:
        buf = Buffers(e, jafs, None, rows)
        table = check(buf, (1, 4, 8), "nan")
        best, val = buf.scan(8)
    assert np.isnan(table[[1, 4]][:, [0, 2]]).all() and np.isneginf(table[[1, 4]][:, [1, 3]]).all()
    assert (best[:, :4] >= 0).all() and (best[:, 4:] == -1).all() and not np.isin(best, [1, 4]).any()


def test_one_place_is_the_table_and_its_arg_max_bit_for_bit():
    import torch
    rng = np.random.default_rng(31)
    n, R = 333, 300
    status = (rng.random(n) < 0.2).astype(np.int32) * 3
    rows = counts(rng, R)
    jafs = spectra(rng, n)
    jafs[100:200] = jafs[:100]                         # ties
    with engine() as e:
        buf = Buffers(e, jafs, status, rows)
        buf.table()
        a_best = torch.empty(R, dtype=torch.int32, device=buf.dev)
        a_val = torch.empty(R, dtype=torch.float64, device=buf.dev)
        torch.cuda.synchronize()
        e.argmax_dev(n, R, buf.d_table.data_ptr(), a_best.data_ptr(), a_val.data_ptr())
        e.sync()
        best, val = buf.scan(1)
    assert np.array_equal(best[:, 0], a_best.cpu().numpy()) and same_bits(val[:, 0], a_val.cpu().numpy())


def test_argument_errors_and_an_empty_call():
    from misti_amd._lib import MistiError
    rng = np.random.default_rng(33)
    with engine() as e:
        buf = Buffers(e, spectra(rng, 5), None, counts(rng, 3))
        for k in (0, 9, -1):
            with pytest.raises(MistiError) as err:
                e.scan_best_dev(5, buf.jafs.data_ptr(), 0, 3, buf.rows.data_ptr(), k, buf.rows.data_ptr(), 0)
            assert err.value.code == -1
        with pytest.raises(MistiError) as err:
            e.scan_best_dev(5, buf.jafs.data_ptr(), 0, 3, buf.rows.data_ptr(), 2, 0, 0)          # best is NULL
        assert err.value.code == -1
        with pytest.raises(MistiError) as err:
            e.scan_best_dev(-1, buf.jafs.data_ptr(), 0, 3, buf.rows.data_ptr(), 2, buf.rows.data_ptr(), 0)
        assert err.value.code == -1
        with pytest.raises(MistiError) as err:
            e.scan_best_dev(2 ** 31, buf.jafs.data_ptr(), 0, 3, buf.rows.data_ptr(), 2, buf.rows.data_ptr(), 0)
        assert err.value.code == -4
        # no replicate: nothing is written
        import torch
        sentinel = torch.full((6,), -7, dtype=torch.int32, device=buf.dev)
        sval = torch.full((6,), 7.0, dtype=torch.float64, device=buf.dev)
        torch.cuda.synchronize()
        e.scan_best_dev(5, buf.jafs.data_ptr(), 0, 0, buf.rows.data_ptr(), 2, sentinel.data_ptr(), sval.data_ptr())
        e.sync()
        assert (sentinel.cpu().numpy() == -7).all() and (sval.cpu().numpy() == 7.0).all()


# ---- through the engine -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def w3():
    from misti_amd import workloads
    from misti_amd.engine import truth_spectrum
    return workloads.config3(lambda *a: truth_spectrum(*a), n_start=24)


def test_scan_of_the_bootstrap_workload_equals_the_host_reduction():
    from misti_amd import workloads
    from misti_amd.engine import Engine, truth_spectrum
    from misti_amd.optimize import _scan_best, best_k_per_replicate, scan_best
    w = workloads.config4(lambda *a: truth_spectrum(*a))
    rows = w.jsfs[:200]
    with Engine(w.times, w.lh, **w.engine_kwargs()) as e:
        host = e.evaluate(w.split_time, w.params, rows)
        best, val, status = scan_best(e, w.split_time, w.params, rows, k=3)
        winner = _scan_best(e, w.split_time, rows)                    # what bootstrap_scan_dev reduces: llk table + arg-max
    want, want_val = best_k_per_replicate(host.llk, 3)
    assert np.array_equal(best, want) and same_bits(val, want_val) and np.array_equal(status, host.status)
    assert (best[:, 0] >= 0).all() and np.array_equal(best[:, 0], winner)
    assert len(set(best[:, 0].tolist())) > 1                           # (the rows do not all agree: the reduction is per row)


def test_candidates_with_a_negative_rate_never_appear(w3):
    from misti_amd import io as mio, synth
    from misti_amd.engine import Engine
    from misti_amd.optimize import best_k_per_replicate, scan_best
    import random
    params = w3.params.copy()
    params[[2, 11, 23], 0] = -0.01
    params[7, 1] = -1.0
    rows = np.array(mio.bootstrap_table(synth.chunk_rows(w3.jsfs[0], 20), 8, random.Random(3)), dtype=np.float64)
    with Engine(w3.times, w3.lh, **w3.engine_kwargs()) as e:
        host = e.evaluate(w3.split_time, params, rows)
        best, val, status = scan_best(e, w3.split_time, params, rows, k=8)
    assert (host.status[[2, 7, 11, 23]] == 1).all() and np.array_equal(status, host.status)
    want, want_val = best_k_per_replicate(host.llk, 8)
    assert np.array_equal(best, want) and same_bits(val, want_val)
    assert (best >= 0).all() and not np.isin(best, [2, 7, 11, 23]).any()


def test_per_candidate_band_bounds_and_pulse_times(w3):
    import random
    from conftest import load_golden
    from misti_amd import io as mio, synth
    from misti_amd.engine import Engine
    from misti_amd.optimize import best_k_per_replicate, scan_best
    rows = np.array(mio.bootstrap_table(synth.chunk_rows(w3.jsfs[0], 20), 5, random.Random(4)), dtype=np.float64)
    n = 12
    bounds = np.array([[[4 + c % 3, -1], [10 + c % 4, 60 if c % 2 else -1]] for c in range(n)], dtype=np.int32)
    bounds[5] = [[12, 8], [10, -1]]                                    # ends before it starts: SetModel refuses it (status 4)
    split = np.array([62.0, 63.5, 64.0, 65.0] * 3)
    with Engine(w3.times, w3.lh, **w3.engine_kwargs()) as e:
        host = e.evaluate(split, w3.params[:n], rows, band_bounds=bounds)
        best, val, status = scan_best(e, split, w3.params[:n], rows, k=4, band_bounds=bounds)
    want, want_val = best_k_per_replicate(host.llk, 4)
    assert host.status[5] == 4 and np.array_equal(status, host.status)
    assert np.array_equal(best, want) and same_bits(val, want_val) and not (best == 5).any()
    assert len({float(v) for v in host.llk[:, 0]}) > 6                 # the bounds reach the values
    # a pulse model: the date of the second pulse per candidate
    g = load_golden("golden_pulse_sweep")[0]["in"]
    ptable = np.array(mio.bootstrap_table(synth.chunk_rows(g["sfs"], 20), 3, random.Random(3)), dtype=np.float64)
    times = np.array([[10, t] for t in (3, 5, 7, 12, 15, 20, 25)], dtype=np.int32)
    sp = np.array([20.0, 20.5, 18.0, 20.0, 20.5, 18.0, 20.0])
    par = np.tile([0.2, 0.1], (len(sp), 1))
    with Engine(g["times"], g["lambdas"], [(0, 4, -1, 0.2, 0)], [(0, 10, 0.05, -1), (1, 3, 0.0, 1)], n_param=2, cpfit=True, smooth=True,
                unfolded=True) as e:
        host = e.evaluate(sp, par, ptable, pulse_times=times)
        best, val, status = scan_best(e, sp, par, ptable, k=3, pulse_times=times)
    want, want_val = best_k_per_replicate(host.llk, 3)
    assert np.array_equal(status, host.status) and np.array_equal(best, want) and same_bits(val, want_val)
    assert len({float(v) for v in host.llk[:, 0] if np.isfinite(v)}) > 3


def test_scan_polish_is_one_search_from_the_listed_candidates(w3):
    import random
    from misti_amd import io as mio, synth
    from misti_amd.engine import Engine
    from misti_amd.optimize import scan_best, scan_polish
    rows = np.array(mio.bootstrap_table(synth.chunk_rows(w3.jsfs[0], 20), 2, random.Random(5)), dtype=np.float64)
    assert rows.shape == (3, 8)
    with Engine(w3.times, w3.lh, **w3.engine_kwargs()) as e:
        best, val, _ = scan_best(e, w3.split_time, w3.params, rows, k=2)
        pol = scan_polish(e, w3.split_time, w3.params, rows, 2, maxiter=300)
        r_of = np.repeat(np.arange(3), 2).astype(np.int32)
        cand = best.ravel()
        hand = e.nm_solve_rows(w3.params[cand], w3.split_time[cand], r_of, rows, maxiter=300)
    assert (best >= 0).all() and np.array_equal(pol["best"], best) and same_bits(pol["best_llk"], val)
    s = pol["searches"]
    assert np.array_equal(s["row"], r_of) and np.array_equal(s["place"], np.tile([0, 1], 3)) and np.array_equal(s["cand"], cand)
    for f in ("x", "llh", "nit", "nfev", "status"):
        assert same_bits(s[f], hand[f]), f
    llh = hand["llh"].reshape(3, 2)
    place = np.argmax(np.where(np.isnan(llh), NINF, llh), axis=1)
    assert np.array_equal(pol["place"], place)
    for f in ("x", "llh", "nit", "nfev", "status"):
        assert same_bits(pol[f], hand[f].reshape((3, 2) + hand[f].shape[1:])[np.arange(3), place]), f
    assert (pol["llh"] >= val[:, 0]).all()                             # a search never ends below its own start
    assert np.array_equal(pol["split"], w3.split_time[best[np.arange(3), place]])
    from misti_amd import workloads
    from misti_amd.engine import truth_spectrum
    w4 = workloads.config4(lambda *a: truth_spectrum(*a), n_split=4, n_rep=3)
    with Engine(w4.times, w4.lh, **w4.engine_kwargs()) as e, pytest.raises(ValueError):
        scan_polish(e, w4.split_time, None, w4.jsfs, 2)


# ---- the command line ---------------------------------------------------------------------------------------------------------------
LINE = re.compile(r"^bs_id = (\S+) \tsplitT = (\S+) \tparams (\S*) \tllh = (\S+) \tstatus = (\S+)$", flags=re.M)


def test_command_line_top_and_polish(tmp_path):
    from test_gpu_cli import run_cli, write_inputs
    f1, f2, fj, inp, row = write_inputs(tmp_path)
    args = [f1, f2, fj, "20", "-mi", "1", "2", "20", "0.1", "1", "--cpfit", "--grid-st", "18", "22", "--grid-mi", "0", "0.001", "0.1", "4", "--all-bs",
            "--funits", str(tmp_path / "x")]
    rc, full = run_cli(args)
    rc2, top = run_cli(args + ["--top", "2"])
    assert rc == 0 and rc2 == 0
    all_lines, top_lines = LINE.findall(full), LINE.findall(top)
    assert len(all_lines) == 5 * 4 * 5 and len(top_lines) == 2 * 5
    for r in range(5):
        mine = [(float(l[1]), float(l[3])) for l in top_lines if l[0] == str(r)]
        theirs = [(float(l[1]), float(l[3]), i) for i, l in enumerate(all_lines) if l[0] == str(r)]      # printed in candidate order
        theirs.sort(key=lambda t: (-t[1], t[2]))
        assert mine == [t[:2] for t in theirs[:2]], r
    keep = lambda t: [l for l in t.splitlines() if l.startswith("best:") or l.startswith("bootstrap:")]
    assert len(keep(top)) == 2 and keep(top) == keep(full)
    assert re.search(r"^Evaluated 20 candidates x 5 replicates in ", top, flags=re.M)
    # --polish: one MiSTI.py:240 line per row, the llh of scan_polish on the same grid
    rc3, pol_text = run_cli(args + ["--top", "2", "--polish"])
    assert rc3 == 0 and len(LINE.findall(pol_text)) == 2 * 5
    got = re.findall(r"^bs_id = (\d+) \tsplitT = (\S+) \ttime = \S+ \tmigration rates optim = \[(\S+)\] \tllh = (\S+)$", pol_text, flags=re.M)
    assert [g[0] for g in got] == [str(r) for r in range(5)], pol_text[-1500:]
    from misti_amd import cli, io as mio
    from misti_amd.engine import Engine
    from misti_amd.optimize import scan_polish
    a = cli.build_parser().parse_args(args + ["--top", "2", "--polish"])
    splits, bands, pulses, k, axes = cli.grid_model(a)
    mesh = np.meshgrid(np.array(splits), *axes, indexing="ij")
    rows, _, _ = mio.read_jsfs(fj)
    with Engine(inp.times, inp.lambdas, bands, pulses, n_param=k, sample_date=inp.sampleDateDiscr, cpfit=True, smooth=True) as e:
        pol = scan_polish(e, mesh[0].ravel(), np.stack([m.ravel() for m in mesh[1:]], axis=1), np.array(rows, dtype=float), 2, tol=a.tol)
    assert [float(g[3]) for g in got] == pol["llh"].tolist() and [float(g[1]) for g in got] == pol["split"].tolist()
    assert [float(g[2]) for g in got] == pol["x"][:, 0].tolist()
