"""Parametric bootstrap on the device (misti_parametric_rows_dev, Engine.parametric_rows_dev / parametric_table, `--parametric N`).  The
reference everywhere is the rule stated in NumPy, optimize.parametric_rows: every comparison is on the float64 bits, nothing by
tolerance.  The sites of a replicate are spread over lanes (256 a workgroup, four Philox blocks a lane and iteration) and, for few
replicates of many sites, over workgroups: shapes on both sides of every such edge, and the geometry query says which regime a shape is in."""
import contextlib
import ctypes as C
import io
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P0 = np.array([.3, .05, .2, .1, .15, .08, .12])
GENOME = 123456.5


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.view(np.int64), b.view(np.int64)) if a.dtype == np.float64 else a.tobytes() == b.tobytes()


def geometry(n_sites, n_rep):
    from misti_amd import _lib
    b = C.c_int32(-1)
    _lib.check(_lib.load().misti_parametric_geometry(n_sites, n_rep, C.byref(b)))
    return b.value


def small_input():
    from misti_amd import synth, io as mio
    return mio.merge_psmc(mio.read_psmc_file(io.StringIO(synth.psmc_text(16, 1, synth.THETA_1))),
                          mio.read_psmc_file(io.StringIO(synth.psmc_text(17, 2, synth.THETA_2))))


@pytest.fixture(scope="module")
def eng():
    from misti_amd.engine import Engine
    inp = small_input()
    with Engine(inp.times, inp.lambdas) as e:
        yield e


def check_rows(rows, n_sites, genome=GENOME):
    """Counts are non-negative integers, sum to n_sites exactly, and column 0 is the genome."""
    assert (rows[:, 0] == genome).all() and (rows[:, 1:] >= 0).all() and (rows[:, 1:] == np.floor(rows[:, 1:])).all()
    assert (rows[:, 1:].astype(np.int64).sum(axis=1) == n_sites).all()


@pytest.mark.parametrize("n_sites", [0, 1, 3, 4, 5, 255, 1023, 1024, 1025, 4 * 256 * 3 - 1, 4 * 256 * 3 + 1])
def test_rows_equal_the_numpy_rule_at_every_edge_of_a_lane(eng, n_sites):
    """A partial last Philox block, a lane with no work, a lane stride crossed by one: one workgroup per replicate."""
    from misti_amd.optimize import parametric_rows
    want, _ = parametric_rows([P0], 5, n_sites, GENOME, seed=5)
    rows, status = eng.parametric_rows_dev(P0[None, :], 5, n_sites, GENOME, seed=5, row_status=True)
    assert geometry(n_sites, 5) == 1
    assert same_bits(rows.cpu().numpy(), want) and not status.cpu().numpy().any()
    check_rows(want, n_sites)


def test_one_replicate_over_many_workgroups(eng):
    from misti_amd.optimize import parametric_rows
    n_sites = 2 ** 22 + 3
    assert geometry(n_sites, 1) > 1
    want, _ = parametric_rows([P0], 1, n_sites, GENOME, seed=9, first=4)
    assert same_bits(eng.parametric_rows_dev(P0, 1, n_sites, GENOME, seed=9, first=4).cpu().numpy(), want)
    check_rows(want, n_sites)


def test_many_replicates_of_one_workgroup_each(eng):
    from misti_amd.optimize import parametric_rows
    assert geometry(1000, 700) == 1                                   # the grid's second dimension passes 256
    want, _ = parametric_rows([P0], 700, 1000, GENOME, seed=2)
    assert same_bits(eng.parametric_rows_dev(P0, 700, 1000, GENOME, seed=2).cpu().numpy(), want)
    check_rows(want, 1000)


def test_spec_of_cycles_over_spectra_and_unusable_ones_give_zero_rows(eng):
    import torch
    from misti_amd.optimize import parametric_rows
    spectra = np.array([P0 * 37.5,                                    # unnormalised
                        [.2, .1, .3, .4, 0, 0, 0],                    # trailing zeros
                        [0, 0, 0, 2.0, 0, 0, 0],                      # a single class
                        [.2, .1, float("nan"), .1, .1, .1, .1]])      # unusable
    n, n_sites = 23, 1025
    of = (np.arange(n) % 3).astype(np.int32)
    clean, st = parametric_rows(spectra, n, n_sites, GENOME, seed=3, spec_of=of)
    assert not st.any() and (clean[2::3, 4] == n_sites).all() and (clean[1::3, 5:] == 0).all()
    of[[4, 11]] = 3                                                   # the unusable spectrum
    of[[7, 20]] = [4, -1]                                             # out of range
    want, want_status = parametric_rows(spectra, n, n_sites, GENOME, seed=3, spec_of=of)
    rows, status = eng.parametric_rows_dev(spectra, n, n_sites, GENOME, seed=3, spec_of=of, row_status=True)
    got = rows.cpu().numpy()
    assert same_bits(got, want) and status.cpu().numpy().tolist() == want_status.tolist()
    bad = np.isin(np.arange(n), [4, 7, 11, 20])
    assert want_status[bad].all() and not want_status[~bad].any() and (got[bad, 1:] == 0).all() and (got[bad, 0] == GENOME).all()
    assert same_bits(got[~bad], clean[~bad])                          # the other rows are unaffected
    with pytest.raises(ValueError, match="4 of 23"):
        eng.parametric_rows_dev(spectra, n, n_sites, GENOME, seed=3, spec_of=of)
    # a status without a value makes a spectrum unusable too, on tensors of the device as on arrays
    dev = torch.device("cuda", eng.device)
    st_in = np.array([0, 5, 0, 0], dtype=np.int32)
    of6 = np.array([0, 1, 2, 0, 1, 2], dtype=np.int32)
    want, want_status = parametric_rows(spectra[:3], 6, 100, GENOME, seed=3, spec_of=of6, status=st_in[:3])
    rows, status = eng.parametric_rows_dev(torch.as_tensor(spectra[:3], device=dev), 6, 100, GENOME, seed=3,
                                           spec_of=torch.as_tensor(of6, device=dev), status=torch.as_tensor(st_in[:3], device=dev), row_status=True)
    assert same_bits(rows.cpu().numpy(), want) and status.cpu().numpy().tolist() == want_status.tolist() == [0, 1, 0, 0, 1, 0]


@pytest.mark.parametrize("seed, first", [(5, 0), (2 ** 64 - 1, 2 ** 32 + 5)])
def test_two_calls_equal_one_and_nothing_is_written_beyond_the_rows(eng, seed, first):
    import torch
    from misti_amd import _lib
    from misti_amd.optimize import parametric_rows
    n, n_sites = 300, 1500
    want, _ = parametric_rows([P0], n, n_sites, GENOME, seed=seed, first=first)
    dev = torch.device("cuda", eng.device)
    sp = torch.as_tensor(P0, device=dev)
    rows = torch.full((n + 1, 8), 7.0, dtype=torch.float64, device=dev)
    status = torch.full((n + 1,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for lo, m in ((0, 137), (137, 163)):
        _lib.check(eng._lib.misti_parametric_rows_dev(eng._ctx, 1, C.c_void_p(sp.data_ptr()), None, None, GENOME, n_sites, C.c_uint64(seed), first + lo, m,
                                                      C.c_void_p(rows.data_ptr() + lo * 64), C.c_void_p(status.data_ptr() + lo * 4)))
    _lib.check(eng._lib.misti_parametric_rows_dev(eng._ctx, 1, None, None, None, GENOME, n_sites, C.c_uint64(seed), first, 0, None, None))   # n_rep == 0: nothing
    eng.sync()
    got, got_status = rows.cpu().numpy(), status.cpu().numpy()
    assert same_bits(got[:n], want) and not got_status[:n].any()
    assert (got[n] == 7.0).all() and got_status[n] == -7              # the guard row keeps its canary
    assert same_bits(eng.parametric_rows_dev(P0, n, n_sites, GENOME, seed=seed, first=first).cpu().numpy(), want)
    check_rows(want, n_sites)
    assert not same_bits(parametric_rows([P0], 4, n_sites, GENOME, seed=seed ^ 1, first=first)[0], want[:4])      # the seed is in the key


def test_rows_drawn_from_a_resident_spectrum_score_like_the_uploaded_rule(eng):
    """evaluate_dev writes d_jafs and d_status; parametric_rows_dev reads those tensors where they are; llk_dev and scan_best_dev score
    its rows - bit for bit what the same calls give on the NumPy rule's rows uploaded from the host."""
    import torch
    from misti_amd.optimize import parametric_rows
    R, n, k, n_sites = 40, 16, 2, 20000
    dev = torch.device("cuda", eng.device)
    split = torch.as_tensor(8.0 + 0.5 * np.arange(n), device=dev)
    jafs = torch.empty((n, 7), dtype=torch.float64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    eng.evaluate_dev(n, split.data_ptr(), 0, 0, 0, 0, d_jafs=jafs.data_ptr(), d_status=status.data_ptr())
    eng.sync()
    of = (np.arange(R) % n).astype(np.int32)
    d_rows, d_status = eng.parametric_rows_dev(jafs, R, n_sites, GENOME, seed=1, spec_of=torch.as_tensor(of, device=dev), status=status, row_status=True)
    h_rows, h_status = parametric_rows(jafs.cpu().numpy(), R, n_sites, GENOME, seed=1, spec_of=of, status=status.cpu().numpy())
    assert same_bits(d_rows.cpu().numpy(), h_rows) and d_status.cpu().numpy().tolist() == h_status.tolist()
    assert (h_status == (status.cpu().numpy()[of] != 0)).all() and (h_status == 0).sum() >= 8        # a candidate without a value gives no replicate
    u_rows = torch.as_tensor(h_rows, device=dev)
    got = []
    for rows in (d_rows, u_rows):
        llk = torch.full((n, R), 7.0, dtype=torch.float64, device=dev)
        best = torch.full((R, k), -7, dtype=torch.int32, device=dev)
        val = torch.full((R, k), 7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        eng.llk_dev(n, jafs.data_ptr(), status.data_ptr(), R, rows.data_ptr(), llk.data_ptr())
        eng.scan_best_dev(n, jafs.data_ptr(), status.data_ptr(), R, rows.data_ptr(), k, best.data_ptr(), val.data_ptr())
        eng.sync()
        got.append((llk.cpu().numpy(), best.cpu().numpy(), val.cpu().numpy()))
    assert np.isfinite(got[0][0][status.cpu().numpy() == 0]).all() and (got[0][1][:, 0] >= 0).all()
    for a, b in zip(got[0], got[1]):
        assert same_bits(a, b)


def test_parametric_table_is_the_rule_on_the_evaluated_spectrum(eng):
    from misti_amd.optimize import parametric_rows, parametric_table
    data = np.array([5000.0, 310, 52, 198, 101, 149, 79, 121.4])
    jafs = eng.evaluate([12.0]).jafs
    n_sites = int(np.rint(data[1:].sum()))
    table = eng.parametric_table(12.0, None, data, 9, seed=4)
    assert isinstance(table, np.ndarray) and same_bits(table, parametric_table(data, parametric_rows(jafs, 9, n_sites, data[0], seed=4)[0]))
    assert same_bits(eng.parametric_table(12.0, None, data, 9, n_sites=77, seed=4)[1:], parametric_rows(jafs, 9, 77, data[0], seed=4)[0])


def test_the_device_list_makes_the_same_table(eng):
    from misti_amd.engine import MultiEngine
    inp = small_input()
    data = np.array([5000.0, 310, 52, 198, 101, 149, 79, 121])
    with MultiEngine(inp.times, inp.lambdas, devices=[0, 0]) as m:
        assert same_bits(m.parametric_table(12.0, None, data, 9, seed=4), eng.parametric_table(12.0, None, data, 9, seed=4))


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def run_cli(args):
    from misti_amd import cli
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc = cli.main(args)
    return rc, out.getvalue()


def test_parametric_run_equals_all_bs_on_the_table_it_wrote(tmp_path):
    from misti_amd import synth, io as mio
    from oracle.batch import oracle_truth_spectrum
    f1, f2, fj, out = (str(tmp_path / n) for n in ("g1.psmc", "g2.psmc", "data.sfs", "t.sfs"))
    open(f1, "w").write(synth.psmc_text(16, 1, synth.THETA_1))
    open(f2, "w").write(synth.psmc_text(17, 2, synth.THETA_2))
    inp = mio.read_psmc(f1, f2)
    data = synth.counts_from_spectrum(oracle_truth_spectrum(inp.times, inp.lambdas, 20, [], [], 0), 200000)      # ONE row: nothing to resample
    open(fj, "w").write(mio.format_jsfs([data]))
    units = str(tmp_path / "nounits.txt")
    rc, text = run_cli([f1, f2, fj, "16", "--parametric", "8", "--bs-seed", "7", "--bootstrap-out", out, "--all-bs", "--grid-st", "15", "17", "--funits", units])
    assert rc == 0 and os.path.exists(out)
    table, _, _ = mio.read_jsfs(out)
    table = np.array(table)
    n_sites = int(np.rint(sum(data[1:])))
    assert table.shape == (9, 8) and table[0].tolist() == [float(v) for v in data]
    assert (table[1:, 0] == data[0]).all() and (table[1:, 1:].sum(axis=1) == n_sites).all()
    marker = [l for l in text.splitlines() if l.startswith("Parametric bootstrap:")]
    assert len(marker) == 1 and "8 replicates of %d sites" % n_sites in marker[0] and "seed 7" in marker[0] and "splitT = 16" in marker[0]
    stage2 = text[text.index("Parametric bootstrap:"):]
    rc2, text2 = run_cli([f1, f2, out, "16", "--all-bs", "--grid-st", "15", "17", "--funits", units])
    lines = lambda t: [l for l in t.splitlines() if l.startswith("bs_id =") or l.startswith("best:") or l.startswith("bootstrap:")]
    assert rc2 == 0 and lines(text2) == lines(stage2)
    assert len([l for l in lines(stage2) if l.startswith("bs_id =")]) == 3 * 9
