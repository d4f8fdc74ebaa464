"""Block bootstrap on the device (misti_bootstrap_rows_dev, Engine.bootstrap_rows_dev / bootstrap_table, `--bootstrap N`).  The
reference everywhere is the rule stated in NumPy, optimize.block_bootstrap: every comparison is on the float64 bits, nothing by
tolerance.  The kernel stages tables of up to 1 024 chunks in LDS and reads larger ones from global memory: tables on both sides of
that switch and exactly at it."""
import contextlib
import ctypes as C
import io
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_REF = 1000          # replicates of every reference; a device call of n < N_REF replicates is compared with its first n rows


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def random_table(seed, n_chunk):
    """Counts in multiples of 0.1 and lengths that are no integers either: the order of the additions shows in the last bits."""
    rng = np.random.default_rng(seed)
    c = np.zeros((n_chunk, 8))
    c[:, 1:] = rng.integers(0, 400, size=(n_chunk, 7)) * 0.1
    c[:, 0] = rng.integers(1, 50, size=n_chunk) * 0.1 + c[:, 1:].sum(axis=1)
    return c


def tables():
    t = {"1": random_table(1, 1)}                                     # every replicate is one draw
    three = random_table(3, 3)
    three[:, 0] = [1.0, 10.0, 100.0]                                  # 2 ... 111 draws a replicate, 4 on average
    t["3"] = three
    for n in (257, 1023, 1024, 1025, 5000):                           # 1 024: the last table staged in LDS
        t[str(n)] = random_table(n, n)
    return t


@pytest.fixture(scope="module")
def case():
    """The tables and, computed once, the NumPy statement of their first N_REF replicates (seed 5) with the draw counts."""
    from misti_amd.optimize import block_bootstrap
    out = {}
    for name, c in tables().items():
        rows, draws = block_bootstrap(c, N_REF, seed=5, draws=True)
        out[name] = (c, rows, draws)
    return out


@pytest.fixture(scope="module")
def eng():
    from misti_amd import synth, io as mio
    from misti_amd.engine import Engine
    inp = mio.merge_psmc(mio.read_psmc_file(io.StringIO(synth.psmc_text(16, 1, synth.THETA_1))),
                         mio.read_psmc_file(io.StringIO(synth.psmc_text(17, 2, synth.THETA_2))))
    with Engine(inp.times, inp.lambdas) as e:
        yield e


@pytest.mark.parametrize("name", ["1", "3", "257", "1023", "1024", "1025", "5000"])
def test_every_table_and_count_equals_the_numpy_rule(eng, case, name):
    c, want, want_draws = case[name]
    for n in (1, 63, 65, 1000):
        rows, draws = eng.bootstrap_rows_dev(c, n, seed=5, draws=True)
        assert same_bits(rows.cpu().numpy(), want[:n]), (name, n)
        assert same_bits(draws.cpu().numpy(), want_draws[:n]), (name, n)
    if name == "1":
        assert (want_draws == 1).all() and (want == c[0]).all()
    if name == "3":
        assert want_draws.min() == 2 and want_draws.max() >= 8       # lanes of one wave end after very different numbers of draws


@pytest.mark.parametrize("name", ["257", "1025"])
def test_two_calls_equal_one_and_nothing_is_written_beyond_the_rows(eng, case, name):
    """first_rep = 500, n_rep = 500 behind 0, 500 through the C ABI into ONE buffer, with guard rows behind it."""
    import torch
    c, want, want_draws = case[name]
    dev = torch.device("cuda", 0)
    rows = torch.full((N_REF + 8, 8), 7.0, dtype=torch.float64, device=dev)
    draws = torch.full((N_REF + 8,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    from misti_amd import _lib
    for first in (0, 500):
        _lib.check(eng._lib.misti_bootstrap_rows_dev(eng._ctx, c.shape[0], c.ctypes.data_as(C.c_void_p), C.c_uint64(5), first, 500, 0,
                                                     C.c_void_p(rows.data_ptr() + first * 64), C.c_void_p(draws.data_ptr() + first * 4)))
    _lib.check(eng._lib.misti_bootstrap_rows_dev(eng._ctx, c.shape[0], c.ctypes.data_as(C.c_void_p), C.c_uint64(5), 0, 0, 0, None, None))   # n_rep == 0: nothing
    eng.sync()
    got, got_draws = rows.cpu().numpy(), draws.cpu().numpy()
    assert same_bits(got[:N_REF], want) and same_bits(got_draws[:N_REF], want_draws)
    assert (got[N_REF:] == 7.0).all() and (got_draws[N_REF:] == -7).all()
    assert same_bits(eng.bootstrap_rows_dev(c, 500, seed=5, first=500).cpu().numpy(), want[500:])
    assert not same_bits(eng.bootstrap_rows_dev(c, 8, seed=6).cpu().numpy(), want[:8])          # the seed is in the key


def test_normalize_and_the_table(eng, case):
    from misti_amd.optimize import block_bootstrap, block_bootstrap_table
    c = case["257"][0]
    want = block_bootstrap(c, 65, seed=9, normalize=True)
    assert same_bits(eng.bootstrap_rows_dev(c, 65, seed=9, normalize=True).cpu().numpy(), want)
    assert not same_bits(want, block_bootstrap(c, 65, seed=9))
    table = eng.bootstrap_table(c, 65, seed=9, normalize=True)
    assert isinstance(table, np.ndarray) and same_bits(table, block_bootstrap_table(c, 65, seed=9, normalize=True))
    assert same_bits(eng.bootstrap_table(c, 65, seed=5), np.vstack([block_bootstrap_table(c, 0), case["257"][1][:65]]))


def test_the_device_list_makes_the_same_table(case):
    from misti_amd import synth, io as mio
    from misti_amd.engine import MultiEngine
    from misti_amd.optimize import block_bootstrap_table
    inp = mio.merge_psmc(mio.read_psmc_file(io.StringIO(synth.psmc_text(16, 1, synth.THETA_1))),
                         mio.read_psmc_file(io.StringIO(synth.psmc_text(17, 2, synth.THETA_2))))
    c = case["3"][0]
    with MultiEngine(inp.times, inp.lambdas, devices=[0, 0]) as m:
        assert same_bits(m.bootstrap_table(c, 65, seed=5), np.vstack([block_bootstrap_table(c, 0), case["3"][1][:65]]))


def test_a_refused_table_raises_with_the_codes_of_the_header(eng):
    from misti_amd._lib import MistiError
    bad = random_table(2, 4)
    bad[2, 0] = 0.0
    with pytest.raises(MistiError) as ei:
        eng.bootstrap_rows_dev(bad, 4)
    assert ei.value.code == -1 and "length" in str(ei.value)
    with pytest.raises(MistiError) as ei:
        eng.bootstrap_rows_dev(np.ones((65536, 8)), 4)
    assert ei.value.code == -4


def test_scan_best_over_the_device_rows_equals_the_scan_over_the_uploaded_table(eng):
    """64 candidates (split times), evaluated without replicates; then the 2 best per replicate over the rows the device drew and over
    optimize.block_bootstrap's rows uploaded: the same lists, the same bits.  Engine.evaluate takes the device rows as they are."""
    import torch
    from misti_amd.optimize import block_bootstrap
    rng = np.random.default_rng(12)
    c = np.zeros((40, 8))
    c[:, 1:] = rng.integers(50, 5000, size=(40, 7))
    c[:, 0] = c[:, 1:].sum(axis=1) + rng.integers(1000, 2000, size=40)
    R, n, k = 200, 64, 2
    dev = torch.device("cuda", 0)
    d_rows = eng.bootstrap_rows_dev(c, R, seed=1)
    h_rows = block_bootstrap(c, R, seed=1)
    u_rows = torch.as_tensor(h_rows, device=dev)
    split_h = 8.0 + 0.25 * np.arange(n)
    split = torch.as_tensor(split_h, device=dev)
    jafs = torch.empty((n, 7), dtype=torch.float64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    eng.evaluate_dev(n, split.data_ptr(), 0, 0, 0, 0, d_jafs=jafs.data_ptr(), d_status=status.data_ptr())
    got = []
    for rows in (d_rows, u_rows):
        best = torch.full((R, k), -7, dtype=torch.int32, device=dev)
        val = torch.full((R, k), 7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        eng.scan_best_dev(n, jafs.data_ptr(), status.data_ptr(), R, rows.data_ptr(), k, best.data_ptr(), val.data_ptr())
        eng.sync()
        got.append((best.cpu().numpy(), val.cpu().numpy()))
    assert (status.cpu().numpy() == 0).any() and (got[0][0] >= 0).all() and np.isfinite(got[0][1]).all()
    assert same_bits(got[0][0], got[1][0]) and same_bits(got[0][1], got[1][1])
    a, b = eng.evaluate(split_h[:3], None, d_rows), eng.evaluate(split_h[:3], None, h_rows)
    assert same_bits(a.llk, b.llk) and a.llk.shape == (3, R)


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def run_cli(args):
    from misti_amd import cli
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc = cli.main(args)
    return rc, out.getvalue()


def test_bootstrap_run_equals_all_bs_on_the_table_it_wrote(tmp_path):
    from misti_amd import synth, io as mio
    from misti_amd.optimize import block_bootstrap_table
    from oracle.batch import oracle_truth_spectrum
    f1, f2, fj, out = (str(tmp_path / n) for n in ("g1.psmc", "g2.psmc", "data.sfs", "table.sfs"))
    open(f1, "w").write(synth.psmc_text(16, 1, synth.THETA_1))
    open(f2, "w").write(synth.psmc_text(17, 2, synth.THETA_2))
    inp = mio.read_psmc(f1, f2)
    chunks = synth.chunk_rows(synth.counts_from_spectrum(oracle_truth_spectrum(inp.times, inp.lambdas, 20, [], [], 0), 200000), 5)
    open(fj, "w").write(mio.format_jsfs(chunks))
    units = str(tmp_path / "nounits.txt")
    rc, text = run_cli([f1, f2, fj, "16", "--bootstrap", "8", "--bs-seed", "3", "--grid-st", "15", "17", "--all-bs", "--bootstrap-out", out, "--funits", units])
    assert rc == 0 and os.path.exists(out)
    table, _, _ = mio.read_jsfs(out)
    assert same_bits(np.array(table), block_bootstrap_table(chunks, 8, seed=3))       # the file reads back as the table, exactly
    rc2, text2 = run_cli([f1, f2, out, "16", "--grid-st", "15", "17", "--all-bs", "--funits", units])
    lines = lambda t: [l for l in t.splitlines() if l.startswith("bs_id =") or l.startswith("best:") or l.startswith("bootstrap:")]
    assert rc2 == 0 and lines(text2) == lines(text)
    assert len([l for l in lines(text) if l.startswith("bs_id =")]) == 3 * 9 and any(l.startswith("bootstrap:") for l in lines(text))
    assert "Bootstrap: 8 replicates of 5 chunks" in text
