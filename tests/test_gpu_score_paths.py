"""The paths that score spectra against replicate rows share their pieces (misti_score.h: the class fold of a row and of a spectrum, the
staged chunk of class logs, the fused multiply-add chain).  One hand-made input at the edges of those pieces goes through every path:
the table (misti_llk_dev) reduced by misti_argmax_dev, the scan at k = 1 (misti_scan_best_dev) and the profile with every candidate in
one group (misti_scan_profile_dev) - index and value bit for bit, whatever the slice count - and the table against the formula in NumPy.

65 candidates are one more than the 64-candidate chunk (the second chunk holds one); candidates 3 and 64 have no value (status != 0) and
candidate 10 has class 3 equal to 0.0 (log 0 = -inf: no row lists it either).  3, 4 and 257 rows: an odd table (unpaired stores), an even
one (16-byte paired stores) and one row past a 256-thread block (the padding lanes repeat the last row)."""
import numpy as np
import pytest

from test_gpu_llk import grid, host_llk

pytestmark = pytest.mark.gpu

N_CAND, NO_VALUE, ZERO_CLASS = 65, (3, 64), 10


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def hand_made(n_rep):
    c, i = np.arange(N_CAND)[:, None], np.arange(7)[None, :]
    jafs = 1.0 + (5 * c + 3 * i + c * i) % 11
    jafs[ZERO_CLASS, 3] = 0.0
    jafs /= jafs.sum(axis=1, keepdims=True)
    status = np.zeros(N_CAND, dtype=np.int32)
    status[list(NO_VALUE)] = 2
    r = np.arange(n_rep)[:, None]
    rows = np.zeros((n_rep, 8))
    rows[:, 1:] = 1 + (977 * r + 131 * i + 7 * r * i) % 40009          # integer counts, every class present
    rows[:, 0] = rows[:, 1:].sum(axis=1)
    return jafs, status, rows


def every_path(e, jafs, status, rows):
    """(table, {path: (best[n_rep], value[n_rep])}) of one engine."""
    import torch
    dev = torch.device("cuda", 0)
    n_rep = rows.shape[0]
    d_j, d_s, d_r = (torch.as_tensor(a, device=dev) for a in (jafs, status, rows))
    d_group = torch.zeros(N_CAND, dtype=torch.int32, device=dev)
    table = torch.full((N_CAND, n_rep), float("nan"), dtype=torch.float64, device=dev)
    best = {p: torch.full((n_rep,), -7, dtype=torch.int32, device=dev) for p in ("argmax", "scan", "profile")}
    val = {p: torch.full((n_rep,), 7.0, dtype=torch.float64, device=dev) for p in best}
    torch.cuda.synchronize()                          # the engine issues on its own non-blocking stream
    e.llk_dev(N_CAND, d_j.data_ptr(), d_s.data_ptr(), n_rep, d_r.data_ptr(), table.data_ptr())
    e.argmax_dev(N_CAND, n_rep, table.data_ptr(), best["argmax"].data_ptr(), val["argmax"].data_ptr())
    e.scan_best_dev(N_CAND, d_j.data_ptr(), d_s.data_ptr(), n_rep, d_r.data_ptr(), 1, best["scan"].data_ptr(), val["scan"].data_ptr())
    e.scan_profile_dev(N_CAND, d_j.data_ptr(), d_s.data_ptr(), d_group.data_ptr(), 1, n_rep, d_r.data_ptr(), val["profile"].data_ptr(),
                       best["profile"].data_ptr())
    e.sync()
    return table.cpu().numpy(), {p: (best[p].cpu().numpy(), val[p].cpu().numpy()) for p in best}


@pytest.mark.parametrize("unfolded", [False, True], ids=["folded", "unfolded"])
def test_every_path_gives_the_same_best_candidate_and_value(unfolded, monkeypatch):
    from misti_amd.engine import Engine
    inp = grid()
    cases = {n_rep: hand_made(n_rep) for n_rep in (3, 4, 257)}
    got = {}
    for slices in (None, "1", "7"):                   # MISTI_SCAN_SLICES is read once per context
        if slices is None:
            monkeypatch.delenv("MISTI_SCAN_SLICES", raising=False)
        else:
            monkeypatch.setenv("MISTI_SCAN_SLICES", slices)
        with Engine(inp.times, inp.lambdas, unfolded=unfolded) as e:
            got[slices] = {n_rep: every_path(e, *case) for n_rep, case in cases.items()}
    for n_rep, (jafs, status, rows) in cases.items():
        table, paths = got[None][n_rep]
        # the table against the formula (tests/test_gpu_llk.py: its reference and its tolerance), where the formula has a value
        with np.errstate(divide="ignore", invalid="ignore"):
            want, mag = host_llk(jafs, status, rows, unfolded)
        listed = np.ones(N_CAND, dtype=bool)
        listed[list(NO_VALUE) + [ZERO_CLASS]] = False
        assert np.isneginf(table[list(NO_VALUE)]).all() and not (table[ZERO_CLASS] > -np.inf).any(), n_rep
        assert np.isfinite(table[listed]).all(), n_rep
        err = np.abs(table[listed] - want[listed])
        print(n_rep, "largest error / magnitude", float((err / mag[listed]).max()))
        assert (err <= 1e-13 * mag[listed]).all(), (n_rep, float((err / mag[listed]).max()))
        # one best candidate and one value on every path, and no candidate without a value among them
        best, val = paths["argmax"]
        assert best.shape == (n_rep,) and listed[best].all(), (n_rep, best)
        assert same_bits(val, table[best, np.arange(n_rep)]), n_rep
        for slices in got:
            for path in ("scan", "profile"):
                b, v = got[slices][n_rep][1][path]
                assert np.array_equal(b, best), (n_rep, slices, path)
                assert same_bits(v, val), (n_rep, slices, path)
