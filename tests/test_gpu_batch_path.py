"""The head and the end of a batch: the chain order the last block of setup_kernel writes (its histogram over the chain lengths, its
prefix sum, its strided loops over the chains) and the one event a lane batch leaves behind it (misti_lanes.cpp reads the context's).

Everything runs on the numT = 32 grid of tests/test_gpu_lane_priorities.py: one band that follows the split, its rate the one parameter,
--cpfit.  A chain is a parameter vector; its length is the largest split among its members.  Every chain case is evaluated on a fresh
context, on a second fresh context, and with its candidates reversed (and the results turned back): llk, jafs and status are the same
bits each time - no result may depend on where a chain stands in the dispatch order or on which context ran it.  No time is asserted."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NUMT = 32
ROWS = np.array([[3e7, 9000, 2500, 10000, 6000, 4000, 2600, 4100], [2.9e7, 9100, 2400, 10100, 6100, 3900, 2500, 4000]])
KW = dict(bands=[(0, 4, -1, 0.0, 0)], n_param=1, cpfit=True, smooth=True)


@pytest.fixture(scope="module")
def model():
    from misti_amd import synth
    inp = synth.psmc_pair(16, 17)
    times, lh, _ = synth.self_consistent(inp, 20, [[1, 4, 20, 0.2, 0]], [])
    assert len(lh) == NUMT
    return times, lh


def rates(n):
    return np.logspace(-3, np.log10(0.5), n)


def batch_one_chain():
    """8 candidates, one parameter vector"""
    return np.arange(16, 24, dtype=np.float64), np.full((8, 1), 0.2)


def batch_eight_of_eight():
    """as many chains as candidates: no trunk is built"""
    return np.arange(16, 24, dtype=np.float64), rates(8)[:, None].copy()


def batch_one_length():
    """64 chains, each with the splits 18 and 20: one length"""
    st, rr = np.meshgrid(np.array([18.0, 20.0]), rates(64), indexing="ij")
    return st.ravel().copy(), rr.ravel()[:, None].copy()


def batch_every_length():
    """numT chains; chain j holds the splits j - 3 .. j (from 1 on), so its length is that of split j: every length from 1 to numT"""
    split, par = [], []
    for j, r in zip(range(1, NUMT + 1), rates(NUMT)):
        for s in range(max(1, j - 3), j + 1):
            split.append(float(s))
            par.append(r)
    return np.array(split), np.array(par)[:, None]


def batch_257_chains():
    """257 chains of two members each: one more than the last block has threads; eight lengths"""
    r = np.linspace(0.01, 0.5, 257)
    split = np.concatenate([16.0 + np.arange(257) % 8, 14.0 + np.arange(257) % 8])
    return split, np.concatenate([r, r])[:, None]


def batch_300_of_one():
    return 16.0 + np.arange(300) % 8, np.full((300, 1), 0.2)


def batch_300_of_300():
    return 16.0 + (np.arange(300) * 5) % 8, np.linspace(0.01, 0.5, 300)[:, None].copy()


def run(model, batches, reverse=False):
    """the batches one after the other on ONE fresh context"""
    from misti_amd.engine import Engine
    out = []
    with Engine(*model, **KW) as e:
        for split, par in batches:
            r = e.evaluate(split[::-1].copy(), par[::-1].copy(), ROWS) if reverse else e.evaluate(split, par, ROWS)
            got = (r.llk, r.jafs, r.status)
            out.append(tuple(a[::-1] for a in got) if reverse else got)
    return out


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


CASES = {"one_chain": [batch_one_chain], "eight_of_eight": [batch_eight_of_eight], "one_length": [batch_one_length],
         "every_length": [batch_every_length], "chains_257": [batch_257_chains], "stale_hint_pair": [batch_300_of_one, batch_300_of_300]}


@pytest.mark.parametrize("name", list(CASES))
def test_chain_order_leaves_no_trace_in_the_results(model, name):
    batches = [make() for make in CASES[name]]
    first, again, turned = run(model, batches), run(model, batches), run(model, batches, reverse=True)
    for k, (split, par) in enumerate(batches):
        llk, jafs, status = first[k]
        assert llk.shape == (split.size, ROWS.shape[0]) and jafs.shape == (split.size, 7) and status.shape == (split.size,)
        assert (status == 0).any() and np.isfinite(llk[status == 0]).all(), (name, k)     # a computation, not a table of failures
        assert same(first[k], again[k]), (name, k, "a second fresh context")
        assert same(first[k], turned[k]), (name, k, "candidates reversed")
    if name == "stale_hint_pair":
        # the second batch met the hint {1 chain, 300 candidates} of the first: alone on a fresh context it gives the same bits
        assert same(first[1], run(model, batches[1:])[0])


# ---- lane state with one event per batch --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lane_case(model):
    """16 candidates (4 splits x 4 rates), two grids, and what a plain context makes of them"""
    import torch
    from misti_amd.engine import Engine
    st, rr = np.meshgrid(np.arange(18, 22, dtype=np.float64), rates(4), indexing="ij")
    split, par = st.ravel().copy(), [rr.ravel()[:, None].copy() * f for f in (1.0, 1.07)]
    want = []
    for p in par:                                       # a fresh context each
        with Engine(*model, **KW) as e:
            want.append(e.evaluate(split, p, ROWS))
    dev = torch.device("cuda", 0)
    d = dict(split=torch.as_tensor(split, device=dev), par=[torch.as_tensor(p, device=dev).contiguous() for p in par],
             rows=torch.as_tensor(ROWS, device=dev).contiguous())
    torch.cuda.synchronize()
    return dict(n=split.size, R=ROWS.shape[0], dev=dev, d=d, want=want)


def issue(pool, c, lane, g):
    import torch
    llk = torch.empty((c["n"], c["R"]), dtype=torch.float64, device=c["dev"])
    jafs = torch.empty((c["n"], 7), dtype=torch.float64, device=c["dev"])
    st = torch.empty(c["n"], dtype=torch.int32, device=c["dev"])
    used = pool.evaluate_dev(lane, c["n"], c["d"]["split"].data_ptr(), c["d"]["par"][g].data_ptr(), c["R"], c["d"]["rows"].data_ptr(), llk.data_ptr(),
                             jafs.data_ptr(), 0, 0, st.data_ptr())
    return used, g, (llk, jafs, st)


def right(c, g, out):
    w = c["want"][g]
    return same([t.cpu().numpy() for t in out], (w.llk, w.jafs, w.status))


def test_lane_is_idle_before_a_batch_and_after_sync(model, lane_case):
    from misti_amd.engine import Lanes
    c = lane_case
    with Lanes(*model, lanes=2, **KW) as pool:
        assert not pool.busy(0) and not pool.busy(1)
        _, g, out = issue(pool, c, 0, 0)
        pool.sync()
        assert not pool.busy(0) and not pool.busy(1)
        assert right(c, g, out)
        pool.wait(1)                                     # a lane that never had a batch: nothing to wait for
        assert not pool.busy(1)


def test_lane_any_picks_the_idle_lane(model, lane_case):
    """Lane 0 holds a batch - queued behind device work on its stream that outlasts the next two calls by far - so MISTI_LANE_ANY,
    whose round-robin position is lane 0, has to take lane 1."""
    import torch
    from misti_amd.engine import Lanes
    c = lane_case
    with Lanes(*model, lanes=2, **KW) as pool:
        ballast = torch.zeros(64 * 1024 * 1024, dtype=torch.float32, device=c["dev"])
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.ExternalStream(pool.engine(0).stream_handle(), device=c["dev"])):
            for _ in range(200):
                ballast.add_(1.0)
        used0, g0, out0 = issue(pool, c, 0, 0)
        assert used0 == 0 and pool.busy(0) and not pool.busy(1)
        used1, g1, out1 = issue(pool, c, None, 1)
        assert used1 == 1
        pool.sync()
        assert not pool.busy(0) and not pool.busy(1)
        assert right(c, g0, out0) and right(c, g1, out1)
        assert float(ballast[0]) == 200.0


def test_rejected_call_leaves_the_lane_idle(model, lane_case):
    import torch
    from misti_amd._lib import MistiError
    from misti_amd.engine import Lanes
    c = lane_case
    with Lanes(*model, lanes=2, **KW) as pool:
        for round_ in range(2):                           # on a lane without a batch, and on one whose last batch is complete
            with pytest.raises(MistiError, match="llk is NULL"):
                pool.evaluate_dev(0, c["n"], c["d"]["split"].data_ptr(), c["d"]["par"][0].data_ptr(), c["R"], c["d"]["rows"].data_ptr(), 0)
            assert not pool.busy(0)
            pool.wait(0)
            _, g, out = issue(pool, c, 0, round_)
            pool.sync()
            assert not pool.busy(0)
            assert right(c, g, out)


def test_two_batches_back_to_back_on_one_lane(model, lane_case):
    from misti_amd.engine import Lanes
    c = lane_case
    with Lanes(*model, lanes=2, **KW) as pool:
        a = issue(pool, c, 1, 0)
        b = issue(pool, c, 1, 1)
        pool.wait(1)
        assert not pool.busy(1) and not pool.busy(0)
        assert right(c, a[1], a[2]) and right(c, b[1], b[2])
