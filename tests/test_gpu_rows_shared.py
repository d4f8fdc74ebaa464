"""What the three row sources share on the host: the context itself (misti_ctx.h) - its stream, its chunk-table buffer
(misti_boot.hip: upload_chunks, behind the bootstrap and the jackknife) and its draw-count buffer (misti_parametric.hip).  Six calls
one after another on ONE context: a small chunk table, a large one that makes the buffer grow and needs a second tile of the
jackknife, the same large one on the bootstrap's unstaged path (above BOOT_STAGED_MAX_CHUNKS), the small one again in the buffer
the large one left, the parametric rows with a partial last Philox block, and the first call once more.  Every result must equal its
rule in NumPy (optimize.block_bootstrap, jackknife_rows, parametric_rows) bit for bit, and the first call must equal itself.

Counts and lengths are integers that differ from chunk to chunk: a table that is stale, or that lies where another one was, changes
sums that are exact - nothing hides in rounding."""
import numpy as np
import pytest

from test_bootstrap_rows_cpu import small_table
from test_gpu_parametric_rows import GENOME, P0, same_bits, small_input

pytestmark = pytest.mark.gpu

SMALL = small_table(np.random.default_rng(3), 3)
LARGE = small_table(np.random.default_rng(1030), 1030)


@pytest.fixture(scope="module")
def world():
    """({name: rows of the device}, {name: rows of the rule}): the six calls on one context, in this order; each rule once."""
    from misti_amd.engine import Engine
    from misti_amd.optimize import block_bootstrap, jackknife_rows, parametric_rows
    inp = small_input()
    got = {}
    with Engine(inp.times, inp.lambdas) as e:
        got["boot_small"] = e.bootstrap_rows_dev(SMALL, 5, seed=11).cpu().numpy()
        got["jack_large"] = e.jackknife_rows_dev(LARGE, 7).cpu().numpy()
        got["boot_large"] = e.bootstrap_rows_dev(LARGE, 5, seed=12).cpu().numpy()
        got["boot_small_after_large"] = e.bootstrap_rows_dev(SMALL, 5, seed=13).cpu().numpy()
        got["parametric"] = e.parametric_rows_dev(P0, 3, 1001, GENOME, seed=5).cpu().numpy()
        got["boot_small_again"] = e.bootstrap_rows_dev(SMALL, 5, seed=11).cpu().numpy()
    want = {"boot_small": block_bootstrap(SMALL, 5, seed=11), "jack_large": jackknife_rows(LARGE, 7),
            "boot_large": block_bootstrap(LARGE, 5, seed=12), "boot_small_after_large": block_bootstrap(SMALL, 5, seed=13),
            "parametric": parametric_rows([P0], 3, 1001, GENOME, seed=5)[0]}
    want["boot_small_again"] = want["boot_small"]
    return got, want


@pytest.mark.parametrize("name", ["boot_small", "jack_large", "boot_large", "boot_small_after_large", "parametric", "boot_small_again"])
def test_every_call_equals_its_numpy_rule(world, name):
    got, want = world
    print(name, got[name].shape, got[name].ravel()[:8], want[name].ravel()[:8])
    assert same_bits(got[name], want[name]), name


def test_the_first_call_is_the_same_before_and_after_the_others(world):
    got = world[0]
    assert same_bits(got["boot_small"], got["boot_small_again"])
    # the sequence went where it says: 148 groups of the large table (a second tile: 1 030 > 1 024), tables of different sums
    assert got["jack_large"].shape == (148, 8) and got["boot_small"].shape == got["boot_large"].shape == (5, 8)
    assert SMALL[:, 0].sum() != LARGE[:, 0].sum() and len(set(SMALL[:, 0])) == 3
    assert (got["parametric"][:, 1:].sum(axis=1) == 1001).all() and 1001 % 4 != 0
