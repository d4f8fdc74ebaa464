"""Every branch of the pair chain's exponential (pair_expv, misti_pair.h) against 50-digit arithmetic through the forward map
(misti_forward_rates: one exp(M T) v per genome and interval, no solver): the seven Taylor classes and their edges, the
uniformisation series and its hand-over at nbmax = 6, the one-way closed form in divided differences (pair_cascade, both
directions, rate x length up to 3e5, coinciding rates) - and the claim that a lane's bits do not depend on its company in the wave.
The exact values are tests/golden/golden_pair_branches.json.gz (tests/golden/make_pair_branches.py; no mpmath needed here)."""
import gzip
import json
import os

import numpy as np
import pytest

import pair_branches as pb

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx():
    with gzip.open(os.path.join(HERE, "golden", "golden_pair_branches.json.gz"), "rt") as f:
        return json.load(f)


def _engine(m):
    from misti_amd.engine import Engine
    numT = len(m["lh"])
    return Engine(m["times"], m["lh"], [(0, 0, numT - 1, 0.0, 0), (1, 0, numT - 1, 0.0, 1)], [], n_param=2, cpfit=True)


def _forward(e, m, params):
    numT = len(m["lh"])
    lh, pr, status = e.forward_rates([float(numT - 1)] * len(params), params, want_pr=True, hold_mu=False)
    assert (status == 0).all()
    return lh, pr


def test_fixture_covers_what_it_promises(fx):
    assert pb.coverage_forward(fx) >= 1000
    assert fx["bound"] == 2e-13 and fx["norm_floor"] == 1e-280


def test_every_branch_against_50_digits(fx):
    from parity import record
    worst, count, over = {}, {}, []
    for m in fx["models"]:
        params = np.array([c["params"] for c in m["candidates"]])
        with _engine(m) as e:
            _, pr = _forward(e, m, params)
        for ci, c in enumerate(m["candidates"]):
            for t, iv in enumerate(c["intervals"]):
                want = c["exact"][t]
                scale = max(abs(x) for x in want)
                if scale < pb.NORM_FLOOR:
                    continue
                err = max(abs(pr[ci][t + 1][j] - want[j]) for j in range(6)) / scale
                keys = [iv["branch"]] + ["%s_%s" % (iv["branch"], tag) for tag in iv.get("tags", ())]
                if 0.99 <= 2 * iv["nbmax"] / min(pb.TAYLOR_EDGES, key=lambda x: abs(x - 2 * iv["nbmax"])) <= 1.01:
                    keys.append("taylor_edges")
                if 5.9 < iv["nbmax"] <= 6.06:
                    keys.append("hand_over_at_6")
                for k in keys:
                    worst[k] = max(worst.get(k, 0.0), err)
                    count[k] = count.get(k, 0) + 1
                if not err <= pb.W_BOUND:
                    over.append((m["name"], c["params"], t, iv, err))
    for k in sorted(worst):
        print("pair_branches %-28s n=%4d worst=%.3e of bound %.0e" % (k, count[k], worst[k], pb.W_BOUND))
    record("pair_branches_forward", bound=pb.W_BOUND, worst=worst, intervals=count)
    assert set(pb.BRANCHES) <= set(worst)
    assert not over, over[:8]


def test_lanes_do_not_depend_on_their_company(fx):
    """All candidates of a model in one call (full waves of mixed one-way, two-way, stiff and ordinary lanes), the same in reverse
    order, and one per call (a wave with one live lane): bit-identical."""
    for m in fx["models"]:
        params = np.array([c["params"] for c in m["candidates"]])
        n = len(params)
        assert n >= 64
        kinds = {iv["branch"] for c in m["candidates"][:64] for iv in c["intervals"]}
        assert len(kinds) >= 3, kinds
        with _engine(m) as e:
            lh_a, pr_a = _forward(e, m, params)
            lh_r, pr_r = _forward(e, m, params[::-1].copy())
            singles = [_forward(e, m, params[i:i + 1]) for i in range(n)]
        lh_1 = np.concatenate([s[0] for s in singles])
        pr_1 = np.concatenate([s[1] for s in singles])
        bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
        for name, a, b in (("reversed lh", lh_a, lh_r[::-1]), ("reversed pr", pr_a, pr_r[::-1]), ("alone lh", lh_a, lh_1), ("alone pr", pr_a, pr_1)):
            diff = np.argwhere(bits(a) != bits(b))
            assert diff.size == 0, (m["name"], name, len(diff), diff[:4].tolist())
