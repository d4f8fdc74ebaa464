"""The four public sampler rules of misti_amd.optimize (ensemble_rule, ensemble_prior_rule, tempered_rule, tempered_prior_rule) against
tests/golden/golden_sampler_rules.json.gz, bit for bit: the rules are the oracle of the device samplers (tests/test_gpu_ens.py,
test_gpu_pt.py, test_gpu_prior.py), and where one rule is stated through another a comparison between the two says little - the
fixture holds each from outside.  The cases, their objectives and the fixture's coverage live in tests/golden/make_sampler_rules.py."""
import gzip
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_sampler_rules as gen         # noqa: E402

KEYS = {"ensemble": ["chain", "chain_llh", "accepted", "last", "last_llh", "n_points"],
        "tempered": ["chain", "chain_llh", "accepted", "swap_proposed", "swap_accepted", "last", "last_llh", "rung_llh", "logz", "n_points"]}


@pytest.fixture(scope="module")
def fx():
    with gzip.open(gen.OUT, "rt") as f:
        return json.load(f)


def test_the_fixture_reaches_what_it_promises(fx):
    n = gen.coverage(fx)
    assert len(fx["cases"]) == len(gen.cases()) == 19
    assert n["parity0"] >= 1 and n["parity1"] >= 1 and n["outside"] >= 1 and n["inf"] >= 1 and n["nan"] >= 1
    assert os.path.getsize(gen.OUT) < os.path.getsize(os.path.join(HERE, "golden", "golden_exact_forward.json.gz")) // 2


@pytest.mark.parametrize("case", gen.cases(), ids=lambda c: "%s-%s" % (c["rule"], c["name"]))
def test_every_array_of_the_rule_bit_for_bit(fx, case):
    want = [r for r in fx["cases"] if (r["rule"], r["name"]) == (case["rule"], case["name"])]
    assert len(want) == 1
    want = want[0]
    got, saw = gen.run(case)
    assert list(got) == KEYS[case["rule"].split("_")[0]] == list(want["out"])        # the keys and their order
    assert saw == want["saw"]
    for k, v in got.items():
        w = want["out"][k]
        if k == "n_points":
            assert isinstance(v, int) and v == w
            continue
        v = np.asarray(v)
        assert list(v.shape) == w["shape"], (k, v.shape, w["shape"])
        if "bits" in w:
            assert v.dtype == np.float64 and np.ascontiguousarray(v).reshape(-1).view(np.uint64).tolist() == w["bits"], k
        else:
            assert v.dtype == np.int32 and v.reshape(-1).tolist() == w["ints"], k
