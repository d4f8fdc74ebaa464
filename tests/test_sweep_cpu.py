"""Named sweeps without a GPU: the refusals of `--sweep`, the expansion of the reference's GNU-parallel recipe (README.md:110-115 of
the reference) into per-model split times, band bounds and parameter slots, the SetModel filter against a transcription of the
reference's checks, optimize.sweep_interval against bootstrap_profile_interval, and misti_nm_solve_bounds' argument errors through
the loaded library."""
import ctypes as C

import numpy as np
import pytest

RECIPE = ("{st} -uf -mi 1 0 {mc} {mi1} 0 -mi 2 0 {mc} {mi2} 0 -mi 1 {mc} {st} {mi3} 0 -mi 2 {mc} {st} {mi4} 0 "
          "--sweep st 20 21 22 23 24 25 --sweep mc 8 9 10 11 12 --sweep mi1 00.0 00.5 02.0 05.0 --sweep mi2 05.0 10.0 15.0 20.0 "
          "--sweep mi3 00.0 00.5 02.0 05.0 --sweep mi4 01.0 05.0 10.0 15.0")


def parse(tail):
    from misti_amd import cli
    return cli.build_parser().parse_args(["g1.psmc", "g2.psmc", "sim.jafs"] + tail.split())


@pytest.mark.parametrize("tail, why", [
    ("{st} -mi 1 4 {st} 0.1 0", "{st} is used but not declared: add --sweep st"),
    ("20 -mi 1 4 20 0.1 0 --sweep st 20 21", "--sweep st: the name is declared but {st} is used nowhere"),
    ("{st} -mi 1 4 {st} 0.1 0 --sweep st 20 --sweep st 21", "--sweep st: the name is declared twice"),
    ("20 -mi 1 {mc} 20 0.1 0 --sweep mc 8 8.5", "--sweep mc: 8.5 is not an integer, and {mc} is a band start or end"),
    ("{st} -mi 1 4 {st} 0.1 0 --sweep st 20 x", "--sweep st: x is not a number"),
    ("{st} -mi 1 4 {st} 0.1 0 -pu 1 {t} 0.1 0 --sweep st 20 --sweep t 5", "a pulse takes no placeholder (per-candidate pulse times"),
    ("{st} -mi 1 4 {st} 0.1 0 --sweep st 20 21 --grid-st 18 20", "--sweep and --grid-st exclude each other: write the split time as {st}"),
    ("20 -mi 1 4 20 {r} 1 --sweep r 0.1 --grid-mi 0 0.01 1 3", "--sweep and --grid-mi exclude each other: write the rate of that -mi as {NAME}"),
    ("{st} -mi 1 4 {st} 0.1 0 --sweep st 20 21 --gpus 2", "--sweep runs on one GPU (--device): the sharded gathers"),
    ("{st} -mi 1 4 {st} 0.1 0 --sweep st 20 21 --devices 0,1", "--sweep runs on one GPU (--device): the sharded gathers"),
    ("{st} -mi 1 4 {st} {r} 0 -mi 2 4 {st} 0.1 1 --sweep st 20 --sweep r 0.1 --grid-solve", "--grid-solve: {r} is the rate of a fixed band"),
    ("{st} -mi {p} 4 {st} 0.1 0 --sweep st 20 --sweep p 1", "placeholders stand in the split time and in the start, end and rate fields"),
    ("{st} -mi 1 {x} {st} {x} 0 --sweep st 20 --sweep x 4", "{x} stands in a rate field and in a time field"),
    ("{st} -mi 1 4 {st} 0.1 0 --sweep st 20 --grid-solve", "--grid-solve needs at least one optimised parameter"),
    # an evaluation would print `optim = [initial value]` for a rate the reference fits: optimised parameters need --grid-solve
    ("{st} -mi 1 4 {st} {r} 1 --sweep st 20 21 --sweep r 0.1 0.2",
     "-mi 1 4 {st} {r} 1 is optimised (flag 1): --sweep alone evaluates fixed models; add --grid-solve"),
    ("{st} -mi 1 4 {st} 0.1 0 -mi 2 4 {st} 0.2 1 --sweep st 20 21", "-mi 2 4 {st} 0.2 1 is optimised (flag 1)"),
    ("{st} -mi 1 4 {st} 0.1 0 -pu 1 6 0.1 1 --sweep st 20 21", "-pu 1 6 0.1 1 is optimised (flag 1)"),
])
def test_refusals(capsys, tail, why):
    """Each refusal is one line on stderr, before any file is read (none of the inputs exist) or the GPU is touched."""
    from misti_amd import cli
    rc = cli.main(["a.psmc", "b.psmc", "d.sfs"] + tail.split())
    err = capsys.readouterr().err
    assert rc == 2 and why in err, err
    assert len(err.strip().splitlines()) == 1


def test_command_lines_without_placeholders_are_unchanged():
    from misti_amd.sweep import sweep_error
    a = parse("19.5 -mi 1 4 20 0.1 1 --grid-st 18 20 --all-bs")
    assert a.st == 19.5 and isinstance(a.st, float) and a.sweep == [] and sweep_error(a) is None
    with pytest.raises(SystemExit):                      # a bad split is argparse's error, as before
        parse("abc")


def test_recipe_expansion():
    from misti_amd.sweep import expand, sweep_error
    a = parse(RECIPE)
    assert sweep_error(a) is None
    p = expand(a)
    assert p.n_model == 6 * 5 * 4 ** 4 == 7680
    assert p.k == 0 and p.n_param == 4                       # four fixed swept rates: four parameter slots, no optimised one
    assert [b[4] for b in p.bands] == [0, 1, 2, 3] and [b[0] for b in p.bands] == [0, 1, 0, 1]
    # GNU parallel's order: the first sweep outermost, the last innermost
    assert p.assign[0] == dict(st="20", mc="8", mi1="00.0", mi2="05.0", mi3="00.0", mi4="01.0")
    assert p.assign[1]["mi4"] == "05.0" and p.assign[4]["mi3"] == "00.5" and p.assign[4]["mi4"] == "01.0"
    assert p.assign[4 ** 4]["mc"] == "9" and p.assign[5 * 4 ** 4]["st"] == "21"
    st = np.repeat([20.0, 21, 22, 23, 24, 25], 5 * 256)
    mc = np.tile(np.repeat([8, 9, 10, 11, 12], 256), 6)
    assert np.array_equal(p.split, st)
    # bounds: [0, mc) for the first two bands, [mc, split) - end -1 - for the last two
    want = np.stack([np.stack([np.zeros_like(mc), mc], 1), np.stack([np.zeros_like(mc), mc], 1),
                     np.stack([mc, -np.ones_like(mc)], 1), np.stack([mc, -np.ones_like(mc)], 1)], 1)
    assert p.bounds.dtype == np.int32 and np.array_equal(p.bounds, want)
    # the fixed rates, moved into the parameter slots: the same doubles as the literal values
    grid = np.array(np.meshgrid([0.0, 0.5, 2.0, 5.0], [5.0, 10.0, 15.0, 20.0], [0.0, 0.5, 2.0, 5.0], [1.0, 5.0, 10.0, 15.0], indexing="ij"))
    assert np.array_equal(p.params, np.tile(grid.reshape(4, -1).T, (30, 1)))
    # the -mi options as the single run of that model would have them (what the result line prints)
    assert p.mi[1] == [["1", "0", "8", "00.0", "0"], ["2", "0", "8", "05.0", "0"], ["1", "8", "20", "00.0", "0"], ["2", "8", "20", "05.0", "0"]]
    assert np.array_equal(p.values[:, :2], np.stack([st, mc], 1))


def test_grid_solve_expansion():
    """--grid-solve: the time variables make the models, the rate variables of optimised bands the starts."""
    from misti_amd.sweep import expand, sweep_error
    a = parse("{st} -mi 1 2 {mc} {r} 1 -mi 2 {mc} {st} 0.25 1 -mi 1 {mc} {st} 0.5 0 --sweep st 19.5 20 --sweep r 0.1 0.2 0.3 "
              "--sweep mc 3 4 --grid-solve --all-bs")
    assert sweep_error(a) is None
    p = expand(a)
    assert p.model_names == ["st", "mc"] and p.rate_names == ["r"]
    assert p.n_model == 4 and p.k == 2 and p.n_param == 2
    assert np.array_equal(p.split, [19.5, 19.5, 20, 20])
    assert np.array_equal(p.bounds[1], [[2, 4], [4, -1], [4, -1]])
    assert np.array_equal(p.starts, [[0.1, 0.25], [0.2, 0.25], [0.3, 0.25]])
    assert [b[4] for b in p.bands] == [0, 1, -1] and p.bands[2][3] == 0.5


def test_only_flag_one_is_optimised():
    """SetModel optimises a band or pulse whose flag is exactly 1 (migOpt == 1); the checks and the expansion agree on it: a rate
    placeholder under flag 2 is a fixed rate - its own parameter slot, refused by --grid-solve - and the same line with flag 1
    needs --grid-solve and then makes the starts."""
    from misti_amd.sweep import expand, sweep_error
    a = parse("{st} -mi 1 4 {st} {r} 2 -pu 2 6 0.1 2 --sweep st 20 21 --sweep r 0.1 0.2")
    assert sweep_error(a) is None
    p = expand(a)
    assert p.k == 0 and p.n_param == 1 and p.bands[0][4] == 0 and p.pulses[0][3] == -1
    assert p.model_names == ["st", "r"] and np.array_equal(p.params[:, 0], [0.1, 0.2, 0.1, 0.2])
    assert "is the rate of a fixed band" in sweep_error(parse("{st} -mi 1 4 {st} {r} 2 -mi 2 4 {st} 0.1 1 --sweep st 20 --sweep r 0.1 --grid-solve"))
    a = parse("{st} -mi 1 4 {st} {r} 1 -pu 2 6 0.1 2 --sweep st 20 21 --sweep r 0.1 0.2 --grid-solve")
    assert sweep_error(a) is None
    p = expand(a)
    assert p.k == 1 and p.n_param == 1 and p.pulses[0][3] == -1 and p.model_names == ["st"]
    assert np.array_equal(p.starts, [[0.1], [0.2]])


def reference_set_model(split, mis, sample_date, n_times):
    """MigrationInference.__init__ (:85-107) and SetModel (:229-255) of the reference, transcribed: True where it would run, False
    where it exits in PrintError or fails with IndexError.  ``mis`` are (pop 0/1, start, end) with end -1 = the split index."""
    if split < sample_date:
        return False
    frac, s = split % 1, int(split)
    if s - 1 > n_times:
        return False
    numT = n_times + 1
    if frac != 0.0:
        if s >= n_times:
            return False                         # times[splitT]: IndexError
        numT += 1
        s += 1
    mi = [[None, None] for _ in range(numT)]
    for pop, start, end in mis:
        end = s if end == -1 else end
        if start < sample_date or end <= start:
            return False
        for i in range(start, end):
            if i >= numT:
                return False                     # self.mi[i]: IndexError
            if mi[i][pop] is not None:
                return False
            mi[i][pop] = 0.0
    return True


def test_structure_filter_against_set_model():
    from misti_amd.sweep import structure_error
    rng = np.random.default_rng(5)
    numT, pops = 12, [0, 1, 0]
    n_bad = 0
    for _ in range(4000):
        split = float(rng.integers(4, 14)) + (0.5 if rng.random() < 0.3 else 0.0)
        sd = int(rng.random() < 0.2)
        b = rng.integers(0, 8, size=(3, 2))
        b[:, 1] = b[:, 0] + rng.integers(-1, 5, size=3) + (b[:, 0] >= 4) * 4       # mostly after the start, sometimes beyond the grid
        b[rng.random(3) < 0.3, 1] = -1
        want = reference_set_model(split, [(p, int(s), int(e)) for p, (s, e) in zip(pops, b)], sd, numT - 1)
        got = structure_error(split, b, pops, sd, numT)
        assert (got is None) == want, (split, b.tolist(), sd, got)
        n_bad += got is not None
    assert 400 < n_bad < 3600, n_bad


def test_sweep_interval_equals_bootstrap_profile_interval_for_a_split_sweep():
    from misti_amd.optimize import bootstrap_profile_interval, sweep_interval
    rng = np.random.default_rng(17)
    splits = np.array([15.0, 15.5, 16.0, 17.0, 18.0, 19.0])
    for R in (2, 5, 101):
        llh = -1e5 + np.round(rng.normal(size=(R, splits.size)) * 3)      # rounded: ties happen
        llh[rng.random(llh.shape) < 0.1] = -np.inf
        llh[R // 2] = -np.inf                                            # a row without a value
        x = rng.random((R, splits.size, 2))
        want = bootstrap_profile_interval(llh, splits, x)
        got = sweep_interval(llh, splits[:, None], x)
        v = got["variables"][0]
        for key in ("data_split", "data_llh", "mean", "interval", "n_boot", "n_excluded"):
            assert v[key] == want[key] or (v[key] is not None and np.array_equal(v[key], want[key], equal_nan=True)), key
        assert np.array_equal(v["best_split"], want["best_split"], equal_nan=True)
        assert np.array_equal(got["data_x"], want["data_x"]) and got["data_llh"] == want["data_llh"]
        assert got["n_boot"] == want["n_boot"] and got["n_excluded"] == want["n_excluded"]
        best = got["best_model"]
        ok = best >= 0
        assert np.array_equal(splits[best[ok]], want["best_split"][ok]) and np.isnan(want["best_split"][~ok]).all()


def test_sweep_interval_per_variable():
    """Two variables: each takes the value of the first best model per row."""
    from misti_amd.optimize import sweep_interval
    values = np.array([[20, 8], [20, 9], [21, 8], [21, 9]], dtype=float)
    llh = np.array([[-5.0, -1.0, -1.0, -3.0],
                    [-2.0, -4.0, -3.0, -1.0],
                    [-1.0, -2.0, -3.0, -4.0],
                    [-3.0, -3.0, -2.0, -9.0]])
    iv = sweep_interval(llh, values)
    assert list(iv["best_model"]) == [1, 3, 0, 2] and iv["data_model"] == 1
    st, mc = iv["variables"]
    assert st["data_split"] == 20 and mc["data_split"] == 9
    assert st["mean"] == np.mean([21, 20, 21]) and mc["mean"] == np.mean([9, 8, 8])


def test_nm_solve_bounds_rejects_its_arguments_through_the_library():
    from misti_amd import _lib
    lib = _lib.load()
    d = (C.c_double * 16)()
    i = (C.c_int32 * 8)()
    rc = lib.misti_nm_solve_bounds(None, 1, d, d, i, i, 1, d, 1e-4, 1e-4, 10, d, d, None, None, None)
    assert rc == -1                                   # MISTI_E_ARG
    assert b"ctx is NULL" in lib.misti_last_error()
