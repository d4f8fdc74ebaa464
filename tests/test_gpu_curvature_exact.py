"""misti_curvature (Engine.curvature) and misti_curvature_assemble_dev against exact derivatives of the model's own spectrum: the smooth
model (cpfit, true_eps - the exact-spectrum engine), every point and every relative step of
tests/golden/golden_curvature_exact.json.gz (tests/golden/make_curvature_exact.py; nothing but that fixture is read).

 1. Device against the EXACT STENCIL at the same h - the rule of optimize.curvature_from_spectra applied in 50-digit arithmetic to the
    exact spectra of the device's own candidates - within the bound DERIVED in tests/curvature_exact.py from what
    tests/test_gpu_exact_spectrum.py holds the spectra to.  That isolates the kernels from truncation: it holds at every step of the
    ladder, at the point whose stencil straddles the series / contour switch (q = 96) and at the rate of 1e-6.  Where the bound
    exceeds the value (small steps) the assertion is vacuous; the printed lines say where.
 2. Bit-level facts: the Hessian symmetric, llh0 evaluate's value, the boundary point status 7 and NaN with its neighbour untouched,
    all points in one call and each alone the same bits.
 3. Standard errors from the device's Hessian and from the exact stencil's at the same h within cond(H) |dH| / |H|, dH the bound of
    1., wherever that is below 0.1.

 4. Through the lambda-correction (cpfit, true_eps off), where S(theta) is defined by where a trust-region iteration stops: three models
    against the derivatives of the spectrum taken with the 100-digit root of the cpfit system.  No bound can be derived there; the
    fixture holds the error of the project's float64 oracle (SciPy's least_squares) over the same stencils, and the device is allowed
    SELF_FACTOR (tests/parity.py) times that, per entry, plus the bound of 1. - only at entries where the oracle's own error is below
    10 % of the exact value; the others are reported.

Every figure is printed before it is asserted (lines `curvature_exact ...`; profiles/curvature_exact.txt).  The truncation itself
needs no GPU: tests/test_curvature_exact_cpu.py."""
import numpy as np
import pytest

import curvature_exact as cx
from parity import SELF_FACTOR

pytestmark = pytest.mark.gpu

FX = cx.load()
POINTS = cx.points(FX)
IDS = ["%s-%s" % (m["name"], p["name"]) for m, p in POINTS]
FIELDS = ("llh0", "grad", "hess", "dlog", "status")
N_ROWS = 17


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _engine(m, true_eps=True):
    from misti_amd.engine import Engine
    return Engine(m["times"], m["lh"], [tuple(b) for b in m["bands"]], [tuple(p) for p in m["pulses"]], n_param=m["n_param"],
                  cpfit=True, true_eps=true_eps, unfolded=m["unfolded"], sample_date=m["sample_date"])


def _through_assemble(e, m, p, s, table):
    """The step's stencil through Engine.evaluate and misti_curvature_assemble_dev: d2log (which misti_curvature does not return)
    with dlog, grad, hess and the point status, and the llk of the centre against row 0."""
    import torch
    dev = torch.device("cuda", 0)
    D = m["n_param"]
    pts = np.array(s["stencil"])
    res = e.evaluate(np.full(len(pts), p["split"]), pts, table)
    up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=dev)
    d_j, d_s, d_h = up(res.jafs, np.float64), up(res.status, np.int32), up(np.array(s["h"]), np.float64)
    d_r, d_t = up(np.zeros(1), np.int32), up(table, np.float64)
    outs = {k: torch.full(shape, 7.0, dtype=torch.float64, device=dev)
            for k, shape in (("dlog", (1, D, 7)), ("d2log", (1, D, D, 7)), ("grad", (1, D)), ("hess", (1, D, D)))}
    pst = torch.full((1,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    e.curvature_assemble_dev(1, d_j.data_ptr(), d_s.data_ptr(), d_h.data_ptr(), d_r.data_ptr(), table.shape[0], d_t.data_ptr(),
                             outs["dlog"].data_ptr(), outs["d2log"].data_ptr(), outs["grad"].data_ptr(), outs["hess"].data_ptr(), pst.data_ptr())
    e.sync()
    return {k: v.cpu().numpy()[0] for k, v in outs.items()}, int(pst.cpu().numpy()[0]), float(res.llk[0, 0])


@pytest.fixture(scope="module")
def device():
    """Every device result the tests below need, computed once: per model and (abs_step, rel_step) one misti_curvature call over all
    the model's points of that step (their tables stacked: point i takes row 17 i), one call per point alone, and per point the stencil
    through evaluate and the assembly."""
    out = {}
    for m in FX["models"]:
        with _engine(m) as e:
            groups = {}
            for p in m["points"]:
                for rel in ([s["rel_step"] for s in p["steps"]] if not p["boundary"] else [cx.DEFAULT_STEP]):
                    groups.setdefault((p["abs_step"], rel), []).append(p)
            for (abs_step, rel), ps in groups.items():
                tables = [np.array(p.get("table", ps[0]["table"]), dtype=np.float64) for p in ps]   # a boundary point scores nothing
                x, splits = np.array([p["x"] for p in ps]), np.array([p["split"] for p in ps])
                rows = (N_ROWS * np.arange(len(ps))).astype(np.int32)
                together = e.curvature(x, splits, rows, np.vstack(tables), rel_step=rel, abs_step=abs_step)
                for i, p in enumerate(ps):
                    alone = e.curvature(x[i:i + 1], splits[i:i + 1], [0], tables[i], rel_step=rel, abs_step=abs_step)
                    rec = dict(together={k: getattr(together, k)[i] for k in FIELDS}, alone={k: getattr(alone, k)[0] for k in FIELDS},
                               h=alone.h[0])
                    if not p["boundary"]:
                        s = next(s for s in p["steps"] if s["rel_step"] == rel)
                        rec["assembled"], rec["assembled_status"], rec["llk0"] = _through_assemble(e, m, p, s, tables[i])
                    out[(m["name"], p["name"], rel)] = rec
    return out


def _want(p, s, unfolded):
    g = cx.exact_contract(s["dlog"], p["table"][0], unfolded)
    H = cx.exact_contract(s["d2log"], p["table"][0], unfolded)
    return dict(dlog=cx.pad7(cx.arr(s["dlog"])), d2log=cx.pad7(cx.arr(s["d2log"])), grad=cx.arr(g), hess=cx.arr(H))


@pytest.mark.parametrize("mp_", POINTS, ids=IDS)
def test_device_meets_the_exact_stencil_within_the_derived_bound(mp_, device):
    m, p = mp_
    unf = m["unfolded"]
    exact = _want(p, p["exact"], unf)
    failures = []
    for s in p["steps"]:
        rec = device[(m["name"], p["name"], s["rel_step"])]
        got = dict(dlog=rec["alone"]["dlog"], d2log=rec["assembled"]["d2log"], grad=rec["alone"]["grad"], hess=rec["alone"]["hess"])
        assert rec["alone"]["status"] == 0 and rec["assembled_status"] == 0 and same_bits(rec["h"], np.array(s["h"]))
        want = _want(p, s, unf)
        b = cx.bounds(cx.arr(s["jafs"]), np.array(s["h"]), unf, p["table"][0])
        line = "curvature_exact device %-16s %-15s rel_step %-6g" % (m["name"], p["name"], s["rel_step"])
        for k in ("dlog", "d2log", "grad", "hess"):
            err = np.abs(got[k] - want[k])
            scale = np.abs(exact[k]).max()
            over = float((err[b[k] > 0] / b[k][b[k] > 0]).max())
            vacuous = int((b[k] >= np.abs(want[k]))[b[k] > 0].sum())          # entries whose bound exceeds the value itself
            line += " | %s err/stencil %.1e bound %.1e (%d of %d entries vacuous) err/exact %.1e" % (
                k, err.max() / scale, b[k].max() / scale, vacuous, int((b[k] > 0).sum()), np.abs(got[k] - exact[k]).max() / scale)
            if not (np.isfinite(got[k]).all() and (err <= b[k]).all()):
                failures.append((s["rel_step"], k, over))
        print(line)
        # the assembly's other outputs are held to the same bound: the spectra came through evaluate instead of the driver
        for k in ("dlog", "grad", "hess"):
            assert (np.abs(rec["assembled"][k] - want[k]) <= b[k]).all(), (s["rel_step"], k, "assembled")
    assert not failures, failures


def test_bit_level_facts(device):
    checked, saw_boundary = 0, False
    for (model, point, rel), rec in device.items():
        p = next(p for m in FX["models"] if m["name"] == model for p in m["points"] if p["name"] == point)
        a, t = rec["alone"], rec["together"]
        # (this is also "the boundary point's neighbour is untouched": one_step_inside shares its call with one_step_outside, and
        #  must be, bit for bit, what it is alone)
        for k in FIELDS:
            assert same_bits(a[k], t[k]), (model, point, rel, k, "all points in one call against the point alone")
        if p["boundary"]:
            assert a["status"] == 7 and all(np.isnan(a[k]).all() for k in ("llh0", "grad", "hess", "dlog")), (model, point)
            saw_boundary = True
            continue
        assert a["status"] == 0
        assert same_bits(a["hess"], a["hess"].T) and same_bits(rec["assembled"]["d2log"], np.swapaxes(rec["assembled"]["d2log"], 0, 1))
        assert same_bits(a["llh0"], np.float64(rec["llk0"])), (model, point, rel, "llh0 is evaluate's value")
        checked += 1
    assert saw_boundary and checked > 30 and ("two_way_folded", "one_step_inside", cx.DEFAULT_STEP) in device


@pytest.mark.parametrize("mp_", POINTS, ids=IDS)
def test_standard_errors_within_the_perturbation_bound(mp_, device):
    m, p = mp_
    unf = m["unfolded"]
    table = np.array(p["table"], dtype=np.float64)
    se_exact = cx.arr(p["exact"]["se_observed"]), cx.arr(p["exact"]["se_sandwich"])
    applied = 0
    for s in p["steps"]:
        rec = device[(m["name"], p["name"], s["rel_step"])]
        want = _want(p, s, unf)
        b = cx.bounds(cx.arr(s["jafs"]), np.array(s["h"]), unf, table[0])
        room = cx.se_bound(want["hess"], b["hess"])
        got_se = cx.standard_errors(rec["alone"]["hess"], rec["alone"]["dlog"], table, unf)
        want_se = cx.standard_errors(want["hess"], want["dlog"], table, unf)
        diff = [cx.rel_diff(g, w) for g, w in zip(got_se, want_se)]
        off = [cx.rel_diff(g, w) for g, w in zip(got_se, se_exact)]
        print("curvature_exact se     %-16s %-15s rel_step %-6g observed: device/stencil %.1e device/exact %.1e | sandwich: device/stencil %.1e "
              "device/exact %.1e | bound %.1e%s" % (m["name"], p["name"], s["rel_step"], diff[0], off[0], diff[1], off[1], room,
                                                    "" if room < cx.SE_BOUND_APPLIES else " (left out)"))
        if room < cx.SE_BOUND_APPLIES:
            applied += 1
            assert max(diff) <= room, (s["rel_step"], diff, room)
        if s["rel_step"] in (1e-2, 1e-3) and not p["tiny_rate"]:
            assert room < cx.SE_BOUND_APPLIES, "the fixture promises that the bound applies here"
    assert applied or p["tiny_rate"]


# ---- 4. through the lambda-correction ------------------------------------------------------------------------------------------------
CORRECTION = FX["correction"]


@pytest.mark.parametrize("c", CORRECTION, ids=[c["model"] for c in CORRECTION])
def test_through_the_correction_within_the_oracle_s_own_error(c):
    m = next(m for m in FX["models"] if m["name"] == c["model"])
    p = next(p for p in m["points"] if p["name"] == c["point"])
    unf = m["unfolded"]
    table = np.array(p["table"], dtype=np.float64)
    from misti_amd.optimize import class_counts
    f = np.abs(class_counts(table[:1], unf)[0])
    exact = dict(dlog=cx.pad7(cx.arr(c["exact"]["dlog"])), d2log=cx.pad7(cx.arr(c["exact"]["d2log"])),
                 grad=cx.arr(cx.exact_contract(c["exact"]["dlog"], table[0], unf)), hess=cx.arr(cx.exact_contract(c["exact"]["d2log"], table[0], unf)))
    failures = []
    with _engine(m, true_eps=False) as e:
        for sb, sa in zip(c["steps"], p["steps"]):
            assert sb["rel_step"] == sa["rel_step"]
            r = e.curvature([p["x"]], [p["split"]], [0], table, rel_step=sa["rel_step"], abs_step=p["abs_step"])
            asm, asm_status, _ = _through_assemble(e, m, p, sa, table)
            assert r.status[0] == 0 and asm_status == 0 and same_bits(r.h[0], np.array(sa["h"]))
            got = dict(dlog=r.dlog[0], d2log=asm["d2log"], grad=r.grad[0], hess=r.hess[0])
            b = cx.bounds(np.array(sb["oracle_jafs"]), np.array(sa["h"]), unf, table[0])
            o = dict(dlog=cx.pad7(np.array(sb["oracle_err_dlog"])), d2log=cx.pad7(np.array(sb["oracle_err_d2log"])))
            ok = dict(dlog=cx.pad7(np.array(sb["qualifies_dlog"], dtype=float)) > 0, d2log=cx.pad7(np.array(sb["qualifies_d2log"], dtype=float)) > 0)
            K = 7 if unf else 4
            # grad / hess: the oracle's error contracted with the absolute class counts; held where every class of the entry qualifies
            o["grad"], o["hess"] = o["dlog"] @ f, o["d2log"] @ f
            ok["grad"], ok["hess"] = ok["dlog"][..., :K].all(axis=-1), ok["d2log"][..., :K].all(axis=-1)
            line = "curvature_exact correction %-16s rel_step %-6g" % (c["model"], sa["rel_step"])
            for k in ("dlog", "d2log", "grad", "hess"):
                err = np.abs(got[k] - exact[k])
                tol = SELF_FACTOR * o[k] + b[k]
                scale = np.abs(exact[k]).max()
                held = ok[k] & (tol > 0)
                line += " | %s device %.1e oracle %.1e (held %d, skipped %d)" % (k, err.max() / scale, o[k].max() / scale, int(held.sum()),
                                                                                int((tol > 0).sum() - held.sum()))
                if not (np.isfinite(got[k]).all() and (err[held] <= tol[held]).all()):
                    failures.append((sa["rel_step"], k, float((err[held] / tol[held]).max())))
            print(line)
            if sa["rel_step"] == cx.DEFAULT_STEP:
                assert all(ok[k][..., :K].all() if k in ("dlog", "d2log") else ok[k].all() for k in ok), "the fixture promises the default step"
    assert not failures, failures
