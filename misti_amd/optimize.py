"""Batched Nelder-Mead: many independent simplices advanced together, every round of
objective evaluations issued as ONE batch to the likelihood engine.

The reference optimises one model at a time with SciPy's Nelder-Mead
(``MigrationInference.Solve``, ``/root/reference/MigrationInference.py:718-733``:
``method='Nelder-Mead', xatol = fatol = tol, maxiter = 1000``, started from the
``-mi``/``-pu`` initial values; a basin-hopping variant exists but is unreachable from
its CLI).  BASELINE config 3 runs that search from 16 384 random starts.  Each start
here follows exactly SciPy's (non-adaptive) iteration - same initial simplex, same
reflection / expansion / contraction / shrink decisions, same termination test - so a
start's trajectory equals ``scipy.optimize.minimize(..., method='Nelder-Mead')`` on the
same objective; only the evaluation is batched: per iteration at most three engine
calls (reflection points of all live starts; their expansion/contraction points; the
shrunk vertices of those that shrink).
"""
from __future__ import annotations

import numpy as np

RHO, CHI, PSI, SIGMA = 1.0, 2.0, 0.5, 0.5          # scipy/optimize/_optimize.py, adaptive=False
NONZDELT, ZDELT = 0.05, 0.00025


class NMResult:
    __slots__ = ("x", "fun", "nit", "nfev", "converged", "simplex", "fsim")

    def __init__(self, x, fun, nit, nfev, converged, simplex, fsim):
        self.x, self.fun, self.nit, self.nfev, self.converged = x, fun, nit, nfev, converged
        self.simplex, self.fsim = simplex, fsim


def initial_simplex(x0):
    """[S, N] starts -> [S, N+1, N] simplices as SciPy builds them."""
    x0 = np.asarray(x0, dtype=float)
    S, N = x0.shape
    sim = np.repeat(x0[:, None, :], N + 1, axis=1)
    for k in range(N):
        y = x0[:, k]
        sim[:, k + 1, k] = np.where(y != 0, (1 + NONZDELT) * y, ZDELT)
    return sim


def box_clip(x, lo, hi):
    """A point, or an array of points, clipped to the box as SciPy's bounded Nelder-Mead clips every point it evaluates
    (``np.clip(x, lower_bound, upper_bound)``): NaN passes through, an infinite bound never binds, ``lo == hi`` pins the coordinate.
    What ``misti_nm_solve_box`` applies per coordinate on the device (``box_clip`` in ``misti_nm.hip``)."""
    return np.clip(np.asarray(x, dtype=float), np.asarray(lo, dtype=float), np.asarray(hi, dtype=float))


def box_initial_simplex(x0, lo, hi):
    """[S, N] starts (or one ``[N]`` start) -> [S, N+1, N] (``[N+1, N]``) initial simplices as SciPy builds them under
    ``bounds=Bounds(lo, hi)`` (``_minimize_neldermead``, SciPy 1.15.3): the start is clipped, the 5 % / 0.00025 simplex is built from the
    clipped start, a vertex beyond its upper bound is reflected into the interior (``2 * hi - x``), and the simplex is clipped.
    ``lo`` / ``hi``: ``[N]``, or ``[S, N]`` for a box per start.  The rule of ``nm_init_kernel`` under a box."""
    x0 = np.asarray(x0, dtype=float)
    one = x0.ndim == 1
    x0 = np.atleast_2d(x0)
    lo = np.broadcast_to(np.asarray(lo, dtype=float), x0.shape)[:, None, :]
    hi = np.broadcast_to(np.asarray(hi, dtype=float), x0.shape)[:, None, :]
    sim = initial_simplex(np.clip(x0, lo[:, 0], hi[:, 0]))
    with np.errstate(invalid="ignore"):                   # 2 * inf - x where the mask is False anyway
        sim = np.where(sim > hi, 2 * hi - sim, sim)
    sim = np.clip(sim, lo, hi)
    return sim[0] if one else sim


def _sort(sim, fsim):
    order = np.argsort(fsim, axis=1)          # as SciPy: default argsort (insertion sort at these sizes)
    return np.take_along_axis(sim, order[:, :, None], axis=1), np.take_along_axis(fsim, order, axis=1)


def batched_nelder_mead(fun_batch, x0, xatol=1e-4, fatol=1e-4, maxiter=None, maxfun=None):
    """Minimise ``fun`` from every row of ``x0``.

    ``fun_batch(X[M, N]) -> f[M]`` evaluates M points at once (``+inf`` allowed).
    Returns an ``NMResult`` of arrays over the S starts.
    """
    x0 = np.atleast_2d(np.asarray(x0, dtype=float))
    S, N = x0.shape
    if maxiter is None and maxfun is None:              # SciPy's defaults (_minimize_neldermead)
        maxiter = maxfun = N * 200
    elif maxiter is None:
        maxiter = N * 200 if maxfun == np.inf else np.inf
    elif maxfun is None:
        maxfun = N * 200 if maxiter == np.inf else np.inf
    sim = initial_simplex(x0)
    fsim = np.asarray(fun_batch(sim.reshape(S * (N + 1), N)), dtype=float).reshape(S, N + 1)
    nfev = np.full(S, N + 1)
    sim, fsim = _sort(sim, fsim)
    nit = np.ones(S, dtype=int)                 # SciPy starts its iteration counter at 1
    live = np.ones(S, dtype=bool)

    def done_mask():
        dx = np.max(np.abs(sim[:, 1:, :] - sim[:, :1, :]), axis=(1, 2))
        with np.errstate(invalid="ignore"):
            df = np.max(np.abs(fsim[:, :1] - fsim[:, 1:]), axis=1)
        return (dx <= xatol) & (df <= fatol)

    while True:
        live &= ~done_mask()
        live &= (nit < maxiter) & (nfev < maxfun)
        idx = np.where(live)[0]
        if idx.size == 0:
            break
        xbar = sim[idx, :-1, :].sum(axis=1) / N
        worst = sim[idx, -1, :]
        xr = (1 + RHO) * xbar - RHO * worst
        fxr = np.asarray(fun_batch(xr), dtype=float)
        nfev[idx] += 1
        f0, fn1, fn = fsim[idx, 0], fsim[idx, -2], fsim[idx, -1]
        want_e = fxr < f0
        mid = ~want_e & (fxr < fn1)
        want_c = ~want_e & ~mid & (fxr < fn)
        want_cc = ~want_e & ~mid & ~want_c
        # second round: one extra point for everything but the plain reflections
        x2 = np.where(want_e[:, None], (1 + RHO * CHI) * xbar - RHO * CHI * worst,
                      np.where(want_c[:, None], (1 + PSI * RHO) * xbar - PSI * RHO * worst,
                               (1 - PSI) * xbar + PSI * worst))
        need2 = ~mid
        f2 = np.full(idx.size, np.nan)
        if need2.any():
            f2[need2] = np.asarray(fun_batch(x2[need2]), dtype=float)
            nfev[idx[need2]] += 1
        new_x = xr.copy()
        new_f = fxr.copy()
        shrink = np.zeros(idx.size, dtype=bool)
        take_e = want_e & (f2 < fxr)
        new_x[take_e], new_f[take_e] = x2[take_e], f2[take_e]
        ok_c = want_c & (f2 <= fxr)
        new_x[ok_c], new_f[ok_c] = x2[ok_c], f2[ok_c]
        shrink |= want_c & ~ok_c
        ok_cc = want_cc & (f2 < fn)
        new_x[ok_cc], new_f[ok_cc] = x2[ok_cc], f2[ok_cc]
        shrink |= want_cc & ~ok_cc
        keep = ~shrink
        sim[idx[keep], -1, :] = new_x[keep]
        fsim[idx[keep], -1] = new_f[keep]
        if shrink.any():
            si = idx[shrink]
            sim[si, 1:, :] = sim[si, :1, :] + SIGMA * (sim[si, 1:, :] - sim[si, :1, :])
            fs = np.asarray(fun_batch(sim[si, 1:, :].reshape(si.size * N, N)), dtype=float).reshape(si.size, N)
            fsim[si, 1:] = fs
            nfev[si] += N
        s2, f2s = _sort(sim[idx], fsim[idx])
        sim[idx], fsim[idx] = s2, f2s
        nit[idx] += 1
    return NMResult(sim[:, 0, :].copy(), fsim[:, 0].copy(), nit, nfev, done_mask(), sim, fsim)


def solve_batched(engine, split_time, starts, jsfs_row, tol=1e-4, maxiter=1000):
    """``MigrationInference.Solve`` for many starts: maximise the likelihood of one data JSFS
    over the optimised band/pulse parameters from each row of ``starts`` ([S, P]).

    ``engine`` is a ``misti_amd.engine.Engine``; negative parameters give ``-inf`` exactly as
    the reference's guard (MigrationInference.py:569-572).  Returns (params[S, P], llh[S], NMResult).
    """
    starts = np.atleast_2d(np.asarray(starts, dtype=float))
    row = np.asarray(jsfs_row, dtype=float).reshape(1, 8)

    def objective(X):
        res = engine.evaluate(np.full(X.shape[0], float(split_time)), X, row)
        return -res.llk[:, 0]

    r = batched_nelder_mead(objective, starts, xatol=tol, fatol=tol, maxiter=maxiter)
    return r.x, -r.fun, r


def _world(group=None):
    """Ranks of the process group this process belongs to (1 without torch.distributed or before it is initialised)."""
    try:
        import torch.distributed as dist
    except ImportError:
        return 1
    return dist.get_world_size(group) if dist.is_initialized() else 1


def solve_batched_dev(engine, split_time, starts, jsfs_row, tol=1e-4, maxiter=1000, group=None):
    """``solve_batched`` with the simplices resident on the device (``misti_nm_solve``): no host round trip per
    iteration - per iteration three engine batches and four one-thread-per-start kernels on the engine's stream.
    Same decisions as SciPy's Nelder-Mead, hence the same result as ``solve_batched`` / ``MigrationInference.Solve``.
    Inside a process group (one rank per GPU: ``misti_amd.dist.init_from_env``) the starts are dealt to the ranks in contiguous
    blocks, every rank searches its block on its own GPU and one all_gather returns all starts on every rank
    (``dist.search_sharded``) - BASELINE config 3's 16 384 starts are 2 048 per GPU on a node; results are those of one device.
    Returns (params[S, P], llh[S], dict with nit, nfev, status)."""
    if _world(group) > 1:
        from . import dist as mdist
        r = mdist.search_sharded(lambda st: engine.nm_solve(st, split_time, jsfs_row, tol=tol, maxiter=maxiter), starts,
                                 ("x", "llh", "nit", "nfev", "status"), group=group)
        return r["x"], r["llh"], r
    r = engine.nm_solve(starts, split_time, jsfs_row, tol=tol, maxiter=maxiter)
    return r["x"], r["llh"], r


def basinhopping_dev(engine, split_time, starts, jsfs_row, rngs, group=None, **kw):
    """The reference's global search (``MigrationInference.Solve(globalOpt=True)``, ``/root/reference/MigrationInference.py:723-725``)
    from every row of ``starts`` (``Engine.basinhopping``: SciPy's runner step for step); inside a process group the starts - and
    their generators ``rngs`` - are dealt to the ranks in contiguous blocks and gathered once (``dist.search_sharded``).
    Returns dict(x, llh, nfev, failures, accepted)."""
    if _world(group) > 1:
        from . import dist as mdist
        return mdist.search_sharded(lambda st, rngs: engine.basinhopping(st, split_time, jsfs_row, rngs, **kw), starts,
                                    ("x", "llh", "nfev", "failures", "accepted"), group=group, rngs=list(rngs))
    return engine.basinhopping(starts, split_time, jsfs_row, rngs, **kw)


def solve_grouped_dev(engines, split_time, starts, jsfs_row, tol=1e-4, maxiter=1000):
    """``solve_batched_dev`` with the starts dealt out to several engine contexts (one host thread each; ctypes releases the
    GIL for the duration of ``misti_nm_solve``): the three engine batches of an iteration depend on each other, the searches of
    different groups do not, so their batches overlap on the GPU.  A start's trajectory does not depend on which batch its
    points travel in: results equal ``solve_batched_dev`` on one context, bit for bit.
    Returns (params[S, P], llh[S], dict with nit, nfev, status and per-group work counters)."""
    import threading
    starts = np.atleast_2d(np.asarray(starts, dtype=float))
    G = len(engines)
    parts = [np.arange(g, starts.shape[0], G) for g in range(G)]              # interleaved: every group sees the same mix of starts
    res, err = [None] * G, []

    def work(g):
        try:
            res[g] = engines[g].nm_solve(starts[parts[g]], split_time, jsfs_row, tol=tol, maxiter=maxiter)
        except BaseException as e:                                           # surfaces in the caller's thread
            err.append(e)
    threads = [threading.Thread(target=work, args=(g,)) for g in range(G)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if err:
        raise err[0]
    S, P = starts.shape
    out = dict(x=np.empty((S, P)), llh=np.empty(S), nit=np.empty(S, dtype=np.int32), nfev=np.empty(S, dtype=np.int32), status=np.empty(S, dtype=np.int32))
    for g in range(G):
        for k in out:
            out[k][parts[g]] = res[g][k]
    out["iterations_issued"] = max(r["iterations_issued"] for r in res)
    out["slots"] = sum(r["slots"] for r in res)
    out["speculative_iterations"] = max(r["speculative_iterations"] for r in res)
    out["groups"] = G
    return out["x"], out["llh"], out


def bootstrap_split_interval(llk, split_values, level=0.95):
    """Confidence interval of the split time from bootstrap replicates, as in the reference's
    ``test.bs/bs_conf_int.ipynb``: per replicate the arg-max split over the scan, then a
    Student-t interval of those maxima.  ``llk`` is ``[n_split, n_rep]`` (row r = candidate r)."""
    from scipy import stats
    llk = np.asarray(llk, dtype=float)
    best = np.asarray(split_values, dtype=float)[np.argmax(np.where(np.isfinite(llk), llk, -np.inf), axis=0)]
    n = best.size
    mean, sd = best.mean(), best.std(ddof=1) if n > 1 else 0.0
    half = stats.t.ppf(0.5 + level / 2, n - 1) * sd / np.sqrt(n) if n > 1 else 0.0
    return mean, (mean - half, mean + half), best


def _t_interval(b, level):
    from scipy import stats
    m = b.size
    mean, sd = b.mean(), b.std(ddof=1) if m > 1 else 0.0
    half = stats.t.ppf(0.5 + level / 2, m - 1) * sd / np.sqrt(m) if m > 1 else 0.0
    return mean, (mean - half, mean + half), b


def bootstrap_scan_dev(engine, split_values, jsfs_rows, params=None, level=0.95, group=None):
    """A bootstrap scan that keeps the [n_split x n_rep] likelihood table on the device: one
    ``misti_eval_batch_dev`` over the split values x all replicates, then ``misti_argmax_dev`` per
    replicate; only the n_rep winning indices come back.  Returns what ``bootstrap_split_interval``
    returns (mean, interval, per-replicate best split).  Inside a process group the REPLICATES are dealt to the ranks in
    contiguous blocks (BASELINE config 4: 1 000 replicates = 125 per GPU on a node), each rank scans its block on its own GPU and
    one all_gather of the winning indices follows (``dist.bootstrap_sharded``)."""
    rows = np.asarray(jsfs_rows, dtype=float).reshape(-1, 8)
    if _world(group) > 1:
        from . import dist as mdist
        idx = mdist.bootstrap_sharded(lambda a, b: _scan_best(engine, split_values, rows[a:b], params), rows.shape[0], group=group)
    else:
        idx = _scan_best(engine, split_values, rows, params)
    if (idx < 0).any():
        raise ValueError("a replicate has no finite likelihood over the scan")
    return _t_interval(np.asarray(split_values, dtype=float)[idx], level)


def _scan_best(engine, split_values, jsfs_rows, params=None):
    """Per replicate the index of the best split value, reduced on the device (misti_eval_batch_dev + misti_argmax_dev)."""
    import torch
    dev = torch.device("cuda", engine.device)
    split = torch.as_tensor(np.asarray(split_values, dtype=float), device=dev)
    rows = torch.as_tensor(np.asarray(jsfs_rows, dtype=float).reshape(-1, 8), device=dev).contiguous()
    n, R = split.numel(), rows.shape[0]
    par = None
    if engine.n_param:
        par = torch.as_tensor(np.asarray(params, dtype=float).reshape(n, engine.n_param), device=dev).contiguous()
    llk = torch.empty((n, R), dtype=torch.float64, device=dev)
    best = torch.empty(R, dtype=torch.int32, device=dev)
    torch.cuda.current_stream(dev).synchronize()      # the engine's stream is non-blocking: inputs must have landed
    engine.evaluate_dev(n, split.data_ptr(), par.data_ptr() if par is not None else 0, R, rows.data_ptr(), llk.data_ptr())
    engine.argmax_dev(n, R, llk.data_ptr(), best.data_ptr())
    engine.sync()
    return best.cpu().numpy().astype(np.int64)


def best_k_per_replicate(llk, k):
    """The order rule of ``misti_scan_best_dev`` stated on the host, for a table ``llk[n_cand][n_rep]``: per replicate (column) the
    candidates that have a value - ``v > -inf``; NaN never qualifies - ordered by value descending and by candidate index ascending
    on equal values, the first ``k`` of them.  Returns ``(best[n_rep][k]`` int64, ``best_llk[n_rep][k])``; places beyond the last
    candidate with a value hold -1 / -inf.  ``k = 1`` is ``dist.best_per_replicate``."""
    llk = np.asarray(llk, dtype=np.float64)
    llk = llk.reshape(llk.shape[0], -1)
    n, R = llk.shape
    k = int(k)
    with np.errstate(invalid="ignore"):
        has = llk > -np.inf
    key = np.where(has, -llk, np.inf)                       # ascending; a STABLE sort leaves equal values in index order
    order = np.argsort(key, axis=0, kind="stable")[:k]
    best = np.full((R, k), -1, dtype=np.int64)
    best_llk = np.full((R, k), -np.inf)
    m = order.shape[0]
    listed = np.take_along_axis(has, order, axis=0).T       # [R][m]
    best[:, :m] = np.where(listed, order.T, -1)
    best_llk[:, :m] = np.where(listed, np.take_along_axis(llk, order, axis=0).T, -np.inf)
    return best, best_llk


def _per_candidate(a, n, shape):
    """int32 ``[n, *shape]`` from per-candidate values, or from one set that every candidate shares."""
    a = np.asarray(a, dtype=np.int32)
    return np.broadcast_to(a.reshape((-1,) + shape), (n,) + shape).copy()


def scan_best(engine, split, params, jsfs_rows, k=1, band_bounds=None, pulse_times=None):
    """Scan and keep the ``k`` best candidates per replicate WITHOUT the likelihood table: one evaluation without replicates into
    device spectra and statuses (``misti_eval_batch_dev``; with ``pulse_times`` ``misti_eval_batch_pulses_dev``), then
    ``misti_scan_best_dev`` - device memory is ``O(n_cand + n_rep * k)``, and only the lists and the statuses come back.
    ``split`` is ``[n]``, ``params`` ``[n][n_param]``, ``jsfs_rows`` ``[R][8]``, ``band_bounds`` (``[n][n_band][2]``) and
    ``pulse_times`` (``[n][n_pulse]``) per candidate as in ``Engine.evaluate`` (one set is shared by every candidate).
    Returns ``(best[R][k]`` int64, ``best_llk[R][k]``, ``status[n])`` under ``best_k_per_replicate``'s rule."""
    import torch
    dev = torch.device("cuda", engine.device)
    k = int(k)
    split_h = np.asarray(split, dtype=float).reshape(-1)
    n = split_h.size
    rows = torch.as_tensor(np.asarray(jsfs_rows, dtype=float).reshape(-1, 8), device=dev).contiguous()
    R = rows.shape[0]
    d_split = torch.as_tensor(split_h, device=dev)
    par = bb = pt = None
    if engine.n_param:
        par = torch.as_tensor(np.asarray(params, dtype=float).reshape(n, engine.n_param), device=dev).contiguous()
    if band_bounds is not None and engine.n_band:
        bb = torch.as_tensor(_per_candidate(band_bounds, n, (engine.n_band, 2)), device=dev)
    if pulse_times is not None and engine.n_pulse:
        pt = torch.as_tensor(_per_candidate(pulse_times, n, (engine.n_pulse,)), device=dev)
    jafs = torch.empty((n, 7), dtype=torch.float64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    best = torch.empty((R, k), dtype=torch.int32, device=dev)
    best_llk = torch.empty((R, k), dtype=torch.float64, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None else 0
    torch.cuda.current_stream(dev).synchronize()      # the engine's stream is non-blocking: inputs must have landed
    engine.evaluate_dev(n, ptr(d_split), ptr(par), 0, 0, 0, d_jafs=ptr(jafs), d_status=ptr(status), d_bounds=ptr(bb), d_pulse_times=ptr(pt))
    engine.scan_best_dev(n, ptr(jafs), ptr(status), R, ptr(rows), k, ptr(best), ptr(best_llk))
    engine.sync()
    return best.cpu().numpy().astype(np.int64), best_llk.cpu().numpy(), status.cpu().numpy()


def scan_polish(engine, split, params, jsfs_rows, k, band_bounds=None, pulse_times=None, tol=1e-4, maxiter=1000, box=None):
    """Scan, keep the ``k`` best candidates per replicate, polish those: ``scan_best``, then ONE batched search whose starts are the
    listed candidates - row r's j-th place is a start with that candidate's parameters, split, band bounds and pulse times against
    row r (row outermost, place innermost; a -1 place gives no start) - ``misti_search`` with whichever of the arrays are given.
    Per row the best polished search is kept (``_best_start_profile``'s rule: the first maximum, NaN never wins).  Where ``--grid-solve`` searches from every (row, split, start) triple, this searches from ``k`` per row.
    ``box``: ``(lo, hi)``, each ``[n_param]`` - the polish runs inside it (``misti_nm_solve_box``: SciPy's ``bounds=``); the scan is not
    touched.
    Returns dict(best[R][k], best_llk[R][k], scan_status[n] (the scan's), x[R][n_param], split[R], llh[R], nit / nfev / status[R],
    place[R] (which place of the row's list was kept; a row without a start: -1, with x nan, llh -inf, status -1), searches (every
    search: row, place, cand, x, llh, nit, nfev, status), and the search's work counters)."""
    N = engine.n_param
    if N < 1:
        raise ValueError("scan_polish polishes optimised parameters: the model has none (n_param == 0)")
    split = np.asarray(split, dtype=float).reshape(-1)
    n = split.size
    params = np.asarray(params, dtype=float).reshape(n, N)
    rows = np.asarray(jsfs_rows, dtype=float).reshape(-1, 8)
    R = rows.shape[0]
    best, best_llk, scan_status = scan_best(engine, split, params, rows, k, band_bounds, pulse_times)
    r_of, j_of = np.nonzero(best >= 0)                                    # row outermost, place innermost
    cand = best[r_of, j_of]
    bb = _per_candidate(band_bounds, n, (engine.n_band, 2))[cand] if band_bounds is not None and engine.n_band else None
    pt = _per_candidate(pulse_times, n, (engine.n_pulse,))[cand] if pulse_times is not None and engine.n_pulse else None
    if cand.size == 0:
        res = dict(x=np.empty((0, N)), llh=np.empty(0), nit=np.empty(0, dtype=np.int32), nfev=np.empty(0, dtype=np.int32),
                   status=np.empty(0, dtype=np.int32), iterations_issued=0, slots=0, speculative_iterations=0)
    else:
        res = engine.search(params[cand], rows, split_times=split[cand], rows=r_of.astype(np.int32), band_bounds=bb, pulse_times=pt, box=box,
                            xatol=tol, fatol=tol, maxiter=maxiter)
    llh = np.full(best.shape, -np.inf)
    llh[r_of, j_of] = np.where(np.isnan(res["llh"]), -np.inf, res["llh"])
    place = np.where((best >= 0).any(axis=1), np.argmax(llh, axis=1), -1)           # first maximum: the lowest place
    at = np.full(best.shape, -1, dtype=np.int64)
    at[r_of, j_of] = np.arange(cand.size)
    kept = at[np.arange(R), np.maximum(place, 0)]                                    # index of the kept search (-1: none)
    has = kept >= 0
    out = dict(best=best, best_llk=best_llk, scan_status=scan_status, place=place,
               x=np.full((R, N), np.nan), split=np.full(R, np.nan), llh=np.full(R, -np.inf),
               nit=np.zeros(R, dtype=np.int32), nfev=np.zeros(R, dtype=np.int32), status=np.full(R, -1, dtype=np.int32))
    for f in ("x", "llh", "nit", "nfev", "status"):
        out[f][has] = res[f][kept[has]]
    out["split"][has] = split[cand[kept[has]]]
    out["searches"] = dict(row=r_of, place=j_of, cand=cand, **{f: res[f] for f in ("x", "llh", "nit", "nfev", "status")})
    out.update({f: res[f] for f in ("iterations_issued", "slots", "speculative_iterations")})
    return out


def profile_per_group(llk, group, n_group):
    """The rule of ``misti_scan_profile_dev`` stated on the host, for a table ``llk[n_cand][n_rep]`` and one label per candidate:
    candidate ``c`` takes part in group ``group[c]`` only if ``0 <= group[c] < n_group`` (any other label: in no group); per
    replicate and group the largest value ``v > -inf`` among the group's candidates - NaN never qualifies - and the LOWEST candidate
    index that attains it; a group without such a candidate holds -inf / -1.  Returns ``(prof_llk[n_rep][n_group]``,
    ``prof_best[n_rep][n_group]`` int64).  One group is ``best_k_per_replicate(llk, 1)``."""
    llk = np.asarray(llk, dtype=np.float64)
    llk = llk.reshape(llk.shape[0], -1)
    n, R = llk.shape
    group = np.asarray(group, dtype=np.int64).reshape(-1)
    G = int(n_group)
    if group.size != n:
        raise ValueError("one label per candidate: %d labels for %d candidates" % (group.size, n))
    if G < 1:
        raise ValueError("n_group must be at least 1")
    prof_llk = np.full((R, G), -np.inf)
    prof_best = np.full((R, G), -1, dtype=np.int64)
    for c in range(n):                                       # ascending index and a strict comparison: the lowest index keeps a tie
        g = group[c]
        if not 0 <= g < G:
            continue
        with np.errstate(invalid="ignore"):
            wins = llk[c] > prof_llk[:, g]                   # false for NaN and for -inf
        prof_llk[wins, g] = llk[c, wins]
        prof_best[wins, g] = c
    return prof_llk, prof_best


def axis_groups(shape, axes):
    """Group labels for the candidates of a C-ordered product grid of ``shape`` (what ``numpy.meshgrid(..., indexing="ij")`` and a
    ``ravel`` make): ``axes`` is one axis, or a tuple of two or more, and a candidate's label is its index along that axis - for
    several axes the row-major index over them in the order given, so a two-dimensional profile SURFACE is the same call with
    ``n_group = shape[i] * shape[j]``.  Returns ``(group[prod(shape)]`` int32, ``n_group)``."""
    shape = tuple(int(s) for s in shape)
    axes = (int(axes),) if np.isscalar(axes) else tuple(int(a) for a in axes)
    if not axes or len(set(axes)) != len(axes) or any(not 0 <= a < len(shape) for a in axes):
        raise ValueError("axes must be distinct axes of a %d-axis grid (got %r)" % (len(shape), axes))
    index = np.indices(shape)
    label = np.zeros(shape, dtype=np.int64)
    n_group = 1
    for a in axes:
        label = label * shape[a] + index[a]
        n_group *= shape[a]
    return label.ravel().astype(np.int32), n_group


def scan_profile(engine, split, params, jsfs_rows, group, n_group, band_bounds=None, pulse_times=None):
    """Scan and keep, per replicate and GROUP of candidates, the group's best candidate WITHOUT the likelihood table: one evaluation
    without replicates into device spectra and statuses, exactly as ``scan_best`` does it, then ``misti_scan_profile_dev`` - device
    memory is ``O(n_cand + n_rep * n_group)``, and only the profile and the statuses come back.  ``group`` is one int label per
    candidate (``axis_groups`` makes them for a product grid; a label outside ``0 ... n_group - 1`` is in no group); the other
    arguments as for ``scan_best``.  Returns ``(prof_llk[R][n_group]``, ``prof_best[R][n_group]`` int64, ``status[n])`` under
    ``profile_per_group``'s rule."""
    import torch
    dev = torch.device("cuda", engine.device)
    split_h = np.asarray(split, dtype=float).reshape(-1)
    n = split_h.size
    G = int(n_group)
    label = np.ascontiguousarray(np.asarray(group).reshape(-1), dtype=np.int32)
    if label.size != n:
        raise ValueError("one label per candidate: %d labels for %d candidates" % (label.size, n))
    rows = torch.as_tensor(np.asarray(jsfs_rows, dtype=float).reshape(-1, 8), device=dev).contiguous()
    R = rows.shape[0]
    d_split = torch.as_tensor(split_h, device=dev)
    d_group = torch.as_tensor(label, device=dev)
    par = bb = pt = None
    if engine.n_param:
        par = torch.as_tensor(np.asarray(params, dtype=float).reshape(n, engine.n_param), device=dev).contiguous()
    if band_bounds is not None and engine.n_band:
        bb = torch.as_tensor(_per_candidate(band_bounds, n, (engine.n_band, 2)), device=dev)
    if pulse_times is not None and engine.n_pulse:
        pt = torch.as_tensor(_per_candidate(pulse_times, n, (engine.n_pulse,)), device=dev)
    jafs = torch.empty((n, 7), dtype=torch.float64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    prof_llk = torch.empty((R, G), dtype=torch.float64, device=dev)
    prof_best = torch.empty((R, G), dtype=torch.int32, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None else 0
    torch.cuda.current_stream(dev).synchronize()      # the engine's stream is non-blocking: inputs must have landed
    engine.evaluate_dev(n, ptr(d_split), ptr(par), 0, 0, 0, d_jafs=ptr(jafs), d_status=ptr(status), d_bounds=ptr(bb), d_pulse_times=ptr(pt))
    engine.scan_profile_dev(n, ptr(jafs), ptr(status), ptr(d_group), G, R, ptr(rows), ptr(prof_llk), ptr(prof_best))
    engine.sync()
    return prof_llk.cpu().numpy(), prof_best.cpu().numpy().astype(np.int64), status.cpu().numpy()


def profile_interval(prof_llk, values, drop):
    """Per row of a one-axis profile ``prof_llk[R][G]`` (group ``g`` stands for ``values[g]``): the value of the first maximal group
    and that maximum, and the smallest and the largest ``values[g]`` among the groups with ``prof_llk[r][g] >= max - drop``.  A row
    without any value (nothing above -inf; NaN never counts) gives NaN in all four.
    What this is: a likelihood-ratio SUPPORT interval - the values whose profile log-likelihood lies within ``drop`` of the best one.
    The likelihood here is a composite one (sites are treated as independent), so ``drop = chi2.ppf(0.95, 1) / 2`` does NOT make it a
    calibrated 95 % confidence interval; the bootstrap t-interval (``bootstrap_split_interval``) remains the confidence statement.
    The interval is the hull of the supported values: a profile with two separated supported stretches is covered by one interval.
    Returns dict(best[R], llh[R], lo[R], hi[R])."""
    p = np.asarray(prof_llk, dtype=np.float64)
    p = p.reshape(-1, p.shape[-1])
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    if values.size != p.shape[1]:
        raise ValueError("one value per group: %d values for %d groups" % (values.size, p.shape[1]))
    if not drop >= 0:
        raise ValueError("drop must be >= 0")
    with np.errstate(invalid="ignore"):
        p = np.where(p > -np.inf, p, -np.inf)                # NaN never counts
    R = p.shape[0]
    top = p.max(axis=1) if p.shape[1] else np.full(R, -np.inf)
    has = top > -np.inf
    first = np.argmax(p, axis=1) if p.shape[1] else np.zeros(R, dtype=np.int64)      # the first maximum
    out = dict(best=np.full(R, np.nan), llh=np.full(R, np.nan), lo=np.full(R, np.nan), hi=np.full(R, np.nan))
    for r in np.where(has)[0]:
        inside = values[p[r] >= top[r] - drop]
        out["best"][r], out["llh"][r], out["lo"][r], out["hi"][r] = values[first[r]], top[r], inside.min(), inside.max()
    return out


def bootstrap_profile(engine, split_values, jsfs_rows, starts, tol=1e-4, maxiter=1000, box=None):
    """The bootstrap profiles of the reference's ``test.bs`` scripts (``for bs in 0..B; for st in A..Z: MiSTI.py ... ${st} -bs ${bs}
    -mi ...``: one ``MigrationInference.Solve`` per (replicate, split) pair, MigrationInference.py:718-733 of the reference) in ONE
    ``misti_nm_solve_rows`` call: every (row, split, start) triple is a start of the batched search.  ``jsfs_rows`` is ``[R][8]``,
    ``split_values`` ``[P]``, ``starts`` ``[Q][N]``.  Per (row, split) the best start is kept (ties: the lowest start index).
    ``box``: ``(lo, hi)``, each ``[N]`` - every search runs inside it (``misti_nm_solve_box``: SciPy's ``bounds=``).
    Returns dict(x[R][P][N], llh[R][P], nit / nfev / status / start[R][P], and the search's work counters)."""
    rows = np.asarray(jsfs_rows, dtype=float).reshape(-1, 8)
    splits = np.asarray(split_values, dtype=float).reshape(-1)
    if box is not None:
        return _best_start_profile(lambda r_of, p_of, st: engine.nm_solve_box(st, r_of, rows, box, split_times=splits[p_of], tol=tol, maxiter=maxiter),
                                   rows.shape[0], splits.size, starts)
    return _best_start_profile(lambda r_of, p_of, st: engine.nm_solve_rows(st, splits[p_of], r_of, rows, tol=tol, maxiter=maxiter),
                               rows.shape[0], splits.size, starts)


def _best_start_profile(search, R, P, starts, per_start=("nit", "nfev", "status")):
    """What bootstrap_profile and sweep_profile share: ``search(r_of, p_of, starts)`` runs ONE batched search over every
    (row, point, start) triple (row outermost, start innermost; ``r_of`` int32), then per (row, point) the best start is kept - the
    first maximum, i.e. the lowest start index on ties; NaN never wins.  ``per_start``: the search's per-start results kept beside
    ``x`` and ``llh``."""
    starts = np.atleast_2d(np.asarray(starts, dtype=float))
    Q = starts.shape[0]
    r_of, p_of, q_of = (a.ravel() for a in np.meshgrid(np.arange(R), np.arange(P), np.arange(Q), indexing="ij"))
    res = search(r_of.astype(np.int32), p_of, starts[q_of])
    llh = res["llh"].reshape(R, P, Q)
    best = np.argmax(np.where(np.isnan(llh), -np.inf, llh), axis=2)              # first maximum: the lowest start index
    pick = lambda a: np.take_along_axis(a.reshape(R, P, Q, *a.shape[1:]), best.reshape(R, P, 1, *([1] * (a.ndim - 1))), axis=2)[:, :, 0]
    out = dict(x=pick(res["x"]), llh=pick(res["llh"]), **{k: pick(res[k]) for k in per_start}, start=best)
    out.update({k: res[k] for k in ("iterations_issued", "slots", "speculative_iterations")})
    return out


_HOP_RESULTS = ("nfev", "failures", "accepted")


def _hop_generators(seed, R, n):
    """The generators of a ``*_global`` call of R rows x n searches per row, in the flattened (row, point, start) order: search j of
    every row (point outermost, start innermost) draws from a fresh ``numpy.random.default_rng([seed, j])``.  j does not count the
    rows: what a row's searches draw does not depend on how many rows the call holds, or on which (the rows of a bootstrap share
    their random numbers - only the data differ between them)."""
    return [np.random.default_rng([int(seed), j]) for _ in range(R) for j in range(n)]


def bootstrap_profile_global(engine, split_values, jsfs_rows, starts, seed=0, niter=100, T=0.5, stepsize=0.5, box=None, **hop_options):
    """``bootstrap_profile`` with hops: per (row, split, start) triple the reference's global search - ``Solve(globalOpt=True)``,
    ``scipy.optimize.basinhopping(T=0.5, Nelder-Mead)``, MigrationInference.py:723-725 of the reference - instead of its local one, all
    triples in ONE ``misti_basinhopping_rows`` call.  Same triple layout (row outermost, start innermost) and the same best-start rule.
    The generator of search j is ``numpy.random.default_rng([seed, j])``, j = the search's index in the flattened (row, point, start)
    order taken WITHIN its row (``_hop_generators``), so a row's result does not depend on which other rows are in the call.
    ``hop_options``: ``interval``, ``target_accept_rate``, ``stepwise_factor``, ``xatol``, ``fatol``, ``nm_maxiter``, ``nm_maxfev`` of
    ``Engine.basinhopping_rows`` (SciPy's defaults).  ``box`` as in ``bootstrap_profile`` (``misti_basinhopping_box``).
    Returns dict(x[R][P][N], llh[R][P], nfev / failures / accepted / start[R][P], and the search's work counters)."""
    rows = np.asarray(jsfs_rows, dtype=float).reshape(-1, 8)
    splits = np.asarray(split_values, dtype=float).reshape(-1)
    R = rows.shape[0]

    def search(r_of, p_of, st):
        gens = _hop_generators(seed, R, r_of.size // R)
        if box is not None:
            return engine.basinhopping_box(st, r_of, rows, gens, box, split_times=splits[p_of], niter=niter, T=T, stepsize=stepsize, **hop_options)
        return engine.basinhopping_rows(st, splits[p_of], r_of, rows, gens, niter=niter, T=T, stepsize=stepsize, **hop_options)
    return _best_start_profile(search, R, splits.size, starts, _HOP_RESULTS)


def bootstrap_profile_interval(llh, split_values, x=None):
    """The reduction of the reference's ``test.bs/bs_conf_int.ipynb`` (``conf_int_bs``) over a profile table ``llh[R][P]`` (row 0 the
    data, rows 1.. the bootstrap replicates; split p = ``split_values[p]``): per row the split of its largest llh (the first on ties,
    np.argmax), row 0 reported on its own - its split, llh and, given ``x[R][P][N]``, rates - and over rows 1..R-1
    ``scipy.stats.t.interval(0.975, B - 1, loc=mean, scale=sem)`` of their best splits.  A row without a finite llh has no best
    split: it is left out (and counted).  Fewer than two bootstrap rows with a best split: no interval.
    Returns dict(best_split[R] (nan: none), data_split / data_llh / data_x (None: none), mean, interval ((lo, hi) or None),
    n_boot, n_excluded)."""
    from scipy import stats
    llh = np.atleast_2d(np.asarray(llh, dtype=float))
    splits = np.asarray(split_values, dtype=float).reshape(-1)
    finite = np.isfinite(llh)
    has = finite.any(axis=1)
    idx = np.argmax(np.where(finite, llh, -np.inf), axis=1)
    best = np.where(has, splits[idx], np.nan)
    out = dict(best_split=best, data_split=None, data_llh=None, data_x=None, mean=None, interval=None)
    if has[0]:
        out["data_split"] = float(splits[idx[0]])
        out["data_llh"] = float(llh[0, idx[0]])
        if x is not None:
            out["data_x"] = np.asarray(x)[0, idx[0]]
    a = best[1:][has[1:]]
    out["n_boot"], out["n_excluded"] = int(a.size), int((~has[1:]).sum())
    if a.size >= 1:
        out["mean"] = float(np.mean(a))
    if a.size >= 2:
        with np.errstate(invalid="ignore"):               # every replicate on one split: sem = 0, the interval is (nan, nan) as there
            out["interval"] = tuple(float(v) for v in stats.t.interval(0.975, len(a) - 1, loc=np.mean(a), scale=stats.sem(a)))
    return out


def _split_pairs(engine, starts, splits, band_bounds, pulse_times):
    """What split_fit and split_fit_global share: the (start, initial split) pairs ``[Q x P][n_param + 1]`` (start outermost, initial
    split innermost; a model without an optimised parameter has the splits alone), and ``per_search(S)``: the one set of band bounds
    and pulse times repeated for S searches (``None`` stays ``None``)."""
    st = np.asarray(starts, dtype=float).reshape(-1, engine.n_param) if engine.n_param else np.empty((1, 0))
    pairs = np.hstack([np.repeat(st, splits.size, axis=0), np.tile(splits, st.shape[0])[:, None]])
    tile = lambda a, shape, S: None if a is None else np.repeat(np.asarray(a, dtype=np.int32).reshape(shape), S, axis=0)
    return pairs, lambda S: dict(band_bounds=tile(band_bounds, (1, -1, 2), S), pulse_times=tile(pulse_times, (1, -1), S))


def split_fit(engine, jsfs_rows, starts, split_starts, band_bounds=None, pulse_times=None, tol=1e-4, maxiter=1000, box=None):
    """The split time FITTED per row instead of scanned (the ``for st in A..Z`` loops of the reference's ``test.bs`` scripts and the
    arg-max over them): for every row of ``jsfs_rows`` (``[R][8]``) one search from every (start, initial split) pair - ``starts``
    ``[Q][n_param]`` (ignored for a model without an optimised parameter), ``split_starts`` ``[P]`` - with the split as the last
    coordinate of the simplex, all R x Q x P searches in ONE ``misti_nm_solve_split`` call (row outermost, initial split innermost).
    Per row the best search is kept (``_best_start_profile``'s rule: the first maximum, NaN never wins).  ``band_bounds``
    (``[n_band][2]``, end -1: the point's own split index) and ``pulse_times`` (``[n_pulse]``) apply to every search.
    ``box``: ``(lo, hi)``, each ``[n_param + 1]``, the split last - every search runs inside it (``misti_nm_solve_box``).
    Returns dict(x[R][n_param + 1], split[R], llh[R], nit / nfev / status / start[R] (index into the (start, split) pairs), and the
    search's work counters)."""
    rows = np.asarray(jsfs_rows, dtype=float).reshape(-1, 8)
    splits = np.asarray(split_starts, dtype=float).reshape(-1)
    pairs, per_search = _split_pairs(engine, starts, splits, band_bounds, pulse_times)

    def search(r_of, p_of, x0):
        per = dict(per_search(r_of.size), tol=tol, maxiter=maxiter)
        return engine.nm_solve_split(x0, r_of, rows, **per) if box is None else engine.nm_solve_box(x0, r_of, rows, box, **per)
    out = _best_start_profile(search, rows.shape[0], 1, pairs)
    out = {k: (v[:, 0] if isinstance(v, np.ndarray) else v) for k, v in out.items()}
    out["split"] = out["x"][:, -1].copy()
    return out


def split_fit_global(engine, jsfs_rows, starts, split_starts, band_bounds=None, pulse_times=None, seed=0, niter=100, T=0.5, stepsize=0.5,
                     box=None, **hop_options):
    """``split_fit`` with hops: per row one basin-hopping search over (optimised parameters, split) from every (start, initial split)
    pair - the answer to an objective that is piecewise in the split, where a local simplex search stops at the first kink it meets -
    all R x Q x P searches in ONE ``misti_basinhopping_split`` call.  Same layout of the triples (row outermost, initial split
    innermost), same best-search rule (``_best_start_profile``).  The generator of search j is
    ``numpy.random.default_rng([seed, j])``, j = the search's index in the flattened (row, point, start) order taken WITHIN its row
    (``_hop_generators``), so a row's result does not depend on which other rows are in the call.  ``hop_options`` as
    ``bootstrap_profile_global`` (``nm_maxiter`` / ``nm_maxfev`` default to ``200 x (n_param + 1)``).  ``box`` as in ``split_fit``
    (``misti_basinhopping_box``): a hop may leave the box, the minimisation from it is clipped back.
    Returns dict(x[R][n_param + 1], split[R], llh[R], nfev / failures / accepted / start[R], and the search's work counters);
    ``split_fit_interval`` takes ``split`` and ``llh`` unchanged."""
    rows = np.asarray(jsfs_rows, dtype=float).reshape(-1, 8)
    splits = np.asarray(split_starts, dtype=float).reshape(-1)
    pairs, per_search = _split_pairs(engine, starts, splits, band_bounds, pulse_times)
    R = rows.shape[0]

    def search(r_of, p_of, x0):
        gens = _hop_generators(seed, R, r_of.size // R)
        per = dict(per_search(r_of.size), niter=niter, T=T, stepsize=stepsize, **hop_options)
        return engine.basinhopping_split(x0, r_of, rows, gens, **per) if box is None else engine.basinhopping_box(x0, r_of, rows, gens, box, **per)
    out = _best_start_profile(search, R, 1, pairs, _HOP_RESULTS)
    out = {k: (v[:, 0] if isinstance(v, np.ndarray) else v) for k, v in out.items()}
    out["split"] = out["x"][:, -1].copy()
    return out


def split_fit_interval(split, llh, level=0.95):
    """The ``test.bs/bs_conf_int.ipynb`` reduction over FITTED splits: ``split[R]`` and ``llh[R]`` per row (row 0 the data, rows 1..
    the bootstrap replicates, as ``split_fit`` returns them); row 0 is reported on its own, and over rows 1..R-1 the Student-t
    interval (``_t_interval``) of their fitted, fractional splits.  A row without a finite llh (or split) has no fitted split: it is
    left out and counted, as in ``bootstrap_profile_interval``.  Fewer than two bootstrap rows with a value: no interval.
    Returns dict(best_split[R] (nan: none), data_split / data_llh (None: none), mean, interval ((lo, hi) or None), n_boot, n_excluded)."""
    split = np.asarray(split, dtype=float).reshape(-1)
    llh = np.asarray(llh, dtype=float).reshape(-1)
    has = np.isfinite(llh) & np.isfinite(split)
    out = dict(best_split=np.where(has, split, np.nan), data_split=None, data_llh=None, mean=None, interval=None)
    if has[0]:
        out["data_split"], out["data_llh"] = float(split[0]), float(llh[0])
    b = split[1:][has[1:]]
    out["n_boot"], out["n_excluded"] = int(b.size), int((~has[1:]).sum())
    if b.size >= 1:
        out["mean"] = float(b.mean())
    if b.size >= 2:
        mean, (lo, hi), _ = _t_interval(b, level)
        out["interval"] = (float(lo), float(hi))
    return out


def sweep_profile(engine, models, jsfs_rows, starts, tol=1e-4, maxiter=1000):
    """``bootstrap_profile`` with a MODEL axis instead of a split axis: ``models`` is a list of ``(split, band_bounds[n_band][2])``
    (end -1: the model's split index) - the boundary profiles "when did migration start or stop" (the test.bs scripts' Solve per
    (replicate, split) pair with a loop over a band boundary added, one Engine per boundary there) in ONE ``misti_search``
    call: every (row, model, start) triple is a start of the batched search.  ``jsfs_rows`` is ``[R][8]``, ``starts`` ``[Q][N]``.
    Per (row, model) the best start is kept (ties: the lowest start index).  A model may carry its own pulse times as a third
    element, ``(split, band_bounds, pulse_times[n_pulse])`` - the pulse-date profile "when did the pulse happen".
    Returns dict(x[R][M][N], llh[R][M], nit / nfev / status / start[R][M], and the search's work counters)."""
    rows = np.asarray(jsfs_rows, dtype=float).reshape(-1, 8)
    splits = np.array([float(m[0]) for m in models], dtype=float)
    bounds = np.array([np.asarray(m[1], dtype=np.int32).reshape(-1, 2) for m in models], dtype=np.int32).reshape(len(models), -1, 2)
    times = None
    if any(len(m) > 2 for m in models):
        if not all(len(m) > 2 for m in models):
            raise ValueError("sweep_profile: either every model carries pulse times or none does")
        times = np.array([np.asarray(m[2], dtype=np.int32).reshape(-1) for m in models], dtype=np.int32).reshape(len(models), -1)
    search = lambda r_of, m_of, st: engine.search(st, rows, split_times=splits[m_of], rows=r_of, band_bounds=bounds[m_of],
                                                  pulse_times=None if times is None else times[m_of], xatol=tol, fatol=tol, maxiter=maxiter)
    return _best_start_profile(search, rows.shape[0], splits.size, starts)


def sweep_interval(llh, values, x=None):
    """The ``test.bs/bs_conf_int.ipynb`` reduction of a sweep table ``llh[R][M]`` (row 0 the data, rows 1.. the bootstrap replicates;
    model m has the value ``values[m][v]`` of swept variable v) for every swept variable: per row the FIRST model with the largest
    llh, row 0 reported on its own, and over rows 1..R-1 the mean and the 97.5 % t-interval of that model's value of each variable.
    Per variable exactly ``bootstrap_profile_interval`` with the variable's values as the split axis (same helper, same exclusions:
    a row without a finite llh is left out and counted) - so with only the split swept it IS ``bootstrap_profile_interval``.
    Returns dict(best_model[R] (-1: none), data_model / data_llh / data_x (None: none), variables: one
    ``bootstrap_profile_interval`` dict per variable (its ``best_split`` / ``data_split`` are that variable's values), n_boot, n_excluded)."""
    llh = np.atleast_2d(np.asarray(llh, dtype=float))
    values = np.asarray(values, dtype=float).reshape(llh.shape[1], -1)
    finite = np.isfinite(llh)
    has = finite.any(axis=1)
    idx = np.argmax(np.where(finite, llh, -np.inf), axis=1)
    out = dict(best_model=np.where(has, idx, -1), data_model=None, data_llh=None, data_x=None,
               variables=[bootstrap_profile_interval(llh, values[:, v], x) for v in range(values.shape[1])],
               n_boot=int(has[1:].sum()), n_excluded=int((~has[1:]).sum()))
    if has[0]:
        out["data_model"], out["data_llh"] = int(idx[0]), float(llh[0, idx[0]])
        if x is not None:
            out["data_x"] = np.asarray(x)[0, idx[0]]
    return out


# ---- curvature at a fitted point: Hessians, observed information, the sandwich covariance ---------------------------------------------
# For a fixed candidate the log-likelihood of row r is llh_const_r + sum_k d_{r,k} log S_k(theta) (MigrationInference.py:600-609 of the
# reference; S the class spectrum).  Gradient and Hessian of EVERY row are therefore contractions of the row's class counts with the
# first and second derivatives of L_k = log S_k, which do not depend on the data; the derivatives of log S are what is differenced,
# not the llk values themselves: those are ~1e6 x log S (the counts), and their differences would carry the counts' rounding.
# The two functions below ARE the rule of misti_curvature / misti_curvature_assemble_dev (include/misti_hip.h): the kernels perform
# the same floating-point operations in the same order.
CURV_BOUNDARY = 7         # MISTI_CURV_BOUNDARY
CURV_NUMERIC = 5          # MISTI_NUMERIC
CURV_REL_STEP = 1e-2      # default relative step: its truncation is measured in DESIGN.md section 4 ("Measured"; tests/test_curvature_exact_cpu.py)


def curvature_size(D):
    """Stencil candidates of a point of D parameters: the centre, 2 D single steps, 4 per pair."""
    return 1 + 2 * int(D) * int(D)


def curvature_stencil(x, rel_step=CURV_REL_STEP, abs_step=0.0):
    """The stencil of ``misti_curvature``.  ``x`` is ``[P][D]`` (or ``[D]``: one point).  Steps ``h_i = (x_i + max(rel_step |x_i|,
    abs_step)) - x_i`` in float64 - the nominal step moved by at most half an ulp of ``x_i`` to the one for which ``x_i + h_i`` and
    ``x_i - h_i`` are both exact (for ``h_i <= x_i``; a larger step makes a boundary point anyway), so that the quotients divide by the step the candidates really take (a rounded abscissa costs a second
    difference ``ulp(x) |dL| / h^2``, which does not fall with ``h``; a nominal step below half an ulp of ``x_i`` gives ``h_i == 0``);
    ``M = 1 + 2 D^2`` points per stencil: 0 the centre; ``1 + 2i`` is ``+h_i``, ``2 + 2i`` is ``-h_i``; for the pairs ``i < j`` in
    lexicographic order, of rank q, ``1 + 2D + 4q + (0, 1, 2, 3)`` are ``(+h_i, +h_j)``, ``(+h_i, -h_j)``, ``(-h_i, +h_j)``,
    ``(-h_i, -h_j)``.  A point with some ``x_i - h_i < 0`` (or ``h_i == 0``: a rate of 0 under a purely relative step) is a BOUNDARY
    point: it has no two-sided stencil, and the engine evaluates none of its stencil points (they are laid out here all the same).
    Returns ``(points[P][M][D], h[P][D], boundary[P] bool)``."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    rel_step, abs_step = float(rel_step), float(abs_step)
    if not (np.isfinite(rel_step) and np.isfinite(abs_step) and rel_step >= 0 and abs_step >= 0 and (rel_step > 0 or abs_step > 0)):
        raise ValueError("rel_step and abs_step must be finite and not negative, and one of them positive")
    if not np.isfinite(x).all():
        raise ValueError("x must be finite")
    P, D = x.shape
    if D < 1:
        raise ValueError("a point needs at least one parameter")
    h = (x + np.maximum(rel_step * np.abs(x), abs_step)) - x          # the step the doubles realise: x + h and x - h are exact
    boundary = ((x - h < 0) | (h == 0)).any(axis=1)
    pts = np.repeat(x[:, None, :], curvature_size(D), axis=1)
    up, down = x + h, x - h
    for i in range(D):
        pts[:, 1 + 2 * i, i] = up[:, i]
        pts[:, 2 + 2 * i, i] = down[:, i]
    q = 0
    for i in range(D):
        for j in range(i + 1, D):
            c = 1 + 2 * D + 4 * q
            for w, (si, sj) in enumerate(((up, up), (up, down), (down, up), (down, down))):
                pts[:, c + w, i] = si[:, i]
                pts[:, c + w, j] = sj[:, j]
            q += 1
    return pts, h, boundary


def fold_classes(v, unfolded, pad=False):
    """The classes the likelihood distinguishes, as a list: all 7 of ``v``, or folded the sums 0+6, 1+5, 2+4 and 3 (``pad``: then three
    zeros).  ``v`` is a sequence of seven values, or an array with the seven along its last axis - the one fold of the Python side, as
    ``row_counts`` / ``class_value`` (misti_score.h) are of the device's."""
    at = (lambda i: v[..., i]) if isinstance(v, np.ndarray) and v.ndim > 1 else (lambda i: v[i])
    if unfolded:
        return [at(i) for i in range(7)]
    return [at(0) + at(6), at(1) + at(5), at(2) + at(4), at(3)] + ([np.zeros_like(at(3))] * 3 if pad else [])


def _class_values(jafs, unfolded):
    """The class values the likelihood takes the logs of: all 7, or folded 0+6, 1+5, 2+4 and 3."""
    return np.stack(fold_classes(np.asarray(jafs, dtype=np.float64), unfolded), axis=-1)


def curvature_from_spectra(jafs, status, h, unfolded):
    """Derivatives of ``L_k = log S_k`` from the spectra of a stencil: ``jafs[P][M][7]``, ``status[P][M]`` (None: all 0), ``h[P][D]``.

        dL_k/dx_i        = (L_k(+i) - L_k(-i)) / (2 h_i)
        d2L_k/dx_i^2     = ((L_k(+i) - 2 L_k(0)) + L_k(-i)) / (h_i h_i)
        d2L_k/dx_i dx_j  = (((L_k(++) - L_k(+-)) - L_k(-+)) + L_k(--)) / ((4 h_i) h_j)     one value for both triangles

    (the brackets are the order of the floating-point operations).  Folded models use classes 0..3 and leave entries 4..6 at 0.  A
    stencil candidate has no value if its status is not 0 or one of its class values is not positive and finite; the point's status
    is then that of the FIRST such candidate in stencil order (5, MISTI_NUMERIC, where that candidate's status was 0) and all its
    derivatives are NaN.  Returns ``(dlog[P][D][7], d2log[P][D][D][7], point_status[P] int32)``."""
    jafs = np.asarray(jafs, dtype=np.float64)
    h = np.atleast_2d(np.asarray(h, dtype=np.float64))
    P, D = h.shape
    M = curvature_size(D)
    jafs = jafs.reshape(P, M, 7)
    st = np.zeros((P, M), dtype=np.int32) if status is None else np.asarray(status, dtype=np.int32).reshape(P, M)
    S = _class_values(jafs, unfolded)
    K = S.shape[-1]
    with np.errstate(invalid="ignore", divide="ignore"):
        bad = (st != 0) | ~((S > 0) & np.isfinite(S)).all(axis=2)
        L = np.log(S)
    point_status = np.zeros(P, dtype=np.int32)
    for p in np.where(bad.any(axis=1))[0]:
        m = int(np.argmax(bad[p]))
        point_status[p] = st[p, m] if st[p, m] != 0 else CURV_NUMERIC
    dlog = np.zeros((P, D, 7))
    d2log = np.zeros((P, D, D, 7))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = 0
        for i in range(D):
            hi = h[:, i, None]
            lp, lm = L[:, 1 + 2 * i], L[:, 2 + 2 * i]
            dlog[:, i, :K] = (lp - lm) / (2.0 * hi)
            d2log[:, i, i, :K] = ((lp - 2.0 * L[:, 0]) + lm) / (hi * hi)
            for j in range(i + 1, D):
                c = 1 + 2 * D + 4 * q
                v = (((L[:, c] - L[:, c + 1]) - L[:, c + 2]) + L[:, c + 3]) / ((4.0 * hi) * h[:, j, None])
                d2log[:, i, j, :K] = v
                d2log[:, j, i, :K] = v
                q += 1
    dlog[point_status != 0] = np.nan
    d2log[point_status != 0] = np.nan
    return dlog, d2log, point_status


def class_counts(table, unfolded):
    """``[R][7]`` class counts of the rows of a replicate table ``[R][8]`` as the replicate epilogue forms them (folded: d0+d6,
    d1+d5, d2+d4, d3, then zeros)."""
    d = np.asarray(table, dtype=np.float64).reshape(-1, 8)[:, 1:]
    return np.stack(fold_classes(d, unfolded, pad=True), axis=-1)


def curvature_contract(dlog, d2log, table, rows, unfolded):
    """``grad[P][D] = sum_k d_k dlog[.][k]`` and ``hess[P][D][D] = sum_k d_k d2log[.][k]`` for row ``rows[p]`` of ``table[R][8]``: the sum
    over the classes in ascending order from 0.0, every product and every sum rounded on its own (what ``curv_contract_kernel`` does)."""
    dlog, d2log = np.asarray(dlog, dtype=np.float64), np.asarray(d2log, dtype=np.float64)
    f = class_counts(table, unfolded)[np.asarray(rows, dtype=np.int64).reshape(-1)]
    grad = np.zeros(dlog.shape[:2])
    hess = np.zeros(d2log.shape[:3])
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(7 if unfolded else 4):
            grad = grad + f[:, k, None] * dlog[:, :, k]
            hess = hess + f[:, k, None, None] * d2log[:, :, :, k]
    return grad, hess


def observed_covariance(hess):
    """Inverse of the observed information, ``inv(-H)``, per point of ``hess[P][D][D]`` (or one ``[D][D]``).  Where ``-H`` is not
    positive definite (an eigenvalue that is not positive, or not finite) the point sits on a saddle, a boundary or a flat
    direction - the "runaway" rates of DESIGN.md section 2 - and has no such covariance: NaN, and the point is flagged.  For a
    COMPOSITE likelihood this is not the covariance of the estimate (``sandwich_covariance`` is); it is its curvature.
    Returns dict(cov[P][D][D], ok[P] bool, cond[P]: largest / smallest eigenvalue of -H (inf or NaN where not positive definite),
    eigenvalues[P][D] of -H ascending)."""
    H = np.asarray(hess, dtype=np.float64)
    H = H.reshape((-1,) + H.shape[-2:])
    P, D = H.shape[0], H.shape[1]
    cov = np.full((P, D, D), np.nan)
    ok = np.zeros(P, dtype=bool)
    cond = np.full(P, np.nan)
    eig = np.full((P, D), np.nan)
    for p in range(P):
        if not np.isfinite(H[p]).all():
            continue
        info = -0.5 * (H[p] + H[p].T)
        w = np.linalg.eigvalsh(info)
        eig[p] = w
        if w[0] > 0:
            ok[p] = True
            cond[p] = w[-1] / w[0]
            cov[p] = np.linalg.inv(info)
        else:
            cond[p] = np.inf
    return dict(cov=cov, ok=ok, cond=cond, eigenvalues=eig)


def score_covariance(dlog, table, rows=slice(1, None), unfolded=False):
    """``A C A^T`` per point: the covariance of the score over bootstrap rows, with ``A = dlog[P][D][7]`` and ``C`` the sample
    covariance (``ddof = 1``) of the class counts over ``table[rows]`` - by default every row but row 0, which in a ``-bs`` file is the
    data (the sum of the chunks), not a resample.  Needs at least two rows."""
    A = np.asarray(dlog, dtype=np.float64)
    A = A.reshape((-1,) + A.shape[-2:])
    f = class_counts(np.asarray(table, dtype=np.float64).reshape(-1, 8)[rows], unfolded)
    if f.shape[0] < 2:
        raise ValueError("the score covariance needs at least two bootstrap rows (got %d)" % f.shape[0])
    Cm = np.atleast_2d(np.cov(f, rowvar=False, ddof=1))
    return np.einsum("pik,kl,pjl->pij", A, Cm, A)


def sandwich_covariance(hess, dlog, table, rows=slice(1, None), unfolded=False):
    """The sandwich (Godambe) covariance ``H^-1 (A C A^T) H^-1`` per point of ``hess[P][D][D]``, ``dlog[P][D][7]``: what a composite
    likelihood - linked sites treated as independent - reports in the place of ``inv(-H)``; the middle is ``score_covariance`` over
    the bootstrap rows of ``table``, computed on the host.  The bootstrap rows must be resamples of the SAME size as the row the
    Hessian was taken against (a ``-bs`` file's are).  NaN where ``H`` is singular or not finite.  Returns ``cov[P][D][D]``."""
    H = np.asarray(hess, dtype=np.float64)
    H = H.reshape((-1,) + H.shape[-2:])
    J = score_covariance(dlog, table, rows, unfolded)
    out = np.full(H.shape, np.nan)
    for p in range(H.shape[0]):
        if not (np.isfinite(H[p]).all() and np.isfinite(J[p]).all()):
            continue
        try:
            Hi = np.linalg.inv(H[p])
        except np.linalg.LinAlgError:
            continue
        out[p] = Hi @ J[p] @ Hi.T
    return out


def standard_errors(cov):
    """Square roots of the diagonal of ``cov[...][D][D]``; NaN where an entry is negative or NaN."""
    c = np.asarray(cov, dtype=np.float64)
    d = np.diagonal(c, axis1=-2, axis2=-1)
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.where(d >= 0, d, np.nan))


def correlation(cov):
    """The correlation matrix of ``cov[...][D][D]`` (NaN where a variance is not positive)."""
    c = np.asarray(cov, dtype=np.float64)
    se = standard_errors(c)
    with np.errstate(invalid="ignore", divide="ignore"):
        return c / (se[..., :, None] * se[..., None, :])


# ------------------------------------------------------------------------------------------------ block bootstrap ----
# The rule of misti_bootstrap_rows_dev stated on the host (include/misti_hip.h, "block bootstrap"): the device result is this, bit for
# bit.  The stream is the project's own - counter-based, replicate r a function of (seed, r) alone - and NOT the reference's:
# migrationIO.BootstrapJAFS draws from Python's Mersenne Twister, a sequential stream (io.bootstrap_jsfs / io.bootstrap_table keep that one).
BOOT_MAX_CHUNKS, BOOT_MAX_DRAWS = 65535, 1 << 24


def philox_draws(seed, rep, n_chunk, n):
    """The first ``n`` chunk indices of replicate ``rep`` (``misti_bootstrap_draws``): draw j is element j of
    ``numpy.random.Philox(key=[seed, rep]).random_raw`` - Philox4x64-10 from counter 0, which NumPy advances before its first block -
    and its chunk the high 64 bits of the 128-bit product ``raw * n_chunk``.  No rejection step: a chunk's probability is within
    ``n_chunk / 2**64`` of ``1 / n_chunk``.  ``seed`` is a uint64, ``1 <= n_chunk < 2**32``.  Returns int64 ``[n]``."""
    n_chunk = int(n_chunk)
    if not 1 <= n_chunk < 1 << 32 or int(rep) < 0 or int(n) < 0:
        raise ValueError("philox_draws: n_chunk must be 1 ... 2**32 - 1, rep and n not negative")
    raw = np.random.Philox(key=np.array([int(seed), int(rep)], dtype=np.uint64)).random_raw(int(n))
    raw = np.atleast_1d(np.asarray(raw, dtype=np.uint64))
    m, s32 = np.uint64(n_chunk), np.uint64(32)
    hi, lo = raw >> s32, raw & np.uint64(0xFFFFFFFF)                  # raw m = hi m 2^32 + lo m, every term below 2^64
    return ((hi * m + ((lo * m) >> s32)) >> s32).astype(np.int64)


def _in_order_sum(a):
    """The sum along axis 0 by plain additions in index order, from 0.0 (``np.sum`` adds pairwise)."""
    a = np.asarray(a, dtype=np.float64)
    return np.cumsum(np.concatenate([np.zeros((1,) + a.shape[1:]), a]), axis=0)[-1]


def _seg_of(rows):
    """``((c1 + c2) + ... + c7)`` of every row of ``rows[...][8]``."""
    t = rows[..., 1] + rows[..., 2]
    for k in range(3, 8):
        t = t + rows[..., k]
    return t


def check_chunks(chunks):
    """The chunk table as ``misti_bootstrap_rows_dev`` takes it - float64 ``[n_chunk][8]``, column 0 the chunk's length, columns 1..7
    its class counts - with the checks the ABI makes before it touches the device, as a ``ValueError`` of one line: at least one
    chunk and at most ``BOOT_MAX_CHUNKS``, every entry finite, every length > 0 (which bounds the loop), no negative count, and
    ``ceil(genome / smallest length) <= BOOT_MAX_DRAWS``.  Returns ``(chunks, genome, seg)``: the lengths added in chunk order, and the
    running sum over the chunks of ``((c1 + c2) + ... + c7)``."""
    c = np.ascontiguousarray(chunks, dtype=np.float64)
    if c.ndim != 2 or c.shape[1] != 8 or c.shape[0] < 1:
        raise ValueError("the chunk table must be [n_chunk][8] with at least one chunk (got shape %s)" % (c.shape,))
    if c.shape[0] > BOOT_MAX_CHUNKS:
        raise ValueError("%d chunks, beyond the limit of %d" % (c.shape[0], BOOT_MAX_CHUNKS))
    if not np.isfinite(c).all():
        raise ValueError("chunk %d has an entry that is not finite" % int(np.argmax(~np.isfinite(c).all(axis=1))))
    if not (c[:, 0] > 0).all():
        raise ValueError("chunk %d has length %g: a chunk's length must be > 0" % (int(np.argmax(~(c[:, 0] > 0))), c[np.argmax(~(c[:, 0] > 0)), 0]))
    if (c[:, 1:] < 0).any():
        raise ValueError("chunk %d has a negative count" % int(np.argmax((c[:, 1:] < 0).any(axis=1))))
    genome, seg = float(_in_order_sum(c[:, 0])), float(_in_order_sum(_seg_of(c)))
    if not (np.isfinite(genome) and np.isfinite(seg)):
        raise ValueError("the chunk lengths or counts do not sum to a finite number")
    if not np.ceil(genome / c[:, 0].min()) <= BOOT_MAX_DRAWS:
        raise ValueError("a replicate may need ceil(%g / %g) draws, beyond the limit of %d" % (genome, c[:, 0].min(), BOOT_MAX_DRAWS))
    return c, genome, seg


def block_bootstrap(chunks, n, seed=0, first=0, normalize=False, draws=False):
    """The rule of ``misti_bootstrap_rows_dev`` on the host: replicates ``first ... first + n - 1`` of the chunk table (``check_chunks``),
    float64 ``[n][8]`` - with ``draws`` also the number of chunks each drew (int32 ``[n]``).  Replicate r, as ``BootstrapJAFS`` builds
    one: ``sfs = 0``; while ``sfs[0] < genome`` the next index of ``philox_draws(seed, r, n_chunk, ...)`` names a chunk and its 8
    columns are added to ``sfs``, each column in draw order, one float64 addition per draw - nothing is summed in any other order (and,
    as in the kernel, never more than ``BOOT_MAX_DRAWS`` draws: a table that passes the checks stays below).  ``normalize``: the
    reference's ``normalize=True`` - all 8 entries times ``seg / seg_bs``, ``seg_bs = ((s1 + s2) + ... + s7)`` of the replicate, the
    division first and then 8 products.  Replicate r depends on ``(seed, r)`` and the table alone, not on ``n`` or ``first``."""
    c, genome, seg = check_chunks(chunks)
    n, first, n_chunk = int(n), int(first), c.shape[0]
    if n < 0 or first < 0:
        raise ValueError("block_bootstrap: n and first must not be negative")
    rows, count = np.empty((n, 8)), np.empty(n, dtype=np.int32)
    guess = int(min(BOOT_MAX_DRAWS, np.ceil(genome / c[:, 0].mean()) + 8 * np.sqrt(n_chunk) + 16))
    for i in range(n):
        m = guess
        while True:
            idx = philox_draws(seed, first + i, n_chunk, m)
            run = np.cumsum(np.concatenate([np.zeros((1, 8)), c[idx]]), axis=0)      # run[j]: the row after j draws, added in draw order
            reached = run[1:, 0] >= genome
            if reached.any() or m >= BOOT_MAX_DRAWS:
                break
            m = min(2 * m, BOOT_MAX_DRAWS)
        count[i] = int(np.argmax(reached)) + 1 if reached.any() else m
        rows[i] = run[count[i]]
    if normalize:
        with np.errstate(invalid="ignore", divide="ignore"):
            rows = rows * (seg / _seg_of(rows))[:, None]
    return (rows, count) if draws else rows


def block_bootstrap_table(chunks, n, seed=0, normalize=False):
    """The table ``io.bootstrap_table`` lays out, under this rule: row 0 the column sums of all chunks, added in chunk order (never
    normalised: it is the data), row 1 + r replicate r of ``block_bootstrap``.  Float64 ``[1 + n][8]``."""
    c, _, _ = check_chunks(chunks)
    return np.vstack([_in_order_sum(c)[None, :], block_bootstrap(c, n, seed=seed, normalize=normalize)])


# ------------------------------------------------------------------------------------------------ block jackknife ----
# The rule of misti_jackknife_rows_dev stated on the host (include/misti_hip.h, "block jackknife"): the device result is this, bit for
# bit.  The delete-m block jackknife: deterministic - no stream, no seed - G fits instead of a thousand, and a bias-corrected estimate
# besides the standard error (jackknife_estimate).  The reference has no counterpart.
def check_jackknife(chunks, m=1):
    """The chunk table as ``misti_jackknife_rows_dev`` takes it, with the checks the ABI makes before it touches the device, as a
    ``ValueError`` of one line: everything ``check_chunks`` refuses except its draw limit (nothing is drawn here), fewer than 2 chunks,
    ``m < 1``, and ``m >= n_chunk`` - a single group would leave nothing behind.  Returns ``(chunks, G)``, ``G = ceil(n_chunk / m)``."""
    c = np.ascontiguousarray(chunks, dtype=np.float64)
    m = int(m)
    if c.ndim != 2 or c.shape[1] != 8 or c.shape[0] < 2:
        raise ValueError("the chunk table of a jackknife must be [n_chunk][8] with at least 2 chunks (got shape %s)" % (c.shape,))
    if c.shape[0] > BOOT_MAX_CHUNKS:
        raise ValueError("%d chunks, beyond the limit of %d" % (c.shape[0], BOOT_MAX_CHUNKS))
    if m < 1:
        raise ValueError("m must be at least 1 (got %d)" % m)
    if m >= c.shape[0]:
        raise ValueError("groups of m = %d chunks out of %d: a single group would leave nothing behind" % (m, c.shape[0]))
    if not np.isfinite(c).all():
        raise ValueError("chunk %d has an entry that is not finite" % int(np.argmax(~np.isfinite(c).all(axis=1))))
    if not (c[:, 0] > 0).all():
        raise ValueError("chunk %d has length %g: a chunk's length must be > 0" % (int(np.argmax(~(c[:, 0] > 0))), c[np.argmax(~(c[:, 0] > 0)), 0]))
    if (c[:, 1:] < 0).any():
        raise ValueError("chunk %d has a negative count" % int(np.argmax((c[:, 1:] < 0).any(axis=1))))
    with np.errstate(over="ignore"):
        if not (np.isfinite(_in_order_sum(c[:, 0])) and np.isfinite(_in_order_sum(_seg_of(c)))):
            raise ValueError("the chunk lengths or counts do not sum to a finite number")
    return c, -(-c.shape[0] // m)


def jackknife_rows(chunks, m=1, first=0, n=None):
    """The rule of ``misti_jackknife_rows_dev`` on the host: leave-out rows ``first ... first + n - 1`` (``n`` None: all from ``first``) of
    the chunk table (``check_jackknife``), float64 ``[n][8]``.  Group g covers chunks ``g m ... min((g + 1) m, n_chunk) - 1`` - there are
    ``G = ceil(n_chunk / m)``, the last may be short.  Row g starts at eight zeros and walks the chunks in chunk order; for every chunk
    OUTSIDE group g it adds the chunk's 8 columns to its own, one float64 addition per column per chunk.  A chunk inside the group is
    skipped: it is not added as zero, and nothing is subtracted from a total - the fixed order is what makes the result a matter of
    bits for counts that are no integers.  No stream, no normalisation (scaling a row does not move the arg-max of the multinomial
    log-likelihood).  Column 0 of a row is the length left in."""
    c, G = check_jackknife(chunks, m)
    m, first, n_chunk = int(m), int(first), c.shape[0]
    n = G - first if n is None else int(n)
    if first < 0 or n < 0 or first + n > G:
        raise ValueError("jackknife_rows: groups %d ... %d of G = %d" % (first, first + n - 1, G))
    before = np.cumsum(np.concatenate([np.zeros((1, 8)), c]), axis=0)     # before[i]: the row after chunks 0 ... i - 1, added in chunk order
    rows = np.empty((n, 8))
    for i in range(n):
        lo, hi = (first + i) * m, min((first + i + 1) * m, n_chunk)
        # the additions behind the group simply go on from where the ones in front of it stopped
        rows[i] = np.cumsum(np.concatenate([before[lo][None, :], c[hi:]]), axis=0)[-1]
    return rows


def jackknife_table(chunks, m=1):
    """Row 0 - the column sums of all chunks, added in chunk order: exactly row 0 of ``block_bootstrap_table`` - in front of the ``G``
    leave-out rows of ``jackknife_rows``.  Float64 ``[1 + G][8]``; its column 0 carries everything ``jackknife_estimate`` needs."""
    c, _ = check_jackknife(chunks, m)
    return np.vstack([_in_order_sum(c)[None, :], jackknife_rows(c, m)])


def jackknife_weights(lengths):
    """``(n, m_g[G], h_g[G])`` from column 0 of a jackknife table (``lengths[1 + G]``: the whole, then what every leave-out row keeps):
    ``m_g = n - lengths[g]`` the length of group g, ``h_g = n / m_g``.  ``ValueError`` where the column is not such a table's: fewer
    than two leave-out rows, or a row that keeps nothing or everything."""
    l = np.asarray(lengths, dtype=np.float64).reshape(-1)
    if l.size < 3:
        raise ValueError("a jackknife table has row 0 and at least 2 leave-out rows (got %d rows)" % l.size)
    n = l[0]
    if not (np.isfinite(l).all() and n > 0 and (l[1:] > 0).all() and (l[1:] < n).all()):
        raise ValueError("column 0 is not a jackknife table's: every leave-out row keeps a length > 0 and below row 0's")
    m_g = n - l[1:]
    return n, m_g, n / m_g


def _jackknife_one(theta, n, m_g, h_g, level):
    from scipy import stats
    if not np.isfinite(theta[0]):
        return None
    est = float(theta[0])
    has = np.isfinite(theta[1:])
    t, mg, hg = theta[1:][has], m_g[has], h_g[has]
    G = int(t.size)
    out = dict(estimate=est, jackknife=None, bias=None, se=None, interval=None, n_group=G)
    if G < 1:
        return out
    jack = G * est - float(np.sum((1.0 - mg / n) * t))
    out["jackknife"], out["bias"] = jack, est - jack
    if G < 2:
        return out
    tau = hg * est - (hg - 1.0) * t
    se = float(np.sqrt(np.sum((tau - jack) ** 2 / (hg - 1.0)) / G))
    half = float(stats.t.ppf(0.5 + level / 2, G - 1)) * se
    out["se"], out["interval"] = se, (jack - half, jack + half)
    return out


def jackknife_estimate(theta, lengths, level=0.95):
    """The weighted delete-m jackknife of Busing, Meijer and van der Leeden (1999, Statistics and Computing 9: 3-8) from the rows'
    estimates and COLUMN 0 of the table alone (``jackknife_weights``) - a table read back from a file carries everything it needs.
    ``theta[1 + G]`` holds row 0's estimate first, then the leave-out estimates; ``lengths[1 + G]`` is the table's column 0.  With
    ``n = lengths[0]``, ``m_g = n - lengths[g]`` and ``h_g = n / m_g``:
    ``jackknife = G estimate - sum_g (1 - m_g / n) theta_(g)``; pseudo-values ``tau_g = h_g estimate - (h_g - 1) theta_(g)``;
    ``se^2 = (1 / G) sum_g (tau_g - jackknife)^2 / (h_g - 1)``.
    Returns dict(estimate, jackknife, bias (= estimate - jackknife), se, interval (jackknife -+ t.ppf(0.975, G - 1) se), n_group).
    Leave-out rows without a finite estimate are dropped and ``n_group`` counts the rest (G above is that count); fewer than 2 give no
    ``se`` and no ``interval`` (None), none gives no ``jackknife`` either.  A row-0 estimate that is not finite gives no result: None.
    ``theta[1 + G][K]`` is handled per column: every entry an array over the K columns (``interval[K][2]``), NaN where a column has
    none, ``n_group`` 0 for a column without a row-0 estimate."""
    th = np.asarray(theta, dtype=np.float64)
    n, m_g, h_g = jackknife_weights(lengths)
    if th.shape[0] != 1 + m_g.size or th.ndim not in (1, 2):
        raise ValueError("jackknife_estimate: theta must be [1 + G] or [1 + G][K] for the table's G = %d (got shape %s)" % (m_g.size, th.shape))
    if th.ndim == 1:
        return _jackknife_one(th, n, m_g, h_g, level)
    cols = [_jackknife_one(th[:, k], n, m_g, h_g, level) for k in range(th.shape[1])]
    num = lambda v: np.nan if v is None else v
    out = {key: np.array([num(c[key]) if c else np.nan for c in cols], dtype=np.float64) for key in ("estimate", "jackknife", "bias", "se")}
    out["interval"] = np.array([c["interval"] if c and c["interval"] else (np.nan, np.nan) for c in cols], dtype=np.float64).reshape(-1, 2)
    out["n_group"] = np.array([c["n_group"] if c else 0 for c in cols], dtype=np.int64)
    return out


# ------------------------------------------------------------------------------------------- parametric bootstrap ----
# The rule of misti_parametric_rows_dev stated on the host (include/misti_hip.h, "parametric bootstrap"): the device result is this, bit
# for bit.  Replicates for inputs that have no chunks to resample: every site is drawn INDEPENDENTLY from the seven classes of a
# spectrum - the multinomial the data are scored as.  Real sites are linked: intervals from these replicates are narrower than the block
# bootstrap's on the same genome, which remains the confidence statement where chunks exist (pass an effective n_sites to allow for it).
PARAM_MAX_SITES = 1 << 36


def parametric_thresholds(p):
    """The six thresholds of a spectrum ``p[7]`` (``misti_parametric_thresholds``), or None where it is unusable.  ``c_k`` is the running
    sum in class order (one float64 addition per class), ``q_k = c_k / c_6`` one float64 division each, ``T_k = ceil(q_k * 2**53)`` a
    uint64 in ``[0, 2**53]`` - every step exact or correctly rounded, so host, device and NumPy agree.  Unusable: an entry that is
    negative or not finite, or a running sum ``c_6`` that is not finite or not > 0.  ``p`` need not be normalised.  A class's
    probability is quantised to ``2**-53``: no rejection step corrects that."""
    p = np.asarray(p, dtype=np.float64)
    if p.shape != (7,):
        raise ValueError("parametric_thresholds: a spectrum is 7 numbers (got shape %s)" % (p.shape,))
    with np.errstate(over="ignore", invalid="ignore"):
        c = np.cumsum(p)                                              # sequential: ((p0 + p1) + p2) + ...
    if not (np.isfinite(p).all() and (p >= 0).all() and np.isfinite(c[6]) and c[6] > 0):
        return None
    return np.ceil((c[:6] / c[6]) * 2.0 ** 53).astype(np.uint64)


def parametric_counts(T, n_sites, seed, rep):
    """The seven class counts of replicate ``rep`` under thresholds ``T`` (``misti_parametric_counts``): draw j is element j of
    ``numpy.random.Philox(key=[seed, rep]).random_raw`` - the block bootstrap's stream and counter convention (``philox_draws``) -
    ``u = raw >> 11``, and its class the number of k with ``u >= T[k]``: ``numpy.searchsorted(q, Generator(Philox(...)).random(n_sites),
    side='right')``.  With ``g_k = #{j : u_j >= T_k}``: ``n_0 = n_sites - g_0``, ``n_k = g_(k-1) - g_k``, ``n_6 = g_5``.  int64 ``[7]``."""
    n_sites = int(n_sites)
    g = np.zeros(6, dtype=np.int64)
    gen = np.random.Philox(key=np.array([int(seed), int(rep)], dtype=np.uint64))
    left = n_sites
    while left > 0:                                                   # in pieces of whole Philox blocks: the stream simply goes on
        m = min(left, 1 << 22)
        u = np.atleast_1d(np.asarray(gen.random_raw(m), dtype=np.uint64)) >> np.uint64(11)
        u.sort()
        g += m - np.searchsorted(u, T, side="left")                   # #{u >= T_k}
        left -= m
    return np.concatenate([[n_sites - g[0]], g[:-1] - g[1:], [g[5]]]).astype(np.int64)


def parametric_rows(spectra, n, n_sites, genome, seed=0, first=0, spec_of=None, status=None):
    """The rule of ``misti_parametric_rows_dev`` on the host: ``(rows, row_status)`` - replicates ``first ... first + n - 1`` as float64
    ``[n][8]`` and int32 ``[n]``.  Replicate i (global index ``rep = first + i``) draws ``n_sites`` sites from spectrum ``spec_of[i]`` of
    ``spectra[n_spec][7]`` (spectrum 0 without ``spec_of``) and is the row ``[genome, n_0, ..., n_6]`` of ``parametric_counts``: integers
    that sum to ``n_sites`` exactly.  A replicate whose spectrum is unusable (``parametric_thresholds``), whose ``status`` entry is not 0
    (the scorer's rule: only status 0 has a value) or whose index is outside ``0 ... n_spec - 1`` is ``[genome, 0 x 7]`` with row status 1.
    A replicate depends on ``(seed, rep, p, n_sites)`` alone.  The sites are independent - see the note above."""
    sp = np.ascontiguousarray(spectra, dtype=np.float64).reshape(-1, 7)
    n, n_sites, first = int(n), int(n_sites), int(first)
    if n < 0 or first < 0 or not 0 <= n_sites <= PARAM_MAX_SITES or sp.shape[0] < 1 or not np.isfinite(genome):
        raise ValueError("parametric_rows: n and first not negative, 0 <= n_sites <= 2**36, at least one spectrum, a finite genome")
    of = np.zeros(n, dtype=np.int64) if spec_of is None else np.asarray(spec_of, dtype=np.int64).reshape(n)
    st = None if status is None else np.asarray(status, dtype=np.int64).reshape(sp.shape[0])
    T = [parametric_thresholds(p) if st is None or st[s] == 0 else None for s, p in enumerate(sp)]
    rows, row_status = np.zeros((n, 8)), np.zeros(n, dtype=np.int32)
    rows[:, 0] = float(genome)
    for i in range(n):
        t = T[of[i]] if 0 <= of[i] < sp.shape[0] else None
        if t is None:
            row_status[i] = 1
        else:
            rows[i, 1:] = parametric_counts(t, n_sites, seed, first + i)
    return rows, row_status


def parametric_table(data_row, rows):
    """The data row in front of the replicates, as ``block_bootstrap_table`` lays a table out: float64 ``[1 + n][8]``."""
    return np.vstack([np.asarray(data_row, dtype=np.float64).reshape(1, 8), np.asarray(rows, dtype=np.float64).reshape(-1, 8)])


# ----------------------------------------------------------------------------------------- differential evolution ----
# The rule of misti_de_search stated on the host (include/misti_hip.h, "differential evolution per search"): the device result is this,
# bit for bit, on the engine's own objective.  The rule is the project's own, not SciPy's: scipy.optimize.differential_evolution redraws
# a coordinate that leaves the bounds, so the number of its draws depends on the data; here every member of every generation owns a
# fixed piece of a counter-based stream and a crossed bound is repaired without a draw.  Modelled on SciPy's best1bin, updating='deferred'.
DE_BLOCKS, DE_MAX_POP, DE_MAX_N = 5, 256, 16


def _mulhi_index(raw, n):
    """The high 64 bits of ``raw x n`` per element (``boot_index`` of misti_boot.h), ``1 <= n < 2**32``: int64."""
    raw = np.asarray(raw, dtype=np.uint64)
    m, s32 = np.uint64(n), np.uint64(32)
    hi, lo = raw >> s32, raw & np.uint64(0xFFFFFFFF)
    return ((hi * m + ((lo * m) >> s32)) >> s32).astype(np.int64)


def _de_generation(seed, id_, generation, pop, n):
    """What the ``pop`` members of generation ``generation`` of the stream ``Philox(key=[seed, id_])`` draw: member i owns the
    ``DE_BLOCKS`` blocks from block ``(generation * pop + i) * DE_BLOCKS`` on (NumPy advances the counter before every block, so the
    stream's block b is the counter b + 1: a generator set to counter b starts with it), 4 ``DE_BLOCKS`` words ``w``: ``w[0]`` r1,
    ``w[1]`` r2, ``w[2]`` jrand, ``w[3]`` F's uniform, ``w[4 + k]`` the uniform of coordinate k.
    Returns r1[pop], r2[pop], jrand[pop] (int64), u_F[pop], u[pop][n] (float64)."""
    pop, n = int(pop), int(n)
    if not 4 <= pop <= DE_MAX_POP or not 1 <= n <= DE_MAX_N or int(generation) < 0:
        raise ValueError("de_draws: pop must be 4 ... %d, n 1 ... %d, the generation not negative" % (DE_MAX_POP, DE_MAX_N))
    counter = np.array([int(generation) * pop * DE_BLOCKS, 0, 0, 0], dtype=np.uint64)
    gen = np.random.Philox(key=np.array([int(seed), int(id_)], dtype=np.uint64), counter=counter)
    w = np.asarray(gen.random_raw(pop * 4 * DE_BLOCKS), dtype=np.uint64).reshape(pop, 4 * DE_BLOCKS)
    i = np.arange(pop)
    r1 = _mulhi_index(w[:, 0], pop - 1)
    r1 = r1 + (r1 >= i)                                               # the P - 1 members other than i, in member order
    a, b = np.minimum(i, r1), np.maximum(i, r1)
    r2 = _mulhi_index(w[:, 1], pop - 2)
    r2 = r2 + (r2 >= a)                                               # the P - 2 members other than i and r1
    r2 = r2 + (r2 >= b)
    jrand = _mulhi_index(w[:, 2], n)
    uniform = lambda raw: (raw >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return r1, r2, jrand, uniform(w[:, 3]), uniform(w[:, 4:4 + n])


def de_draws(seed, id_, generation, member, pop, n):
    """``misti_de_draws``: what member ``member`` of generation ``generation`` of the stream ``numpy.random.Philox(key=[seed, id_])``
    draws in a search of ``pop`` members and ``n`` coordinates.  Returns dict(r1, r2, jrand, u_F, u[n]); generation 0 uses ``u`` alone."""
    if not 0 <= int(member) < int(pop):
        raise ValueError("de_draws: member must be 0 ... pop - 1")
    r1, r2, jrand, u_F, u = _de_generation(seed, id_, generation, pop, n)
    m = int(member)
    return dict(r1=int(r1[m]), r2=int(r2[m]), jrand=int(jrand[m]), u_F=float(u_F[m]), u=u[m].copy())


def differential_evolution_rule(fun_batch, starts, lo, hi, pop=16, maxiter=100, tol=0.01, atol=0.0, F=(0.5, 1.0), CR=0.7, seed=0, ids=None):
    """The rule of ``misti_de_search``, operation for operation.  ``fun_batch(X[M][N], s[M]) -> f[M]`` evaluates M points at once, point
    m belonging to search ``s[m]`` (``+inf``: no value; a NaN counts as ``+inf``).  ``starts`` ``[S][N]``: member 0 of every search;
    ``lo`` / ``hi``: the finite box, ``[N]`` or ``[S][N]``, ``lo == hi`` holds a coordinate fixed; ``ids[s]`` (default s): the stream of
    search s is ``numpy.random.Philox(key=[seed, ids[s]])``.

    Generation 0: member 0 is the start clipped to the box, member i > 0 ``clip(lo + u * (hi - lo))``.  Generation g >= 1, member i:
    ``best`` the member with the lowest f (ties: the lowest index), ``v = best + F * (x[r1] - x[r2])`` with ``F = F_lo + u_F * (F_hi -
    F_lo)``; the trial takes ``v[k]`` where ``k == jrand`` or ``u[k] < CR`` and ``x[i][k]`` elsewhere; a ``v[k]`` beyond a bound becomes
    ``x[i][k] + 0.5 * (bound - x[i][k])``; a fixed coordinate stays at ``lo``.  All trials of a generation are evaluated as one batch
    against the population of the generation before; member i is replaced iff ``f(trial) <= f(x[i])``.  After every generation, the
    initial one included, a search stops with status 0 when every member has a value and ``q / P <= (atol + tol * abs(m)) ** 2`` with
    ``m = (f[0] + f[1] + ...) / P`` and ``q = (f[0] - m) ** 2 + (f[1] - m) ** 2 + ...`` (sums in member order, from f[0] and from 0.0);
    with status 2 after ``maxiter`` generations.  A stopped search submits no further points.
    Returns dict(x[S][N], llh[S] (= -f of the best member; -inf: no point ever had a value), nit[S], nfev[S], status[S],
    population[S][P][N], population_llh[S][P], n_points: the points handed to ``fun_batch`` in all)."""
    x0 = np.atleast_2d(np.asarray(starts, dtype=float))
    S, N = x0.shape
    P = int(pop)
    F_lo, F_hi = (float(v) for v in F)
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=float), (S, N)))
    hi = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, dtype=float), (S, N)))
    with np.errstate(over="ignore", invalid="ignore"):
        usable = np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all() and np.isfinite(hi - lo).all() and np.isfinite(x0).all()
    if not usable:
        raise ValueError("differential_evolution_rule: the box must be finite with lo <= hi, the starts finite")
    if not 4 <= P <= DE_MAX_POP or int(maxiter) < 1:
        raise ValueError("differential_evolution_rule: pop must be 4 ... %d, maxiter >= 1" % DE_MAX_POP)
    ids = np.arange(S) if ids is None else np.asarray(ids).reshape(S)
    fixed = lo == hi

    def values(X, s_of):
        f = np.asarray(fun_batch(X.reshape(-1, N), np.repeat(s_of, P)), dtype=float).reshape(-1, P)
        return np.where(np.isnan(f), np.inf, f)

    x = np.empty((S, P, N))
    for s in range(S):
        u = _de_generation(seed, ids[s], 0, P, N)[4]
        x[s] = lo[s] + u * (hi[s] - lo[s])
        x[s, 0] = x0[s]
        x[s] = np.clip(x[s], lo[s], hi[s])
    f = values(x, np.arange(S))
    n_points = S * P
    nit = np.zeros(S, dtype=np.int32)
    status = np.full(S, 2, dtype=np.int32)
    best = np.zeros(S, dtype=np.int64)
    live = np.arange(S)
    for g in range(0, int(maxiter) + 1):
        if g >= 1:
            t = np.empty((live.size, P, N))
            for j, s in enumerate(live):
                r1, r2, jrand, u_F, u = _de_generation(seed, ids[s], g, P, N)
                Fd = (F_lo + u_F * (F_hi - F_lo))[:, None]
                v = x[s, best[s]][None, :] + Fd * (x[s, r1] - x[s, r2])
                up = x[s] + 0.5 * (hi[s] - x[s])
                dn = x[s] + 0.5 * (lo[s] - x[s])
                v = np.clip(np.where(v > hi[s], up, np.where(v < lo[s], dn, v)), lo[s], hi[s])
                cross = (np.arange(N)[None, :] == jrand[:, None]) | (u < CR)
                t[j] = np.where(fixed[s], lo[s], np.where(cross, v, x[s]))
            ft = values(t, live)
            n_points += live.size * P
            take = ft <= f[live]
            x[live] = np.where(take[:, :, None], t, x[live])
            f[live] = np.where(take, ft, f[live])
            nit[live] = g
        go = []
        for s in live:
            fs = f[s]
            best[s] = int(np.argmin(fs))                      # the first minimum: the lowest index on ties
            stop = False
            if (fs < np.inf).all():
                total = fs[0]
                for m in range(1, P):
                    total = total + fs[m]
                mean = total / P
                q = 0.0
                with np.errstate(invalid="ignore", over="ignore"):
                    for m in range(P):
                        d = fs[m] - mean
                        q = q + d * d
                    thr = atol + tol * abs(mean)
                    stop = bool(q / P <= thr * thr)
            if stop:
                status[s] = 0
            elif g < int(maxiter):
                go.append(s)
        live = np.asarray(go, dtype=np.int64)
        if live.size == 0:
            break
    bi = best[:, None]
    return dict(x=np.take_along_axis(x, bi[:, :, None], axis=1)[:, 0], llh=-np.take_along_axis(f, bi, axis=1)[:, 0], nit=nit,
                nfev=(P * (nit + 1)).astype(np.int32), status=status, population=x, population_llh=-f, n_points=int(n_points))


def _de_profile(R, n_per_row, search, polish):
    """What bootstrap_profile_de and split_fit_de share: ``search(r_of, j_of, ids)`` is ONE differential-evolution call over every
    (row, search-within-row) pair, row outermost; the stream id of a search is its index WITHIN its row, so a row's result does not depend
    on which other rows the call holds.  With ``polish`` one boxed Nelder-Mead call (``search`` with the DE's ``x`` as its last argument)
    starts from the DE results and a search keeps the better of the two (the polished one on ties)."""
    r_of, j_of = (a.ravel() for a in np.meshgrid(np.arange(R), np.arange(n_per_row), indexing="ij"))
    de = search(r_of.astype(np.int32), j_of, j_of.astype(np.uint64), None)
    out = dict(de, de_llh=de["llh"].copy(), polished=np.zeros(r_of.size, dtype=bool))
    if polish:
        nm = search(r_of.astype(np.int32), j_of, None, de["x"])
        better = nm["llh"] >= de["llh"]                       # NaN never wins
        out["x"] = np.where(better[:, None], nm["x"], de["x"])
        out["llh"] = np.where(better, nm["llh"], de["llh"])
        out["polished"] = better
        out["polish_nfev"] = nm["nfev"]
    return out


def bootstrap_profile_de(engine, split_values, jsfs_rows, start, box, pop=16, maxiter=50, tol=0.01, atol=0.0, F=(0.5, 1.0), CR=0.7, seed=0,
                         polish=False, polish_tol=1e-4, polish_maxiter=1000, return_population=False):
    """``bootstrap_profile_global`` with differential evolution in place of basin hopping: per (row, split) pair ONE population search
    inside ``box`` (``(lo, hi)``, each ``[n_param]``, finite), all R x P searches in ONE ``misti_de_search`` call - every generation one
    dense engine batch, no inner minimisations.  ``start`` ``[n_param]`` is member 0 of every search.  The stream id of a search is its
    split's index, so a row's result does not depend on the other rows.  ``polish``: one ``nm_solve_box`` call from the DE results
    under the same box (the ``scan_polish`` pattern); a search keeps the better result.
    Returns dict(x[R][P][N], llh[R][P], de_llh[R][P], nit / nfev / status[R][P] (the DE's), polished[R][P], n_points) and, with
    ``return_population``, the DE's final population[R][P][pop][N] and population_llh[R][P][pop] (an initial ensemble for
    ``bootstrap_profile_mcmc``)."""
    rows = np.asarray(jsfs_rows, dtype=float).reshape(-1, 8)
    splits = np.asarray(split_values, dtype=float).reshape(-1)
    R, Q = rows.shape[0], splits.size
    x0 = np.asarray(start, dtype=float).reshape(1, engine.n_param)

    def search(r_of, j_of, ids, polish_from):
        if polish_from is not None:
            return engine.nm_solve_box(polish_from, r_of, rows, box, split_times=splits[j_of], tol=polish_tol, maxiter=polish_maxiter)
        return engine.differential_evolution(np.repeat(x0, r_of.size, axis=0), r_of, rows, box, split_times=splits[j_of], pop=pop,
                                             maxiter=maxiter, tol=tol, atol=atol, F=F, CR=CR, seed=seed, ids=ids, return_population=return_population)
    out = _de_profile(R, Q, search, polish)
    return {k: (v.reshape(R, Q, *v.shape[1:]) if isinstance(v, np.ndarray) else v) for k, v in out.items()}


def split_fit_de(engine, jsfs_rows, start, box, band_bounds=None, pulse_times=None, pop=16, maxiter=50, tol=0.01, atol=0.0, F=(0.5, 1.0), CR=0.7,
                 seed=0, polish=False, polish_tol=1e-4, polish_maxiter=1000, return_population=False):
    """``split_fit_global`` with differential evolution in place of basin hopping: per row ONE population search over (optimised
    parameters, split) inside ``box`` (``(lo, hi)``, each ``[n_param + 1]``, finite, the split last), all R searches in ONE
    ``misti_de_search`` call.  ``start`` ``[n_param + 1]`` is member 0 of every search; every row draws from stream 0 (the rows of a
    bootstrap share their random numbers - only the data differ).  ``band_bounds`` / ``pulse_times`` apply to every search.
    ``polish``: one ``nm_solve_box`` call from the DE results under the same box; a row keeps the better result.
    Returns dict(x[R][n_param + 1], split[R], llh[R], de_llh[R], nit / nfev / status[R] (the DE's), polished[R], n_points) and, with
    ``return_population``, the DE's final population[R][pop][n_param + 1] and population_llh[R][pop];
    ``split_fit_interval`` takes ``split`` and ``llh`` unchanged."""
    rows = np.asarray(jsfs_rows, dtype=float).reshape(-1, 8)
    R = rows.shape[0]
    x0 = np.asarray(start, dtype=float).reshape(1, engine.n_param + 1)
    tile = lambda a, shape, S: None if a is None else np.repeat(np.asarray(a, dtype=np.int32).reshape(shape), S, axis=0)

    def search(r_of, j_of, ids, polish_from):
        per = dict(band_bounds=tile(band_bounds, (1, -1, 2), r_of.size), pulse_times=tile(pulse_times, (1, -1), r_of.size))
        if polish_from is not None:
            return engine.nm_solve_box(polish_from, r_of, rows, box, tol=polish_tol, maxiter=polish_maxiter, **per)
        return engine.differential_evolution(np.repeat(x0, r_of.size, axis=0), r_of, rows, box, fit_split=True, pop=pop, maxiter=maxiter,
                                             tol=tol, atol=atol, F=F, CR=CR, seed=seed, ids=ids, return_population=return_population, **per)
    out = _de_profile(R, 1, search, polish)
    out["split"] = out["x"][:, -1].copy()
    return out


# --------------------------------------------------------------------------------------------------- ensemble MCMC ----
# The rule of misti_ensemble_sample stated on the host (include/misti_hip.h, "ensemble MCMC per search"): the device result is this, bit
# for bit, on the engine's own objective.  The affine-invariant ensemble sampler (Goodman & Weare's stretch move, the algorithm of
# emcee); the rule is the project's own - emcee draws from a Mersenne Twister in an order that depends on the ensemble; here walker i
# of step t owns block t W + i of a counter-based stream - and so is the exponential of the decision: neither numpy.exp nor the
# device's exp is specified to the bit.
ENS_MAX_WALKERS = 256
_ENS_INV_LN2, _ENS_LN2_HI, _ENS_LN2_LO = float.fromhex("0x1.71547652b82fep+0"), float.fromhex("0x1.62e42feep-1"), float.fromhex("0x1.a39ef35793c76p-33")
_ENS_ROUND = 6755399441055744.0                                     # 1.5 x 2^52: adding and subtracting it rounds to the nearest integer
_ENS_COEF = [1.0, 1.0, 1.0 / 2, 1.0 / 6, 1.0 / 24, 1.0 / 120, 1.0 / 720, 1.0 / 5040, 1.0 / 40320, 1.0 / 362880, 1.0 / 3628800, 1.0 / 39916800,
             1.0 / 479001600, 1.0 / 6227020800.0]


def ens_exp(x):
    """The sampler's exponential (``misti_ens_exp``), from additions, multiplications, comparisons and one ``ldexp``, each rounded on
    its own: ``kd`` the integer nearest to ``x / ln 2``, ``r = (x - kd LN2_HI) - kd LN2_LO`` (``kd LN2_HI`` is exact: the constant has
    32 trailing zero bits), the Taylor polynomial of degree 13 in Horner form on ``|r| <= 0.35``, then ``ldexp(., kd)``.  0 below -746,
    ``+inf`` above 710, NaN for NaN.  Within 4 ulp of the exponential on [-745, 709] (measured: DESIGN.md)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        kd = (x * _ENS_INV_LN2 + _ENS_ROUND) - _ENS_ROUND
        r = x - kd * _ENS_LN2_HI
        r = r - kd * _ENS_LN2_LO
        p = np.full(x.shape, _ENS_COEF[13])
        for n in range(12, -1, -1):
            p = p * r + _ENS_COEF[n]
        k = np.where(np.abs(kd) < 4096.0, kd, 0.0).astype(np.int32)
        y = np.ldexp(p, k)
    y = np.where(x > 710.0, np.inf, np.where(x < -746.0, 0.0, y))
    y = np.where(np.isnan(x), x, y)
    return y if y.ndim else float(y)


def _ens_raw(seed, id_, first_step, n_steps, W):
    """The words of steps ``first_step ... first_step + n_steps - 1``: ``[n_steps][W][4]`` uint64.  Walker i of step t owns block
    ``t W + i`` (NumPy advances the counter before every block: a generator set to counter b starts with the stream's block b)."""
    counter = np.array([int(first_step) * int(W), 0, 0, 0], dtype=np.uint64)
    gen = np.random.Philox(key=np.array([int(seed), int(id_)], dtype=np.uint64), counter=counter)
    return np.asarray(gen.random_raw(int(n_steps) * W * 4), dtype=np.uint64).reshape(int(n_steps), W, 4)


def _ens_uniform(raw):
    return (raw >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def ens_draws(seed, id_, step, walker, W):
    """``misti_ens_draws``: what walker ``walker`` of step ``step`` of the stream ``numpy.random.Philox(key=[seed, id_])`` draws in an
    ensemble of ``W`` walkers - block ``step W + walker``: ``w[0]`` the partner among the ``W / 2`` walkers of the other half (the high
    64 bits of ``raw x W / 2``), ``w[1]`` the stretch's uniform, ``w[2]`` the decision's.  Returns dict(partner, u_z, u_acc)."""
    W = int(W)
    if not 4 <= W <= ENS_MAX_WALKERS or W % 2 or int(step) < 0 or not 0 <= int(walker) < W:
        raise ValueError("ens_draws: W must be even, 4 ... %d, the step not negative, the walker 0 ... W - 1" % ENS_MAX_WALKERS)
    w = _ens_raw(seed, id_, step, 1, W)[0, int(walker)]
    return dict(partner=int(_mulhi_index(w[0], W // 2)), u_z=float(_ens_uniform(w[1])), u_acc=float(_ens_uniform(w[2])))


def ens_decision(z, d, llk_old, llk_new, T, u_acc):
    """The decision on an evaluated proposal (``misti_ens_accept``), elementwise: a proposal without a value (not finite) is rejected, a
    walker without a value accepts any proposal that has one, otherwise ``g = z^d`` by d successive multiplications from 1.0,
    ``e = (llk_new - llk_old) / T``, ``p = g ens_exp(e)``, accepted iff ``u_acc < p``.  ``d`` broadcasts (an integer per element)."""
    z, old, new, T, u = (np.asarray(v, dtype=np.float64) for v in (z, llk_old, llk_new, T, u_acc))
    d = np.asarray(d, dtype=np.int64)
    shape = np.broadcast(z, d, old, new, T, u).shape
    z, d, old, new, T, u = (np.broadcast_to(v, shape) for v in (z, d, old, new, T, u))
    g = np.ones(shape)
    with np.errstate(all="ignore"):
        for k in range(int(d.max()) if d.size else 0):
            g = np.where(k < d, g * z, g)
        p = g * ens_exp((new - old) / T)
        take = u < p
    return np.isfinite(new) & (~np.isfinite(old) | take)


def ensemble_rule(fun_batch, init, lo, hi, n_step, thin=1, temperature=1.0, a=2.0, seed=0, ids=None):
    """The rule of ``misti_ensemble_sample``, operation for operation.  ``fun_batch(X[M][N], s[M]) -> f[M]`` evaluates M points at once,
    point m belonging to search ``s[m]`` (f = -llk; ``+inf``: no value; a NaN counts as ``+inf``).  ``init`` ``[S][W][N]``: the initial
    ensembles, W even, every walker inside its box; ``lo`` / ``hi``: the finite box, ``[N]`` or ``[S][N]``, ``lo == hi`` holds a
    coordinate fixed; ``temperature``: a scalar or ``[S]``, the target is ``llk / T`` inside the box (a uniform prior on it);
    ``ids[s]`` (default s): the stream of search s is ``numpy.random.Philox(key=[seed, ids[s]])``.

    All initial walkers are ONE batch.  Step t = 1 ... n_step: in half 0 walkers ``0 ... W/2 - 1`` move against the second half as it
    stands, in half 1 walkers ``W/2 ... W - 1`` against the first half as half 0 left it; a half-step of all searches is ONE batch.
    Walker i of step t owns block ``t W + i`` (``ens_draws``): partner j, ``z = ((a - 1) u_z + 1)^2 / a``, proposal
    ``y = x_j + z (x_i - x_j)`` (a fixed coordinate: ``lo``), every operation rounded on its own.  A proposal with a coordinate outside
    ``[lo, hi]`` (or NaN) is rejected without an evaluation - it is never passed to ``fun_batch``.  The decision is ``ens_decision`` with
    ``d = N_free - 1``.  No stopping rule.
    Returns dict(chain[S][n_keep][W][N], chain_llh[S][n_keep][W] (the ensembles after steps thin, 2 thin, ...; n_keep = n_step // thin),
    accepted[S][W] int32, last[S][W][N], last_llh[S][W], n_points: the PROPOSALS handed to ``fun_batch`` - the S W initial evaluations
    are not counted).

    A search is a fit of ONE rung at its temperature, without swap rounds: the lines are ``_sampler_steps``'s."""
    return _one_rung("ensemble_rule", fun_batch, init, lo, hi, n_step, None, thin, temperature, a, seed, ids)


def _one_rung(who, fun_batch, init, lo, hi, n_step, prior, thin, temperature, a, seed, ids):
    """``ensemble_rule`` / ``ensemble_prior_rule`` through ``_sampler_steps``: every search a fit of one rung at its own temperature, no
    swap rounds; what comes back loses the rung's axis."""
    x = np.asarray(init, dtype=np.float64)
    if x.ndim != 3:
        raise ValueError("%s: init must be [S][W][N]" % who)
    T = np.broadcast_to(np.asarray(temperature, dtype=float), x.shape[:1])[:, None]
    r = _sampler_steps(who, fun_batch, x[:, None], lo, hi, T, n_step, prior, thin, 0, 0, a, seed, ids, "the temperature must be finite and positive")
    return dict(chain=r["chain"], chain_llh=r["chain_llh"][:, 0], accepted=r["accepted"][:, 0], last=r["last"][:, 0], last_llh=r["last_llh"][:, 0],
                n_points=r["n_points"])


def ensemble_start(x, lo, hi, W, spread=1e-2, seed=0, id_=0):
    """An initial ensemble ``[W][N]`` around the point ``x`` inside the box: walker 0 is ``clip(x)``, walker i > 0 is
    ``clip(x + spread (hi - lo) (2 u - 1))`` per coordinate.  The uniforms are words ``i N + k`` of
    ``numpy.random.Philox(key=[seed, id_], counter=[0, 1, 0, 0])``: the sampler's key, in a part of the counter space (second counter word
    1) that no step of the sampler reaches - the W blocks below the first step's hold 4 W words, too few for ``(W - 1) N`` uniforms once
    N > 4.  A fixed coordinate comes out at ``lo``.  Host only."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    N, W = x.size, int(W)
    lo, hi = (np.broadcast_to(np.asarray(v, dtype=np.float64), (N,)) for v in (lo, hi))
    gen = np.random.Philox(key=np.array([int(seed), int(id_)], dtype=np.uint64), counter=np.array([0, 1, 0, 0], dtype=np.uint64))
    u = _ens_uniform(np.asarray(gen.random_raw(W * N), dtype=np.uint64)).reshape(W, N)
    pts = x[None, :] + float(spread) * (hi - lo)[None, :] * (2.0 * u - 1.0)
    pts[0] = x
    return np.clip(pts, lo, hi)


def composite_temperature(H, J):
    """The magnitude adjustment of a composite likelihood: ``T = |trace(H^-1 J)| / p`` with ``H`` the Hessian of the log-likelihood at
    the fit (``curvature``'s ``hess``, one point ``[p][p]``) and ``J`` the covariance of the score (``score_covariance``) - the two
    matrices the sandwich covariance is built from.  Sampling ``llk / T`` gives the composite posterior the average spread of the
    sandwich: ``curvature`` provides the calibration, the sampler the shape.  ``J = H`` gives 1, ``J = c H`` gives c (the Hessian's
    sign drops out).  Raises where ``H`` is flagged not negative definite (``observed_covariance``) or ``J`` is not finite."""
    H = np.asarray(H, dtype=np.float64)
    J = np.asarray(J, dtype=np.float64).reshape(H.shape)
    if H.ndim != 2 or H.shape[0] != H.shape[1]:
        raise ValueError("composite_temperature: H and J must be [p][p]")
    if not observed_covariance(H)["ok"][0]:
        raise ValueError("composite_temperature: the Hessian is not negative definite - no calibration at this point")
    if not np.isfinite(J).all():
        raise ValueError("composite_temperature: J is not finite")
    T = abs(float(np.trace(np.linalg.solve(H, J)) / H.shape[0]))
    if not (np.isfinite(T) and T > 0):
        raise ValueError("composite_temperature: trace(H^-1 J) / p = %g is not a temperature" % T)
    return T


def autocorrelation_time(series, c=5.0):
    """The integrated autocorrelation time of a 1-D series, ``tau = 1 + 2 sum_{k=1}^{M} rho_k`` with Sokal's window: the smallest M
    with ``M >= c tau(M)``.  A constant series returns 1."""
    y = np.asarray(series, dtype=np.float64).reshape(-1)
    n = y.size
    y = y - y.mean()
    var = float(np.dot(y, y))
    if n < 2 or var == 0.0:
        return 1.0
    size = 1 << (2 * n - 1).bit_length()
    f = np.fft.rfft(y, size)
    rho = np.fft.irfft(f * np.conj(f), size)[:n] / var
    tau = 2.0 * np.cumsum(rho) - 1.0
    ok = np.arange(n) >= c * tau
    M = int(np.argmax(ok)) if ok.any() else n - 1
    return float(max(tau[M], 1.0))


def ensemble_summary(chain, burn=0, accepted=None, n_step=None):
    """Per coordinate of one search's ``chain[n_keep][W][N]`` after dropping the first ``burn`` kept steps: ``mean``, ``median``,
    ``q025`` / ``q975`` (the 2.5 % / 97.5 % quantiles over steps and walkers), ``tau`` (``autocorrelation_time`` of the ensemble-mean
    series, in kept steps) and ``short`` (True where fewer than 50 ``tau`` kept steps remain).  ``acceptance``: the fraction of moves
    accepted - ``accepted.sum() / (W n_step)`` where both are given, otherwise the fraction of kept (step, walker) pairs whose position
    differs from the kept step before."""
    c = np.asarray(chain, dtype=np.float64)
    if c.ndim != 3:
        raise ValueError("ensemble_summary: chain must be [n_keep][W][N]")
    K, W, N = c.shape
    burn = int(burn)
    if not 0 <= burn < K:
        raise ValueError("ensemble_summary: burn must be 0 ... n_keep - 1 (n_keep = %d)" % K)
    k = c[burn:]
    flat = k.reshape(-1, N)
    tau = np.array([autocorrelation_time(k[:, :, j].mean(axis=1)) for j in range(N)])
    if accepted is not None and n_step:
        acc = float(np.sum(accepted)) / (W * int(n_step))
    else:
        acc = float((c[1:] != c[:-1]).any(axis=2).mean()) if K > 1 else float("nan")
    q = np.quantile(flat, [0.025, 0.5, 0.975], axis=0)
    return dict(mean=flat.mean(axis=0), median=q[1], q025=q[0], q975=q[2], tau=tau, short=(K - burn) < 50.0 * tau, acceptance=acc, n=K - burn)


# ----------------------------------------------------------------------------------- posterior summaries on the device ----
# The rule of misti_ens_summary_dev / misti_ensemble_posterior stated on the host (include/misti_hip.h, "posterior summaries on the
# device"): the device result is this, bit for bit.  Every operation is rounded on its own; NumPy's elementwise arithmetic does that.
POST_MAX_PROBS = 8
_POST_LANES = 64


def post_order_key(x):
    """The rule's total order: the 64-bit key of a double's bits - a set sign bit flips all bits, a clear one only the sign bit.
    -0.0 sorts before +0.0, NaN (of a clear sign bit) last."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b ^ np.uint64(1 << 63))


def lsum(v):
    """The only way the rule sums over steps, along axis 0 of ``v[count][...]`` (count >= 1): 64 partials, partial l =
    ``v[l] + v[l + 64] + ...`` in increasing index over ``ceil(count / 64)`` terms, an absent term being +0.0; then
    ``partial[l] += partial[l + stride]`` for ``l < stride``, stride = 32, 16, 8, 4, 2, 1; the result is ``partial[0]``."""
    v = np.asarray(v, dtype=np.float64)
    rows = -(-v.shape[0] // _POST_LANES)
    pad = np.zeros((rows * _POST_LANES,) + v.shape[1:])
    pad[:v.shape[0]] = v
    pad = pad.reshape((rows, _POST_LANES) + v.shape[1:])
    with np.errstate(all="ignore"):
        part = pad[0].copy()
        for r in range(1, rows):
            part = part + pad[r]
        stride = _POST_LANES // 2
        while stride >= 1:
            part[:stride] = part[:stride] + part[stride:2 * stride]
            stride //= 2
    return part[0]


def ensemble_posterior_rule(chain, chain_llh=None, burn=0, probs=(0.025, 0.5, 0.975), max_lag=None, c=5.0):
    """The rule of ``misti_ens_summary_dev``, operation for operation, for ``chain[S][K][W][N]`` (or one search ``[K][W][N]``) and
    ``chain_llh[S][K][W]`` (or None).  Search s has ``x[t][w][j]`` for the kept steps ``t = burn ... K - 1``: ``n = K - burn`` steps,
    ``m = n W`` samples.
      order     the samples of a coordinate by ``post_order_key``: ``x_(0) <= ... <= x_(m-1)``
      quantile  ``h = double(m - 1) p``, ``i = floor(h)``, ``g = h - i``; ``g == 0`` or ``i >= m - 1``: ``x_(min(i, m - 1))``
                exactly, otherwise ``x_(i) + g (x_(i+1) - x_(i))``
      mean      ``e_t[j] = (x[t][0][j] + x[t][1][j] + ...) / W`` in walker order, ``mean[j] = lsum(e)[j] / n``
      cov       ``lsum_t(sum over w in walker order of (x[t][w][j] - mean[j]) (x[t][w][k] - mean[k])) / (m - 1)``, j <= k, mirrored
      tau       ``y_t = e_t[j] - mean[j]``, ``L = min(max_lag, n - 1)`` (``max_lag`` None: ``n - 1``), ``c_k = lsum_{t < n - k}(y_t
                y_{t+k})``; ``c_0 == 0`` and ``L >= 1``: tau = 1, window = 0; otherwise ``rho_k = c_k / c_0``, ``tau_0 = 1``, ``tau_M =
                tau_{M-1} + 2 rho_M``, window the smallest M in 0 ... L with ``double(M) >= c tau_M``; none: window = -1 and ``tau_L``
                (so ``L == 0`` gives window = -1 and tau = 1).  Reported: ``tau_window``, or 1 where that is below 1.  This is
                ``autocorrelation_time``'s estimator by direct sums, with the lag capped
      best      among the kept (t, w) whose ``chain_llh`` is neither NaN nor -inf the largest, ties to the lowest t, then the lowest w:
                ``best_llh``, ``best_x``, ``best_at = (t - burn, w)``; none, or no ``chain_llh``: -inf, NaN, (-1, -1)
    A chain element that is not finite is no error: the key order and IEEE arithmetic define the result, and since IEEE leaves a NaN's
    sign and payload open, a NaN in ``mean``, ``cov``, ``quant`` or ``tau`` is the canonical quiet NaN (``best_x`` copies the sample's bits).
    Returns dict(mean[S][N], cov[S][N][N], quant[S][N][P], tau[S][N], window[S][N] int32, best_llh[S], best_x[S][N], best_at[S][2]
    int32, order[S][N][m]: the order statistics themselves) - without the leading axis for one search."""
    x = np.asarray(chain, dtype=np.float64)
    one = x.ndim == 3
    if one:
        x = x[None]
        chain_llh = None if chain_llh is None else np.asarray(chain_llh, dtype=np.float64)[None]
    if x.ndim != 4:
        raise ValueError("ensemble_posterior_rule: chain must be [S][K][W][N] or [K][W][N]")
    S, K, W, N = x.shape
    burn = int(burn)
    pr = np.asarray(probs, dtype=np.float64).reshape(-1)
    P = pr.size
    if not 0 <= burn < K or not 1 <= P <= POST_MAX_PROBS or not ((pr >= 0) & (pr <= 1)).all() or W < 1 or N < 1:
        raise ValueError("ensemble_posterior_rule: burn must be 0 ... K - 1, 1 ... %d probabilities in [0, 1]" % POST_MAX_PROBS)
    n = K - burn
    m = n * W
    max_lag = n - 1 if max_lag is None else int(max_lag)
    c = float(c)
    if max_lag < 0 or not (np.isfinite(c) and c > 0):
        raise ValueError("ensemble_posterior_rule: max_lag must not be negative, c finite and positive")
    L = min(max_lag, n - 1)
    llh = None if chain_llh is None else np.asarray(chain_llh, dtype=np.float64).reshape(S, K, W)
    out = dict(mean=np.empty((S, N)), cov=np.empty((S, N, N)), quant=np.empty((S, N, P)), tau=np.empty((S, N)), window=np.empty((S, N), dtype=np.int32),
               best_llh=np.full(S, -np.inf), best_x=np.full((S, N), np.nan), best_at=np.full((S, 2), -1, dtype=np.int32), order=np.empty((S, N, m)))
    with np.errstate(all="ignore"):
        for s in range(S):
            k = x[s, burn:]                                                   # [n][W][N]
            flat = k.reshape(m, N)
            for j in range(N):
                v = np.ascontiguousarray(flat[:, j])
                o = v[np.argsort(post_order_key(v), kind="stable")]
                out["order"][s, j] = o
                for p in range(P):
                    h = float(m - 1) * pr[p]
                    i = int(np.floor(h))
                    g = h - np.floor(h)
                    out["quant"][s, j, p] = o[min(i, m - 1)] if g == 0.0 or i >= m - 1 else o[i] + g * (o[i + 1] - o[i])
            e = k[:, 0, :].copy()
            for w in range(1, W):
                e = e + k[:, w, :]
            e = e / float(W)
            mean = lsum(e) / float(n)
            out["mean"][s] = mean
            d = k - mean                                                      # [n][W][N]
            for j in range(N):
                for q in range(j, N):
                    prod = d[:, :, j] * d[:, :, q]
                    acc = prod[:, 0].copy()
                    for w in range(1, W):
                        acc = acc + prod[:, w]
                    out["cov"][s, j, q] = out["cov"][s, q, j] = lsum(acc) / float(m - 1)
            y = e - mean
            for j in range(N):
                yj = y[:, j]
                c0 = lsum(yj * yj)
                tau, window = 1.0, -1
                if c0 == 0.0 and L >= 1:
                    window = 0
                else:
                    for M in range(0, L + 1):
                        if M:
                            tau = tau + 2.0 * (lsum(yj[:n - M] * yj[M:]) / c0)
                        if float(M) >= c * tau:
                            window = M
                            break
                out["tau"][s, j] = 1.0 if tau < 1.0 else tau
                out["window"][s, j] = window
            if llh is not None:
                f = llh[s, burn:].reshape(m)
                ok = ~np.isnan(f) & (f != -np.inf)
                if ok.any():
                    i = int(np.argmax(np.where(ok, f, -np.inf)))
                    out["best_llh"][s], out["best_x"][s], out["best_at"][s] = f[i], flat[i], (i // W, i % W)
    for k_ in ("mean", "cov", "quant", "tau"):                                 # a NaN result: the canonical quiet NaN
        out[k_][np.isnan(out[k_])] = np.nan
    return {k_: v[0] for k_, v in out.items()} if one else out


def hpd_window(m, mass):
    """The samples in the window of a shortest interval of ``mass`` in (0, 1] over m samples: the smallest integer k with
    ``double(k) >= double(m) mass`` (one rounded product), clamped to 1 ... m."""
    import math
    return min(max(int(math.ceil(float(m) * float(mass))), 1), int(m))


def ensemble_hpd_rule(chain, burn=0, masses=(0.95,), order=False):
    """The rule of the shortest (highest-posterior-density) intervals of ``misti_ens_summary_dev`` (``hpd``, ``hpd_at``, ``order``),
    operation for operation, for ``chain[S][K][W][N]`` (or one search ``[K][W][N]``).  Per search and coordinate, with the ``m = n W``
    kept samples in the order of ``post_order_key`` (``ensemble_posterior_rule``'s ``order``), ``x_(0) <= ... <= x_(m-1)``, and per mass:
      k         ``hpd_window(m, mass)`` samples in the window
      w_i       ``x_(i+k-1) - x_(i)`` for ``i = 0 ... m - k``, one rounded subtraction each
      i*        walking i upward from ``i* = 0``, i replaces i* iff ``w_i < w_i*``, or ``w_i*`` is NaN and ``w_i`` is not: the lowest
                i among the minima, any number before a NaN (``inf - inf``, a NaN sample), all NaN: 0.  On the pairs
                ``(isnan(w), w, i)`` this is a total order - the device reduces it in parallel
      hpd       ``(x_(i*), x_(i*+k-1))``: the samples' own bits, copied - no arithmetic, no canonical NaN; ``hpd_at = i*``
    ``mass = 1`` is (minimum, maximum), ``m = 1`` the sample twice.  The interval is the shortest IN THE SAMPLING COORDINATE: HPD is not
    invariant under the log map, so for a LOG coordinate the image of this interval is an interval of that mass in natural units, not
    the shortest one there.  A search's result depends on its own chain alone.
    Returns dict(hpd[S][N][len(masses)][2], hpd_at[S][N][len(masses)] int32), and with ``order`` the sorted marginals
    ``order[S][N][m]`` - without the leading axis for one search."""
    x = np.asarray(chain, dtype=np.float64)
    one = x.ndim == 3
    if one:
        x = x[None]
    if x.ndim != 4:
        raise ValueError("ensemble_hpd_rule: chain must be [S][K][W][N] or [K][W][N]")
    S, K, W, N = x.shape
    burn = int(burn)
    ms = np.asarray(masses, dtype=np.float64).reshape(-1)
    if not 0 <= burn < K or ms.size > POST_MAX_PROBS or not ((ms > 0) & (ms <= 1)).all() or W < 1 or N < 1:
        raise ValueError("ensemble_hpd_rule: burn must be 0 ... K - 1, at most %d masses in (0, 1]" % POST_MAX_PROBS)
    m = (K - burn) * W
    out = dict(hpd=np.empty((S, N, ms.size, 2)), hpd_at=np.empty((S, N, ms.size), dtype=np.int32), order=np.empty((S, N, m)))
    with np.errstate(all="ignore"):
        for s in range(S):
            flat = x[s, burn:].reshape(m, N)
            for j in range(N):
                v = np.ascontiguousarray(flat[:, j])
                o = v[np.argsort(post_order_key(v), kind="stable")]
                out["order"][s, j] = o
                for q, mass in enumerate(ms):
                    k = hpd_window(m, mass)
                    w = o[k - 1:] - o[:m - k + 1]
                    ok = np.flatnonzero(~np.isnan(w))
                    at = int(ok[np.argmin(w[ok])]) if ok.size else 0        # argmin: the first of the minima
                    out["hpd"][s, j, q] = o[[at, at + k - 1]]                # an indexed copy: the bits, NaN payloads included
                    out["hpd_at"][s, j, q] = at
    if not order:
        del out["order"]
    return {k_: v[0] for k_, v in out.items()} if one else out


def posterior_table(result, n_step, walkers=None, prior=None):
    """What one reads off ``ensemble_posterior`` / ``ensemble_posterior_rule`` per coordinate, with ``n_step`` = n, the kept steps
    behind the summary, and W ``walkers`` (default: those of ``result["last"]``): dict(mean, sd (the square root of the covariance's
    diagonal), quant, tau, n_eff = n W / tau, short: fewer than 50 tau kept steps or no lag closed the window (window == -1), corr: the
    correlation matrix).  With ``prior`` (the call's) also ``coordinate`` (per coordinate "linear" or "log": what ``mean`` and ``sd``
    are in), ``quant_natural`` (``quant`` with the LOG coordinates in natural units) and, where the result has ``best_x``,
    ``best_x_natural``.  Where the result has ``hpd`` (``masses``: the shortest intervals), ``hpd`` too, and with ``prior``
    ``hpd_natural``: its endpoints in natural units - an interval of that mass, but shortest in the SAMPLING coordinate only: HPD is
    not invariant under the log map."""
    n, W = int(n_step), int(np.asarray(result["last"]).shape[-2] if walkers is None else walkers)
    cov = np.asarray(result["cov"], dtype=np.float64)
    tau = np.asarray(result["tau"], dtype=np.float64)
    with np.errstate(all="ignore"):
        sd = np.sqrt(np.diagonal(cov, axis1=-2, axis2=-1))
        corr = cov / (sd[..., :, None] * sd[..., None, :])
        n_eff = float(n * W) / tau
    out = dict(mean=np.asarray(result["mean"]), sd=sd, quant=np.asarray(result["quant"]), tau=tau, n_eff=n_eff,
                short=(n < 50.0 * tau) | (np.asarray(result["window"]) == -1), corr=corr)
    if prior is not None:
        # quantiles and the best sample of a LOG coordinate in natural units as well (monotone: exact up to numpy.exp); mean and sd stay
        # in the sampling coordinate, which `coordinate` names
        log = np.asarray(prior["scale"]) == COORD_LOG
        out.update(coordinate=np.where(log, "log", "linear"), quant_natural=from_sampling(np.swapaxes(out["quant"], -1, -2), prior).swapaxes(-1, -2))
        if "best_x" in result:
            out.update(best_x_natural=from_sampling(result["best_x"], prior))
    if "hpd" in result:
        out.update(hpd=np.asarray(result["hpd"]))
        if prior is not None:                                  # [...][N][masses][2]: the coordinate axis last for from_sampling, and back
            out.update(hpd_natural=np.moveaxis(from_sampling(np.moveaxis(out["hpd"], -3, -1), prior), -1, -3))
    return out


# ---------------------------------------------------------------------------- joint regions of coordinate pairs ----
# The rule of misti_ens_joint_dev stated on the host (include/misti_hip.h, "joint credible regions of coordinate pairs"): a
# two-dimensional histogram per search and pair, its mode, and the count level that encloses a mass.  Behind the bin of a sample
# everything is integer arithmetic: the device result is this, bit for bit.
JOINT_MAX_PAIRS, JOINT_MAX_BINS = 120, 128


def joint_pairs(pairs, bins, N=None):
    """``pairs`` as ``[n_pair][2]`` int32 and ``bins`` (a scalar, ``(Ba, Bb)`` for every pair, or ``[n_pair][2]``) as ``[n_pair][2]``
    int32, checked as the C ABI checks them, with ``offsets[n_pair + 1]``: pair q's ``Ba x Bb`` cells lie at ``offsets[q] ...
    offsets[q + 1]`` of a search's packed counts."""
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2), dtype=np.int32)
    if not 1 <= pr.shape[0] <= JOINT_MAX_PAIRS or (pr[:, 0] == pr[:, 1]).any() or (pr < 0).any() or (N is not None and (pr >= N).any()):
        raise ValueError("joint: 1 ... %d pairs of two distinct coordinates in 0 ... N - 1 (got %s)" % (JOINT_MAX_PAIRS, pr.tolist()))
    try:
        bn = np.ascontiguousarray(np.broadcast_to(np.asarray(bins, dtype=np.int64), pr.shape), dtype=np.int32)
    except ValueError:
        raise ValueError("joint: bins must be a scalar, (Ba, Bb) or [n_pair][2]")
    if (bn < 1).any() or (bn > JOINT_MAX_BINS).any():
        raise ValueError("joint: a bin count must be 1 ... %d" % JOINT_MAX_BINS)
    return pr, bn, np.concatenate([[0], np.cumsum(bn[:, 0].astype(np.int64) * bn[:, 1])])


def joint_bin(x, lo, hi, B):
    """The bin of INSIDE samples ``x`` (``lo <= x <= hi``) on an axis of B bins: ``scale = double(B) / (hi - lo)``, ``t = (x - lo)
    scale``, each operation rounded on its own; 0 where ``!(t >= 0)`` (``hi == lo``: 0 inf is NaN; an infinite ``hi - lo``), ``B - 1``
    where ``t >= double(B)`` (so ``x == hi``), otherwise ``(int)t``."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        scale = np.float64(B) / (np.float64(hi) - np.float64(lo))
        t = (x - np.float64(lo)) * scale
        top = t >= float(B)
        mid = (t >= 0.0) & ~top
    i = np.zeros(x.shape, dtype=np.int64)
    i[mid] = t[mid].astype(np.int64)
    i[top] = B - 1
    return i


def joint_need(inside, mass):
    """The samples a region of ``mass`` must hold: ``hpd_window`` on the samples inside the window."""
    return hpd_window(inside, mass)


def joint_counts(result, q, s=None):
    """Pair q's histogram ``[S][Ba][Bb]`` (``[Ba][Bb]`` for search ``s``, or where the result has no search axis) out of a result's
    packed ``counts``."""
    c = np.asarray(result["counts"])
    Ba, Bb = (int(v) for v in np.asarray(result["bins"])[q])
    c = c[..., int(result["offsets"][q]):int(result["offsets"][q + 1])].reshape(c.shape[:-1] + (Ba, Bb))
    return c if s is None or c.ndim == 2 else c[s]


def ensemble_joint_rule(chain, pairs, bins=32, burn=0, range=None, masses=(0.95,)):
    """The rule of ``misti_ens_joint_dev`` for ``chain[S][K][W][N]`` (or one search ``[K][W][N]``): per search and pair ``(a, b)`` of
    distinct coordinates, on the ``m = n W`` kept samples ``t = burn ... K - 1``, with ``Ba x Bb`` bins (``joint_pairs``):
      range     ``(lo, hi)`` per axis from ``range[S][n_pair][2][2]`` (anything that broadcasts to it), or with None taken from the
                data: the smallest and largest FINITE kept sample of the coordinate in the order of ``post_order_key`` (-0.0 before
                +0.0), bits copied; no finite sample: both the canonical quiet NaN
      inside    a sample is inside the window iff ``lo <= x && x <= hi`` on both axes: a NaN anywhere, or ``lo > hi``, is outside
      bin       ``joint_bin`` per axis; ``counts[ia][ib]`` the inside samples per cell, ``inside`` their sum, ``outside = m - inside``
      mode      the cell with the largest count, ties to the lowest ia, then the lowest ib; (-1, -1) where ``inside == 0``
      region    per mass p in (0, 1]: ``k = joint_need(inside, p)``; ``level`` the LARGEST count c >= 1 such that the cells with count
                >= c hold at least k samples; ``cells`` their number, ``held`` the samples in them; ties at the level are all in the
                region ``{cells: count >= level}``; ``inside == 0``: 0, 0, 0
    The histogram lives in the SAMPLING coordinate: the region of a LOG coordinate is not the image of the region of its natural
    value.  A search's result depends on its own chain and ranges alone.
    Returns dict(counts[S][sum_q Ba Bb] int32 (pairs packed in order, row-major: ``joint_counts``), range[S][n_pair][2][2], inside,
    outside [S][n_pair], mode[S][n_pair][2], level, cells, held [S][n_pair][len(masses)] - all int32 -, and pairs, bins, offsets,
    masses as they were read) - without the search axis for one search."""
    x = np.asarray(chain, dtype=np.float64)
    one = x.ndim == 3
    if one:
        x = x[None]
    if x.ndim != 4:
        raise ValueError("ensemble_joint_rule: chain must be [S][K][W][N] or [K][W][N]")
    S, K, W, N = x.shape
    burn = int(burn)
    ms = np.asarray(masses, dtype=np.float64).reshape(-1)
    if not 0 <= burn < K or ms.size > POST_MAX_PROBS or not ((ms > 0) & (ms <= 1)).all() or W < 1 or N < 1:
        raise ValueError("ensemble_joint_rule: burn must be 0 ... K - 1, at most %d masses in (0, 1]" % POST_MAX_PROBS)
    pr, bn, off = joint_pairs(pairs, bins, N)
    P, m = pr.shape[0], (K - burn) * W
    if range is None:
        rg = np.full((S, P, 2, 2), np.nan)
    else:
        rg = np.array(np.broadcast_to(np.asarray(range, dtype=np.float64), (S, P, 2, 2)))
    out = dict(counts=np.zeros((S, int(off[-1])), dtype=np.int32), range=rg, inside=np.zeros((S, P), dtype=np.int32), outside=np.zeros((S, P), dtype=np.int32),
               mode=np.full((S, P, 2), -1, dtype=np.int32), level=np.zeros((S, P, ms.size), dtype=np.int32), cells=np.zeros((S, P, ms.size), dtype=np.int32),
               held=np.zeros((S, P, ms.size), dtype=np.int32))
    for s in np.arange(S):
        flat = x[s, burn:].reshape(m, N)
        for q in np.arange(P):
            Ba, Bb = int(bn[q, 0]), int(bn[q, 1])
            v = [np.ascontiguousarray(flat[:, pr[q, ax]]) for ax in (0, 1)]
            if range is None:
                for ax in (0, 1):
                    f = v[ax][np.isfinite(v[ax])]
                    if f.size:
                        key = post_order_key(f)
                        rg[s, q, ax] = f[[np.argmin(key), np.argmax(key)]]          # an indexed copy: the bits
            (lo_a, hi_a), (lo_b, hi_b) = rg[s, q]
            with np.errstate(all="ignore"):
                ok = (lo_a <= v[0]) & (v[0] <= hi_a) & (lo_b <= v[1]) & (v[1] <= hi_b)
            cell = joint_bin(v[0][ok], lo_a, hi_a, Ba) * Bb + joint_bin(v[1][ok], lo_b, hi_b, Bb)
            cnt = np.bincount(cell, minlength=Ba * Bb).astype(np.int64)
            inside = int(cnt.sum())
            out["counts"][s, off[q]:off[q + 1]] = cnt
            out["inside"][s, q], out["outside"][s, q] = inside, m - inside
            if not inside:
                continue
            top = int(np.argmax(cnt))                                               # argmax: the first of the maxima, row-major
            out["mode"][s, q] = top // Bb, top % Bb
            levels = np.unique(cnt[cnt > 0])
            holds = np.array([cnt[cnt >= c].sum() for c in levels])
            for i, mass in enumerate(ms):
                level = int(levels[holds >= joint_need(inside, mass)].max())
                out["level"][s, q, i], out["cells"][s, q, i], out["held"][s, q, i] = level, (cnt >= level).sum(), cnt[cnt >= level].sum()
    out = {k_: v[0] for k_, v in out.items()} if one else out
    out.update(pairs=pr, bins=bn, offsets=off, masses=ms)
    return out


def joint_table(result, prior=None):
    """What one reads off a joint result (``ensemble_joint_rule``, ``Engine.ensemble_joint_dev``, ``r["joint"]`` of the samplers; it
    must hold counts, range, inside, mode, and level with masses): per search a list over the pairs of dict(pair, window ((lo, hi) per
    axis), edges (the ``B + 1`` bin edges per axis: ``lo + i (hi - lo) / B``, the last one ``hi``), inside, mode, mode_centre (the
    centre of the mode cell per axis; NaN where no sample is inside), regions: per mass dict(mass, level, cells, held, mask[Ba][Bb]
    (``count >= level``), area (the region's share of the window's cells), extent ((lo, hi) per axis: the edges that enclose the
    region; NaN where it is empty))).  Everything is in SAMPLING units.  With ``prior`` (the call's) each pair also has ``coordinate``
    ("linear" | "log" per axis) and, flagged by ``natural_is_image`` (True where an axis is LOG), ``window_natural``,
    ``edges_natural``, ``mode_centre_natural`` and per region ``extent_natural``: the IMAGE of the sampling-unit values in natural
    units - a region of that mass, but highest-density in the sampling coordinate only.  A result without a search axis gives one such
    list."""
    cnt_all = np.asarray(result["counts"])
    one = cnt_all.ndim == 1
    get = lambda k: np.asarray(result[k])[None] if one else np.asarray(result[k])
    rg, inside, mode = get("range"), get("inside"), get("mode")
    masses = np.asarray(result.get("masses", ()), dtype=np.float64).reshape(-1)
    level = get("level") if "level" in result and masses.size else None
    pairs, bins = np.asarray(result["pairs"]), np.asarray(result["bins"])
    scale = None if prior is None else np.asarray(prior["scale"])
    tables = []
    for s in np.arange(rg.shape[0]):
        rows = []
        for q in np.arange(pairs.shape[0]):
            B = [int(bins[q, 0]), int(bins[q, 1])]
            cnt = joint_counts(result, q, s).astype(np.int64)
            with np.errstate(all="ignore"):
                edges = [np.linspace(rg[s, q, ax, 0], rg[s, q, ax, 1], B[ax] + 1) for ax in (0, 1)]
            centre = [float(0.5 * (edges[ax][mode[s, q, ax]] + edges[ax][mode[s, q, ax] + 1])) if inside[s, q] else np.nan for ax in (0, 1)]
            row = dict(pair=(int(pairs[q, 0]), int(pairs[q, 1])), window=tuple((float(rg[s, q, ax, 0]), float(rg[s, q, ax, 1])) for ax in (0, 1)),
                       edges=edges, inside=int(inside[s, q]), mode=(int(mode[s, q, 0]), int(mode[s, q, 1])), mode_centre=tuple(centre), regions=[])
            for i in np.arange(masses.size if level is not None else 0):
                lv = int(level[s, q, i])
                mask = (cnt >= lv) if lv >= 1 else np.zeros(cnt.shape, dtype=bool)
                extent = []
                for ax in (0, 1):
                    hit = np.flatnonzero(mask.any(axis=1 - ax))
                    extent.append((float(edges[ax][hit[0]]), float(edges[ax][hit[-1] + 1])) if hit.size else (np.nan, np.nan))
                row["regions"].append(dict(mass=float(masses[i]), level=lv, cells=int(mask.sum()), held=int(cnt[mask].sum()), mask=mask,
                                           area=float(mask.sum()) / float(mask.size), extent=tuple(extent)))
            if scale is not None:
                log = [bool((scale[s] if scale.ndim == 2 else scale)[pairs[q, ax]] == COORD_LOG) for ax in (0, 1)]
                with np.errstate(all="ignore"):
                    nat = lambda v, ax: np.exp(v) if log[ax] else v
                    row.update(coordinate=tuple("log" if l else "linear" for l in log), natural_is_image=any(log),
                               window_natural=tuple(tuple(float(nat(np.float64(e), ax)) for e in row["window"][ax]) for ax in (0, 1)),
                               edges_natural=[nat(edges[ax], ax) for ax in (0, 1)],
                               mode_centre_natural=tuple(float(nat(np.float64(centre[ax]), ax)) for ax in (0, 1)))
                    for reg in row["regions"]:
                        reg["extent_natural"] = tuple(tuple(float(nat(np.float64(e), ax)) for e in reg["extent"][ax]) for ax in (0, 1))
            rows.append(row)
        tables.append(rows)
    return tables[0] if one else tables


# ------------------------------------------------------------------ trajectory bands of the corrected rates ----
# The rule of misti_traj_bands_dev / misti_traj_bands stated on the host (include/misti_hip.h, "trajectory bands"): per group, interval
# of the common grid and population the members among m samples of lc, their count, quantiles, mean and extremes.  The device result is
# this, bit for bit.
def bands_rank(n, p):
    """The order statistics behind the quantile of probability ``p`` among ``n >= 1`` members: ``h = double(n - 1) p``, ``i =
    floor(h)``, ``g = h - i``; ``g == 0`` or ``i >= n - 1``: ``x_(min(i, n - 1))`` exactly, otherwise ``x_(i) + g (x_(i+1) - x_(i))``.
    Returns ``(lo, hi, g)`` with ``lo == hi`` where the quantile is a sample (``misti_bands_rank``)."""
    h = float(n - 1) * float(p)
    fl = float(np.floor(h))
    i, g = int(fl), h - fl
    if g == 0.0 or i >= n - 1:
        i = min(i, n - 1)
        return i, i, g
    return i, i + 1, g


def trajectory_bands_rule(lc, split, status=None, probs=(0.025, 0.5, 0.975), order=False):
    """The rule of ``misti_traj_bands_dev``, operation for operation, for ``lc[G][m][numT+1][2]`` (the corrected coalescence rates of
    ``evaluate(want_lc=True)``), ``split[G][m]`` and ``status[G][m]`` (int, or None: every sample is OK) - or one group without the
    leading axis.  All results are on the COMMON grid ``j = 0 ... numT - 1``: a sample's own grid gains an interval at ``floor(split)``
    when its split is fractional, but for every ``j`` with ``double(j) < split`` its own row ``j`` is common interval ``j`` and above
    that the populations have merged, so nothing is regridded and row ``numT`` is never read.  Per series ``(g, j, pop)``:
      member    sample i iff ``status == 0``, ``double(j) < split[g][i]`` (a NaN split is a member of nothing) and
                ``lc[g][i][j][pop]`` is not NaN
      count     the members, n: ``count / m`` is the share of samples whose populations are still separate at interval j
      sorted    the members by ``post_order_key``: -0.0 before +0.0, +-inf ordinary members
      quant     ``bands_rank(n, p)``: ``x_(lo)``, or ``x_(lo) + g (x_(hi) - x_(lo))`` - ``ensemble_posterior_rule``'s expression with
                the series' own n
      mean      ``lsum(sorted members) / double(n)``
      lo, hi    ``x_(0)``, ``x_(n-1)``: bits copied
    ``n == 0``: count 0 and the canonical quiet NaN everywhere else; a NaN in quant or mean is the canonical one.  The results are
    RATES, not sizes ``1 / lc``: an order statistic maps through ``1 / x`` exactly (the order reversed), an interpolated quantile and
    the mean do not.
    Returns dict(count[G][numT][2] int32, mean, lo, hi [G][numT][2], quant[G][numT][2][P]) and with ``order`` also
    ``sorted[G][numT][2][m]`` (the members first, NaN behind them) - without the leading axis for one group."""
    x = np.asarray(lc, dtype=np.float64)
    one = x.ndim == 3
    if one:
        x = x[None]
    if x.ndim != 4 or x.shape[2] < 2 or x.shape[3] != 2 or x.shape[1] < 1:
        raise ValueError("trajectory_bands_rule: lc must be [G][m][numT + 1][2] or [m][numT + 1][2], m >= 1")
    G, m, T1, _ = x.shape
    numT = T1 - 1
    st = np.asarray(split, dtype=np.float64).reshape(G, m)
    ok = np.ones((G, m), dtype=bool) if status is None else np.asarray(status).reshape(G, m) == 0
    pr = np.asarray(probs, dtype=np.float64).reshape(-1)
    P = pr.size
    if not 1 <= P <= POST_MAX_PROBS or not ((pr >= 0) & (pr <= 1)).all():
        raise ValueError("trajectory_bands_rule: 1 ... %d probabilities in [0, 1]" % POST_MAX_PROBS)
    out = dict(count=np.zeros((G, numT, 2), dtype=np.int32), mean=np.full((G, numT, 2), np.nan), lo=np.full((G, numT, 2), np.nan),
               hi=np.full((G, numT, 2), np.nan), quant=np.full((G, numT, 2, P), np.nan), sorted=np.full((G, numT, 2, m), np.nan))
    with np.errstate(all="ignore"):
        for g in range(G):
            for j in range(numT):
                below = ok[g] & (float(j) < st[g])                          # a NaN split compares false
                for pop in range(2):
                    v = np.ascontiguousarray(x[g, :, j, pop])
                    v = v[below & ~np.isnan(v)]
                    n = v.size
                    out["count"][g, j, pop] = n
                    if n == 0:
                        continue
                    o = v[np.argsort(post_order_key(v), kind="stable")]
                    out["sorted"][g, j, pop, :n] = o
                    out["lo"][g, j, pop], out["hi"][g, j, pop] = o[0], o[n - 1]
                    out["mean"][g, j, pop] = lsum(o) / float(n)
                    for p in range(P):
                        a, b, w = bands_rank(n, pr[p])
                        out["quant"][g, j, pop, p] = o[a] if a == b else o[a] + w * (o[b] - o[a])
    for k_ in ("mean", "quant"):                                               # a NaN result: the canonical quiet NaN
        out[k_][np.isnan(out[k_])] = np.nan
    if not order:
        del out["sorted"]
    return {k_: v[0] for k_, v in out.items()} if one else out


def trajectory_bands_table(result, times):
    """What one prints and saves of ``trajectory_bands`` / ``trajectory_bands_rule`` for ONE group (``count[numT][2]`` ...; give
    ``{k: v[g] ...}`` for group g of several): a row per interval of the common grid that has a member in either population, as
    dict(interval, time (the interval's lower edge: 0, then ``times`` - edges, the running sum of a grid given as lengths), count[2], lo[2], quant[2][P], mean[2], hi[2]) - RATES, as the
    rule says; ``1 / lo`` and ``1 / hi`` are the extremes of the size, the other way round."""
    count = np.asarray(result["count"])
    if count.ndim != 2:
        raise ValueError("trajectory_bands_table: one group at a time (count[numT][2])")
    edges = np.concatenate([[0.0], np.asarray(times, dtype=np.float64).reshape(-1)])
    rows = []
    for j in range(count.shape[0]):
        if count[j].any():
            rows.append(dict(interval=j, time=float(edges[j]) if j < edges.size else float("nan"), count=count[j].copy(),
                             **{k: np.asarray(result[k])[j].copy() for k in ("lo", "quant", "mean", "hi") if k in result}))
    return rows


# ------------------------------------------------------------------------------- priors and log-scale coordinates ----
# What a prior adds to the rules above and below (include/misti_hip.h, "priors and log-scale coordinates"; misti_prior.h): per
# coordinate a SAMPLING COORDINATE (the engine's value or its logarithm) and a prior density on it.  Stated here once; the device result
# is ensemble_prior_rule / tempered_prior_rule, bit for bit.
COORD_LINEAR, COORD_LOG = 0, 1
PRIOR_FLAT, PRIOR_NORMAL, PRIOR_EXPONENTIAL = 0, 1, 2


def prior_spec(N, log=(), normal=None, exponential=None):
    """The four arrays of a prior over N coordinates: dict(scale[N], kind[N] int32, p0[N], p1[N]).  ``log``: the coordinates sampled on
    the log scale; ``normal``: ``{k: (mean, sd)}``; ``exponential``: ``{k: scale}`` - both on the SAMPLING coordinate, so a normal on a
    log coordinate is a log-normal and a coordinate named in neither is flat (on a log coordinate: log-uniform).  Host only."""
    N = int(N)
    normal, exponential = dict(normal or {}), dict(exponential or {})
    names = list(log) + list(normal) + list(exponential)
    if any(not 0 <= int(k) < N for k in names) or set(normal) & set(exponential):
        raise ValueError("prior_spec: a coordinate is outside 0 ... %d, or has two priors" % (N - 1))
    out = dict(scale=np.zeros(N, dtype=np.int32), kind=np.zeros(N, dtype=np.int32), p0=np.zeros(N), p1=np.zeros(N))
    for k in log:
        out["scale"][int(k)] = COORD_LOG
    for k, (mean, sd) in normal.items():
        out["kind"][int(k)], out["p0"][int(k)], out["p1"][int(k)] = PRIOR_NORMAL, float(mean), float(sd)
    for k, scale in exponential.items():
        out["kind"][int(k)], out["p0"][int(k)] = PRIOR_EXPONENTIAL, float(scale)
    return out


def _prior_arrays(prior, S, N, lo, hi, who):
    """``prior`` (None, or dict(scale, kind, p0, p1), each ``[N]`` or ``[S][N]``) against the boxes ``lo`` / ``hi`` ``[S][N]``: the four
    arrays as ``[S][N]``, or None for a prior that says nothing (None, or every coordinate LINEAR and FLAT): such a call takes the path
    without one.  Raises what the library refuses."""
    if prior is None:
        return None
    try:
        scale, kind = (np.ascontiguousarray(np.broadcast_to(np.asarray(prior[k]), (S, N)), dtype=np.int32) for k in ("scale", "kind"))
        p0, p1 = (np.ascontiguousarray(np.broadcast_to(np.asarray(prior[k], dtype=np.float64), (S, N))) for k in ("p0", "p1"))
    except (KeyError, TypeError, ValueError):
        raise ValueError("%s: a prior is dict(scale, kind, p0, p1), each [N] or [S][N]" % who)
    if not (np.isin(scale, (COORD_LINEAR, COORD_LOG)).all() and np.isin(kind, (PRIOR_FLAT, PRIOR_NORMAL, PRIOR_EXPONENTIAL)).all()):
        raise ValueError("%s: an unknown scale or kind" % who)
    nrm, exn, log = kind == PRIOR_NORMAL, kind == PRIOR_EXPONENTIAL, scale == COORD_LOG
    if not ((np.isfinite(p1) & (p1 > 0))[nrm].all() and (np.isfinite(p0) & (p0 > 0))[exn].all()):
        raise ValueError("%s: a normal's sd or an exponential's scale is not finite and positive" % who)
    if not np.isfinite(p0[nrm]).all():
        raise ValueError("%s: a normal's mean is not finite" % who)
    if ((hi > 709.0) | (lo < -745.0))[log].any():
        raise ValueError("%s: the box of a log-scale coordinate leaves [-745, 709]" % who)
    if not (log.any() or nrm.any() or exn.any()):
        return None
    return dict(scale=scale, kind=kind, p0=p0, p1=p1)


def ens_natural(scale, y):
    """The point the engine is handed, elementwise: ``y`` where ``scale`` is LINEAR, ``ens_exp(y)`` where it is LOG."""
    y = np.asarray(y, dtype=np.float64)
    return np.where(np.asarray(scale) == COORD_LOG, ens_exp(y), y)


def ens_log_prior(kind, p0, p1, lo, hi, y):
    """The log prior of walkers ``y[...][N]`` (``misti_ens_log_prior``; the arguments broadcast against ``y``): the sum, in increasing k
    from +0.0, over the coordinates that are neither fixed (``lo == hi``) nor FLAT, of one term each - NORMAL(mean ``p0``, sd ``p1``):
    ``u = (y - p0) / p1``, ``-0.5 (u u)``; EXPONENTIAL(scale ``p0``): ``-((y - lo) / p0)`` - every operation rounded on its own.
    Unnormalised.  Entries of ``p0`` / ``p1`` that the kind does not read are not looked at."""
    y = np.asarray(y, dtype=np.float64)
    kind, p0, p1, lo, hi = (np.broadcast_to(np.asarray(v), y.shape) for v in (kind, p0, p1, lo, hi))
    lp = np.zeros(y.shape[:-1])
    with np.errstate(all="ignore"):
        for k in range(y.shape[-1]):
            u = (y[..., k] - p0[..., k]) / p1[..., k]
            term = np.where(kind[..., k] == PRIOR_NORMAL, -0.5 * (u * u), -((y[..., k] - lo[..., k]) / p0[..., k]))
            lp = np.where((lo[..., k] != hi[..., k]) & (kind[..., k] != PRIOR_FLAT), lp + term, lp)
    return lp


def ens_decision_prior(z, d, llk_old, llk_new, T, lp_old, lp_new, u_acc):
    """``ens_decision`` with a prior (``misti_ens_accept_prior``): the same, with ``e = (llk_new - llk_old) / T + (lp_new - lp_old)`` -
    the prior is not tempered."""
    z, old, new, T, lo_, ln_, u = (np.asarray(v, dtype=np.float64) for v in (z, llk_old, llk_new, T, lp_old, lp_new, u_acc))
    d = np.asarray(d, dtype=np.int64)
    shape = np.broadcast(z, d, old, new, T, lo_, ln_, u).shape
    z, d, old, new, T, lo_, ln_, u = (np.broadcast_to(v, shape) for v in (z, d, old, new, T, lo_, ln_, u))
    g = np.ones(shape)
    with np.errstate(all="ignore"):
        for k in range(int(d.max()) if d.size else 0):
            g = np.where(k < d, g * z, g)
        p = g * ens_exp((new - old) / T + (ln_ - lo_))
        take = u < p
    return np.isfinite(new) & (~np.isfinite(old) | take)


def ensemble_prior_rule(fun_batch, init, lo, hi, n_step, prior, thin=1, temperature=1.0, a=2.0, seed=0, ids=None):
    """The rule of ``misti_ensemble_sample_prior``, operation for operation: ``ensemble_rule`` with a sampling coordinate and a prior per
    coordinate.  ``prior``: None, or dict(scale, kind, p0, p1) (``prior_spec``), each ``[N]`` (one for all searches) or ``[S][N]``.

    Everything the caller sees is in the sampling coordinate y: ``init``, the box ``[lo, hi]`` (finite), the stretch, the test against
    the box, ``chain`` and ``last``.  Only the point handed to ``fun_batch`` changes: its coordinate k is ``y_k`` (LINEAR) or
    ``ens_exp(y_k)`` (LOG) - ``ens_natural`` -, the initial ensemble's and a fitted split's alike; a fixed coordinate is ``lo``, or
    ``ens_exp(lo)``, exactly.  The decision on an evaluated proposal is ``ens_decision_prior`` with ``lp = ens_log_prior`` of the old
    walker and of the proposal: ``e = (llk_new - llk_old) / T + (lp_new - lp_old)``.  The prior is NOT tempered.  The draws, the blocks,
    the halves, the rejection in advance and the counters are ``ensemble_rule``'s.
    A prior that says nothing (None, or every coordinate LINEAR and FLAT) IS ``ensemble_rule``: the existing lines, not the new formula
    with a zero added.  Returns what ``ensemble_rule`` returns."""
    return _one_rung("ensemble_prior_rule", fun_batch, init, lo, hi, n_step, prior, thin, temperature, a, seed, ids)


def to_sampling(x, prior, box=None):
    """Natural values ``x[...][N]`` as sampling coordinates: ``numpy.log`` of the LOG coordinates.  ``box`` (``(lo, hi)`` in sampling
    coordinates): the result is clipped into it - a bound whose logarithm lands one ulp outside stays a point of the box.  Host only;
    never part of a rule's bits."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        y = np.where(np.asarray(prior["scale"]) == COORD_LOG, np.log(x), x)
    return y if box is None else np.clip(y, np.asarray(box[0], dtype=np.float64), np.asarray(box[1], dtype=np.float64))


def from_sampling(y, prior):
    """Sampling coordinates ``y[...][N]`` in natural units: ``numpy.exp`` of the LOG coordinates.  Host only, for reports."""
    y = np.asarray(y, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(np.asarray(prior["scale"]) == COORD_LOG, np.exp(y), y)


# ------------------------------------------------------------------------------------------- tempered ensemble MCMC ----
# The rule of misti_tempered_sample stated on the host (include/misti_hip.h, "tempered ensemble MCMC"): the device result is this, bit
# for bit, on the engine's own objective.  Replica exchange over the ensemble sampler: a ladder of ensembles per fit, neighbouring rungs
# trading walkers, the cold rung carrying the posterior.
PT_MAX_RUNGS = 64


def temperature_ladder(T0, Tmax_ratio, L):
    """A geometric ladder of L temperatures from ``T0`` to ``T0 Tmax_ratio``: ``T_l = T0 ratio^(l / (L - 1))``, and ``T0`` alone for
    L = 1 (the ratio is not looked at).  Host only."""
    T0, ratio, L = float(T0), float(Tmax_ratio), int(L)
    if not 1 <= L <= PT_MAX_RUNGS or not (np.isfinite(T0) and T0 > 0):
        raise ValueError("temperature_ladder: 1 ... %d rungs, T0 finite and positive" % PT_MAX_RUNGS)
    if L == 1:
        return np.array([T0])
    if not (np.isfinite(ratio) and ratio > 1.0):
        raise ValueError("temperature_ladder: the ratio must be finite and > 1")
    return T0 * ratio ** (np.arange(L) / float(L - 1))


def pt_swap_decision(T_lo, T_hi, llk_lo, llk_hi, u):
    """The decision on a pair of walkers of neighbouring rungs (``misti_pt_swap``), elementwise: no swap where either walker has no
    value (not finite); otherwise ``db = 1.0 / T_lo - 1.0 / T_hi``, ``e = db (llk_hi - llk_lo)``, swapped iff ``u < ens_exp(e)`` -
    every operation rounded on its own."""
    T_lo, T_hi, lo, hi, u = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (T_lo, T_hi, llk_lo, llk_hi, u)))
    with np.errstate(all="ignore"):
        db = 1.0 / T_lo - 1.0 / T_hi
        take = u < ens_exp(db * (hi - lo))
    return np.isfinite(lo) & np.isfinite(hi) & take


def tempered_reduction(chain_llh, ladder, burn=0):
    """The thermodynamic-integration part of ``tempered_rule`` on ``chain_llh[S][L][K][W]`` (or one fit ``[L][K][W]``) with ``ladder``
    ``[L]`` or ``[S][L]``: over the kept steps ``burn ... K - 1`` (n of them) ``e_t = (llh[t][0] + ... + llh[t][W - 1] in walker order)
    / W``, ``rung_llh[l] = lsum(e) / n``; ``beta_l = 1.0 / T_l``; ``logz`` the sum for l = 0 ... L - 2 in increasing l, from +0.0, of
    ``(0.5 (E_l + E_{l+1})) (beta_l - beta_{l+1})``, every operation rounded on its own (L = 1: +0.0).  K = 0 leaves no step: every
    ``rung_llh`` is NaN.  A NaN is the canonical quiet NaN.  Returns (rung_llh, logz)."""
    v = np.asarray(chain_llh, dtype=np.float64)
    one = v.ndim == 3
    if one:
        v = v[None]
    S, L, K, W = v.shape
    T = np.ascontiguousarray(np.broadcast_to(np.asarray(ladder, dtype=np.float64), (S, L)))
    burn = int(burn)
    if K and not 0 <= burn < K:
        raise ValueError("tempered_reduction: burn must be 0 ... K - 1 (K = %d)" % K)
    n = K - burn
    with np.errstate(all="ignore"):
        if K:
            k = np.moveaxis(v[:, :, burn:], 2, 0)                            # [n][S][L][W]
            e = k[..., 0].copy()
            for w in range(1, W):
                e = e + k[..., w]
            E = lsum(e / float(W)) / float(n)
        else:
            E = np.full((S, L), np.nan)
        beta = 1.0 / T
        logz = np.zeros(S)
        for l in range(L - 1):
            logz = logz + (0.5 * (E[:, l] + E[:, l + 1])) * (beta[:, l] - beta[:, l + 1])
    E = E.copy()
    E[np.isnan(E)] = np.nan
    logz[np.isnan(logz)] = np.nan
    return (E[0], float(logz[0])) if one else (E, logz)


def tempered_rule(fun_batch, init, lo, hi, ladder, n_step, thin=1, swap_every=1, burn=0, a=2.0, seed=0, ids=None):
    """The rule of ``misti_tempered_sample``, operation for operation: parallel tempering (replica exchange) over ``ensemble_rule``.
    Fit s has L rungs (1 ... ``PT_MAX_RUNGS``) at the temperatures ``ladder[s][0] < ladder[s][1] < ...`` (finite, positive; ``ladder``
    is ``[L]`` or ``[S][L]``); rung l is an ensemble of W walkers ``init[s][l][W][N]`` inside the fit's box whose target is
    ``llk / T_l``.  ``fun_batch``, ``lo`` / ``hi``, ``a``, ``seed`` and ``ids`` as in ``ensemble_rule`` (``s`` handed to ``fun_batch``
    is the FIT).

    A rung moves exactly as a search of ``ensemble_rule`` moves - the halves, the stretch, rejection in advance outside the box,
    ``ens_decision`` with ``d = N_free - 1`` and ``T = T_l`` - except that walker i of rung l of step t owns block ``(t L + l) W + i``
    of ``Philox(key=[seed, ids[s]])``: with L = 1 this IS ``ensemble_rule``.  The initial evaluation of all rungs of all fits is ONE
    batch, and so is a half-step of all rungs of all fits.

    Swaps: behind half 1 of step t with ``swap_every >= 1`` and ``t % swap_every == 0``, round ``n = t / swap_every`` treats the pairs
    (l, l + 1) for l = p, p + 2, ... < L - 1 with ``p = (n - 1) & 1``.  Walker i of rung l faces walker i of rung l + 1; its uniform
    is the fourth word of the lower rung's own block ``(t L + l) W + i``, ``(w[3] >> 11) 2^-53``.  ``pt_swap_decision`` decides; the
    walkers trade coordinates and values.  A pair in which either walker has no value is neither proposed nor counted.
    ``swap_every = 0``: no swaps.

    Kept: step t with ``t % thin == 0`` leaves row ``t / thin - 1`` (K = n_step // thin rows), the state AFTER the step's swap round:
    the coordinates of the cold rung only, the values of every rung.  ``rung_llh`` and ``logz`` are ``tempered_reduction`` of
    ``chain_llh`` over the kept steps ``burn ... K - 1``: ``logz[s]`` is the thermodynamic-integration estimate, by the trapezoid rule
    on the ladder's own points, of ``log Z(beta_0) - log Z(beta_{L-1})`` with ``Z(beta) = integral of exp(beta llk)`` against the
    NORMALISED uniform prior on the box.  The piece below ``beta_{L-1}`` (down to the prior, beta = 0) is NOT included.
    Returns dict(chain[S][K][W][N], chain_llh[S][L][K][W], accepted[S][L][W] int32 (stretch moves), swap_proposed[S][L-1] and
    swap_accepted[S][L-1] int32, last[S][L][W][N], last_llh[S][L][W], rung_llh[S][L], logz[S], n_points: the PROPOSALS handed to
    ``fun_batch``).

    The lines are ``_sampler_steps``'s; the reduction is ``tempered_reduction``."""
    return _tempered("tempered_rule", fun_batch, init, lo, hi, ladder, n_step, None, thin, swap_every, burn, a, seed, ids)


def _tempered(who, fun_batch, init, lo, hi, ladder, n_step, prior, thin, swap_every, burn, a, seed, ids):
    """``tempered_rule`` / ``tempered_prior_rule``: ``_sampler_steps`` and the reduction of the values it kept."""
    r = _sampler_steps(who, fun_batch, init, lo, hi, ladder, n_step, prior, thin, swap_every, burn, a, seed, ids,
                       "a ladder must be finite, positive and strictly increasing")
    T, n_points = r.pop("T"), r.pop("n_points")
    rung_llh, logz = tempered_reduction(r["chain_llh"], T, burn) if len(T) else (np.empty((0, T.shape[1])), np.empty(0))
    return dict(r, rung_llh=rung_llh, logz=logz, n_points=n_points)


def _sampler_steps(who, fun_batch, init, lo, hi, ladder, n_step, prior, thin, swap_every, burn, a, seed, ids, ladder_says):
    """The one stepping loop behind the four sampler rules, as ``tempered_rule`` states it: the arguments checked (``who`` and
    ``ladder_says`` word the refusals), the S L rungs moved as S L searches - the temperature and the block are the rung's, everything
    else the fit's -, the swap rounds, the kept rows.  ``prior`` (None: without one; a prior that says nothing takes the lines without
    one): the point handed to ``fun_batch`` and the ``e`` of a rung's decision change (``ensemble_prior_rule``), the swaps do not.
    Returns dict(chain, chain_llh, accepted, swap_proposed, swap_accepted, last, last_llh, T[S][L], n_points)."""
    x = np.array(init, dtype=np.float64)
    if x.ndim != 4:
        raise ValueError(who + ": init must be [S][L][W][N]")
    S, L, W, N = x.shape
    H = W // 2
    n_step, thin, swap_every, burn, a = int(n_step), int(thin), int(swap_every), int(burn), float(a)
    if not 1 <= L <= PT_MAX_RUNGS:
        raise ValueError(who + ": 1 ... %d rungs" % PT_MAX_RUNGS)
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=float), (S, N)))
    hi = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, dtype=float), (S, N)))
    T = np.ascontiguousarray(np.broadcast_to(np.asarray(ladder, dtype=float), (S, L)))
    if not 4 <= W <= ENS_MAX_WALKERS or W % 2 or n_step < 0 or thin < 1 or not (np.isfinite(a) and a > 1.0):
        raise ValueError(who + ": W must be even, 4 ... %d, n_step >= 0, thin >= 1, a finite and > 1" % ENS_MAX_WALKERS)
    if not (np.isfinite(T) & (T > 0)).all() or not (T[:, 1:] > T[:, :-1]).all():
        raise ValueError(who + ": " + ladder_says)
    K = n_step // thin
    if swap_every < 0 or (K and not 0 <= burn < K):
        raise ValueError(who + ": swap_every >= 0, burn 0 ... K - 1")
    with np.errstate(over="ignore", invalid="ignore"):
        usable = np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all() and np.isfinite(hi - lo).all()
    if not usable:
        raise ValueError(who + ": the box must be finite with lo <= hi")
    fixed = lo == hi
    if S and fixed.all(axis=1).any():
        raise ValueError(who + ": every coordinate of a box is fixed")
    if not (np.isfinite(x).all() and (x >= lo[:, None, None, :]).all() and (x <= hi[:, None, None, :]).all()):
        raise ValueError(who + ": every walker of init must be finite and inside its box")
    ids = np.arange(S) if ids is None else np.asarray(ids).reshape(S)
    am1 = a - 1.0
    # the S L rungs as searches: everything but the temperature and the block is the fit's
    G = S * L
    x = x.reshape(G, W, N)
    fit = np.repeat(np.arange(S), L)
    glo, ghi, gfixed, gT = lo[fit], hi[fit], fixed[fit], T.reshape(G)
    d = (~gfixed).sum(axis=1) - 1
    pr = _prior_arrays(prior, S, N, lo, hi, who)
    gpr = None if pr is None else {k: v[fit][:, None] for k, v in pr.items()}                 # [G][1][N]

    def values(X, s_of):
        if pr is not None:
            X = ens_natural(pr["scale"][s_of], X)
        f = np.asarray(fun_batch(X, s_of), dtype=float).reshape(-1)
        llk = -np.where(np.isnan(f), np.inf, f)
        return np.where(np.isfinite(llk), llk, -np.inf)

    llh = values(x.reshape(-1, N).copy(), np.repeat(fit, W)).reshape(G, W) if G else np.empty((0, W))
    n_points = 0
    chain, chain_llh = np.empty((S, K, W, N)), np.empty((S, L, K, W))
    accepted = np.zeros((G, W), dtype=np.int32)
    proposed, swapped = np.zeros((S, max(L - 1, 0)), dtype=np.int32), np.zeros((S, max(L - 1, 0)), dtype=np.int32)
    CHUNK = max(512 // L, 1)
    raw = None
    gidx, fidx = np.arange(G)[:, None], fit[:, None]
    for t in range(1, n_step + 1):
        if (t - 1) % CHUNK == 0:                                          # steps t ...: blocks t L W ... of every fit's stream
            n = min(CHUNK, n_step - t + 1)
            raw = (np.stack([_ens_raw(seed, ids[s], t * L, n * L, W).reshape(n, L, W, 4) for s in range(S)]) if S
                   else np.empty((0, 1, L, W, 4), dtype=np.uint64))
        w = raw[:, (t - 1) % CHUNK].reshape(G, W, 4)
        for half in (0, 1):
            mine = slice(half * H, half * H + H)
            j = (1 - half) * H + _mulhi_index(w[:, mine, 0], H)            # [G][H]
            u_z, u_acc = _ens_uniform(w[:, mine, 1]), _ens_uniform(w[:, mine, 2])
            sz = am1 * u_z + 1.0
            z = (sz * sz) / a
            xi, xj = x[:, mine], x[gidx, j]
            with np.errstate(all="ignore"):
                y = xj + z[:, :, None] * (xi - xj)
            y = np.where(gfixed[:, None, :], glo[:, None, :], y)
            inside = ((y >= glo[:, None, :]) & (y <= ghi[:, None, :])).all(axis=2)
            new = np.full((G, H), -np.inf)
            if inside.any():
                new[inside] = values(y[inside], np.broadcast_to(fidx, (G, H))[inside])
                n_points += int(inside.sum())
            if pr is None:
                take = inside & ens_decision(z, d[:, None], llh[:, mine], new, gT[:, None], u_acc)
            else:
                lp_old, lp_new = (ens_log_prior(gpr["kind"], gpr["p0"], gpr["p1"], glo[:, None], ghi[:, None], v) for v in (xi, y))
                take = inside & ens_decision_prior(z, d[:, None], llh[:, mine], new, gT[:, None], lp_old, lp_new, u_acc)
            x[:, mine] = np.where(take[:, :, None], y, xi)
            llh[:, mine] = np.where(take, new, llh[:, mine])
            accepted[:, mine] += take
        if swap_every >= 1 and t % swap_every == 0:
            xs, ls, us = x.reshape(S, L, W, N), llh.reshape(S, L, W), _ens_uniform(w[:, :, 3]).reshape(S, L, W)
            for l in range((t // swap_every - 1) & 1, L - 1, 2):
                both = np.isfinite(ls[:, l]) & np.isfinite(ls[:, l + 1])
                take = pt_swap_decision(T[:, l, None], T[:, l + 1, None], ls[:, l], ls[:, l + 1], us[:, l])     # [S][W]
                proposed[:, l] += both.sum(axis=1).astype(np.int32)
                swapped[:, l] += take.sum(axis=1).astype(np.int32)
                a_, b_ = xs[:, l].copy(), ls[:, l].copy()
                xs[:, l] = np.where(take[:, :, None], xs[:, l + 1], a_)
                xs[:, l + 1] = np.where(take[:, :, None], a_, xs[:, l + 1])
                ls[:, l] = np.where(take, ls[:, l + 1], b_)
                ls[:, l + 1] = np.where(take, b_, ls[:, l + 1])
        if t % thin == 0:
            chain[:, t // thin - 1] = x.reshape(S, L, W, N)[:, 0]
            chain_llh[:, :, t // thin - 1] = llh.reshape(S, L, W)
    return dict(chain=chain, chain_llh=chain_llh, accepted=accepted.reshape(S, L, W), swap_proposed=proposed, swap_accepted=swapped,
                last=x.reshape(S, L, W, N), last_llh=llh.reshape(S, L, W), T=T, n_points=int(n_points))


def tempered_prior_rule(fun_batch, init, lo, hi, ladder, n_step, prior, thin=1, swap_every=1, burn=0, a=2.0, seed=0, ids=None):
    """The rule of ``misti_tempered_sample_prior``, operation for operation: ``tempered_rule`` whose rungs move as the searches of
    ``ensemble_prior_rule`` move (``prior`` per fit: ``[N]`` or ``[S][N]``).  Rung l targets ``prior(y) exp(llk / T_l)`` - the prior is
    not tempered -, so it cancels in a swap: ``pt_swap_decision`` decides as before.  ``logz`` is the same trapezoid rule, now for
    ``Z(beta)`` = the integral of ``exp(beta llk)`` against the NORMALISED prior on the box, in sampling coordinates.  One rung is
    ``ensemble_prior_rule``; a prior that says nothing is ``tempered_rule``.  Returns what ``tempered_rule`` returns."""
    return _tempered("tempered_prior_rule", fun_batch, init, lo, hi, ladder, n_step, prior, thin, swap_every, burn, a, seed, ids)


def _mcmc_call(engine, summary, n_step, thin, ladder=None, swap_every=1, prior=None):
    """``Engine.ensemble_sample``, or with ``summary`` (a dict of ``burn``, ``probs``, ``max_lag``, ``keep_chain``, ``c``; ``burn``
    defaults to half the kept steps) ``Engine.ensemble_posterior``.  With ``ladder`` (``[L]`` or per ensemble ``[S][L]``):
    ``Engine.tempered_sample`` on it - every rung starts from the ensemble's ``init``, ``temperature`` is not looked at (the ladder's
    first entry is the cold rung's), ``rung_llh`` / ``logz`` drop the summary's ``burn`` (without a summary: half the kept steps).
    ``prior`` (``prior_spec``; None: none) is passed on."""
    half = (int(n_step) // int(thin)) // 2
    extra = {} if prior is None else dict(prior=prior)                  # without one the existing calls, argument for argument
    if ladder is not None:
        L = np.asarray(ladder).shape[-1]
        opts = None if summary is None else dict(summary)

        def tempered(x0, *a, temperature=None, **kw):
            x0 = np.asarray(x0, dtype=float)
            return engine.tempered_sample(np.ascontiguousarray(np.broadcast_to(x0[:, None], (x0.shape[0], L) + x0.shape[1:])), *a, ladder=ladder,
                                          swap_every=swap_every, burn=half if opts is None else opts.setdefault("burn", half), post=opts, **extra, **kw)
        return tempered
    if summary is None:
        return lambda *a, **kw: engine.ensemble_sample(*a, **kw, **extra)
    opts = dict(summary)
    opts.setdefault("burn", half)
    return lambda *a, **kw: engine.ensemble_posterior(*a, **kw, **opts, **extra)


def bootstrap_profile_mcmc(engine, split_values, jsfs_rows, init, box, n_step=100, thin=1, temperature=1.0, a=2.0, seed=0, summary=None,
                           ladder=None, swap_every=1, prior=None):
    """``bootstrap_profile_de``'s sampler: per (row, split) pair ONE ensemble inside ``box`` (``(lo, hi)``, each ``[n_param]``, finite), all
    R x P ensembles in ONE ``misti_ensemble_sample`` call - every half-step one dense engine batch.  ``init`` is ``[W][n_param]`` (every
    pair starts from it) or ``[R][P][W][n_param]``.  The stream id of an ensemble is its split's index: the rows of a bootstrap share
    their random numbers, and a row's result does not depend on the other rows.
    ``summary``: None, or a dict of ``Engine.ensemble_posterior``'s options (``burn`` - default half the kept steps -, ``probs``,
    ``max_lag``, ``keep_chain``, ``c``): the call goes through ``misti_ensemble_posterior`` and the chain stays on the device.
    ``ladder`` (``[L]`` temperatures, strictly increasing, in place of ``temperature``) with ``swap_every``: every pair is a tempered
    ladder of L ensembles started from ``init`` and the call goes through ``misti_tempered_sample`` (``Engine.tempered_sample``).
    ``prior`` (``prior_spec``, one for all pairs): sampling coordinates and priors per coordinate - ``init``, ``box`` and the result
    are then in sampling coordinates (``to_sampling`` / ``from_sampling``).
    Returns what ``Engine.ensemble_sample`` (``Engine.ensemble_posterior``, ``Engine.tempered_sample``) returns with the leading axis
    reshaped to ``[R][P]``."""
    rows = np.asarray(jsfs_rows, dtype=float).reshape(-1, 8)
    splits = np.asarray(split_values, dtype=float).reshape(-1)
    R, Q = rows.shape[0], splits.size
    r_of, j_of = (v.ravel() for v in np.meshgrid(np.arange(R), np.arange(Q), indexing="ij"))
    x0 = np.asarray(init, dtype=float)
    x0 = np.broadcast_to(x0, (R, Q) + x0.shape[-2:]).reshape((R * Q,) + x0.shape[-2:])
    out = _mcmc_call(engine, summary, n_step, thin, ladder, swap_every, prior)(x0, r_of.astype(np.int32), rows, box, split_times=splits[j_of], n_step=n_step, thin=thin,
                                                    temperature=temperature, a=a, seed=seed, ids=j_of.astype(np.uint64))
    return {k: (v.reshape(R, Q, *v.shape[1:]) if isinstance(v, np.ndarray) else v) for k, v in out.items()}


def split_fit_mcmc(engine, jsfs_rows, init, box, band_bounds=None, pulse_times=None, n_step=100, thin=1, temperature=1.0, a=2.0, seed=0, summary=None,
                   ladder=None, swap_every=1, prior=None):
    """``split_fit_de``'s sampler: per row ONE ensemble over (optimised parameters, split) inside ``box`` (``(lo, hi)``, each
    ``[n_param + 1]``, finite, the split last), all R ensembles in ONE ``misti_ensemble_sample`` call.  ``init`` is ``[W][n_param + 1]``
    (every row starts from it) or ``[R][W][n_param + 1]``; every row draws from stream 0 (the rows of a bootstrap share their random
    numbers - only the data differ).  ``band_bounds`` / ``pulse_times`` apply to every ensemble.
    ``summary``: None, or a dict of ``Engine.ensemble_posterior``'s options (``burn`` - default half the kept steps -, ``probs``,
    ``max_lag``, ``keep_chain``, ``c``): the call goes through ``misti_ensemble_posterior`` and the chain stays on the device.
    ``ladder`` / ``swap_every`` / ``prior`` as in ``bootstrap_profile_mcmc``: ``misti_tempered_sample``; the prior covers the split
    (the last coordinate) too.
    Returns what ``Engine.ensemble_sample`` (``Engine.ensemble_posterior``, ``Engine.tempered_sample``) returns (leading axis: the row)."""
    rows = np.asarray(jsfs_rows, dtype=float).reshape(-1, 8)
    R = rows.shape[0]
    x0 = np.asarray(init, dtype=float)
    x0 = np.ascontiguousarray(np.broadcast_to(x0, (R,) + x0.shape[-2:]))
    tile = lambda v, shape: None if v is None else np.repeat(np.asarray(v, dtype=np.int32).reshape(shape), R, axis=0)
    return _mcmc_call(engine, summary, n_step, thin, ladder, swap_every, prior)(x0, np.arange(R, dtype=np.int32), rows, box, fit_split=True, band_bounds=tile(band_bounds, (1, -1, 2)),
                                                     pulse_times=tile(pulse_times, (1, -1)), n_step=n_step, thin=thin, temperature=temperature,
                                                     a=a, seed=seed, ids=np.zeros(R, dtype=np.uint64))
