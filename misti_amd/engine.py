"""Python host of the HIP likelihood engine.

Two layers:

``Engine``
    thin, batch-shaped wrapper of the C ABI (``include/misti_hip.h``): one
    model (merged PSMC grid, band/pulse structure, flags) on one GPU, evaluated
    for a batch of candidates x bootstrap JSFS replicates.

``MigrationInference``
    mirror of the reference class of the same name
    (``/root/reference/MigrationInference.py:35-739``): same constructor
    signature, keyword flags, attributes (``.JAFS .lc .lh .mi .pu .Pr .llh
    .times .numT .splitT .dataJAFS .llh_const``), ``JAFSLikelihood(mu)``,
    ``Solve(tol)``, counters and messages - so callers such as ``MiSTI.py`` and
    ``migrationIO.OutputMigration`` work unchanged on top of the GPU path.

There is no CPU path here: if ``libmisti_hip.so`` cannot be loaded or no HIP
device is present, construction fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
import math
import sys

import numpy as np

from . import _lib
from ._lib import CPFIT, SMOOTH, TRUE_EPS, UNFOLDED, MistiError, STATUS_TEXT
from .optimize import fold_classes

__all__ = ["Engine", "MigrationInference", "ModelError", "BatchResult", "CurvatureResult"]


class ModelError(SystemExit):
    """Raised where the reference prints an error and calls ``sys.exit(0)``
    (``PrintError``, MigrationInference.py:300-303).  Uncaught, the process exits
    with status 0 exactly as the reference does; a caller may also catch it."""

    def __init__(self, func, text):
        self.message = "MigrationInference class error in function %s(): %s" % (func, text)
        print(self.message)
        super().__init__(0)


class BatchResult:
    """Outputs of one batch: ``llk[C][R]``, ``jafs[C][7]``, ``status[C]`` and, if
    requested, ``lc[C][numT+1][2]`` and ``pr[C][numT+2][6]``."""
    __slots__ = ("llk", "jafs", "status", "lc", "pr", "runaway")

    def __init__(self, llk, jafs, status, lc=None, pr=None, runaway=None):
        self.llk, self.jafs, self.status, self.lc, self.pr = llk, jafs, status, lc, pr
        self.runaway = runaway      # largest corrected rate x interval length (>= ~5: reference-indeterminate)

    @property
    def fraction_failed(self):
        return float((self.status != 0).mean()) if self.status.size else 0.0


class CurvatureResult:
    """Outputs of ``Engine.curvature``: per point ``llh0[P]`` (the centre's log-likelihood against its row), ``grad[P][D]`` and
    ``hess[P][D][D]`` of that row's log-likelihood, ``dlog[P][D][7]`` (the derivatives of the class logs: the score covariance over
    bootstrap rows is ``dlog Cov(d) dlog^T``), the steps ``h[P][D]`` and ``status[P]`` (0, 7 = no two-sided stencil at this point, or
    the engine's status of the first stencil candidate without a value; every other output of such a point is NaN)."""
    __slots__ = ("llh0", "grad", "hess", "dlog", "h", "status")

    def __init__(self, llh0, grad, hess, dlog, h, status):
        self.llh0, self.grad, self.hess, self.dlog, self.h, self.status = llh0, grad, hess, dlog, h, status


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _box_arrays(box, N):
    """``(lo, hi)``, each ``[N]`` or ``[S][N]``, as the ``box_lo`` / ``box_hi`` arrays ``[n_box][N]`` of a search."""
    lo, hi = (_f64(a) for a in box)
    if lo.shape != hi.shape or lo.ndim not in (1, 2) or lo.shape[-1] != N:
        raise ValueError("box: lo and hi must both be [%d] or [S][%d] (got %s and %s)" % (N, N, lo.shape, hi.shape))
    return lo.reshape(-1, N), hi.reshape(-1, N)


def _model_struct(times, lh, bands, pulses, n_param, cpfit, true_eps, smooth, unfolded, sample_date, mixture_th):
    """(misti_model_t, objects that must stay alive while it is used) from the constructor arguments Engine / Lanes share."""
    times = _f64(times)
    lh = _f64(lh)
    numT = int(lh.shape[0])
    if lh.ndim != 2 or lh.shape[1] != 2 or times.shape != (numT - 1,):
        raise ValueError("times must have numT-1 entries and lh shape [numT][2]")
    flags = (CPFIT if cpfit else 0) | (TRUE_EPS if true_eps else 0) | (SMOOTH if smooth else 0) | (UNFOLDED if unfolded else 0)
    bands, pulses = list(bands), list(pulses)
    b_arr = (_lib.Band * max(1, len(bands)))()
    for i, (pop, start, end, value, param) in enumerate(bands):
        b_arr[i] = _lib.Band(int(pop), int(start), int(end), int(param), float(value))
    p_arr = (_lib.Pulse * max(1, len(pulses)))()
    for i, (pop, time, value, param) in enumerate(pulses):
        p_arr[i] = _lib.Pulse(int(pop), int(time), int(param), 0, float(value))
    m = _lib.Model(numT, int(sample_date), flags, len(bands), len(pulses), int(n_param), float(mixture_th),
                   times.ctypes.data_as(C.POINTER(C.c_double)), lh.ctypes.data_as(C.POINTER(C.c_double)), b_arr, p_arr)
    return m, (times, lh, b_arr, p_arr)


def _bootstrap_rows(lib, ctx, device, chunks, n, seed, first, normalize, draws):
    """``misti_bootstrap_rows_dev`` on context ``ctx`` of ``device`` into fresh torch tensors: ``rows[n][8]`` float64 and, with ``draws``,
    the draw counts ``[n]`` int32 (else None).  Waits for the context's stream: the tensors are ready for any stream."""
    import torch
    c = _f64(chunks, (-1, 8))
    n = int(n)
    if n < 0:
        raise ValueError("bootstrap: the number of replicates must not be negative (got %d)" % n)
    dev = torch.device("cuda", int(device))
    rows = torch.empty((n, 8), dtype=torch.float64, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev) if draws else None
    v = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    torch.cuda.current_stream(dev).synchronize()      # the engine's stream is non-blocking: whatever last used this memory must have finished
    _lib.check(lib.misti_bootstrap_rows_dev(ctx, c.shape[0], c.ctypes.data_as(C.c_void_p), C.c_uint64(int(seed)), int(first), n,
                                            _lib.BOOT_NORMALIZE if normalize else 0, v(rows), v(count)))
    _lib.check(lib.misti_sync(ctx))
    return rows, count


def _bootstrap_table(rows_dev, chunks):
    """Row 0 - the column sums of all chunks, added in chunk order - in front of the replicates a device made: ``io.bootstrap_table``'s layout."""
    from .optimize import _in_order_sum
    return np.vstack([_in_order_sum(_f64(chunks, (-1, 8)))[None, :], rows_dev.cpu().numpy()])


def _jackknife_rows(lib, ctx, device, chunks, m, first, n):
    """``misti_jackknife_rows_dev`` on context ``ctx`` of ``device`` into a fresh torch tensor ``rows[n][8]`` float64: leave-out rows
    ``first ... first + n - 1`` (``n`` None: all from ``first``; ``misti_jackknife_geometry`` says how many there are).  Waits for the
    context's stream: the tensor is ready for any stream."""
    import torch
    c = _f64(chunks, (-1, 8))
    m, first = int(m), int(first)
    if n is None:
        G = C.c_int64(0)
        _lib.check(lib.misti_jackknife_geometry(c.shape[0], m, C.byref(G)))
        n = G.value - first
    n = int(n)
    if n < 0 or first < 0:
        raise ValueError("jackknife: first and the number of rows must not be negative (got %d, %d)" % (first, n))
    dev = torch.device("cuda", int(device))
    rows = torch.empty((n, 8), dtype=torch.float64, device=dev)
    torch.cuda.current_stream(dev).synchronize()      # the engine's stream is non-blocking: whatever last used this memory must have finished
    _lib.check(lib.misti_jackknife_rows_dev(ctx, c.shape[0], c.ctypes.data_as(C.c_void_p), m, first, n, 0,
                                            C.c_void_p(rows.data_ptr()) if n else None))
    _lib.check(lib.misti_sync(ctx))
    return rows


def _parametric_rows(lib, ctx, device, spectra, n, n_sites, genome, seed, first, spec_of, status, row_status):
    """``misti_parametric_rows_dev`` on context ``ctx`` of ``device`` into fresh torch tensors: ``rows[n][8]`` float64 and the row
    statuses ``[n]`` int32.  ``spectra`` (``[n_spec][7]`` float64), ``spec_of`` and ``status`` (int32) are ndarrays - uploaded - or
    tensors of this device, read where they are.  Waits for the context's stream.  Raises if a row status is set, unless
    ``row_status`` asks for the array: returns ``rows`` or ``(rows, statuses)``."""
    import torch
    n, n_sites = int(n), int(n_sites)
    if n < 0:
        raise ValueError("parametric bootstrap: the number of replicates must not be negative (got %d)" % n)
    dev = torch.device("cuda", int(device))

    def on_device(a, dtype, shape):
        if a is None:
            return None
        if hasattr(a, "data_ptr"):
            if a.device != dev or a.dtype != dtype or not a.is_contiguous():
                raise ValueError("parametric bootstrap: a tensor argument must be contiguous %s on %s" % (dtype, dev))
            return a.reshape(shape)
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64 if dtype == torch.float64 else np.int32).reshape(shape), device=dev)

    sp = on_device(spectra, torch.float64, (-1, 7))
    of = on_device(spec_of, torch.int32, (n,))
    st = on_device(status, torch.int32, (sp.shape[0],))
    rows = torch.empty((n, 8), dtype=torch.float64, device=dev)
    flags = torch.empty(n, dtype=torch.int32, device=dev)
    v = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    torch.cuda.current_stream(dev).synchronize()      # the engine's stream is non-blocking: the uploads and whatever last used this memory must have finished
    _lib.check(lib.misti_parametric_rows_dev(ctx, sp.shape[0], v(sp), v(st), v(of), float(genome), n_sites, C.c_uint64(int(seed)), int(first), n,
                                             v(rows), v(flags)))
    _lib.check(lib.misti_sync(ctx))
    if row_status:
        return rows, flags
    bad = int(flags.count_nonzero())
    if bad:
        raise ValueError("parametric bootstrap: %d of %d replicates have no usable spectrum (an entry negative or not finite, a sum that is "
                         "not > 0, a status without a value or an index out of range); row_status=True returns the flags" % (bad, n))
    return rows


def _parametric_table(engine, ctx, device, split, params, data_row, n, n_sites, seed, band_bounds=None, pulse_times=None):
    """``Engine.parametric_table`` with the point evaluated by ``engine`` (an Engine or a MultiEngine) and the rows drawn on ``ctx``."""
    from .optimize import parametric_table
    row = _f64(data_row, (8,))
    kw = {} if pulse_times is None else {"pulse_times": pulse_times}
    res = engine.evaluate([float(split)], [list(params)] if params is not None and len(params) else None, band_bounds=band_bounds, **kw)
    if int(res.status[0]) != 0:
        raise MistiError(int(res.status[0]), "parametric bootstrap: the generating point has no value: " + STATUS_TEXT.get(int(res.status[0]), "?"))
    if n_sites is None:
        n_sites = int(np.rint(row[1:].sum()))
    rows = _parametric_rows(engine._lib, ctx, device, res.jafs[:1], n, n_sites, row[0], seed, 0, None, None, False)
    return parametric_table(row, rows.cpu().numpy())


class Engine:
    """One model on one GPU (``misti_create`` ... ``misti_destroy``).

    Parameters
    ----------
    times : [numT-1] interval lengths;  lh : [numT][2] PSMC rates.
    bands : iterable of ``(pop, start, end, value, param)`` with pop in {0,1},
        ``end == -1`` meaning "the candidate's split index" and ``param`` the index
        into the candidate parameter vector or -1 for a fixed rate.
    pulses : iterable of ``(pop, time, value, param)``.
    """

    def __init__(self, times, lh, bands=(), pulses=(), n_param=0, cpfit=False, true_eps=False, smooth=False,
                 unfolded=False, sample_date=0, mixture_th=0.0, device=0):
        self._ctx = C.c_void_p()
        self._lib = _lib.load()
        times = _f64(times)
        lh = _f64(lh)
        self.numT = int(lh.shape[0])
        if lh.ndim != 2 or lh.shape[1] != 2 or times.shape != (self.numT - 1,):
            raise ValueError("times must have numT-1 entries and lh shape [numT][2]")
        self.n_param = int(n_param)
        self.flags = (CPFIT if cpfit else 0) | (TRUE_EPS if true_eps else 0) | (SMOOTH if smooth else 0) | (UNFOLDED if unfolded else 0)
        self.unfolded = bool(unfolded)
        bands = list(bands)
        pulses = list(pulses)
        self.n_band = len(bands)
        self.n_pulse = len(pulses)
        b_arr = (_lib.Band * max(1, len(bands)))()
        for i, (pop, start, end, value, param) in enumerate(bands):
            b_arr[i] = _lib.Band(int(pop), int(start), int(end), int(param), float(value))
        p_arr = (_lib.Pulse * max(1, len(pulses)))()
        for i, (pop, time, value, param) in enumerate(pulses):
            p_arr[i] = _lib.Pulse(int(pop), int(time), int(param), 0, float(value))
        m = _lib.Model(self.numT, int(sample_date), self.flags, len(bands), len(pulses), self.n_param, float(mixture_th),
                       times.ctypes.data_as(C.POINTER(C.c_double)), lh.ctypes.data_as(C.POINTER(C.c_double)),
                       b_arr, p_arr)
        ctx = C.c_void_p()
        _lib.check(self._lib.misti_create(C.byref(m), int(device), C.byref(ctx)))
        self._ctx = ctx
        self._pid = os.getpid()
        self.device = int(device)

    # -- lifetime --------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx:
            # a context belongs to the process that created it: in a child forked later (a worker pool of the caller)
            # the HIP runtime is not usable - a garbage-collected copy of this object there must not call into it
            if getattr(self, "_pid", None) == os.getpid() and not getattr(self, "_borrowed", False):     # a lane of a Lanes object belongs to it
                self._lib.misti_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- host-buffer evaluation ----------------------------------------------
    def evaluate(self, split_time, params=None, jsfs=None, want_lc=False, want_pr=False, band_bounds=None, pulse_times=None):
        """``misti_eval_batch``: NumPy in, NumPy out (copies over PCIe).

        ``band_bounds`` ([n][n_band][2] ints, optional): per-candidate (start, end) of every band, replacing the
        model's (``end == -1``: the candidate's split index) - the README's ``::: st ... ::: mc ...`` sweep in one call.

        ``pulse_times`` ([n][n_pulse] ints, optional): per-candidate time of every pulse, replacing the model's
        (``misti_eval_batch_pulses``) - the same recipe with ``-pu 2 {t} {f} 0`` in the place of a band.  An index on the
        candidate's own grid; a candidate whose times break SetModel's checks gets status 4 and -inf."""
        split = _f64(np.atleast_1d(split_time))
        n = split.shape[0]
        P = self.n_param
        par = None
        if P:
            par = _f64(params, (n, P))
        if hasattr(jsfs, "data_ptr"):              # a device tensor (bootstrap_rows_dev): this is the host-buffer form
            jsfs = jsfs.cpu().numpy()
        rows = _f64(jsfs, (-1, 8)) if jsfs is not None and len(jsfs) else np.zeros((0, 8))
        R = rows.shape[0]
        llk = np.empty((n, R))
        jafs = np.empty((n, 7))
        status = np.empty(n, dtype=np.int32)
        lc = np.empty((n, self.numT + 1, 2)) if want_lc else None
        pr = np.empty((n, self.numT + 2, 6)) if want_pr else None
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
        bb = None
        if band_bounds is not None and self.n_band:
            bb = np.ascontiguousarray(band_bounds, dtype=np.int32).reshape(n, self.n_band, 2)
        if pulse_times is not None and self.n_pulse:
            pt = np.ascontiguousarray(pulse_times, dtype=np.int32).reshape(n, self.n_pulse)
            _lib.check(self._lib.misti_eval_batch_pulses(self._ctx, n, ptr(split), ptr(par), ptr(bb), ptr(pt), R, ptr(rows), ptr(llk),
                                                         ptr(jafs), ptr(lc), ptr(pr), ptr(status)))
        else:
            _lib.check(self._lib.misti_eval_batch(self._ctx, n, ptr(split), ptr(par), ptr(bb), R, ptr(rows), ptr(llk), ptr(jafs),
                                                  ptr(lc), ptr(pr), ptr(status)))
        return BatchResult(llk, jafs, status, lc, pr, self.last_diag(n) if n else np.zeros(0))

    def forward_rates(self, split_time, params=None, want_pr=False, hold_mu=False):
        """``misti_forward_rates``: the model's rates taken as the truth -> the rates a single-genome
        analysis would see under each candidate's migration model (CoalescentRates, :542-564).
        ``hold_mu=True`` reproduces the reference exactly (every interval evaluated with the
        migration rates of the last two-population interval, see include/misti_hip.h).
        Returns (lh[n][numT+1][2], pr[n][numT+2][6] or None, status[n])."""
        split = _f64(np.atleast_1d(split_time))
        n = split.shape[0]
        par = _f64(params, (n, self.n_param)) if self.n_param else None
        lh = np.empty((n, self.numT + 1, 2))
        pr = np.empty((n, self.numT + 2, 6)) if want_pr else None
        status = np.empty(n, dtype=np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
        _lib.check(self._lib.misti_forward_rates(self._ctx, n, ptr(split), ptr(par), 1 if hold_mu else 0, ptr(lh), ptr(pr), ptr(status)))
        return lh, pr, status

    def pair_residuals(self, problems, cpfit=True):
        """``misti_pair_residuals`` (introspection, for the suite): the pair-chain residual as the chain kernels evaluate it, one problem
        ``[mu0, mu1, P[3], tgt, x0, x1, role, red]`` per lane.  Returns ``out[n][4]``: the residual and ``w = e^M P``."""
        p = _f64(problems, (-1, 10))
        out = np.empty((p.shape[0], 4))
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
        _lib.check(self._lib.misti_pair_residuals(self._ctx, 1 if cpfit else 0, p.shape[0], ptr(p), ptr(out)))
        return out

    LSQ_KINDS = {"SCALAR": 0, "SVD2": 1, "SVD4": 2, "STEP": 3, "STEPN": 4, "SELECT": 5, "UPDATE": 6, "SOLVE3": 7}
    LSQ_IN, LSQ_OUT = 20, 16

    def lsq_probe(self, kind, problems):
        """``misti_lsq_probe`` (introspection, for the suite): the solver's linear algebra as the chain kernels run it, one problem per
        lane.  ``kind`` is a name of ``LSQ_KINDS`` or its number; a row of ``problems`` may be shorter than ``LSQ_IN`` (the rest is 0).
        Returns ``out[n][LSQ_OUT]``; the layouts are in include/misti_hip.h."""
        k = self.LSQ_KINDS[kind] if isinstance(kind, str) else int(kind)
        a = np.asarray(problems, dtype=np.float64)
        a = a.reshape(-1, a.shape[-1]) if a.size else a.reshape(0, self.LSQ_IN)
        p = np.zeros((a.shape[0], self.LSQ_IN))
        p[:, :a.shape[1]] = a
        out = np.empty((p.shape[0], self.LSQ_OUT))
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
        _lib.check(self._lib.misti_lsq_probe(self._ctx, k, p.shape[0], ptr(p), ptr(out)))
        return out

    def last_diag(self, n_cand):
        """Largest corrected rate x interval length per candidate of the last batch (misti_last_diag)."""
        out = np.empty(int(n_cand))
        _lib.check(self._lib.misti_last_diag(self._ctx, int(n_cand), out.ctypes.data_as(C.c_void_p)))
        return out

    # -- device-buffer evaluation (torch tensors on this device) ------------------
    def use_stream(self, stream_handle):
        """Issue kernels on an existing hipStream_t (int handle), e.g.
        ``torch.cuda.current_stream().cuda_stream``; ``None`` restores the own stream."""
        _lib.check(self._lib.misti_set_stream(self._ctx, C.c_void_p(stream_handle) if stream_handle else None))

    def stream_handle(self):
        """The hipStream_t (int) this engine issues on - its own non-blocking stream unless replaced."""
        h = C.c_void_p()
        _lib.check(self._lib.misti_get_stream(self._ctx, C.byref(h)))
        return h.value or 0

    def set_hints(self, integer_splits=False):
        """``misti_set_hints``: what the caller knows about the batches it will issue on this context (device-buffer form: the split times live in
        HBM).  ``integer_splits``: no split time has a fractional part - the launch that only serves fractional splits is not made (a batch that
        has one after all gets status 4 for that candidate, never a wrong value)."""
        _lib.check(self._lib.misti_set_hints(self._ctx, _lib.HINT_INTEGER_SPLITS if integer_splits else 0))

    def evaluate_dev(self, n_cand, d_split, d_params, n_rep, d_jsfs, d_llk, d_jafs=0, d_lc=0, d_pr=0, d_status=0, d_bounds=0, d_pulse_times=0):
        """``misti_eval_batch_dev``: raw device addresses (ints); asynchronous.  With ``d_pulse_times`` ([n][n_pulse] int32 on the
        device): ``misti_eval_batch_pulses_dev``."""
        v = lambda p: C.c_void_p(int(p)) if p else None
        if d_pulse_times:
            _lib.check(self._lib.misti_eval_batch_pulses_dev(self._ctx, int(n_cand), v(d_split), v(d_params), v(d_bounds), v(d_pulse_times),
                                                             int(n_rep), v(d_jsfs), v(d_llk), v(d_jafs), v(d_lc), v(d_pr), v(d_status)))
            return
        _lib.check(self._lib.misti_eval_batch_dev(self._ctx, int(n_cand), v(d_split), v(d_params), v(d_bounds), int(n_rep), v(d_jsfs),
                                                  v(d_llk), v(d_jafs), v(d_lc), v(d_pr), v(d_status)))

    def llk_dev(self, n_cand, d_jafs, d_status, n_rep, d_jsfs, d_llk):
        v = lambda p: C.c_void_p(int(p)) if p else None
        _lib.check(self._lib.misti_llk_dev(self._ctx, int(n_cand), v(d_jafs), v(d_status), int(n_rep), v(d_jsfs), v(d_llk)))

    def argmax_dev(self, n_cand, n_rep, d_llk, d_best, d_best_llk=0):
        """``misti_argmax_dev``: per replicate the index of the best candidate (raw device addresses; asynchronous)."""
        v = lambda p: C.c_void_p(int(p)) if p else None
        _lib.check(self._lib.misti_argmax_dev(self._ctx, int(n_cand), int(n_rep), v(d_llk), v(d_best), v(d_best_llk)))

    def scan_best_dev(self, n_cand, d_jafs, d_status, n_rep, d_jsfs, k, d_best, d_best_llk=0):
        """``misti_scan_best_dev``: per replicate the ``k`` best candidates (``d_best[n_rep][k]`` int32, ``d_best_llk[n_rep][k]``), value
        descending and index ascending on ties, -1 / -inf where fewer have a value - from spectra alone, without the ``[n_cand][n_rep]``
        table (raw device addresses; asynchronous).  ``k = 1`` is ``llk_dev`` followed by ``argmax_dev``."""
        v = lambda p: C.c_void_p(int(p)) if p else None
        _lib.check(self._lib.misti_scan_best_dev(self._ctx, int(n_cand), v(d_jafs), v(d_status), int(n_rep), v(d_jsfs), int(k), v(d_best),
                                                 v(d_best_llk)))

    def scan_profile_dev(self, n_cand, d_jafs, d_status, d_group, n_group, n_rep, d_jsfs, d_prof_llk, d_prof_best=0):
        """``misti_scan_profile_dev``: per replicate and group the best candidate of the group (``d_prof_llk[n_rep][n_group]``,
        ``d_prof_best[n_rep][n_group]`` int32) among the candidates labelled ``d_group[c] == g`` (int32; a label outside
        ``0 ... n_group - 1`` is in no group), value descending and index ascending on ties, -inf / -1 for a group without a value - from
        spectra alone, without the ``[n_cand][n_rep]`` table (raw device addresses; asynchronous)."""
        v = lambda p: C.c_void_p(int(p)) if p else None
        _lib.check(self._lib.misti_scan_profile_dev(self._ctx, int(n_cand), v(d_jafs), v(d_status), v(d_group), int(n_group), int(n_rep), v(d_jsfs),
                                                    v(d_prof_llk), v(d_prof_best)))

    def bootstrap_rows_dev(self, chunks, n, seed=0, first=0, normalize=False, draws=False):
        """``misti_bootstrap_rows_dev``: block-bootstrap replicates ``first ... first + n - 1`` of the chunk table ``chunks[n_chunk][8]``
        (host; column 0 the chunk's length, columns 1..7 its class counts) made on this device - a torch tensor ``[n][8]`` float64 and,
        with ``draws``, the number of chunks each replicate drew (``[n]`` int32).  The rule is ``optimize.block_bootstrap``, bit for bit:
        the project's own counter-based stream (replicate r depends on ``(seed, r)`` alone), not the reference's Mersenne Twister.
        ``normalize``: the reference's ``normalize=True``.  The tensor is an ordinary row buffer: ``evaluate`` takes it as it is, and
        ``evaluate_dev``, ``llk_dev``, ``scan_best_dev`` and ``scan_profile_dev`` its ``data_ptr()``.  Returns when the rows are there."""
        rows, count = _bootstrap_rows(self._lib, self._ctx, self.device, chunks, n, seed, first, normalize, draws)
        return (rows, count) if draws else rows

    def bootstrap_table(self, chunks, n, seed=0, normalize=False):
        """The table ``io.bootstrap_table`` lays out, its replicates made by ``bootstrap_rows_dev``: a host ``ndarray [1 + n][8]``, row 0 the
        column sums of all chunks (added in chunk order), row 1 + r replicate r - ``optimize.block_bootstrap_table``, bit for bit."""
        return _bootstrap_table(self.bootstrap_rows_dev(chunks, n, seed=seed, normalize=normalize), chunks)

    def jackknife_rows_dev(self, chunks, m=1, first=0, n=None):
        """``misti_jackknife_rows_dev``: delete-m leave-out rows ``first ... first + n - 1`` (``n`` None: all from ``first``) of the chunk
        table ``chunks[n_chunk][8]``, made on this device - a torch tensor ``[n][8]`` float64.  Row g is the chunks outside group
        ``g m ... min((g + 1) m, n_chunk) - 1`` added in chunk order: ``optimize.jackknife_rows``, bit for bit.  The tensor is an
        ordinary row buffer, usable wherever ``bootstrap_rows_dev``'s is."""
        return _jackknife_rows(self._lib, self._ctx, self.device, chunks, m, first, n)

    def jackknife_table(self, chunks, m=1):
        """A host ``ndarray [1 + G][8]``: row 0 the column sums of all chunks (added in chunk order), row 1 + g leave-out row g of
        ``jackknife_rows_dev`` - ``optimize.jackknife_table``, bit for bit.  Its column 0 is what ``optimize.jackknife_estimate`` weighs by."""
        return _bootstrap_table(self.jackknife_rows_dev(chunks, m), chunks)

    def parametric_rows_dev(self, spectra, n, n_sites, genome, seed=0, first=0, spec_of=None, status=None, row_status=False):
        """``misti_parametric_rows_dev``: parametric-bootstrap replicates ``first ... first + n - 1`` made on this device - ``n_sites``
        sites each, drawn independently from the seven classes of ``spectra[spec_of[r]]`` (spectrum 0 without ``spec_of``); a torch tensor
        ``[n][8]`` float64, column 0 ``genome``.  ``spectra`` is an ndarray or a tensor of this device (the ``d_jafs`` an ``evaluate_dev``
        wrote, read where it is), ``status`` likewise (the evaluation's statuses: a spectrum without a value is unusable).  The rule is
        ``optimize.parametric_rows``, bit for bit; replicate r depends on ``(seed, r, spectrum, n_sites)`` alone.  A replicate without a
        usable spectrum is a row of zeros with status 1: that raises, unless ``row_status=True`` asks for ``(rows, statuses)``.  The
        tensor is an ordinary row buffer, usable wherever ``bootstrap_rows_dev``'s is.  NOTE: independent sites - real sites are
        linked, so intervals from these rows are narrower than the block bootstrap's; where chunks exist that one is the confidence
        statement.  Returns when the rows are there."""
        return _parametric_rows(self._lib, self._ctx, self.device, spectra, n, n_sites, genome, seed, first, spec_of, status, row_status)

    def parametric_table(self, split, params, data_row, n, n_sites=None, seed=0, band_bounds=None, pulse_times=None):
        """The table ``[data_row; n replicates]`` (host ``ndarray [1 + n][8]``) of a parametric bootstrap from the point ``(split,
        params)``: the point is evaluated, and the replicates are drawn from its spectrum with ``genome = data_row[0]`` and ``n_sites``
        sites - by default ``rint`` of the sum of the data row's seven classes.  ``optimize.parametric_table(data_row,
        optimize.parametric_rows(evaluate(...).jafs, ...))``, bit for bit.  Raises if the point has no value."""
        return _parametric_table(self, self._ctx, self.device, split, params, data_row, n, n_sites, seed, band_bounds, pulse_times)

    def curvature(self, x, split_times, rows, table, band_bounds=None, pulse_times=None, rel_step=1e-2, abs_step=0.0, batch_limit=0):
        """``misti_curvature``: gradient and Hessian of the log-likelihood at every point ``x[P][n_param]`` (split ``split_times[p]``
        held fixed, row ``rows[p]`` of ``table[n_rep][8]``, optionally the point's own ``band_bounds[P][n_band][2]`` and
        ``pulse_times[P][n_pulse]``) by central differences of the class logs over ``optimize.curvature_stencil``'s
        ``1 + 2 n_param^2`` candidates per point - laid out on the device, evaluated through the batch path in batches of at most
        ``batch_limit`` candidates (0: the library's choice; whole points only), assembled and contracted there.  ``rel_step`` /
        ``abs_step``: ``h_i = (x_i + max(rel_step |x_i|, abs_step)) - x_i`` (the realised step: ``x_i +- h_i`` are exact doubles); what the default 1e-2 costs in truncation is measured in DESIGN.md
        section 4 ("Curvature at a fitted point", paragraph "Measured"), with the advice for a rate near zero.  A point with
        ``x_i - h_i < 0`` gets status 7 and is not evaluated.  Returns a ``CurvatureResult``; ``optimize.observed_covariance`` /
        ``sandwich_covariance`` / ``standard_errors`` take it from there."""
        D = self.n_param
        xs = _f64(x, (-1, D)) if D else _f64(x)
        P = xs.shape[0] if D else 0
        i32 = lambda a, shape: np.ascontiguousarray(np.asarray(a).reshape(shape), dtype=np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        st = _f64(np.broadcast_to(np.asarray(split_times, dtype=np.float64), (P,)))
        r_of = i32(np.broadcast_to(np.asarray(rows), (P,)), (P,))
        tab = _f64(table, (-1, 8))
        bb = i32(band_bounds, (P, self.n_band, 2)) if band_bounds is not None and self.n_band else None
        pt = i32(pulse_times, (P, self.n_pulse)) if pulse_times is not None and self.n_pulse else None
        llh0, grad, hess, dlog = np.empty(P), np.empty((P, D)), np.empty((P, D, D)), np.empty((P, D, 7))
        status = np.empty(P, dtype=np.int32)
        _lib.check(self._lib.misti_curvature(self._ctx, P, ptr(xs), ptr(st), ptr(r_of), ptr(bb), ptr(pt), tab.shape[0], ptr(tab),
                                             float(rel_step), float(abs_step), int(batch_limit), ptr(llh0), ptr(grad), ptr(hess), ptr(dlog), ptr(status)))
        h = (xs + np.maximum(float(rel_step) * np.abs(xs), float(abs_step))) - xs  # curv_steps_kernel's four operations
        return CurvatureResult(llh0, grad, hess, dlog, h, status)

    def curvature_assemble_dev(self, n_point, d_jafs, d_status, d_h, d_rows, n_rep, d_jsfs, d_dlog=0, d_d2log=0, d_grad=0, d_hess=0, d_point_status=0):
        """``misti_curvature_assemble_dev``: ``dlog[P][D][7]``, ``d2log[P][D][D][7]`` and the point statuses from stencil spectra
        ``d_jafs[P][M][7]`` (``d_status[P][M]`` or 0: all OK) and steps ``d_h[P][D]``, and with ``d_rows[P]`` (int32) the contraction
        ``grad[P][D]`` / ``hess[P][D][D]`` with each point's row of ``d_jsfs[n_rep][8]`` - ``optimize.curvature_from_spectra`` and
        ``curvature_contract`` on the device (raw device addresses; asynchronous)."""
        v = lambda p: C.c_void_p(int(p)) if p else None
        _lib.check(self._lib.misti_curvature_assemble_dev(self._ctx, int(n_point), v(d_jafs), v(d_status), v(d_h), v(d_rows), int(n_rep), v(d_jsfs),
                                                          v(d_dlog), v(d_d2log), v(d_grad), v(d_hess), v(d_point_status)))

    def sync(self):
        _lib.check(self._lib.misti_sync(self._ctx))

    def _nm_stats(self):
        """Work counters of the last search on this context: iterations issued, their batch slots, speculative iterations."""
        stats = (C.c_int64 * 2)()
        _lib.check(self._lib.misti_nm_last_stats(self._ctx, stats))
        spec = C.c_int64(0)
        _lib.check(self._lib.misti_nm_last_spec_iterations(self._ctx, C.byref(spec)))
        return dict(iterations_issued=int(stats[0]), slots=int(stats[1]), speculative_iterations=int(spec.value))

    def _rows_problem(self, S, N, table, split_times, rows, band_bounds, pulse_times, box, ids):
        """What ``misti_search_t``, ``misti_de_t`` and ``misti_ens_t`` share, marshalled once: the arrays (to be kept alive until the
        call returns) and the descriptor fields they fill.  ``table`` is already an array (``[8]``: one data row, or ``[n_rep][8]``)."""
        i32 = lambda a, shape: np.ascontiguousarray(np.asarray(a).reshape(shape), dtype=np.int32)
        lo, hi = _box_arrays(box, N) if box is not None else (None, None)
        keep = dict(jsfs=table, split_times=_f64(split_times, (S,)) if split_times is not None else None,
                    rows=i32(rows, (S,)) if rows is not None else None,
                    band_bounds=i32(band_bounds, (S, self.n_band, 2)) if band_bounds is not None and self.n_band else None,
                    pulse_times=i32(pulse_times, (S, self.n_pulse)) if pulse_times is not None and self.n_pulse else None,
                    box_lo=lo, box_hi=hi, ids=np.ascontiguousarray(np.asarray(ids).reshape(S), dtype=np.uint64) if ids is not None else None)
        fields = {k: v.ctypes.data if v is not None else None for k, v in keep.items()}
        fields.update(n_start=S, n_rep=1 if table.ndim == 1 else table.shape[0], n_box=0 if lo is None else lo.shape[0])
        return keep, fields

    def search(self, starts, table, *, split_time=None, split_times=None, rows=None, band_bounds=None, pulse_times=None, box=None,
               hops=None, rngs=None, xatol=1e-4, fatol=1e-4, maxiter=None):
        """``misti_search``: every batched search and every basin hopping is this call (``misti_search_t`` in include/misti_hip.h
        documents the fields).  ``split_time`` given: one split for all starts and ``table`` the one data row ``[8]``; ``split_times``
        given: a split per start; neither: the split is the last of ``n_param + 1`` coordinates of ``starts``.  ``rows`` ``[S]`` into
        ``table[n_rep][8]``; ``band_bounds`` / ``pulse_times`` per start (``None``, or a model without band / pulse: NULL); ``box``
        ``(lo, hi)``, each ``[N]`` or ``[S][N]``.  ``hops``: a dict of ``niter``, ``T``, ``stepsize``, ``interval``,
        ``target_accept_rate``, ``stepwise_factor``, ``nm_maxfev`` (SciPy's defaults where absent or None) with ``rngs`` one
        generator or seed per start - basin hopping around the search.  ``maxiter`` defaults to 1000, under hops to ``200 x N``.
        Returns dict(x[S][N], llh[S], nit / nfev / status[S] - with hops nfev / failures / accepted[S] -, and the work counters)."""
        one = split_time is not None
        N = self.n_param + (0 if one or split_times is not None else 1)
        st = _f64(starts, (-1, N))
        S = st.shape[0]
        ptr = lambda a: a.ctypes.data if a is not None else None
        arrays, fields = self._rows_problem(S, N, _f64(table, (8,) if one else (-1, 8)), split_times, rows, band_bounds, pulse_times, box, None)
        del fields["ids"]
        x, llh = np.empty((S, N)), np.empty(S)
        counters = dict(zip(("nit", "nfev", "status") if hops is None else ("nfev", "failures", "accepted"),
                            (np.empty(S, dtype=np.int32) for _ in range(3))))
        q = _lib.Search(size=C.sizeof(_lib.Search), split=_lib.SPLIT_ONE if one else _lib.SPLIT_PER_START if split_times is not None else _lib.SPLIT_FITTED,
                        split_time=float(split_time) if one else 0.0, starts=ptr(st), xatol=float(xatol), fatol=float(fatol), x=ptr(x), llh=ptr(llh),
                        **fields)
        if hops is None:
            q.maxiter = int(maxiter if maxiter is not None else 1000)
            q.nit, q.nfev, q.status = (ptr(a) for a in counters.values())
        else:
            h = {k: v for k, v in hops.items() if v is not None}
            uni = draw_uniforms(rngs, S, max(int(h.get("niter", 100)), 0), N)          # (a negative niter is the library's to refuse)
            q.maxiter = int(maxiter if maxiter is not None else 200 * N)
            hop = _lib.Hops(niter=int(h.get("niter", 100)), T=float(h.get("T", 0.5)), stepsize=float(h.get("stepsize", 0.5)),
                            interval=int(h.get("interval", 50)), target_accept_rate=float(h.get("target_accept_rate", 0.5)),
                            stepwise_factor=float(h.get("stepwise_factor", 0.9)), nm_maxfev=int(h.get("nm_maxfev", 200 * N)), uniforms=ptr(uni))
            hop.nfev, hop.failures, hop.accepted = (ptr(a) for a in counters.values())
            q.hops = C.pointer(hop)
        _lib.check(self._lib.misti_search(self._ctx, C.byref(q)))
        return dict(x=x, llh=llh, **counters, **self._nm_stats())

    def nm_solve(self, starts, split_time, jsfs_row, tol=1e-4, maxiter=1000):
        """``misti_nm_solve``: SciPy-exact Nelder-Mead from every row of ``starts`` with the simplices resident in
        HBM (``MigrationInference.Solve`` for many starts; reference semantics :718-733).
        Returns dict(x[S][P], llh[S], nit[S], nfev[S], status[S]) - status 0 converged, 2 iteration budget."""
        return self.search(starts, jsfs_row, split_time=split_time, xatol=tol, fatol=tol, maxiter=maxiter)

    def nm_solve_rows(self, starts, split_times, rows, jsfs, tol=1e-4, maxiter=1000):
        """``misti_nm_solve_rows``: ``nm_solve`` with a split time and a replicate row PER START - start s is SciPy's
        Nelder-Mead at ``split_times[s]`` against ``jsfs[rows[s]]``, all starts in one batched search (the bootstrap profiles of
        the reference's ``test.bs`` scripts, one ``Solve`` per (replicate, split) pair there).  ``jsfs`` is ``[n_rep][8]``.
        Returns what ``nm_solve`` returns; start s equals ``nm_solve(starts[s], split_times[s], jsfs[rows[s]])`` bit for bit."""
        return self.search(starts, jsfs, split_times=split_times, rows=rows, xatol=tol, fatol=tol, maxiter=maxiter)

    def nm_solve_bounds(self, starts, split_times, rows, jsfs, band_bounds, tol=1e-4, maxiter=1000):
        """``misti_nm_solve_bounds``: ``nm_solve_rows`` with the band bounds PER START as well - start s is SciPy's Nelder-Mead at
        ``split_times[s]`` against ``jsfs[rows[s]]`` with the model's bands starting and ending at ``band_bounds[s]``
        (``[n_start][n_band][2]`` ints, ``end == -1``: the start's split index), all starts in one batched search (the boundary
        profiles "when did migration start or stop": one ``Engine`` per bound set and one ``Solve`` per model otherwise).  Bounds
        that break SetModel's checks give that start ``llh = -inf``.  ``band_bounds=None`` is ``nm_solve_rows``.
        Returns what ``nm_solve`` returns; start s equals ``nm_solve(starts[s], split_times[s], jsfs[rows[s]])`` on an engine whose
        bands carry ``band_bounds[s]``, bit for bit."""
        return self.search(starts, jsfs, split_times=split_times, rows=rows, band_bounds=band_bounds, xatol=tol, fatol=tol, maxiter=maxiter)

    def nm_solve_pulses(self, starts, split_times, rows, jsfs, band_bounds, pulse_times, tol=1e-4, maxiter=1000):
        """``misti_nm_solve_pulses``: ``nm_solve_bounds`` with the pulse times PER START as well (``[n_start][n_pulse]`` ints, on
        the start's own grid) - the pulse-date profile with an optimised fraction, ``-pu 2 {t} f 1`` under a loop over t, in one
        batched search.  Times that break SetModel's checks give that start ``llh = -inf``.  ``pulse_times=None`` is
        ``nm_solve_bounds``.
        Returns what ``nm_solve`` returns; start s equals ``nm_solve(starts[s], split_times[s], jsfs[rows[s]])`` on an engine whose
        model carries ``band_bounds[s]`` and ``pulse_times[s]``, bit for bit."""
        return self.search(starts, jsfs, split_times=split_times, rows=rows, band_bounds=band_bounds, pulse_times=pulse_times,
                           xatol=tol, fatol=tol, maxiter=maxiter)

    def nm_solve_split(self, starts, rows, table, band_bounds=None, pulse_times=None, tol=1e-4, maxiter=1000):
        """``misti_nm_solve_split``: the split time as the LAST coordinate of every simplex - ``starts`` is ``[S][n_param + 1]``
        (initial parameters, then the initial split), start s is SciPy's Nelder-Mead over (parameters, split) against
        ``table[rows[s]]`` (``[n_rep][8]``), all starts in one batched search.  Replaces the ``for st in A..Z`` scans of the
        reference's ``test.bs`` scripts with a fitted, fractional split, and gives a model without an optimised parameter
        (``n_param == 0``) its only search.  ``band_bounds`` / ``pulse_times`` per start as in ``nm_solve_pulses`` (band end -1: the
        point's own split index).  A point whose split the engine refuses scores +inf; a start without any value has ``llh = -inf``.
        Returns what ``nm_solve`` returns with ``x[S][n_param + 1]``, plus ``split`` (= ``x[:, -1]``)."""
        return self.nm_solve_box(starts, rows, table, None, None, band_bounds, pulse_times, tol, maxiter)

    def nm_solve_box(self, starts, rows, table, box, split_times=None, band_bounds=None, pulse_times=None, tol=1e-4, maxiter=1000):
        """``misti_nm_solve_box``: the batched search with box constraints - start s is ``scipy.optimize.minimize(f, starts[s],
        method='Nelder-Mead', bounds=Bounds(lo, hi))`` on the engine's objective, bit for bit.  ``box`` is ``(lo, hi)``, each ``[N]`` (one
        box for every start) or ``[S][N]`` (a box per start); ``-inf`` / ``inf`` leave a side open, ``lo == hi`` holds a coordinate fixed, a
        start outside its box is clipped.  ``split_times=None``: the split is the LAST coordinate, ``starts`` is ``[S][n_param + 1]``
        (``nm_solve_split``'s search, the split clipped like any other coordinate); ``split_times`` given: a split per start,
        ``starts`` is ``[S][n_param]`` (``nm_solve_pulses``' search).  ``optimize.box_initial_simplex`` / ``box_clip`` state the rule.
        Returns what ``nm_solve_split`` returns (``split``: the fitted splits, or ``split_times`` themselves)."""
        r = self.search(starts, table, split_times=split_times, rows=rows, band_bounds=band_bounds, pulse_times=pulse_times, box=box,
                        xatol=tol, fatol=tol, maxiter=maxiter)
        r["split"] = r["x"][:, -1].copy() if split_times is None else np.array(split_times, dtype=np.float64).reshape(-1)
        return r

    def basinhopping(self, starts, split_time, jsfs_row, rngs, niter=100, T=0.5, stepsize=0.5, interval=50, target_accept_rate=0.5,
                     stepwise_factor=0.9, xatol=1e-4, fatol=1e-4, nm_maxiter=None, nm_maxfev=None):
        """``misti_basinhopping``: ``scipy.optimize.basinhopping(-JAFSLikelihood, x0, niter, T, stepsize,
        minimizer_kwargs=dict(method='Nelder-Mead'), rng=rngs[s])`` from every row of ``starts`` at once - the reference's
        ``Solve(globalOpt=True)`` (``/root/reference/MigrationInference.py:723-725``, T = 0.5) for many starts.
        ``rngs``: one ``numpy.random.Generator`` per start (or one seed per start): the uniforms SciPy would draw from it
        (per hop ``n_param`` for the displacement, one for the Metropolis test) are drawn here, up front.
        Returns dict(x[S][P], llh[S], nfev[S], failures[S], accepted[S])."""
        r = self.search(starts, jsfs_row, split_time=split_time, rngs=rngs, xatol=xatol, fatol=fatol, maxiter=nm_maxiter,
                        hops=dict(niter=niter, T=T, stepsize=stepsize, interval=interval, target_accept_rate=target_accept_rate,
                                  stepwise_factor=stepwise_factor, nm_maxfev=nm_maxfev))
        del r["speculative_iterations"]
        return r

    def basinhopping_rows(self, starts, split_times, rows, table, rngs, band_bounds=None, pulse_times=None, niter=100, T=0.5, stepsize=0.5,
                          interval=50, target_accept_rate=0.5, stepwise_factor=0.9, xatol=1e-4, fatol=1e-4, nm_maxiter=None, nm_maxfev=None):
        """``misti_basinhopping_rows``: ``basinhopping`` with a split time and a replicate row PER START - start s is SciPy's
        ``basinhopping`` around Nelder-Mead at ``split_times[s]`` against ``table[rows[s]]`` (``[n_rep][8]``), with the model's bands at
        ``band_bounds[s]`` (``[S][n_band][2]``) and its pulses at ``pulse_times[s]`` (``[S][n_pulse]``) where given - the reference's
        ``Solve(globalOpt=True)`` for every (row, split) pair of its ``test.bs`` workflow in one call.  ``rngs`` as ``basinhopping``;
        ``nm_maxiter`` and ``nm_maxfev`` default to ``200 x n_param``.  A start the engine refuses throughout has ``llh = -inf``.
        Returns what ``basinhopping`` returns plus ``speculative_iterations``; start s equals
        ``basinhopping(starts[s:s+1], split_times[s], table[rows[s]], [rngs[s]])`` on an engine whose model carries ``band_bounds[s]`` and
        ``pulse_times[s]``, bit for bit."""
        return self.search(starts, table, split_times=split_times, rows=rows, band_bounds=band_bounds, pulse_times=pulse_times, rngs=rngs,
                           xatol=xatol, fatol=fatol, maxiter=nm_maxiter,
                           hops=dict(niter=niter, T=T, stepsize=stepsize, interval=interval, target_accept_rate=target_accept_rate,
                                     stepwise_factor=stepwise_factor, nm_maxfev=nm_maxfev))

    def basinhopping_split(self, starts, rows, table, rngs, band_bounds=None, pulse_times=None, niter=100, T=0.5, stepsize=0.5, interval=50,
                           target_accept_rate=0.5, stepwise_factor=0.9, xatol=1e-4, fatol=1e-4, nm_maxiter=None, nm_maxfev=None):
        """``misti_basinhopping_split``: basin hopping with the split time as the LAST coordinate - ``starts`` is ``[S][n_param + 1]``,
        start s is ``scipy.optimize.basinhopping`` around Nelder-Mead over (parameters, split) against ``table[rows[s]]``; the random
        displacement moves the split like any other coordinate (one ``stepsize``, the split in grid-index units), so the uniforms are
        drawn for ``n_param + 1`` coordinates, and ``nm_maxiter`` / ``nm_maxfev`` default to ``200 x (n_param + 1)``.  The global
        counterpart of ``nm_solve_split`` on its piecewise objective, and the global search of a model without an optimised
        parameter.  ``band_bounds`` / ``pulse_times`` per start as in ``nm_solve_split``.
        Returns what ``basinhopping_rows`` returns with ``x[S][n_param + 1]``, plus ``split`` (= ``x[:, -1]``)."""
        return self.basinhopping_box(starts, rows, table, rngs, None, None, band_bounds, pulse_times, niter, T, stepsize, interval,
                                     target_accept_rate, stepwise_factor, xatol, fatol, nm_maxiter, nm_maxfev)

    def basinhopping_box(self, starts, rows, table, rngs, box, split_times=None, band_bounds=None, pulse_times=None, niter=100, T=0.5,
                         stepsize=0.5, interval=50, target_accept_rate=0.5, stepwise_factor=0.9, xatol=1e-4, fatol=1e-4, nm_maxiter=None,
                         nm_maxfev=None):
        """``misti_basinhopping_box``: basin hopping around the boxed search - start s is ``scipy.optimize.basinhopping(...,
        minimizer_kwargs=dict(method='Nelder-Mead', bounds=Bounds(lo, hi)))``.  ``box`` and ``split_times`` as in ``nm_solve_box``; the
        displacement is not clipped (SciPy's is not), the minimisation from the trial point clips it.  The other arguments as
        ``basinhopping_split`` / ``basinhopping_rows``.  Returns what ``basinhopping_split`` returns."""
        r = self.search(starts, table, split_times=split_times, rows=rows, band_bounds=band_bounds, pulse_times=pulse_times, box=box,
                        rngs=rngs, xatol=xatol, fatol=fatol, maxiter=nm_maxiter,
                        hops=dict(niter=niter, T=T, stepsize=stepsize, interval=interval, target_accept_rate=target_accept_rate,
                                  stepwise_factor=stepwise_factor, nm_maxfev=nm_maxfev))
        r["split"] = r["x"][:, -1].copy() if split_times is None else np.array(split_times, dtype=np.float64).reshape(-1)
        return r

    def differential_evolution(self, starts, rows, jsfs, box, split_times=None, fit_split=False, band_bounds=None, pulse_times=None, pop=16,
                               maxiter=50, tol=0.01, atol=0.0, F=(0.5, 1.0), CR=0.7, seed=0, ids=None, return_population=False):
        """``misti_de_search``: differential evolution per search - search s is a population of ``pop`` members inside its finite ``box``
        (``(lo, hi)``, each ``[N]`` or ``[S][N]``; ``lo == hi`` holds a coordinate fixed) against ``jsfs[rows[s]]`` (``[n_rep][8]``), member
        0 its row of ``starts``; every generation of all searches is ONE engine batch.  The rule is the project's own, not SciPy's
        (``optimize.differential_evolution_rule`` states it; the result equals it bit for bit): best1bin, dither ``F = (lo, hi)``,
        crossover ``CR``, deferred selection, stop at ``std(f) <= atol + tol |mean(f)|`` or after ``maxiter`` generations.  Exactly one of
        ``split_times`` (``[S]``, ``starts`` is ``[S][n_param]``) and ``fit_split=True`` (the split is the LAST coordinate, ``starts`` is
        ``[S][n_param + 1]``).  Everything random is ``numpy.random.Philox(key=[seed, ids[s]])`` (``ids`` default ``0 ... S - 1``): a
        search's result depends on its own arguments alone.  ``band_bounds`` / ``pulse_times`` per search as in ``nm_solve_pulses``.
        Returns dict(x[S][N], llh[S], nit / nfev / status[S] (0 converged, 2 generation budget), split[S], n_points (points the call handed
        the engine), the work counters ``iterations_issued`` / ``slots`` and, with ``return_population``, population[S][pop][N] and
        population_llh[S][pop])."""
        if (split_times is None) != bool(fit_split):
            raise ValueError("differential_evolution: give exactly one of split_times and fit_split=True")
        N = self.n_param + (1 if fit_split else 0)
        st = _f64(starts, (-1, N))
        S, P = st.shape[0], int(pop)
        ptr = lambda a: a.ctypes.data if a is not None else None
        arrays, fields = self._rows_problem(S, N, _f64(jsfs, (-1, 8)), split_times, rows, band_bounds, pulse_times, box, ids)
        x, llh = np.empty((S, N)), np.empty(S)
        nit, nfev, status = (np.empty(S, dtype=np.int32) for _ in range(3))
        keep = return_population and 4 <= P <= _lib.DE_MAX_POP
        popx, popl = (np.empty((S, P, N)), np.empty((S, P))) if keep else (None, None)
        n_points = np.zeros(1, dtype=np.int64)
        q = _lib.DeSearch(size=C.sizeof(_lib.DeSearch), split=_lib.SPLIT_FITTED if fit_split else _lib.SPLIT_PER_START, starts=ptr(st),
                          pop=P, maxiter=int(maxiter), tol=float(tol), atol=float(atol), F_lo=float(F[0]), F_hi=float(F[1]), CR=float(CR),
                          seed=int(seed), x=ptr(x), llh=ptr(llh), nit=ptr(nit), nfev=ptr(nfev), status=ptr(status), population=ptr(popx),
                          population_llh=ptr(popl), n_points=ptr(n_points), **fields)
        _lib.check(self._lib.misti_de_search(self._ctx, C.byref(q)))
        stats = self._nm_stats()
        out = dict(x=x, llh=llh, nit=nit, nfev=nfev, status=status, n_points=int(n_points[0]),
                   split=x[:, -1].copy() if fit_split else arrays["split_times"].copy(), iterations_issued=stats["iterations_issued"], slots=stats["slots"])
        if return_population:
            out.update(population=popx, population_llh=popl)
        return out

    @staticmethod
    def _prior(prior, S, N, who):
        """``misti_prior_t`` of ``prior`` (dict(scale, kind, p0, p1), each ``[N]`` or ``[S][N]``; ``optimize.prior_spec``): the
        descriptor and the arrays it points into (to be kept alive until the call returns)."""
        try:
            scale, kind = (np.ascontiguousarray(np.asarray(prior[k]), dtype=np.int32) for k in ("scale", "kind"))
            p0, p1 = (_f64(prior[k]) for k in ("p0", "p1"))
        except (KeyError, TypeError):
            raise ValueError("%s: a prior is dict(scale, kind, p0, p1)" % who)
        if any(v.shape != scale.shape for v in (kind, p0, p1)) or scale.shape not in ((N,), (S, N)):
            raise ValueError("%s: the prior's arrays must all be [%d] or [%d][%d] (got %s)" % (who, N, S, N, scale.shape))
        keep = (scale, kind, p0, p1)
        return _lib.Prior(size=C.sizeof(_lib.Prior), n_prior=1 if scale.ndim == 1 else S, scale=scale.ctypes.data, kind=kind.ctypes.data,
                          p0=p0.ctypes.data, p1=p1.ctypes.data), keep

    def ensemble_sample(self, init, rows, table, box, split_times=None, fit_split=False, band_bounds=None, pulse_times=None, n_step=100,
                        thin=1, temperature=1.0, a=2.0, seed=0, ids=None, prior=None, joint=None):
        """``misti_ensemble_sample``: ensemble MCMC per search - search s is an ensemble of W walkers ``init[s]`` (``[S][W][N]``, W even,
        every walker inside its box) against ``table[rows[s]]`` (``[n_rep][8]``), sampling ``llk / temperature`` under a uniform prior on
        its finite ``box`` (``(lo, hi)``, each ``[N]`` or ``[S][N]``; ``lo == hi`` holds a coordinate fixed); every half-step of all
        searches is ONE engine batch.  The stretch move of Goodman & Weare with scale ``a``; the rule is the project's own
        (``optimize.ensemble_rule`` states it; the result equals it bit for bit).  Exactly one of ``split_times`` (``[S]``, N =
        ``n_param``) and ``fit_split=True`` (the split is the LAST coordinate).  ``temperature``: a scalar or ``[S]``.  Everything random
        is ``numpy.random.Philox(key=[seed, ids[s]])`` (``ids`` default ``0 ... S - 1``): a search's result depends on its own arguments
        alone; a later call continues from ``last`` with other ids.  ``band_bounds`` / ``pulse_times`` per search as in ``nm_solve_pulses``.
        Returns dict(chain[S][n_keep][W][N], chain_llh[S][n_keep][W] (the ensembles after steps thin, 2 thin, ...), accepted[S][W],
        last[S][W][N], last_llh[S][W], n_points (proposals the call handed the engine; those that leave the box are rejected without an
        evaluation and not counted, nor are the S W initial evaluations)).
        ``prior`` (None, or dict(scale, kind, p0, p1), each ``[N]`` or ``[S][N]``: ``optimize.prior_spec``): a sampling coordinate (the
        engine's value or its logarithm) and a prior density per coordinate - ``misti_ensemble_sample_prior``, the rule is
        ``optimize.ensemble_prior_rule``.  ``init``, ``box``, ``chain`` and ``last`` are then in SAMPLING coordinates
        (``optimize.to_sampling`` / ``from_sampling``); the engine is handed their natural image.
        ``joint`` (None, or dict(pairs, bins=32, range=None, masses=(0.95,), burn=0, want=None)): the joint regions of coordinate
        pairs of ``ensemble_joint_dev``, reduced on the device from the kept chain - ``misti_ensemble_sample_joint``, the rule is
        ``optimize.ensemble_joint_rule`` -, under ``r["joint"]``; ``range="box"`` takes each window from the search box (finite sides
        only).  The other outputs keep their bits."""
        return self._sampler("ensemble_sample", False, None, True, init, rows, table, box, temperature, split_times, fit_split, band_bounds,
                             pulse_times, n_step, thin, 0, 0, a, seed, ids, prior, joint)

    _POST_OUTPUTS = ("mean", "cov", "quant", "tau", "window", "best_llh", "best_x", "best_at")
    _POST_SORTED = ("hpd", "hpd_at", "order")              # what needs the sorted marginals: only on request

    @staticmethod
    def _post(S, N, K, burn, probs, max_lag, c, empty=None, want=None, masses=None, W=1):
        """``misti_ens_post_t`` for the chains of S searches, N coordinates, K kept steps and W walkers, and the outputs of ``want`` it
        points into (None: the eight summaries, and ``hpd`` / ``hpd_at`` where ``masses`` are given; ``order`` only by name).
        ``max_lag`` None: every lag.  ``masses`` None: no shortest interval.  ``empty(shape, integer)`` allocates one output and
        returns it with its address (default: NumPy, on the host).  Returns (descriptor, outputs, what must stay alive until the call
        returns)."""
        probs = _f64(probs).reshape(-1)
        masses = _f64(() if masses is None else masses).reshape(-1)
        if want is None:
            want = Engine._POST_OUTPUTS + (("hpd", "hpd_at") if masses.size else ())
        P, M, burn = probs.size, masses.size, int(burn)
        max_lag = max(K - burn - 1, 0) if max_lag is None else int(max_lag)
        shapes = dict(mean=(S, N), cov=(S, N, N), quant=(S, N, P), tau=(S, N), window=(S, N), best_llh=(S,), best_x=(S, N), best_at=(S, 2),
                      hpd=(S, N, M, 2), hpd_at=(S, N, M), order=(S, N, max(K - burn, 0) * int(W)))
        if empty is None:
            def empty(shape, integer):
                v = np.empty(shape, dtype=np.int32 if integer else np.float64)
                return v, v.ctypes.data
        made = {k: empty(shapes[k], k in ("window", "best_at", "hpd_at")) for k in Engine._POST_OUTPUTS + Engine._POST_SORTED if k in want}
        p = _lib.EnsPost(size=C.sizeof(_lib.EnsPost), burn=burn, n_prob=P, probs=probs.ctypes.data, max_lag=min(max_lag, 2 ** 31 - 1), c=float(c),
                         n_mass=M, masses=masses.ctypes.data if M else None, **{k: at or None for k, (_, at) in made.items()})
        return p, {k: v for k, (v, _) in made.items()}, (probs, masses)

    _JOINT_OUTPUTS = ("counts", "range", "inside", "mode", "level", "cells", "held")

    @staticmethod
    def _joint(S, N, pairs, bins=32, burn=0, range=None, masses=(0.95,), want=None, empty=None, box=None, address=None):
        """``misti_ens_joint_t`` for the chains of S searches and N coordinates, and the outputs of ``want`` it points into (None:
        all of counts, range, inside, mode, and level, cells, held where ``masses`` are given).  ``range``: None (taken from the
        data), ``"box"`` (the search box ``box`` = ``(lo, hi)`` in sampling coordinates; an infinite side is refused) or what
        broadcasts to ``[S][n_pair][2][2]``; ``address(range)`` turns it into the pointer the door reads (default: NumPy, on the
        host).  ``empty(shape, integer)`` as in ``_post``.  Returns (descriptor, outputs, what must stay alive until the call returns)."""
        from .optimize import joint_pairs
        pr, bn, off = joint_pairs(pairs, bins, N)
        P = pr.shape[0]
        ms = _f64(() if masses is None else masses).reshape(-1)
        if want is None:
            want = ("counts", "range", "inside", "mode") + (("level", "cells", "held") if ms.size else ())
        unknown = [k for k in want if k not in Engine._JOINT_OUTPUTS]
        if unknown:
            raise ValueError("joint: unknown outputs %s (there are %s)" % (unknown, ", ".join(Engine._JOINT_OUTPUTS)))
        if isinstance(range, str):
            if range != "box" or box is None:
                raise ValueError("joint: range is None, \"box\" (where the call has a box) or [S][n_pair][2][2]")
            lo, hi = _box_arrays(box, N)
            if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
                raise ValueError("joint: range=\"box\" needs a finite box")
            lo, hi = (np.broadcast_to(v, (S, N)) for v in (lo, hi))
            range = np.stack([lo[:, pr], hi[:, pr]], axis=-1)                  # [S][n_pair][2 axes][lo, hi]
        rg_at = None
        if range is not None:
            if address is None:
                range = np.ascontiguousarray(np.broadcast_to(_f64(range), (S, P, 2, 2)))
                rg_at = range.ctypes.data
            else:
                range, rg_at = address(range, (S, P, 2, 2))
        if empty is None:
            def empty(shape, integer):
                v = np.empty(shape, dtype=np.int32 if integer else np.float64)
                return v, v.ctypes.data
        M = ms.size
        shapes = dict(counts=(S, int(off[-1])), range=(S, P, 2, 2), inside=(S, P), mode=(S, P, 2), level=(S, P, M), cells=(S, P, M), held=(S, P, M))
        made = {k: empty(shapes[k], k != "range") for k in Engine._JOINT_OUTPUTS if k in want}
        at = {("range_out" if k == "range" else k): a or None for k, (_, a) in made.items()}
        j = _lib.EnsJoint(size=C.sizeof(_lib.EnsJoint), burn=int(burn), n_pair=P, pairs=pr.ctypes.data, bins=bn.ctypes.data, range=rg_at or None,
                          n_mass=M, masses=ms.ctypes.data if M else None, **at)
        out = {k: v for k, (v, _) in made.items()}
        out.update(pairs=pr, bins=bn, offsets=off, masses=ms)
        return j, out, (pr, bn, ms, range)

    def ensemble_joint_dev(self, chain, pairs, bins=32, burn=0, range=None, masses=(0.95,), want=None):
        """``misti_ens_joint_dev``: joint regions of coordinate pairs of a chain that is already on the device - ``chain`` a contiguous
        float64 torch tensor ``[S][K][W][N]`` on this engine's device.  Per search and pair ``(a, b)`` of ``pairs`` (``[n_pair][2]``)
        a histogram of ``bins`` (a scalar, ``(Ba, Bb)`` or ``[n_pair][2]``; each 1 ... 128) cells over the kept steps ``burn ... K -
        1``, inside the window ``range`` (None: the finite extremes of the data; else a torch tensor on the device or an array that
        broadcasts to ``[S][n_pair][2][2]``), its mode, and per mass the count level whose cells enclose it.  Asynchronous on the
        engine's stream; the rule is ``optimize.ensemble_joint_rule``, bit for bit, in the SAMPLING coordinate.  ``want``: the outputs
        to compute among counts, range, inside, mode, level, cells, held (default: all; the last three need ``masses``); one that is
        left out is not computed and the others' bits do not change.  Returns a dict of int32 torch tensors on the device
        (``counts[S][sum_q Ba Bb]`` packed as ``offsets`` says - ``optimize.joint_counts`` -, ``range`` float64), with pairs, bins,
        offsets and masses (NumPy) as they were read."""
        import torch
        want = None if want is None else tuple(want)
        if chain.dim() != 4 or chain.dtype != torch.float64 or not chain.is_contiguous():
            raise ValueError("ensemble_joint_dev: chain must be a contiguous float64 tensor [S][K][W][N]")
        S, K, W, N = chain.shape
        def empty(shape, integer):
            v = torch.empty(shape, dtype=torch.int32 if integer else torch.float64, device=chain.device)
            return v, v.data_ptr()
        def address(r, shape):
            r = torch.as_tensor(r, dtype=torch.float64).to(chain.device).broadcast_to(shape).contiguous()
            return r, r.data_ptr()
        if isinstance(range, str):
            raise ValueError("ensemble_joint_dev: a chain has no box; give the ranges themselves")
        j, out, keep = self._joint(S, N, pairs, bins, burn, range, masses, want, empty, None, address)
        _lib.check(self._lib.misti_ens_joint_dev(self._ctx, S, K, W, N, C.c_void_p(chain.data_ptr()) if chain.data_ptr() else None, C.byref(j)))
        return out

    def _sampler(self, who, tempered, post, keep_chain, init, rows, table, box, temps, split_times, fit_split, band_bounds, pulse_times, n_step,
                 thin, swap_every, burn, a, seed, ids, prior, joint=None):
        """One marshalling for the two sampler descriptors - the rows problem, the outputs, the summaries and the prior - and the call.
        ``tempered`` False: ``misti_ens_t``, ``init`` is ``[S][W][N]`` and ``temps`` the temperature (a scalar or ``[S]``); True:
        ``misti_pt_t``, ``init`` is ``[S][L][W][N]`` and ``temps`` the ladder.  ``post``: None or dict(burn, probs, max_lag, c, masses, want).
        ``joint``: None or dict(pairs, bins, range, masses, burn, want) - the regions of ``_joint`` through ``misti_*_sample_joint``;
        None takes the older entries.
        Returns the door's outputs in the descriptor's order (the coordinate chain only with ``keep_chain``; the plain door's value
        chain too), then the summaries, then ``joint`` (a dict of its own), then ``n_points``."""
        if (split_times is None) != bool(fit_split):
            raise ValueError("%s: give exactly one of split_times and fit_split=True" % who)
        N = self.n_param + (1 if fit_split else 0)
        x0 = _f64(init)
        dims = "[S][L][W]" if tempered else "[S][W]"
        if x0.ndim != (4 if tempered else 3) or x0.shape[-1] != N:
            raise ValueError("%s: init must be %s[%d] (got %s)" % (who, dims, N, x0.shape))
        S, W, rung = x0.shape[0], x0.shape[-2], x0.shape[1:-2]              # rung: (L,) | ()
        T = _f64(temps)
        if tempered and T.shape not in (rung, (S,) + rung):
            raise ValueError("%s: the ladder must be [%d] or [%d][%d] (got %s)" % (who, rung[0], S, rung[0], T.shape))
        n_step, thin = int(n_step), int(thin)
        ptr = lambda v: v.ctypes.data if v is not None else None
        arrays, fields = self._rows_problem(S, N, _f64(table, (-1, 8)), split_times, rows, band_bounds, pulse_times, box, ids)
        K = n_step // thin if thin >= 1 and n_step >= 0 else 0
        out = dict(chain=np.empty((S, K, W, N)) if keep_chain else None, chain_llh=np.empty((S,) + rung + (K, W)) if keep_chain or tempered else None,
                   accepted=np.zeros((S,) + rung + (W,), dtype=np.int32))
        if tempered:
            out.update(swap_proposed=np.zeros((S, max(rung[0] - 1, 0)), dtype=np.int32), swap_accepted=np.zeros((S, max(rung[0] - 1, 0)), dtype=np.int32))
        out.update(last=np.empty((S,) + rung + (W, N)), last_llh=np.empty((S,) + rung + (W,)))
        if tempered:
            out.update(rung_llh=np.empty((S,) + rung), logz=np.empty(S))
        n_points = np.zeros(1, dtype=np.int64)
        common = dict(split=_lib.SPLIT_FITTED if fit_split else _lib.SPLIT_PER_START, init=ptr(x0), walkers=W, n_step=n_step, thin=thin, a=float(a),
                      seed=int(seed), n_points=ptr(n_points), **{k: ptr(v) for k, v in out.items()}, **fields)
        if tempered:
            q = _lib.PtSample(size=C.sizeof(_lib.PtSample), n_rung=rung[0], n_ladder=1 if T.ndim == 1 else S, ladder=ptr(T), swap_every=int(swap_every),
                              burn=int(burn), **common)
        else:
            T = T.reshape(-1)
            q = _lib.EnsSample(size=C.sizeof(_lib.EnsSample), n_temp=T.size, temperature=ptr(T), **common)
        p, s, p_keep = self._post(S, N, K, W=W, **post) if post is not None else (None, {}, None)
        pr, pr_keep = self._prior(prior, S, N, who) if prior is not None else (None, None)
        ref = lambda d: C.byref(d) if d is not None else None
        jd, jout = None, None
        if joint is not None:
            try:
                opts = dict(joint)
                jd, jout, j_keep = self._joint(S, N, opts.pop("pairs"), box=box, **opts)
            except (KeyError, TypeError):
                raise ValueError("%s: joint is dict(pairs, bins, range, masses, burn, want)" % who)
        if jd is not None:
            door = self._lib.misti_tempered_sample_joint if tempered else self._lib.misti_ensemble_sample_joint
            rc = door(self._ctx, C.byref(q), ref(p), ref(pr), C.byref(jd))
        elif pr is not None:
            door = self._lib.misti_tempered_sample_prior if tempered else self._lib.misti_ensemble_sample_prior
            rc = door(self._ctx, C.byref(q), ref(p), C.byref(pr))
        elif tempered:
            rc = self._lib.misti_tempered_sample(self._ctx, C.byref(q), ref(p))
        elif p is not None:
            rc = self._lib.misti_ensemble_posterior(self._ctx, C.byref(q), C.byref(p))
        else:
            rc = self._lib.misti_ensemble_sample(self._ctx, C.byref(q))
        _lib.check(rc)
        return dict({k: v for k, v in out.items() if v is not None}, **s, **({"joint": jout} if jout is not None else {}), n_points=int(n_points[0]))

    def ensemble_posterior(self, init, rows, table, box, split_times=None, fit_split=False, band_bounds=None, pulse_times=None, n_step=100,
                           thin=1, temperature=1.0, a=2.0, seed=0, ids=None, burn=0, probs=(0.025, 0.5, 0.975), max_lag=None, keep_chain=False, c=5.0,
                           prior=None, masses=None, want=None, joint=None):
        """``misti_ensemble_posterior``: ``ensemble_sample`` on the same arguments - the same kernels, stream and bits - followed by the
        posterior summaries of its chain, reduced per search ON THE DEVICE: without ``keep_chain`` the chain never leaves it.  The rule is
        ``optimize.ensemble_posterior_rule`` on the kept steps ``burn ... n_keep - 1`` (n of them), bit for bit: ``probs`` (1 ... 8
        probabilities in [0, 1]) give exact order statistics interpolated, ``max_lag`` caps the lags of the autocorrelation (None:
        ``n - 1``, every lag), ``c`` is Sokal's window constant.
        Returns dict(mean[S][N], cov[S][N][N], quant[S][N][len(probs)], tau[S][N] (in kept steps), window[S][N] (-1: no lag up to the
        cap closed the window), best_llh[S], best_x[S][N], best_at[S][2] ((kept step - burn, walker); (-1, -1): no sample has a value),
        accepted, last, last_llh, n_points as ``ensemble_sample``), and chain, chain_llh with ``keep_chain``.  ``prior`` as in
        ``ensemble_sample``: the summaries are then those of the chain in SAMPLING coordinates (``optimize.posterior_table`` reports
        quantiles and the best sample in natural units too).
        ``masses`` (None, or 1 ... 8 masses in (0, 1]): the SHORTEST (HPD) interval of each mass per coordinate, from a full sort of
        every marginal on the device (``optimize.ensemble_hpd_rule``, bit for bit) - ``hpd[S][N][len(masses)][2]`` and
        ``hpd_at[S][N][len(masses)]`` (the rank of the lower end) join the result; shortest in the SAMPLING coordinate, HPD is not
        invariant under the log map.  ``want``: the summaries to compute, by name (default: the eight above, and hpd, hpd_at with
        ``masses``); ``"order"`` adds the sorted marginals ``order[S][N][n W]`` themselves.
        ``joint`` as in ``ensemble_sample`` (its ``burn`` defaults to this call's): ``r["joint"]``, without the chain leaving the device."""
        if joint is not None:
            joint = dict(joint, burn=dict(joint).get("burn", burn))
        r = self._sampler("ensemble_posterior", False, dict(burn=burn, probs=probs, max_lag=max_lag, c=c, masses=masses, want=want), bool(keep_chain), init, rows, table, box,
                          temperature, split_times, fit_split, band_bounds, pulse_times, n_step, thin, 0, 0, a, seed, ids, prior, joint)
        for k in ("chain", "chain_llh") if keep_chain else ():             # this door's order: the chain behind the summaries
            r[k] = r.pop(k)
        r["n_points"] = r.pop("n_points")
        return r

    def tempered_sample(self, init, rows, table, box, ladder, split_times=None, fit_split=False, band_bounds=None, pulse_times=None, n_step=100,
                        thin=1, swap_every=1, burn=0, a=2.0, seed=0, ids=None, post=None, prior=None, joint=None):
        """``misti_tempered_sample``: parallel tempering over ``ensemble_sample`` - fit s is a ladder of L ensembles ``init[s]``
        (``[S][L][W][N]``) at the temperatures ``ladder`` (``[L]`` or ``[S][L]``, strictly increasing); rung l samples ``llk / T_l``,
        neighbouring rungs trade walkers every ``swap_every`` steps (0: never), the cold rung carries the posterior, and all rungs of all
        fits move in the same engine batch.  The rule is ``optimize.tempered_rule``, bit for bit; L = 1 is ``ensemble_sample``.  The other
        arguments as in ``ensemble_sample``; ``burn``: kept steps dropped before ``rung_llh`` / ``logz``.  ``post``: None, or a dict of
        ``burn`` (default: this call's), ``probs``, ``max_lag``, ``c``, ``masses``, ``want`` and ``keep_chain`` (default False) - the summaries of
        ``ensemble_posterior`` reduced on the device from the cold chain, which then comes back only with ``keep_chain``.
        Returns dict(chain[S][K][W][N] (the cold rung), chain_llh[S][L][K][W], accepted[S][L][W], swap_proposed[S][L-1],
        swap_accepted[S][L-1], last[S][L][W][N], last_llh[S][L][W], rung_llh[S][L], logz[S] (see ``optimize.tempered_rule`` for what it
        is and is not), n_points), plus the summaries with ``post``.  ``prior`` as in ``ensemble_sample`` (one per fit): every rung
        targets ``prior(y) exp(llk / T_l)`` - ``misti_tempered_sample_prior``, the rule is ``optimize.tempered_prior_rule``.
        ``joint`` as in ``ensemble_sample`` (its ``burn`` defaults to this call's), on the cold chain - ``misti_tempered_sample_joint``."""
        if joint is not None:
            joint = dict(joint, burn=dict(joint).get("burn", burn))
        opts = dict(post) if post is not None else None
        keep_chain = opts is None or bool(opts.pop("keep_chain", False))
        if opts is not None:
            opts = dict(burn=opts.get("burn", burn), probs=opts.get("probs", (0.025, 0.5, 0.975)), max_lag=opts.get("max_lag"), c=opts.get("c", 5.0),
                        masses=opts.get("masses"), want=opts.get("want"))
        return self._sampler("tempered_sample", True, opts, keep_chain, init, rows, table, box, ladder, split_times, fit_split, band_bounds,
                             pulse_times, n_step, thin, swap_every, burn, a, seed, ids, prior, joint)

    def ensemble_summary_dev(self, chain, chain_llh=None, burn=0, probs=(0.025, 0.5, 0.975), max_lag=None, c=5.0, want=None, masses=None):
        """``misti_ens_summary_dev``: the posterior summaries of a chain that is already on the device - ``chain`` a contiguous float64
        torch tensor ``[S][K][W][N]`` on this engine's device, ``chain_llh`` ``[S][K][W]`` or None (no best sample).  Asynchronous on
        the engine's stream; the rule is ``optimize.ensemble_posterior_rule``, bit for bit.  ``want``: the outputs to compute (default
        all of mean, cov, quant, tau, window, best_llh, best_x, best_at); one that is left out is not computed and the others' bits do
        not change.  ``masses`` (None, or 1 ... 8 masses in (0, 1]) adds ``hpd[S][N][len(masses)][2]`` and ``hpd_at``, the shortest
        intervals of ``optimize.ensemble_hpd_rule`` from a full sort on the device; ``"order"`` in ``want`` the sorted marginals
        ``order[S][N][(K - burn) W]``.  Returns a dict of torch tensors on the device."""
        import torch
        want = None if want is None else tuple(want)
        if chain.dim() != 4 or chain.dtype != torch.float64 or not chain.is_contiguous():
            raise ValueError("ensemble_summary_dev: chain must be a contiguous float64 tensor [S][K][W][N]")
        S, K, W, N = chain.shape
        if chain_llh is not None and (tuple(chain_llh.shape) != (S, K, W) or chain_llh.dtype != torch.float64 or not chain_llh.is_contiguous()):
            raise ValueError("ensemble_summary_dev: chain_llh must be a contiguous float64 tensor [S][K][W]")
        def empty(shape, integer):
            v = torch.empty(shape, dtype=torch.int32 if integer else torch.float64, device=chain.device)
            return v, v.data_ptr()
        p, out, p_keep = self._post(S, N, K, burn, probs, max_lag, c, empty, want, masses, W)
        _lib.check(self._lib.misti_ens_summary_dev(self._ctx, S, K, W, N, C.c_void_p(chain.data_ptr()) if chain.data_ptr() else None,
                                                   C.c_void_p(chain_llh.data_ptr()) if chain_llh is not None and chain_llh.data_ptr() else None, C.byref(p)))
        return out

    _BANDS_OUTPUTS = ("count", "mean", "quant", "lo", "hi")

    def _bands(self, G, probs, want, empty, workspace_bytes=0, batch_limit=0):
        """``misti_bands_t`` for G groups on this engine's grid and the outputs of ``want`` (None: all five) it points into;
        ``empty(shape, integer)`` as in ``_post``.  Returns (descriptor, outputs, what must stay alive until the call returns)."""
        probs = _f64(probs).reshape(-1)
        want = self._BANDS_OUTPUTS if want is None else tuple(want)
        unknown = [k for k in want if k not in self._BANDS_OUTPUTS]
        if unknown:
            raise ValueError("trajectory bands: unknown outputs %s (there are %s)" % (unknown, ", ".join(self._BANDS_OUTPUTS)))
        shape = (G, self.numT, 2)
        made = {k: empty(shape + ((probs.size,) if k == "quant" else ()), k == "count") for k in self._BANDS_OUTPUTS if k in want}
        b = _lib.Bands(size=C.sizeof(_lib.Bands), n_prob=probs.size, probs=probs.ctypes.data, workspace_bytes=int(workspace_bytes),
                       batch_limit=int(batch_limit), **{k: at or None for k, (_, at) in made.items()})
        out = {k: v for k, (v, _) in made.items()}
        out["probs"] = probs
        return b, out, (probs,)

    def trajectory_bands_dev(self, lc, split, status=None, probs=(0.025, 0.5, 0.975), want=None, workspace_bytes=0):
        """``misti_traj_bands_dev``: bands of the corrected rates that are already on the device - ``lc`` a contiguous float64 torch
        tensor ``[G][m][numT + 1][2]`` (``d_lc`` of ``evaluate_dev`` for G groups of m samples) on this engine's device, ``split``
        ``[G][m]`` float64, ``status`` ``[G][m]`` int32 or None (every sample counts as OK).  Per group, interval ``j < numT`` of the
        common grid and population: the members (status OK, ``j < split``, not NaN), their ``count``, ``quant`` (``[...][len(probs)]``),
        ``mean``, ``lo`` and ``hi`` - RATES, not sizes.  Asynchronous on the engine's stream; the rule is
        ``optimize.trajectory_bands_rule``, bit for bit.  ``want``: the outputs to compute (default all five); one that is left out is
        not computed and the others' bits do not change.  ``workspace_bytes`` bounds the sort's workspace (0: the library's default)
        and does not change the result.  Returns a dict of torch tensors ``[G][numT][2]`` on the device, and ``probs`` as read."""
        import torch
        if lc.dim() != 4 or lc.dtype != torch.float64 or not lc.is_contiguous() or tuple(lc.shape[2:]) != (self.numT + 1, 2):
            raise ValueError("trajectory_bands_dev: lc must be a contiguous float64 tensor [G][m][%d][2]" % (self.numT + 1))
        G, m = lc.shape[:2]
        for name, t in (("lc", lc), ("split", split), ("status", status)):           # a host pointer in a kernel would be a GPU fault
            if t is not None and (not t.is_cuda or t.device.index != self.device):
                raise ValueError("trajectory_bands_dev: %s must be a CUDA tensor on device %d (got %s)" % (name, self.device, t.device))
        if tuple(split.shape) != (G, m) or split.dtype != torch.float64 or not split.is_contiguous():
            raise ValueError("trajectory_bands_dev: split must be a contiguous float64 tensor [G][m]")
        if status is not None and (tuple(status.shape) != (G, m) or status.dtype != torch.int32 or not status.is_contiguous()):
            raise ValueError("trajectory_bands_dev: status must be a contiguous int32 tensor [G][m]")
        def empty(shape, integer):
            v = torch.empty(shape, dtype=torch.int32 if integer else torch.float64, device=lc.device)
            return v, v.data_ptr()
        b, out, keep = self._bands(G, probs, want, empty, workspace_bytes)
        at = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.data_ptr() else None
        _lib.check(self._lib.misti_traj_bands_dev(self._ctx, G, m, at(lc), at(split), at(status), C.byref(b)))
        return out

    def trajectory_bands(self, x, split_times, groups=1, probs=(0.025, 0.5, 0.975), want=None, band_bounds=None, pulse_times=None,
                         workspace_bytes=0, batch_limit=0):
        """``misti_traj_bands``: bands of the corrected rates over points given on the host - ``x[groups m][n_param]`` and
        ``split_times[groups m]``, group g being the points ``g m ... (g + 1) m - 1`` (the fits of a bootstrap table: one group; the
        kept samples of a chain: a group per fit).  The points run through the engine in batches of at most ``batch_limit`` (0: the
        library's default) with the rates kept on the device, and only the bands come back; ``band_bounds`` / ``pulse_times`` as in
        ``evaluate``.  The result is ``optimize.trajectory_bands_rule`` on ``evaluate(want_lc=True)`` of the same points, bit for bit,
        whatever ``batch_limit`` and ``workspace_bytes``.  Returns a dict of NumPy arrays ``[groups][numT][2]`` (``quant``:
        ``[...][len(probs)]``) - RATES, not sizes - and ``probs`` as read."""
        split = _f64(np.atleast_1d(split_times)).reshape(-1)
        G, n = int(groups), split.shape[0]
        if G < 0 or (G == 0) != (n == 0) or (G and n % G):
            raise ValueError("trajectory_bands: %d points do not make %d groups of equal size" % (n, G))
        m = n // G if G else 1
        par = _f64(x, (n, self.n_param)) if self.n_param else None
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
        bb = pt = None
        if band_bounds is not None and self.n_band:
            bb = np.ascontiguousarray(band_bounds, dtype=np.int32).reshape(n, self.n_band, 2)
        if pulse_times is not None and self.n_pulse:
            pt = np.ascontiguousarray(pulse_times, dtype=np.int32).reshape(n, self.n_pulse)
        def empty(shape, integer):
            v = np.empty(shape, dtype=np.int32 if integer else np.float64)
            return v, v.ctypes.data
        b, out, keep = self._bands(G, probs, want, empty, workspace_bytes, batch_limit)
        _lib.check(self._lib.misti_traj_bands(self._ctx, G, m, ptr(par), ptr(split), ptr(bb), ptr(pt), C.byref(b)))
        return out

    def enable_solver_trace(self, on=True):
        """Record, for the following batches, SciPy-comparable solver statistics per candidate and interval
        (``misti_enable_solver_trace``; see ``solver_trace``)."""
        _lib.check(self._lib.misti_enable_solver_trace(self._ctx, 1 if on else 0))

    def solver_trace(self, n_cand, cand=None):
        """Solver trace of the last batch: dict of ``nfev``, ``status``, ``kind`` arrays ``[n_cand][numT+1]``
        (kind 0 none, 1 closed form, 2 bounded TRF, 3 unbounded TRF; status = SciPy's termination code; noise 1 where a
        default-fit solve went on past a gradient test only the reference's noisy residual would have failed; stall 1 where the stall rule returned the
        starting point: status 3 and nfev 1, the reference needs 14 - 23 evaluations to get nowhere) and, with
        ``cand`` given (batches of at most 64 candidates), ``iterates [numT][200][2]``: the trial points of the
        unbounded solves of that candidate's chain (NaN beyond nfev)."""
        n = int(n_cand)
        words = np.empty((n, self.numT + 1), dtype=np.int32)
        its = np.empty((self.numT, _lib.TRACE_MAX_ITER, 2)) if cand is not None else None
        _lib.check(self._lib.misti_last_solver_trace(self._ctx, n, words.ctypes.data_as(C.c_void_p), int(cand) if cand is not None else 0,
                                                     its.ctypes.data_as(C.c_void_p) if its is not None else None))
        out = {"nfev": words & 0xffff, "status": (words >> 16) & 15, "kind": (words >> 20) & 15, "noise": (words >> 24) & 1, "stall": (words >> 25) & 1}
        if its is not None:
            out["iterates"] = its
        return out

    def enable_timing(self, on=True):
        _lib.check(self._lib.misti_enable_timing(self._ctx, 1 if on else 0))

    def kernel_times(self, reset=False):
        """(ms per kernel, launches per kernel) accumulated from HIP events around every launch."""
        ms = (C.c_double * 3)()
        n = (C.c_int64 * 3)()
        _lib.check(self._lib.misti_kernel_times(self._ctx, ms, n, 1 if reset else 0))
        names = ("correct", "spectrum", "llk")
        return {k: ms[i] for i, k in enumerate(names)}, {k: n[i] for i, k in enumerate(names)}


# ------------------------------------------------------------------------------
class Lanes:
    """``misti_create_lanes`` ... ``misti_destroy_lanes``: n engine contexts of one model on one device, each with its own non-blocking
    stream, so that independent batches overlap on the GPU (include/misti_hip.h, "lanes"; the overlapped rate of the headline benchmark).
    The pool itself lives in the library since round 6 - ``misti_amd.lanes.LanePool`` and ``bench.py`` sit on this class.  Same constructor
    as ``Engine`` plus ``lanes``.  Device-buffer form only (raw device addresses, asynchronous); results are bit for bit a single
    context's."""

    def __init__(self, times, lh, bands=(), pulses=(), n_param=0, cpfit=False, true_eps=False, smooth=False,
                 unfolded=False, sample_date=0, mixture_th=0.0, device=0, lanes=20):
        self._h = C.c_void_p()
        self._lib = _lib.load()
        m, keep = _model_struct(times, lh, bands, pulses, n_param, cpfit, true_eps, smooth, unfolded, sample_date, mixture_th)
        self.numT, self.n_param, self.n_band, self.device = int(m.numT), int(n_param), int(m.n_band), int(device)
        h = C.c_void_p()
        _lib.check(self._lib.misti_create_lanes(C.byref(m), int(device), int(lanes), C.byref(h)))
        self._h = h
        self._pid = os.getpid()
        self.n_lanes = int(self._lib.misti_lanes_size(h))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            if getattr(self, "_pid", None) == os.getpid():
                self._lib.misti_destroy_lanes(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def engine(self, i):
        """Lane i's context as an ``Engine`` that does NOT own it (timing, stream handle, solver trace, ``last_diag`` per lane)."""
        ctx = C.c_void_p()
        _lib.check(self._lib.misti_lanes_context(self._h, int(i), C.byref(ctx)))
        e = Engine.__new__(Engine)
        e._lib, e._ctx, e._pid, e._borrowed = self._lib, ctx, self._pid, True
        e.numT, e.n_param, e.n_band, e.device, e.unfolded = self.numT, self.n_param, self.n_band, self.device, False
        return e

    def level(self, i):
        """The stream-priority level lane i was created on (0: the default level).  The library deals the lanes over the levels where
        the runtime's queue limit per level is smaller than the pool (misti_lanes.cpp); an internal entry point, for tests and tools."""
        r = int(self._lib.misti_lanes_level_(self._h, C.c_int(int(i))))
        if r < 0:
            _lib.check(r)
        return r

    def set_hints(self, integer_splits=False):
        _lib.check(self._lib.misti_lanes_set_hints(self._h, _lib.HINT_INTEGER_SPLITS if integer_splits else 0))

    def evaluate_dev(self, lane, n_cand, d_split, d_params, n_rep, d_jsfs, d_llk, d_jafs=0, d_lc=0, d_pr=0, d_status=0, d_bounds=0):
        """``misti_lanes_eval_batch_dev``: one batch on lane ``lane`` (``None`` / -1: an idle lane, else round-robin); returns the lane used."""
        v = lambda p: C.c_void_p(int(p)) if p else None
        used = C.c_int(-1)
        _lib.check(self._lib.misti_lanes_eval_batch_dev(self._h, _lib.LANE_ANY if lane is None else int(lane), int(n_cand), v(d_split), v(d_params), v(d_bounds),
                                                        int(n_rep), v(d_jsfs), v(d_llk), v(d_jafs), v(d_lc), v(d_pr), v(d_status), C.byref(used)))
        return int(used.value)

    def bind_dev(self, lane, n_cand, d_split, d_params, n_rep, d_jsfs, d_llk, d_jafs=0, d_lc=0, d_pr=0, d_status=0, d_bounds=0):
        """``evaluate_dev`` with its arguments converted ONCE: returns a function of no arguments that issues this batch on lane ``lane``
        (an explicit lane).  A sweep that re-issues a batch on fixed device buffers - the bench's steps - saves the ~2 us of ctypes argument
        conversion per call (12.6 -> 10.8 us per step on the headline grid; the rest is the library's three launches and its event record)."""
        v = lambda p: C.c_void_p(int(p)) if p else None
        fn, check = self._lib.misti_lanes_eval_batch_dev, _lib.check
        args = (self._h, C.c_int(int(lane)), C.c_int64(int(n_cand)), v(d_split), v(d_params), v(d_bounds), C.c_int64(int(n_rep)), v(d_jsfs),
                v(d_llk), v(d_jafs), v(d_lc), v(d_pr), v(d_status), None)

        def issue():
            r = fn(*args)
            if r:
                check(r)
        return issue

    def wait(self, lane):
        _lib.check(self._lib.misti_lanes_wait(self._h, int(lane)))

    def busy(self, lane):
        r = self._lib.misti_lanes_busy(self._h, int(lane))
        if r < 0:
            _lib.check(r)
        return bool(r)

    def sync(self):
        _lib.check(self._lib.misti_lanes_sync(self._h))


# ------------------------------------------------------------------------------
class MultiEngine:
    """One model on a LIST of devices from one process (``misti_create_multi`` ... ``misti_destroy_multi``): what a node's 1, 2, 4
    or 8 GPUs are to a caller of the C ABI - the reference's counterpart is ``parallel -j 20 ./MiSTI.py ...``
    (``/root/reference/README.md:110-115``).  Same constructor as ``Engine`` with ``devices`` (a list; an entry may repeat) in
    place of ``device``.  ``evaluate`` deals whole lambda-correction chains to the devices and returns exactly what ``Engine.evaluate``
    returns; ``nm_solve`` / ``basinhopping`` deal contiguous blocks of starts.  Nothing here falls back to fewer devices: a
    device that cannot be opened fails the constructor."""

    def __init__(self, times, lh, bands=(), pulses=(), n_param=0, cpfit=False, true_eps=False, smooth=False,
                 unfolded=False, sample_date=0, mixture_th=0.0, devices=(0,)):
        self._m = C.c_void_p()
        self._lib = _lib.load()
        times = _f64(times)
        lh = _f64(lh)
        self.numT = int(lh.shape[0])
        if lh.ndim != 2 or lh.shape[1] != 2 or times.shape != (self.numT - 1,):
            raise ValueError("times must have numT-1 entries and lh shape [numT][2]")
        self.n_param = int(n_param)
        self.flags = (CPFIT if cpfit else 0) | (TRUE_EPS if true_eps else 0) | (SMOOTH if smooth else 0) | (UNFOLDED if unfolded else 0)
        self.unfolded = bool(unfolded)
        bands, pulses = list(bands), list(pulses)
        self.n_band = len(bands)
        b_arr = (_lib.Band * max(1, len(bands)))()
        for i, (pop, start, end, value, param) in enumerate(bands):
            b_arr[i] = _lib.Band(int(pop), int(start), int(end), int(param), float(value))
        p_arr = (_lib.Pulse * max(1, len(pulses)))()
        for i, (pop, time, value, param) in enumerate(pulses):
            p_arr[i] = _lib.Pulse(int(pop), int(time), int(param), 0, float(value))
        m = _lib.Model(self.numT, int(sample_date), self.flags, len(bands), len(pulses), self.n_param, float(mixture_th),
                       times.ctypes.data_as(C.POINTER(C.c_double)), lh.ctypes.data_as(C.POINTER(C.c_double)), b_arr, p_arr)
        self.devices = [int(d) for d in devices]
        dev = (C.c_int32 * max(1, len(self.devices)))(*self.devices)
        h = C.c_void_p()
        _lib.check(self._lib.misti_create_multi(C.byref(m), len(self.devices), dev, C.byref(h)))
        self._m = h
        self._pid = os.getpid()

    def close(self):
        if getattr(self, "_m", None) is not None and self._m:
            if getattr(self, "_pid", None) == os.getpid():
                self._lib.misti_destroy_multi(self._m)
            self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def evaluate(self, split_time, params=None, jsfs=None, want_lc=False, want_pr=False, band_bounds=None):
        """``misti_multi_eval_batch``: as ``Engine.evaluate`` (``runaway`` is not collected across devices: None)."""
        split = _f64(np.atleast_1d(split_time))
        n = split.shape[0]
        P = self.n_param
        par = _f64(params, (n, P)) if P else None
        rows = _f64(jsfs, (-1, 8)) if jsfs is not None and len(jsfs) else np.zeros((0, 8))
        R = rows.shape[0]
        llk = np.empty((n, R))
        jafs = np.empty((n, 7))
        status = np.empty(n, dtype=np.int32)
        lc = np.empty((n, self.numT + 1, 2)) if want_lc else None
        pr = np.empty((n, self.numT + 2, 6)) if want_pr else None
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
        bb = None
        if band_bounds is not None and self.n_band:
            bb = np.ascontiguousarray(band_bounds, dtype=np.int32).reshape(n, self.n_band, 2)
        _lib.check(self._lib.misti_multi_eval_batch(self._m, n, ptr(split), ptr(par), ptr(bb), R, ptr(rows), ptr(llk), ptr(jafs),
                                                    ptr(lc), ptr(pr), ptr(status)))
        return BatchResult(llk, jafs, status, lc, pr, None)

    def bootstrap_table(self, chunks, n, seed=0, normalize=False):
        """``Engine.bootstrap_table``, made on the first context of the list: a replicate depends on ``(seed, r)`` alone, so one device
        makes the host rows and every context is handed the same ones."""
        ctx, dev = C.c_void_p(), C.c_int(0)
        _lib.check(self._lib.misti_multi_context(self._m, 0, C.byref(ctx), C.byref(dev)))
        rows, _ = _bootstrap_rows(self._lib, ctx, dev.value, chunks, n, seed, 0, normalize, False)
        return _bootstrap_table(rows, chunks)

    def jackknife_table(self, chunks, m=1):
        """``Engine.jackknife_table``, made on the first context of the list: the rows depend on the table and ``m`` alone, so one device
        makes the host rows and every context is handed the same ones."""
        ctx, dev = C.c_void_p(), C.c_int(0)
        _lib.check(self._lib.misti_multi_context(self._m, 0, C.byref(ctx), C.byref(dev)))
        return _bootstrap_table(_jackknife_rows(self._lib, ctx, dev.value, chunks, m, 0, None), chunks)

    def parametric_table(self, split, params, data_row, n, n_sites=None, seed=0, band_bounds=None):
        """``Engine.parametric_table``, its replicates drawn on the first context of the list: a replicate depends on ``(seed, r)`` and the
        spectrum alone, so one device makes the host rows and every context is handed the same ones."""
        ctx, dev = C.c_void_p(), C.c_int(0)
        _lib.check(self._lib.misti_multi_context(self._m, 0, C.byref(ctx), C.byref(dev)))
        return _parametric_table(self, ctx, dev.value, split, params, data_row, n, n_sites, seed, band_bounds)

    def last_shards(self):
        """(candidates per context, chains per context) of the last ``evaluate``."""
        D = len(self.devices)
        a, b = (C.c_int64 * D)(), (C.c_int64 * D)()
        _lib.check(self._lib.misti_multi_last_shards(self._m, a, b))
        return list(a), list(b)

    def last_cost(self):
        """Summed chain cost per context of the last ``evaluate`` (what the dealing balances: chain length + members / 64)."""
        c = (C.c_double * len(self.devices))()
        _lib.check(self._lib.misti_multi_last_cost(self._m, c))
        return list(c)

    def evaluate_dev_gathered(self, n_cand, rows_per_shard, d_split, d_params, n_rep, d_jsfs, d_llk_all, d_status_all=None, d_bounds=None):
        """``misti_multi_eval_batch_dev``: context i evaluates ``n_cand[i]`` candidates from device pointers on ITS device and the
        log-likelihoods are all-gathered on the devices by RCCL inside the library (every ``d_llk_all[i]`` ends as the whole
        ``[D][rows_per_shard][n_rep]`` table).  Arguments are lists (one entry per context) of integer device addresses, e.g.
        ``tensor.data_ptr()``.  Asynchronous; ``sync()`` waits for every context's stream."""
        D = len(self.devices)
        arr = lambda ptrs: (C.c_void_p * D)(*[C.c_void_p(int(p)) if p else None for p in ptrs])
        n = (C.c_int64 * D)(*[int(v) for v in n_cand])
        _lib.check(self._lib.misti_multi_eval_batch_dev(self._m, n, int(rows_per_shard), arr(d_split), arr(d_params) if d_params is not None else None,
                                                        arr(d_bounds) if d_bounds is not None else None, int(n_rep), arr(d_jsfs), arr(d_llk_all),
                                                        arr(d_status_all) if d_status_all is not None else None))

    def sync(self):
        _lib.check(self._lib.misti_multi_sync(self._m))

    def nm_solve(self, starts, split_time, jsfs_row, tol=1e-4, maxiter=1000):
        """``misti_multi_nm_solve``: ``Engine.nm_solve`` with the starts dealt to the devices in contiguous blocks."""
        st = _f64(starts, (-1, self.n_param))
        S = st.shape[0]
        row = _f64(jsfs_row, (8,))
        x = np.empty((S, self.n_param))
        llh = np.empty(S)
        nit, nfev, status = (np.empty(S, dtype=np.int32) for _ in range(3))
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.misti_multi_nm_solve(self._m, S, ptr(st), float(split_time), ptr(row), float(tol), float(tol), int(maxiter),
                                                  ptr(x), ptr(llh), ptr(nit), ptr(nfev), ptr(status)))
        return dict(x=x, llh=llh, nit=nit, nfev=nfev, status=status)

    def basinhopping(self, starts, split_time, jsfs_row, rngs, niter=100, T=0.5, stepsize=0.5, interval=50, target_accept_rate=0.5,
                     stepwise_factor=0.9, xatol=1e-4, fatol=1e-4, nm_maxiter=None, nm_maxfev=None):
        """``misti_multi_basinhopping``: ``Engine.basinhopping`` with the starts dealt to the devices in contiguous blocks."""
        st = _f64(starts, (-1, self.n_param))
        S, N = st.shape
        row = _f64(jsfs_row, (8,))
        uni = draw_uniforms(rngs, S, int(niter), N)
        x = np.empty((S, N))
        llh = np.empty(S)
        nfev, failures, accepted = (np.empty(S, dtype=np.int32) for _ in range(3))
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.misti_multi_basinhopping(self._m, S, ptr(st), float(split_time), ptr(row), int(niter), float(T), float(stepsize), int(interval),
                                                      float(target_accept_rate), float(stepwise_factor), float(xatol), float(fatol),
                                                      int(nm_maxiter if nm_maxiter is not None else 200 * N), int(nm_maxfev if nm_maxfev is not None else 200 * N),
                                                      ptr(uni), ptr(x), ptr(llh), ptr(nfev), ptr(failures), ptr(accepted)))
        return dict(x=x, llh=llh, nfev=nfev, failures=failures, accepted=accepted)


def draw_uniforms(rngs, S, niter, N):
    """The uniforms SciPy's basin hopping would draw from start s's generator, in its order: per hop N for the displacement
    (RandomDisplacement: rng.uniform(-stepsize, stepsize, shape)), then one for the Metropolis test.  ``rngs``: one
    ``numpy.random.Generator`` or seed per start."""
    gens = [g if isinstance(g, np.random.Generator) else np.random.default_rng(g) for g in rngs]
    if len(gens) != S:
        raise ValueError("one generator (or seed) per start")
    uni = np.empty((S, niter, N + 1))
    for s_, g in enumerate(gens):
        for h in range(niter):
            uni[s_, h, :N] = g.random(N)
            uni[s_, h, N] = g.random()
    return uni


def _classes(v, unfolded):
    """The spectrum classes the likelihood distinguishes: all 7, or folded pairs 0+6, 1+5, 2+4 and 3 (:217-227, :600-609)."""
    return fold_classes(v, unfolded)


def _multinomial_const(counts, unfolded):
    """log of the multinomial coefficient of the data (llh_const of SetJAFS)."""
    c = math.lgamma(sum(counts) + 1)
    for v in _classes(counts, unfolded):          # subtracted one by one, as the reference does (same rounding)
        c -= math.lgamma(v + 1)
    return c


def _multinomial_logterm(counts, spectrum, unfolded):
    return sum(c * math.log(p) for c, p in zip(_classes(counts, unfolded), _classes(spectrum, unfolded)))


def _band_record(el, sample_date, error):
    """One ``-mi pop start end value opt`` option -> (pop 0/1, start, end, value, optimised); SetModel's checks :236-247."""
    pop, start, end, value, opt = int(el[0]) - 1, int(el[1]), int(el[2]), float(el[3]), int(el[4]) == 1
    if pop not in (0, 1):
        error("SetModel", "Population index should be 1 or 2.")
    if start < sample_date:
        error("SetModel", "Migration start (" + str(start) + ") should be larger than or equal to sample date (" + str(sample_date) + ").")
    if end <= start:
        error("SetModel", "Migration start (" + str(start) + ") should be strictly less than migration end (" + str(end) + ").")
    return pop, start, end, value, opt


def _pulse_record(el, sample_date, error):
    """One ``-pu pop time value opt`` option -> (pop 0/1, time, value, optimised); SetModel's checks :259-271."""
    pop, t, value, opt = int(el[0]) - 1, int(el[1]), float(el[2]), int(el[3]) == 1
    if pop not in (0, 1):
        error("SetModel", "Population index should be 1 or 2.")
    if t < sample_date:
        error("SetModel", "Pulse migration time (" + str(t) + ") should be larger than or equal to sample date (" + str(sample_date) + ").")
    if value < 0 or value > 1:
        error("SetModel", "Pulse migration rate should be between 0 and 1.")
    return pop, t, value, opt


class MigrationInference:
    """GPU-backed mirror of the reference class (MigrationInference.py:35-739)."""
    COUNT_LLH = 0
    CORRECTION_CALLED = 0
    CORRECTION_FAILED = 0

    def __init__(self, times, lambdas, dataJAFS, splitT, mi=[], pu=[], **kwargs):
        kw = kwargs
        self.debug = bool(kw.get("debug", False))
        self.enableOutput = self.debug or bool(kw.get("enableOutput", False))
        if self.enableOutput:
            print("MigrationInference: output enabled.")
        self.cpfit = bool(kw.get("cpfit", False))
        self.correct = not bool(kw.get("trueEPS", False))
        self.smooth = bool(kw.get("smooth", False))
        self.LLHpsmc = "Tpsmc" in kw
        if self.LLHpsmc:
            self.Tpsmc = kw["Tpsmc"]
        self.unfolded = bool(kw.get("unfolded", False))
        self.thrh = [1.0, 1.0]
        if "thrh" in kw and len(kw["thrh"]) == 2:
            self.thrh = kw["thrh"]
        self.sampleDate = kw.get("sampleDate", 0)
        self.mixtureTH = kw.get("mixtureTH", 0.0)
        self._device = int(kw.get("device", 0))
        if splitT < self.sampleDate:                                            # :85-86
            self.PrintError("__init__", "cannot initialise class with split time being more recent than sample date.")
        self._split_in = float(splitT)
        self._times0 = [float(v) for v in times]
        self._lh0 = [[float(l[0]), float(l[1])] for l in lambdas]
        frac = splitT % 1                                                       # :89-99, incl. the mutation
        splitT = int(splitT)
        if splitT - 1 > len(times):
            self.PrintError("__init__", "Invalid value for split time, cannot create Migration class instance.")
        if frac != 0.0:
            t1 = frac * times[splitT]
            t2 = times[splitT] - t1
            times[splitT] = t1
            times.insert(splitT + 1, t2)
            lambdas.insert(splitT + 1, lambdas[splitT])
            splitT += 1
        self.lh = list(lambdas)
        self.times = times
        self.numT = len(self.lh)
        if len(self.times) != self.numT - 1:                                    # :105-107
            print("Unexpected number of time intervals")
            raise SystemExit(0)
        self.discr = 1
        self.splitT = splitT
        self.SetModel(mi, pu)
        self.SetJAFS(dataJAFS)
        self.JAFSsize = self.snps
        self.lc = [[1, 1] for _ in range(self.numT)]
        self.JAFS = None
        self.Pr = None
        self.llh = None
        self.status = 0
        self.doPlot = False
        # bands/pulses in C-ABI form; every band is expressed on this candidate's grid
        bands = [(pop, start, end, val, -1) for pop, start, end, val in self._fixedMis]
        bands += [(pop, start, end, val, i) for i, (pop, start, end, val) in enumerate(self.optMis)]
        n_opt_mi = len(self.optMis)
        pulses = [(pop, t, val, -1) for pop, t, val in self._fixedPus]
        pulses += [(pop, t, val, n_opt_mi + i) for i, (pop, t, val) in enumerate(self.optPus)]
        self._engine = Engine(self._times0, self._lh0, bands, pulses, n_param=n_opt_mi + len(self.optPus),
                              cpfit=self.cpfit, true_eps=not self.correct, smooth=self.smooth, unfolded=self.unfolded,
                              sample_date=int(self.sampleDate), mixture_th=float(self.mixtureTH), device=self._device)
        if self.debug:
            print("MigrationInference class initialized. Class size", self.numT)

    # -- reference helpers ---------------------------------------------------------
    def PrintError(self, func, text):                                           # :300-303
        raise ModelError(func, text)

    def SetJAFS(self, dataJAFS, normalize=False):                               # :202-227
        """Data spectrum of 8 numbers (total + 7 classes) and the data-only term of the multinomial likelihood."""
        if len(dataJAFS) != 8:
            self.PrintError("SetJAFS", "Unexpected data SFS.")
        self._row = [float(v) for v in dataJAFS]
        self.dataJAFS = list(dataJAFS[1:])
        self.snps = sum(self.dataJAFS)
        self.llh_const = _multinomial_const(self.dataJAFS, self.unfolded)

    def SetModel(self, mis, pus):                                               # :229-289
        """``-mi`` / ``-pu`` descriptors -> band and pulse records (``_bands``, ``_pulses``; what the C ABI takes)
        and, derived from them, the per-interval tables ``mi`` / ``pu`` and the lists ``optMis`` / ``optPus`` the
        reference's callers read.  Errors are the reference's (message and exit status 0)."""
        self._bands = [_band_record(el, self.sampleDate, self.PrintError) for el in mis]
        self._pulses = [_pulse_record(el, self.sampleDate, self.PrintError) for el in pus]
        for pop, start, end, _, _ in self._bands:
            if end > self.numT:                      # the reference runs off the end of its table here (IndexError)
                self.PrintError("SetModel", "Migration end (" + str(end) + ") is beyond the last time interval (" + str(self.numT) + ").")
        for pop, t, _, _ in self._pulses:
            if t >= self.numT:
                self.PrintError("SetModel", "Pulse migration time (" + str(t) + ") is beyond the last time interval (" + str(self.numT - 1) + ").")
        taken = set()
        for pop, start, end, _, _ in self._bands:
            cells = {(pop, t) for t in range(start, end)}
            if cells & taken:
                self.PrintError("SetModel", "Migration rate intervals should not overlap.")
            taken |= cells
        if len({t for _, t, _, _ in self._pulses}) != len(self._pulses):
            self.PrintError("SetModel", "Current version allows only single-direction pulse migration at a time.")
        self.optMis = [[pop, start, end, val] for pop, start, end, val, opt in self._bands if opt]
        self.optPus = [[pop, t, val] for pop, t, val, opt in self._pulses if opt]
        self._fixedMis = [[pop, start, end, val] for pop, start, end, val, opt in self._bands if not opt]
        self._fixedPus = [[pop, t, val] for pop, t, val, opt in self._pulses if not opt]
        self.optMisSize, self.optPusSize = len(self.optMis), len(self.optPus)
        self._fill_tables([b[3] for b in self.optMis] + [q[2] for q in self.optPus])

    def _fill_tables(self, values):
        """Per-interval tables from the records; optimised bands / pulses take ``values`` (bands first, in option order)."""
        self.mi = [[0.0, 0.0] for _ in range(self.numT)]
        self.pu = [[0.0, 0.0] for _ in range(self.numT)]
        free = iter(values)
        rate_of = {}
        for k, (pop, start, end, val, opt) in enumerate(self._bands):
            if opt:
                rate_of[k] = next(free)
        for k, (pop, start, end, val, opt) in enumerate(self._bands):
            for t in range(start, end):
                self.mi[t][pop] = rate_of.get(k, val)
        for pop, t, val, opt in self._pulses:
            self.pu[t][pop] = next(free) if opt else val

    def MapParameters(self, params):                                            # :291-298
        if len(params) != self.optMisSize + self.optPusSize:
            self.PrintError("MapParameters", "Incorrect number of parameters.")
        self._fill_tables(list(params))

    # -- the hot path ----------------------------------------------------------------
    def JAFSLikelihood(self, mu):                                               # :566-614
        cls = MigrationInference
        cls.COUNT_LLH += 1
        self.llh = -10 ** 9
        for v in mu:
            if v < 0:
                print("Hit negative value of migration rate")
                self.status = 1
                return -np.inf
        self.MapParameters(mu)
        self._mu = [float(v) for v in mu]
        cls.CORRECTION_CALLED += 1
        res = self._engine.evaluate([self._split_in], [list(mu)] if len(mu) else None, [self._row], want_lc=True, want_pr=True)
        self.status = int(res.status[0])
        if self.status == 2:
            cls.CORRECTION_FAILED += 1
            print("Lambda correction failed")
            return -np.inf
        if self.status == 3:
            self.PrintError("JAFSpectrum", "Infinite coalescent time. No migration.")
        if self.status != 0:
            # non-finite intermediate / stiff interval: the candidate has no value here
            print("MigrationInference: " + STATUS_TEXT.get(self.status, "status %d" % self.status))
            return -np.inf
        self.runaway = float(res.runaway[0])
        if self.runaway >= 5.0 and self.enableOutput:
            print("MigrationInference: corrected rate x interval length reaches %.3g - the lambda-correction ran into its "
                  "flat regime; the reference's value for such a candidate is not determined to 1e-9" % self.runaway)
        self.lc = [[float(a), float(b)] for a, b in res.lc[0][: self.numT]]
        self.Pr = [[[float(r[0]), float(r[1])], [float(r[2]), float(r[3])], [float(r[4]), float(r[5])]]
                   for r in res.pr[0][: self.splitT + 1]]
        self.JAFS = [float(v) for v in res.jafs[0]]
        self.llh = float(res.llk[0, 0])
        return self.llh

    def CoalescentRates(self):                                                  # :542-564
        """Forward map (TestModel route): ``lc`` := the current rates, ``lh`` := what PSMC would see
        under the current migration model, ``Pr`` := the pair-state trace.  As in the reference, every
        interval is evaluated with the migration rates of the last two-population interval (its
        CorrectLambda object keeps them from the preceding likelihood call); for a per-interval
        forward map use ``Engine.forward_rates``."""
        mu = getattr(self, "_mu", None)
        if mu is None:
            mu = [b[3] for b in self.optMis] + [q[2] for q in self.optPus]
        lh, pr, status = self._engine.forward_rates([self._split_in], [list(mu)] if len(mu) else None, want_pr=True, hold_mu=True)
        for i in range(self.numT):
            self.lc[i] = [self.lh[i][0], self.lh[i][1]]
        for t in range(min(self.splitT, self.numT - 1)):
            self.lh[t] = [float(lh[0][t][0]), float(lh[0][t][1])]
        self.Pr = [[[float(r[0]), float(r[1])], [float(r[2]), float(r[3])], [float(r[4]), float(r[5])]]
                   for r in pr[0][: self.splitT + 1]]

    def JAFSLikelihoodBatch(self, split_times, params=None, jsfs_rows=None, **kw):
        """Batch form without a reference counterpart: many candidates x replicates in
        one call on the same grid and band structure (bands ending at this object's
        split follow each candidate's own split)."""
        return self._engine.evaluate(split_times, params, [self._row] if jsfs_rows is None else jsfs_rows, **kw)

    def MaximumLLHFunction(self):                                               # :696-711
        """Likelihood of the data under its own (saturated) spectrum: the upper bound of JAFSLikelihood."""
        tot = sum(self.dataJAFS)
        return self.llh_const + _multinomial_logterm(self.dataJAFS, [v / tot for v in self.dataJAFS], self.unfolded)

    def ObjectiveFunction(self, mu):                                            # :713-716
        res = -self.JAFSLikelihood(mu)
        print(mu, res)
        return res

    def Solve(self, tol=1e-4, globalOpt=False):                                 # :718-733
        if self.optMisSize + self.optPusSize > 0:
            from scipy import optimize
            init = [v[3] for v in self.optMis] + [v[2] for v in self.optPus]
            if globalOpt:
                res = optimize.basinhopping(self.ObjectiveFunction, init, T=0.5, minimizer_kwargs=dict(method="Nelder-Mead"))
            else:
                res = optimize.minimize(self.ObjectiveFunction, init, method="Nelder-Mead",
                                        options={"xatol": tol, "fatol": tol, "maxiter": 1000, "disp": True})
            return [res.x, -res.fun]
        return [[], self.JAFSLikelihood([])]

    @staticmethod
    def Report():                                                               # :735-739
        print("Total number of likelihood function calls is", MigrationInference.COUNT_LLH)
        print("Lambda correction called", MigrationInference.CORRECTION_CALLED, "times.")
        print("Lambda correction failed", MigrationInference.CORRECTION_FAILED, "times.")


def truth_spectrum(times, lh, split, bands, pulses, sample_date, device=0):
    """Expected JSFS of a fully specified model (``--trueEPS`` route of TestModel.py:95-96)
    computed on the GPU; used to synthesise data spectra for the workloads."""
    with Engine(times, lh, bands, pulses, 0, cpfit=True, true_eps=True, smooth=False, unfolded=True,
                sample_date=sample_date, device=device) as e:
        r = e.evaluate([float(split)])
    if int(r.status[0]) != 0:
        raise MistiError(int(r.status[0]), "truth spectrum failed: " + STATUS_TEXT.get(int(r.status[0]), "?"))
    return [float(v) for v in r.jafs[0]]
