// The searches of the C ABI (include/misti_hip.h) over the rows problem (misti_rows.h): batched Nelder-Mead (misti_nm.hip), basin
// hopping around it, and differential evolution (misti_de.hip) - every point through the batch path (run_dev, misti_api.cpp).
#include <cstdlib>

#include "misti_rows.h"

using namespace misti_host;

namespace {

// Device-resident state of one batched Nelder-Mead run, carved from the context's nm buffers.
struct NmWork {
    misti::NmState st{};
    size_t slots[NM_BATCHES] = {};   // slots of every batch of the search, and of all of them
    size_t n_slots = 0;
    double* llk[NM_BATCHES] = {};    // [slots] the engine's values of every batch
    double *d_starts = nullptr;      // [S][N] in: start points; out: best vertices
    double *d_llh = nullptr;         // [S]    out: their log-likelihood
    double *d_row = nullptr;         // [8]    the data JSFS (MISTI_SPLIT_ONE)
    int32_t *idx[2] = {nullptr, nullptr}, *cnt = nullptr;
    RowsProblem rows;                // what each start hands its points; the rows path's table and evaluation
};

// Live starts up to which an iteration is speculative (misti_nm.hip): all 4 + N points of a start in one batch, as long as the
// batch still runs one chain per wave (FOLLOW_MAX_CHAINS candidates, each its own chain) - there the iteration costs one
// chain latency instead of three.  MISTI_NM_SPEC=0 turns it off (tests compare the two paths).
int64_t nm_spec_cap(int N) {
    const char* e = getenv("MISTI_NM_SPEC");
    if (e && e[0] == '0') return 0;
    return misti::FOLLOW_MAX_CHAINS / (4 + N);
}

// One minimisation of every start from w.d_starts (device); leaves best vertices in w.d_starts, their log-likelihood in w.d_llh,
// SciPy's counters in st.nit / st.nfev and the termination status in st.shrunk (0 converged, 1 evaluation budget, 2 iteration
// budget).  Asynchronous except for the 4-byte live counts; results are complete when the stream is.
int nm_run(misti_ctx* c, NmWork& w, double split_time, double xatol, double fatol, int32_t maxiter, int64_t maxfun) {
    using namespace misti;
    NmState& st = w.st;
    const int N = st.N;
    const size_t S = (size_t)st.S, V = (size_t)N + 1;
    st.maxiter = maxiter; st.maxfun = maxfun; st.xatol = xatol; st.fatol = fatol;
    hipStream_t sm = c->stream;
    const bool rows = w.rows.a.rows_path();
    // what the search knows about its own batches: one split time for every point (empty slots carry -1), distinct points.
    // The rows path knows less: its chains end at different splits (not one length), and every start from the same initial
    // values submits the same initial simplex - one chain for all of them, computed once up to the largest split (shared).
    // The bounds path (a rows path with per-start band bounds) keeps exactly the rows path's set.  RUN_INTEGER_SPLITS speaks of
    // split times alone: bounds are whole interval indices and never add a fractional interval (and the hint is verified on the
    // device).  RUN_UNSHARED stays off: starts with the same initial values AND the same bounds still share their chains (the
    // chain key holds the bounds).  RUN_ONE_LENGTH stays off: the splits differ, and so do the chain lengths.
    // The split as a coordinate (misti_nm_solve_split) is a rows path whose splits are never known to be whole (rows.whole is false):
    // no hint at all - points of different starts with equal parameter bits and bounds still share a chain, computed to the largest
    // split among them.
    static const int hint_mask = [] { const char* e = getenv("MISTI_NM_HINTS"); return e ? atoi(e) : 7; }();       // diagnostic: which hints the search passes on
    const unsigned one_hints = ((split_time == std::floor(split_time) ? RUN_INTEGER_SPLITS : 0u) | RUN_UNSHARED | RUN_ONE_LENGTH) & (unsigned)hint_mask;
    // the first n slots of one batch through the engine: their values against the one data row, or (rows path) each against its own row
    auto eval = [&](int which, int64_t n) -> int {
        const NmBatch& b = st.b[which];
        if (!rows) return run_dev(c, n, b.split, b.pts, nullptr, 1, w.d_row, w.llk[which], nullptr, nullptr, nullptr, nullptr, one_hints);
        return w.rows.eval(c, b, n, w.llk[which], (unsigned)hint_mask);
    };
    int32_t* cnt = w.cnt;
    HIP_TRY(hipMemsetAsync(cnt, 0, 4 * sizeof(int32_t), sm));
    HIP_TRY(hipMemsetAsync(st.b[NM_B_REFLECT].split, 0xBF, S * sizeof(double), sm));    // all-0xBF bytes: a negative double = "no point in this slot"
    // what put_none writes, in every slot nothing has written yet: row 0, all-zero bounds and pulse times (each kind's five arrays
    // lie back to back: nm_per_slot)
    const NmBatch& b0 = st.b[NM_B_INIT];
    if (b0.row) HIP_TRY(hipMemsetAsync(b0.row, 0, w.n_slots * sizeof(int32_t), sm));
    if (b0.bnd) HIP_TRY(hipMemsetAsync(b0.bnd, 0, w.n_slots * st.src.nb2 * sizeof(int32_t), sm));
    if (b0.put) HIP_TRY(hipMemsetAsync(b0.put, 0, w.n_slots * st.src.np * sizeof(int32_t), sm));
    HIP_TRY(launch_nm_init(st, w.d_starts, sm));
    if (int r = eval(NM_B_INIT, (int64_t)(S * V))) return r;
    int cur = 0;
    st.idx_next = w.idx[cur]; st.count_next = cnt + cur;
    HIP_TRY(launch_nm_begin(st, w.llk[NM_B_INIT], sm));
    Pacer pace(c);
    int64_t bound = 0;
    if (int r = pace.start(cnt + cur, bound)) return r;                 // after nm_begin
    int64_t issued = 0, slots = 0, spec_iters = 0;
    bool spec_primed = false;
    const int64_t K = 4 + N;
    for (int it = 0; bound > 0 && it < maxiter; ++it) {
        if (int r = pace.bound(it, bound)) return r;
        if (bound <= 0) break;
        st.idx_cur = w.idx[cur]; st.count_cur = cnt + cur;
        st.idx_next = w.idx[cur ^ 1]; st.count_next = cnt + (cur ^ 1);
        const bool spec = bound <= st.spec_cap;
        if (spec) {
            // speculative iteration: every point SciPy could ask for, one batch, one decision kernel - which also lays out the points
            // of the NEXT iteration (it sees the two lists swapped) and drops the count of live starts into the host's pinned word
            // (nm_spec_step_kernel: the live starts of a speculative iteration fit one workgroup); only the first speculative iteration
            // launches a points kernel
            if (!spec_primed) { HIP_TRY(launch_nm_spec_points(st, bound, sm)); spec_primed = true; }
            if (int r = eval(NM_B_SPEC, bound * K)) return r;
            // (no memsets here: the points step zeroes the next slot counter, and the reflection batch's splits are only read by the
            //  three-batch path, which a search never returns to - the number of live starts only falls)
            HIP_TRY(launch_nm_spec_step(st, bound, w.llk[NM_B_SPEC], pace.word(it), sm));
            ++spec_iters;
        } else {
            if (int r = eval(NM_B_REFLECT, bound)) return r;
            HIP_TRY(launch_nm_reflect(st, bound, w.llk[NM_B_REFLECT], sm));
            if (int r = eval(NM_B_SECOND, bound)) return r;
            HIP_TRY(launch_nm_accept(st, bound, w.llk[NM_B_SECOND], sm));
            if (int r = eval(NM_B_SHRINK, bound * N)) return r;
            HIP_TRY(hipMemsetAsync(cnt + (cur ^ 1), 0, sizeof(int32_t), sm));
            HIP_TRY(hipMemsetAsync(st.b[NM_B_REFLECT].split, 0xBF, (size_t)bound * sizeof(double), sm));
            HIP_TRY(launch_nm_finish(st, bound, w.llk[NM_B_SHRINK], sm));
        }
        if (int r = pace.record(it, spec ? nullptr : cnt + (cur ^ 1))) return r;
        cur ^= 1;
        ++issued;
        slots += bound;
    }
    c->nm_iterations += issued;
    c->nm_slots += slots;
    c->nm_spec_iterations += spec_iters;
    // results (device buffers reused: best vertices over the starts)
    HIP_TRY(launch_nm_result(st, w.d_starts, w.d_llh, st.shrunk, sm));
    return 0;
}

// Best vertices and their log-likelihoods to the host, with the search's own counters where the caller wants them.  Asynchronous.
int nm_copy_back(misti_ctx* c, const NmWork& w, double* x, double* llh, int32_t* nit, int32_t* nfev, int32_t* status) {
    const size_t S = (size_t)w.st.S;
    hipStream_t sm = c->stream;
    HIP_TRY(hipMemcpyAsync(x, w.d_starts, S * w.st.N * sizeof(double), hipMemcpyDeviceToHost, sm));
    HIP_TRY(hipMemcpyAsync(llh, w.d_llh, S * sizeof(double), hipMemcpyDeviceToHost, sm));
    if (nit) HIP_TRY(hipMemcpyAsync(nit, w.st.nit, S * sizeof(int32_t), hipMemcpyDeviceToHost, sm));
    if (nfev) HIP_TRY(hipMemcpyAsync(nfev, w.st.nfev, S * sizeof(int32_t), hipMemcpyDeviceToHost, sm));
    if (status) HIP_TRY(hipMemcpyAsync(status, w.st.shrunk, S * sizeof(int32_t), hipMemcpyDeviceToHost, sm));
    return 0;
}

// The arguments of every search, and of basin hopping around one, checked before the first HIP call, in one order: what does not
// depend on the context, the context, what needs the model.  Bounds or times that break SetModel's checks, and a fitted split the
// engine refuses, are no argument errors: the engine gives such a point status MISTI_BAD_STRUCTURE and no value, the optimiser
// +inf - as SciPy sees -JAFSLikelihood.  Leaves the number of coordinates in N and, in `whole`, whether every split time of the
// rows path is an integer.
int nm_check(const misti_ctx* c, const misti_search_t& q, int& N, bool& whole) {
    const RowsArgs a = rows_args(q);
    const misti_hops_t* h = q.hops;
    if (q.n_start < 0) return fail(MISTI_E_ARG, "negative number of starts");
    if (!q.starts || !q.jsfs || !q.x || !q.llh || (a.rows_path() && !q.rows) || (a.per_start() && !q.split_times))
        return fail(MISTI_E_ARG, "starts / %s / x / llh is NULL", !a.rows_path() ? "jsfs_row" : (a.per_start() ? "split_times / rows / jsfs" : "rows / jsfs"));
    if (q.n_rep < 1) return fail(MISTI_E_ARG, "n_rep must be >= 1 (got %lld)", (long long)q.n_rep);
    if (!h && q.maxiter < 1) return fail(MISTI_E_ARG, "maxiter must be >= 1");
    if (h && h->niter < 0) return fail(MISTI_E_ARG, "negative number of hops");
    if (h && h->niter > 0 && !h->uniforms) return fail(MISTI_E_ARG, "uniforms is NULL");
    if (h && (q.maxiter < 1 || h->nm_maxfev < 1 || h->interval < 1)) return fail(MISTI_E_ARG, "nm_maxiter, nm_maxfev and interval must be >= 1");
    if (int r = check_rows(a, whole)) return r;
    if (int r = check_limits(c, a, 1, "starts", N)) return r;
    if (a.fit_split()) if (int r = check_finite(q.starts, q.n_start, N)) return r;
    // the box: lo == hi holds a coordinate fixed, +-inf leaves a side open, and a start outside its box is clipped (SciPy only warns)
    if (q.n_box) {
        if (int r = check_n_box(a, "starts")) return r;
        if (!q.box_lo || !q.box_hi) return fail(MISTI_E_ARG, "box_lo / box_hi is NULL");
        for (int64_t b = 0; b < q.n_box; ++b) if (int r = check_box(a, N, b, nullptr)) return r;
    }
    return 0;
}

// The device state of a checked search with n_start >= 1: the minimiser's own state for n_start simplices of N coordinates, behind it
// the rows problem (RowsProblem: one of everything a start hands its points per slot of the five batches), behind that whatever
// `extra` takes - one allocation per type (simplices, points and values | counters and slot tables).  Uploads the caller's arrays and
// clears the context's work counters.
template <class Extra>
int nm_setup(misti_ctx* c, const misti_search_t& q, int N, bool whole, NmWork& w, Extra&& extra) {
    HIP_TRY(hipSetDevice(c->device));
    const size_t S = (size_t)q.n_start, V = (size_t)N + 1;
    const size_t cap = (size_t)nm_spec_cap(N), K = 4 + (size_t)N;
    const size_t M = S * V > cap * K ? S * V : cap * K;                         // the largest batch of the search
    misti::NmState& st = w.st;
    st.S = q.n_start; st.N = N; st.spec_cap = (int64_t)cap;
    const size_t slots[NM_BATCHES] = {S * V, S, S, S * N, cap * K};
    w.n_slots = 0;
    for (int b = 0; b < NM_BATCHES; ++b) { w.slots[b] = slots[b]; w.n_slots += slots[b]; }
    w.rows = RowsProblem(c, rows_args(q), N, whole);
    auto layout = [&](Carver<double>& f, Carver<int32_t>& i) {
        nm_per_slot(st.b, w.slots, NM_BATCHES, &NmBatch::pts, f, N);
        st.sim = st.b[misti::NM_B_INIT].pts;            // the initial batch is the simplices themselves
        st.scratch = f.take(S * V * N); st.fsim = f.take(S * V); st.fxr = f.take(S);
        nm_per_slot(st.b, w.slots, NM_BATCHES, &NmBatch::split, f, 1);
        for (int b = 0; b < NM_BATCHES; ++b) w.llk[b] = f.take(w.slots[b]);
        w.d_starts = f.take(S * N); w.d_llh = f.take(S); w.d_row = f.take(8);
        st.nit = i.take(S); st.nfev = i.take(S); st.done = i.take(S); st.kind = i.take(S); st.shrunk = i.take(S);
        w.idx[0] = i.take(S); w.idx[1] = i.take(S);
        w.cnt = i.take(4);                              // [2] live starts of the iteration in progress / of the next one
        w.rows.layout(f, i, st.b, w.slots, NM_BATCHES, M);
        extra(f, i);
    };
    if (int r = carve(c->nm_f64, c->nm_i32, layout)) return r;
    if (int r = live_words(c, "start")) return r;
    w.rows.fill(st.src);
    hipStream_t sm = c->stream;
    HIP_TRY(hipMemcpyAsync(w.d_starts, q.starts, S * N * sizeof(double), hipMemcpyHostToDevice, sm));
    if (!w.rows.a.rows_path()) HIP_TRY(hipMemcpyAsync(w.d_row, q.jsfs, 8 * sizeof(double), hipMemcpyHostToDevice, sm));
    if (int r = w.rows.upload(c)) return r;
    c->nm_iterations = c->nm_slots = c->nm_spec_iterations = 0;
    return 0;
}

// Basin hopping around a checked search with n_start >= 1 (a descriptor with hops): SciPy's runner per start, all starts in
// step - the initial minimisation, then per hop the displacement (bh_step), the minimisation of every trial point and the Metropolis
// test (bh_update).  The hop state lies behind the search's own in the same two allocations; with the split as a coordinate it is
// displaced like any other (bh.N counts it).
int bh_run(misti_ctx* c, const misti_search_t& q, int N, bool whole) {
    const misti_hops_t& h = *q.hops;
    const int niter = h.niter;
    const size_t S = (size_t)q.n_start, U = S * (size_t)niter * (size_t)(N + 1);
    NmWork w;
    misti::BhState bh{};
    bh.S = q.n_start; bh.N = N;
    bh.beta = h.T != 0.0 ? 1.0 / h.T : INFINITY;
    bh.target = h.target_accept_rate; bh.factor = h.stepwise_factor; bh.interval = h.interval;
    double *d_trial = nullptr, *d_uni = nullptr;
    auto bh_layout = [&](Carver<double>& f, Carver<int32_t>& i) {
        bh.x_cur = f.take(S * N); bh.x_best = f.take(S * N); d_trial = f.take(S * N);
        bh.f_cur = f.take(S); bh.f_best = f.take(S); bh.stepsize = f.take(S);
        d_uni = f.take(U);
        bh.ok_cur = i.take(S); bh.ok_best = i.take(S); bh.nstep = i.take(S); bh.naccept = i.take(S);
        bh.nfev = i.take(S); bh.failures = i.take(S); bh.accepted = i.take(S);
    };
    if (int r = nm_setup(c, q, N, whole, w, bh_layout)) return r;
    hipStream_t sm = c->stream;
    if (U) HIP_TRY(hipMemcpyAsync(d_uni, h.uniforms, U * sizeof(double), hipMemcpyHostToDevice, sm));
    {
        std::vector<double> st0(S, h.stepsize);
        HIP_TRY(hipMemcpyAsync(bh.stepsize, st0.data(), S * sizeof(double), hipMemcpyHostToDevice, sm));
        HIP_TRY(hipStreamSynchronize(sm));                  // st0 is a local
    }
    const double split_time = q.split == MISTI_SPLIT_ONE ? q.split_time : 0.0;
    // BasinHoppingRunner.__init__: the initial minimisation from the start itself
    if (int r = nm_run(c, w, split_time, q.xatol, q.fatol, q.maxiter, h.nm_maxfev)) return r;
    HIP_TRY(misti::launch_bh_update(bh, w.st, w.d_starts, w.d_llh, w.st.shrunk, -1, niter, d_uni, sm));
    for (int hop = 0; hop < niter; ++hop) {                 // one_cycle, all starts in step
        HIP_TRY(misti::launch_bh_step(bh, hop, niter, d_uni, d_trial, sm));
        HIP_TRY(hipMemcpyAsync(w.d_starts, d_trial, S * N * sizeof(double), hipMemcpyDeviceToDevice, sm));
        if (int r = nm_run(c, w, split_time, q.xatol, q.fatol, q.maxiter, h.nm_maxfev)) return r;
        HIP_TRY(misti::launch_bh_update(bh, w.st, w.d_starts, w.d_llh, w.st.shrunk, hop, niter, d_uni, sm));
    }
    HIP_TRY(misti::launch_bh_result(bh, w.d_starts, w.d_llh, sm));
    if (int r = nm_copy_back(c, w, q.x, q.llh, nullptr, nullptr, nullptr)) return r;
    if (h.nfev) HIP_TRY(hipMemcpyAsync(h.nfev, bh.nfev, S * sizeof(int32_t), hipMemcpyDeviceToHost, sm));
    if (h.failures) HIP_TRY(hipMemcpyAsync(h.failures, bh.failures, S * sizeof(int32_t), hipMemcpyDeviceToHost, sm));
    if (h.accepted) HIP_TRY(hipMemcpyAsync(h.accepted, bh.accepted, S * sizeof(int32_t), hipMemcpyDeviceToHost, sm));
    HIP_TRY(hipStreamSynchronize(sm));
    return 0;
}

// Every search and every basin hopping, as its descriptor says: the shared path behind misti_search and the ten older entry points.
int search_impl(misti_ctx* c, const misti_search_t& q) {
    int N = 0;
    bool whole = false;
    if (int r = nm_check(c, q, N, whole)) return r;
    if (q.n_start == 0) return 0;
    if (q.hops) return bh_run(c, q, N, whole);
    NmWork w;
    if (int r = nm_setup(c, q, N, whole, w, [](Carver<double>&, Carver<int32_t>&) {})) return r;
    if (int r = nm_run(c, w, q.split == MISTI_SPLIT_ONE ? q.split_time : 0.0, q.xatol, q.fatol, q.maxiter, INT64_MAX)) return r;
    if (int r = nm_copy_back(c, w, q.x, q.llh, q.nit, q.nfev, q.status)) return r;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// misti_nm_solve_box / misti_basinhopping_box took a box always: n_box == 0, "no box" in a descriptor, is theirs to refuse.
int no_box(int64_t n_box, int64_t n_start) {
    if (n_box == 0 && n_start != 0) return fail(MISTI_E_ARG, "n_box must be 1 or n_start (got 0 for %lld starts)", (long long)n_start);
    return 0;
}

// ---- differential evolution per search (misti_de.hip) ----------------------------------------------------------------------------
// The arguments of misti_de_search, before the first HIP call, in the header's order: what does not depend on the context, the
// context, what needs the model.  Leaves the number of coordinates in N and whether every split time is an integer in `whole`.
int de_check(const misti_ctx* c, const misti_de_t& q, int& N, bool& whole) {
    const RowsArgs a = rows_args(q);
    if (q.n_start < 0) return fail(MISTI_E_ARG, "negative number of searches");
    if (!q.starts || !q.rows || !q.jsfs || !q.box_lo || !q.box_hi || !q.x || !q.llh || (a.per_start() && !q.split_times))
        return fail(MISTI_E_ARG, "starts / rows / jsfs / box_lo / box_hi / x / llh%s is NULL", a.per_start() ? " / split_times" : "");
    if (q.n_rep < 1) return fail(MISTI_E_ARG, "n_rep must be >= 1 (got %lld)", (long long)q.n_rep);
    if (q.pop < 4) return fail(MISTI_E_ARG, "pop must be >= 4 (got %d)", (int)q.pop);
    if (q.pop > MISTI_DE_MAX_POP) return fail(MISTI_E_LIMIT, "pop = %d exceeds MISTI_DE_MAX_POP = %d", (int)q.pop, MISTI_DE_MAX_POP);
    if (q.maxiter < 1) return fail(MISTI_E_ARG, "maxiter must be >= 1");
    if (!(q.tol >= 0.0) || !(q.atol >= 0.0) || !std::isfinite(q.tol) || !std::isfinite(q.atol)) return fail(MISTI_E_ARG, "tol and atol must be finite and not negative");
    if (!std::isfinite(q.F_lo) || !std::isfinite(q.F_hi) || q.F_lo < 0.0 || q.F_lo > q.F_hi)
        return fail(MISTI_E_ARG, "F must be a finite range 0 <= F_lo <= F_hi (got %g, %g)", q.F_lo, q.F_hi);
    if (!(q.CR >= 0.0 && q.CR <= 1.0)) return fail(MISTI_E_ARG, "CR must lie in [0, 1] (got %g)", q.CR);
    if (int r = check_n_box(a, "searches")) return r;
    if (int r = check_rows(a, whole)) return r;
    if (int r = check_limits(c, a, q.pop, "searches x members", N)) return r;
    if (int r = check_finite(q.starts, q.n_start, N)) return r;
    for (int64_t b = 0; b < q.n_box; ++b) if (int r = check_box(a, N, b, "a population search needs a finite box")) return r;
    return 0;
}

// A checked call with n_start >= 1.  One batch record of n_start x pop slots serves the initial population and every generation;
// the state lies in the search buffers of the context (the batched Nelder-Mead's two allocations).
int de_run(misti_ctx* c, const misti_de_t& q, int N, bool whole) {
    using namespace misti;
    HIP_TRY(hipSetDevice(c->device));
    const size_t S = (size_t)q.n_start, P = (size_t)q.pop, M = S * P;
    RowsProblem rows(c, rows_args(q), N, whole);
    DeState st{};
    st.S = q.n_start; st.N = N; st.P = q.pop; st.maxiter = q.maxiter;
    st.tol = q.tol; st.atol = q.atol; st.F_lo = q.F_lo; st.F_hi = q.F_hi; st.CR = q.CR; st.seed = q.seed;
    double *llk = nullptr, *d_starts = nullptr, *d_llh = nullptr, *d_popllh = nullptr, *d_points = nullptr;
    int32_t *d_nfev = nullptr, *d_status = nullptr, *idx[2] = {nullptr, nullptr}, *cnt = nullptr;
    auto layout = [&](Carver<double>& f, Carver<int32_t>& i) {
        st.b.pts = f.take(M * N); st.pop = f.take(M * N); st.f = f.take(M); st.b.split = f.take(M); llk = f.take(M);
        d_starts = f.take(S * N); d_llh = f.take(S); d_popllh = f.take(M);
        d_points = f.take(1);                              // the point counter: an 8-byte word of the double buffer
        st.best = i.take(S); st.nit = i.take(S); st.done = i.take(S); d_nfev = i.take(S); d_status = i.take(S);
        idx[0] = i.take(S); idx[1] = i.take(S); cnt = i.take(4);
        rows.layout(f, i, &st.b, &M, 1, M);
    };
    if (int r = carve(c->nm_f64, c->nm_i32, layout)) return r;
    if (int r = live_words(c, "search")) return r;
    rows.fill(st.src);
    st.points = reinterpret_cast<unsigned long long*>(d_points);
    hipStream_t sm = c->stream;
    HIP_TRY(hipMemcpyAsync(d_starts, q.starts, S * N * sizeof(double), hipMemcpyHostToDevice, sm));
    if (int r = rows.upload(c)) return r;
    HIP_TRY(hipMemsetAsync(cnt, 0, 4 * sizeof(int32_t), sm));
    HIP_TRY(hipMemsetAsync(d_points, 0, sizeof(double), sm));
    c->nm_iterations = c->nm_slots = c->nm_spec_iterations = 0;
    // generation 0: every search in its own slot
    HIP_TRY(launch_de_init(st, d_starts, sm));
    if (int r = rows.eval(c, st.b, (int64_t)M, llk)) return r;
    int cur = 0;
    st.idx_cur = idx[cur ^ 1]; st.count_cur = cnt + (cur ^ 1);
    st.idx_next = idx[cur]; st.count_next = cnt + cur;
    HIP_TRY(launch_de_select(st, q.n_start, 0, llk, sm));
    Pacer pace(c);                                         // generations for iterations, live searches for live starts
    int64_t bound = 0;
    if (int r = pace.start(cnt + cur, bound)) return r;
    int64_t issued = 0, slots = 0;
    for (int it = 0; bound > 0 && it < q.maxiter; ++it) {
        if (int r = pace.bound(it, bound)) return r;
        if (bound <= 0) break;
        st.idx_cur = idx[cur]; st.count_cur = cnt + cur;
        st.idx_next = idx[cur ^ 1]; st.count_next = cnt + (cur ^ 1);
        HIP_TRY(launch_de_trial(st, bound, it + 1, sm));
        if (int r = rows.eval(c, st.b, bound * (int64_t)P, llk)) return r;
        HIP_TRY(hipMemsetAsync(cnt + (cur ^ 1), 0, sizeof(int32_t), sm));
        HIP_TRY(launch_de_select(st, bound, it + 1, llk, sm));
        if (int r = pace.record(it, cnt + (cur ^ 1))) return r;
        cur ^= 1;
        ++issued;
        slots += bound;
    }
    c->nm_iterations = issued;
    c->nm_slots = slots;
    HIP_TRY(launch_de_result(st, d_starts, d_llh, d_nfev, d_status, q.population_llh ? d_popllh : nullptr, sm));
    HIP_TRY(hipMemcpyAsync(q.x, d_starts, S * N * sizeof(double), hipMemcpyDeviceToHost, sm));
    HIP_TRY(hipMemcpyAsync(q.llh, d_llh, S * sizeof(double), hipMemcpyDeviceToHost, sm));
    if (q.nit) HIP_TRY(hipMemcpyAsync(q.nit, st.nit, S * sizeof(int32_t), hipMemcpyDeviceToHost, sm));
    if (q.nfev) HIP_TRY(hipMemcpyAsync(q.nfev, d_nfev, S * sizeof(int32_t), hipMemcpyDeviceToHost, sm));
    if (q.status) HIP_TRY(hipMemcpyAsync(q.status, d_status, S * sizeof(int32_t), hipMemcpyDeviceToHost, sm));
    if (q.population) HIP_TRY(hipMemcpyAsync(q.population, st.pop, M * N * sizeof(double), hipMemcpyDeviceToHost, sm));
    if (q.population_llh) HIP_TRY(hipMemcpyAsync(q.population_llh, d_popllh, M * sizeof(double), hipMemcpyDeviceToHost, sm));
    if (q.n_points) HIP_TRY(hipMemcpyAsync(q.n_points, d_points, sizeof(int64_t), hipMemcpyDeviceToHost, sm));
    HIP_TRY(hipStreamSynchronize(sm));
    return 0;
}

}  // namespace

extern "C" {

int misti_de_search(misti_ctx* c, const misti_de_t* q) {
    if (!q) return fail(MISTI_E_ARG, "the search descriptor is NULL");
    if (q->size != sizeof(misti_de_t))
        return fail(MISTI_E_ARG, "the search descriptor's size is %u, this library's misti_de_t has %u bytes", (unsigned)q->size, (unsigned)sizeof(misti_de_t));
    if (q->split != MISTI_SPLIT_PER_START && q->split != MISTI_SPLIT_FITTED)
        return fail(MISTI_E_ARG, "the search descriptor's split mode %d is neither MISTI_SPLIT_PER_START nor MISTI_SPLIT_FITTED", (int)q->split);
    int N = 0;
    bool whole = false;
    if (int r = de_check(c, *q, N, whole)) return r;
    if (q->n_start == 0) return 0;
    return de_run(c, *q, N, whole);
}

int misti_search(misti_ctx* c, const misti_search_t* q) {
    if (!q) return fail(MISTI_E_ARG, "the search descriptor is NULL");
    if (q->size != sizeof(misti_search_t))
        return fail(MISTI_E_ARG, "the search descriptor's size is %u, this library's misti_search_t has %u bytes", (unsigned)q->size, (unsigned)sizeof(misti_search_t));
    if (q->split != MISTI_SPLIT_ONE && q->split != MISTI_SPLIT_PER_START && q->split != MISTI_SPLIT_FITTED)
        return fail(MISTI_E_ARG, "the search descriptor's split mode %d is none of MISTI_SPLIT_*", (int)q->split);
    if (q->hops && (q->nit || q->nfev || q->status)) return fail(MISTI_E_ARG, "with hops, nit / nfev / status of the search must be NULL (the hops report their own)");
    return search_impl(c, *q);
}

// The ten older entry points: each fills the descriptor it is (in the descriptor's field order) and joins the shared path.
int misti_nm_solve(misti_ctx* c, int64_t n_start, const double* starts, double split_time, const double* jsfs_row,
                   double xatol, double fatol, int32_t maxiter,
                   double* x, double* llh, int32_t* nit, int32_t* nfev, int32_t* status) {
    return search_impl(c, {sizeof(misti_search_t), MISTI_SPLIT_ONE, split_time, nullptr, n_start, starts, nullptr, 1, jsfs_row, nullptr, nullptr,
                           0, nullptr, nullptr, xatol, fatol, maxiter, x, llh, nit, nfev, status, nullptr});
}

int misti_nm_solve_rows(misti_ctx* c, int64_t n_start, const double* starts, const double* split_times, const int32_t* rows,
                        int64_t n_rep, const double* jsfs, double xatol, double fatol, int32_t maxiter,
                        double* x, double* llh, int32_t* nit, int32_t* nfev, int32_t* status) {
    return misti_nm_solve_pulses(c, n_start, starts, split_times, rows, nullptr, nullptr, n_rep, jsfs, xatol, fatol, maxiter, x, llh, nit, nfev, status);
}

int misti_nm_solve_bounds(misti_ctx* c, int64_t n_start, const double* starts, const double* split_times, const int32_t* rows,
                          const int32_t* band_bounds, int64_t n_rep, const double* jsfs, double xatol, double fatol, int32_t maxiter,
                          double* x, double* llh, int32_t* nit, int32_t* nfev, int32_t* status) {
    return misti_nm_solve_pulses(c, n_start, starts, split_times, rows, band_bounds, nullptr, n_rep, jsfs, xatol, fatol, maxiter, x, llh, nit, nfev, status);
}

int misti_nm_solve_pulses(misti_ctx* c, int64_t n_start, const double* starts, const double* split_times, const int32_t* rows,
                          const int32_t* band_bounds, const int32_t* pulse_times, int64_t n_rep, const double* jsfs, double xatol, double fatol,
                          int32_t maxiter, double* x, double* llh, int32_t* nit, int32_t* nfev, int32_t* status) {
    return search_impl(c, {sizeof(misti_search_t), MISTI_SPLIT_PER_START, 0.0, split_times, n_start, starts, rows, n_rep, jsfs, band_bounds, pulse_times,
                           0, nullptr, nullptr, xatol, fatol, maxiter, x, llh, nit, nfev, status, nullptr});
}

int misti_nm_solve_split(misti_ctx* c, int64_t n_start, const double* starts, const int32_t* rows, const int32_t* band_bounds,
                         const int32_t* pulse_times, int64_t n_rep, const double* jsfs, double xatol, double fatol, int32_t maxiter,
                         double* x, double* llh, int32_t* nit, int32_t* nfev, int32_t* status) {
    return search_impl(c, {sizeof(misti_search_t), MISTI_SPLIT_FITTED, 0.0, nullptr, n_start, starts, rows, n_rep, jsfs, band_bounds, pulse_times,
                           0, nullptr, nullptr, xatol, fatol, maxiter, x, llh, nit, nfev, status, nullptr});
}

int misti_nm_solve_box(misti_ctx* c, int64_t n_start, const double* starts, const double* split_times, const int32_t* rows,
                       int64_t n_rep, const double* jsfs, const int32_t* band_bounds, const int32_t* pulse_times,
                       int64_t n_box, const double* box_lo, const double* box_hi, double xatol, double fatol, int32_t maxiter,
                       double* x, double* llh, int32_t* nit, int32_t* nfev, int32_t* status) {
    if (int r = no_box(n_box, n_start)) return r;
    return search_impl(c, {sizeof(misti_search_t), split_times ? MISTI_SPLIT_PER_START : MISTI_SPLIT_FITTED, 0.0, split_times, n_start, starts, rows, n_rep, jsfs,
                           band_bounds, pulse_times, n_box, box_lo, box_hi, xatol, fatol, maxiter, x, llh, nit, nfev, status, nullptr});
}

int misti_basinhopping(misti_ctx* c, int64_t n_start, const double* starts, double split_time, const double* jsfs_row,
                       int32_t niter, double T, double stepsize, int32_t interval, double target_accept_rate, double stepwise_factor,
                       double xatol, double fatol, int32_t nm_maxiter, int64_t nm_maxfev, const double* uniforms,
                       double* x, double* llh, int32_t* nfev, int32_t* failures, int32_t* accepted) {
    // (this entry point's own order of checks, older than nm_check's: the context first, no starts before the pointers; what passes
    //  them passes nm_check)
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    if (n_start < 0 || niter < 0) return fail(MISTI_E_ARG, "negative number of starts / hops");
    if (n_start == 0) return 0;
    const int N = c->dm.n_param;
    if (N < 1) return fail(MISTI_E_ARG, "the model has no optimised parameter");
    if (!starts || !jsfs_row || !x || !llh || (niter > 0 && !uniforms)) return fail(MISTI_E_ARG, "starts / jsfs_row / uniforms / x / llh is NULL");
    if (nm_maxiter < 1 || nm_maxfev < 1 || interval < 1) return fail(MISTI_E_ARG, "nm_maxiter, nm_maxfev and interval must be >= 1");
    if (n_start > INT32_MAX / (8 * (N + 1))) return fail(MISTI_E_LIMIT, "too many starts for one call");
    const misti_hops_t h{niter, T, stepsize, interval, target_accept_rate, stepwise_factor, nm_maxfev, uniforms, nfev, failures, accepted};
    return search_impl(c, {sizeof(misti_search_t), MISTI_SPLIT_ONE, split_time, nullptr, n_start, starts, nullptr, 1, jsfs_row, nullptr, nullptr,
                           0, nullptr, nullptr, xatol, fatol, nm_maxiter, x, llh, nullptr, nullptr, nullptr, &h});
}

int misti_basinhopping_rows(misti_ctx* c, int64_t n_start, const double* starts, const double* split_times, const int32_t* rows,
                            const int32_t* band_bounds, const int32_t* pulse_times, int64_t n_rep, const double* jsfs,
                            int32_t niter, double T, double stepsize, int32_t interval, double target_accept_rate, double stepwise_factor,
                            double xatol, double fatol, int32_t nm_maxiter, int64_t nm_maxfev, const double* uniforms,
                            double* x, double* llh, int32_t* nfev, int32_t* failures, int32_t* accepted) {
    const misti_hops_t h{niter, T, stepsize, interval, target_accept_rate, stepwise_factor, nm_maxfev, uniforms, nfev, failures, accepted};
    return search_impl(c, {sizeof(misti_search_t), MISTI_SPLIT_PER_START, 0.0, split_times, n_start, starts, rows, n_rep, jsfs, band_bounds, pulse_times,
                           0, nullptr, nullptr, xatol, fatol, nm_maxiter, x, llh, nullptr, nullptr, nullptr, &h});
}

int misti_basinhopping_split(misti_ctx* c, int64_t n_start, const double* starts, const int32_t* rows,
                             const int32_t* band_bounds, const int32_t* pulse_times, int64_t n_rep, const double* jsfs,
                             int32_t niter, double T, double stepsize, int32_t interval, double target_accept_rate, double stepwise_factor,
                             double xatol, double fatol, int32_t nm_maxiter, int64_t nm_maxfev, const double* uniforms,
                             double* x, double* llh, int32_t* nfev, int32_t* failures, int32_t* accepted) {
    const misti_hops_t h{niter, T, stepsize, interval, target_accept_rate, stepwise_factor, nm_maxfev, uniforms, nfev, failures, accepted};
    return search_impl(c, {sizeof(misti_search_t), MISTI_SPLIT_FITTED, 0.0, nullptr, n_start, starts, rows, n_rep, jsfs, band_bounds, pulse_times,
                           0, nullptr, nullptr, xatol, fatol, nm_maxiter, x, llh, nullptr, nullptr, nullptr, &h});
}

int misti_basinhopping_box(misti_ctx* c, int64_t n_start, const double* starts, const double* split_times, const int32_t* rows,
                           int64_t n_rep, const double* jsfs, const int32_t* band_bounds, const int32_t* pulse_times,
                           int64_t n_box, const double* box_lo, const double* box_hi,
                           int32_t niter, double T, double stepsize, int32_t interval, double target_accept_rate, double stepwise_factor,
                           double xatol, double fatol, int32_t nm_maxiter, int64_t nm_maxfev, const double* uniforms,
                           double* x, double* llh, int32_t* nfev, int32_t* failures, int32_t* accepted) {
    if (int r = no_box(n_box, n_start)) return r;
    const misti_hops_t h{niter, T, stepsize, interval, target_accept_rate, stepwise_factor, nm_maxfev, uniforms, nfev, failures, accepted};
    return search_impl(c, {sizeof(misti_search_t), split_times ? MISTI_SPLIT_PER_START : MISTI_SPLIT_FITTED, 0.0, split_times, n_start, starts, rows, n_rep, jsfs,
                           band_bounds, pulse_times, n_box, box_lo, box_hi, xatol, fatol, nm_maxiter, x, llh, nullptr, nullptr, nullptr, &h});
}

int misti_nm_last_stats(misti_ctx* c, int64_t stats[2]) {
    if (!c || !stats) return fail(MISTI_E_ARG, "ctx / output is NULL");
    stats[0] = c->nm_iterations;
    stats[1] = c->nm_slots;
    return 0;
}

int misti_nm_last_spec_iterations(misti_ctx* c, int64_t* n) {
    if (!c || !n) return fail(MISTI_E_ARG, "ctx / output is NULL");
    *n = c->nm_spec_iterations;
    return 0;
}

}  // extern "C"
