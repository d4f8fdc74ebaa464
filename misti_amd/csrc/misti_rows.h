// What the searches (misti_search.cpp) and the samplers (misti_sampler.cpp) are handed alike: the rows problem with its checks, the
// slots of a search's batches, and the pacing of a search that runs ahead of the device.  Internal: never installed.
#pragma once
#include <cassert>
#include <cmath>

#include "misti_ctx.h"

namespace misti_host __attribute__((visibility("hidden"))) {

using misti::NmBatch;
using misti::NM_BATCHES;

// One array per batch of a search, `width` elements per slot.  The arrays of a kind lie back to back: nm_run clears a whole kind
// of its five batches with ONE memset over all their slots (a memset per batch would be four launches more per kind), so a kind is
// carved here and nowhere else.
template <class T>
void nm_per_slot(NmBatch* b, const size_t* slots, int n_batch, T* NmBatch::*arr, Carver<T>& from, size_t width) {
    size_t all = 0;
    for (int k = 0; k < n_batch; ++k) { b[k].*arr = from.take(slots[k] * width); all += slots[k]; }
    assert(!(b[0].*arr) || b[n_batch - 1].*arr + slots[n_batch - 1] * width == b[0].*arr + all * width);
    (void)all;
}

// ---- the rows problem: what Nelder-Mead, differential evolution and the ensemble sampler are handed alike ------------------------------
// A start or search s with a split time, a row of a replicate table, optional band bounds and pulse times, an optional box, and
// optionally the split as the last coordinate.  A per-start field is added HERE, to RowsProblem below and to PointSource / put_point
// (misti_device.h) - nowhere else.  The public descriptors lay these fields out differently: one rows_args() each.
struct RowsArgs {
    int32_t split;                   // MISTI_SPLIT_*
    double split_time;               // MISTI_SPLIT_ONE
    const double* split_times;       // MISTI_SPLIT_PER_START
    int64_t n_start;
    const int32_t* rows;
    int64_t n_rep;
    const double* jsfs;
    const int32_t *band_bounds, *pulse_times;
    int64_t n_box;
    const double *box_lo, *box_hi;
    const uint64_t* ids;
    bool rows_path() const { return split != MISTI_SPLIT_ONE; }
    bool per_start() const { return split == MISTI_SPLIT_PER_START; }
    bool fit_split() const { return split == MISTI_SPLIT_FITTED; }
};
inline RowsArgs rows_args(const misti_search_t& q) {
    return {q.split, q.split_time, q.split_times, q.n_start, q.rows, q.n_rep, q.jsfs, q.band_bounds, q.pulse_times, q.n_box, q.box_lo, q.box_hi, nullptr};
}
inline RowsArgs rows_args(const misti_de_t& q) {
    return {q.split, 0.0, q.split_times, q.n_start, q.rows, q.n_rep, q.jsfs, q.band_bounds, q.pulse_times, q.n_box, q.box_lo, q.box_hi, q.ids};
}
inline RowsArgs rows_args(const misti_ens_t& q) {
    return {q.split, 0.0, q.split_times, q.n_start, q.rows, q.n_rep, q.jsfs, q.band_bounds, q.pulse_times, q.n_box, q.box_lo, q.box_hi, q.ids};
}
inline RowsArgs rows_args(const misti_pt_t& q) {
    return {q.split, 0.0, q.split_times, q.n_start, q.rows, q.n_rep, q.jsfs, q.band_bounds, q.pulse_times, q.n_box, q.box_lo, q.box_hi, q.ids};
}

// The checks the three doors share.  Each door calls them where its header's order of refusals puts them (nm_check, de_check,
// sampler_check); `noun` is what the door calls its n_start.
inline int check_n_box(const RowsArgs& a, const char* noun) {
    if (a.n_box != 1 && a.n_box != a.n_start)
        return fail(MISTI_E_ARG, "n_box must be 1 or n_start (got %lld for %lld %s)", (long long)a.n_box, (long long)a.n_start, noun);
    return 0;
}
// every row inside the table, every split time of MISTI_SPLIT_PER_START finite; `whole`: every such split time is an integer (a
// fitted split is whole by accident only: never the integer-splits hint)
inline int check_rows(const RowsArgs& a, bool& whole) {
    whole = a.per_start();
    for (int64_t s = 0; a.rows_path() && s < a.n_start; ++s) {
        if (a.rows[s] < 0 || a.rows[s] >= a.n_rep)
            return fail(MISTI_E_ARG, "rows[%lld] = %d is outside the table (n_rep = %lld)", (long long)s, (int)a.rows[s], (long long)a.n_rep);
        if (!a.per_start()) continue;
        if (!std::isfinite(a.split_times[s])) return fail(MISTI_E_ARG, "split_times[%lld] is not finite", (long long)s);
        if (a.split_times[s] != std::floor(a.split_times[s])) whole = false;
    }
    return 0;
}
// the context, the number of coordinates N it gives, and the limits: a search of `per` points per start (`noun` names the product)
// keeps every slot index of its batches below INT32_MAX / 8.  (The limits before any scan of the starts: a call that is refused for
// its size does not read n_start x N doubles first.)
inline int check_limits(const misti_ctx* c, const RowsArgs& a, int64_t per, const char* noun, int& N) {
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    N = c->dm.n_param + (a.fit_split() ? 1 : 0);
    if (N < 1) return fail(MISTI_E_ARG, "the model has no optimised parameter");
    // the sort's local arrays hold MISTI_MAX_PARAMS + 1 vertices (misti_nm.hip: sort_simplex)
    if (N > MISTI_MAX_PARAMS) return fail(MISTI_E_LIMIT, "the split as a coordinate needs n_param + 1 <= %d (n_param = %d)", MISTI_MAX_PARAMS, c->dm.n_param);
    if (a.n_start > INT32_MAX / 8 / (N + 1) / per) return fail(MISTI_E_LIMIT, "too many %s for one call", noun);
    if (a.n_rep > INT32_MAX) return fail(MISTI_E_LIMIT, "too many replicate rows for one call");
    return 0;
}
inline int check_finite(const double* starts, int64_t n_start, int N) {
    for (int64_t s = 0; s < n_start; ++s)
        for (int k = 0; k < N; ++k)
            if (!std::isfinite(starts[s * N + k])) return fail(MISTI_E_ARG, "starts[%lld][%d] is not finite", (long long)s, k);
    return 0;
}
// box b of the call: neither bound NaN, lo <= hi (lo == hi holds a coordinate fixed).  `finite`: why the door needs a finite box -
// then an infinite bound or width is refused as well; NULL: +-inf leaves a side open.
inline int check_box(const RowsArgs& a, int N, int64_t b, const char* finite) {
    for (int k = 0; k < N; ++k) {
        const double lo = a.box_lo[b * N + k], hi = a.box_hi[b * N + k];
        if (!finite && (lo != lo || hi != hi)) return fail(MISTI_E_ARG, "box %lld, coordinate %d: a bound is NaN", (long long)b, k);
        if (finite && (!std::isfinite(lo) || !std::isfinite(hi))) return fail(MISTI_E_ARG, "box %lld, coordinate %d: a bound is not finite (%s)", (long long)b, k, finite);
        if (lo > hi) return fail(MISTI_E_ARG, "box %lld, coordinate %d: the lower bound %g is greater than the upper bound %g", (long long)b, k, lo, hi);
        if (finite && !std::isfinite(hi - lo)) return fail(MISTI_E_ARG, "box %lld, coordinate %d: hi - lo is not finite", (long long)b, k);
    }
    return 0;
}

// The device side of checked RowsArgs with n_start >= 1: what each start hands its points (split, row, bounds, pulse times, box, id),
// one of each per slot of the batches it is given, the compact parameter array of a fitted split, the table with the llh_const of
// every row, and where a batch of the rows path is evaluated into.  A path that is not taken allocates and writes nothing: without
// bounds nothing of the bounds path, and so on; with MISTI_SPLIT_ONE only the box.
struct RowsProblem {
    RowsArgs a{};
    int N = 0;
    bool whole = false;              // every split time is an integer: the rows path's one hint
    size_t S = 0, R = 0, NB2 = 0, NP = 0, NQ = 0, NX = 0;
    double *d_split = nullptr, *d_table = nullptr, *d_consts = nullptr, *d_lo = nullptr, *d_hi = nullptr, *d_ids = nullptr;
    int32_t *d_rowof = nullptr, *d_bounds = nullptr, *d_pulses = nullptr;
    double* rjafs = nullptr;         // [M][7]  a batch is evaluated without replicates into rjafs / rstatus, then llk_rows_kernel scores
    int32_t* rstatus = nullptr;      // [M]     every candidate against its own row of the table

    RowsProblem() = default;
    RowsProblem(const misti_ctx* c, const RowsArgs& a_, int N_, bool whole_) : a(a_), N(N_), whole(whole_) {
        S = (size_t)a.n_start; R = (size_t)a.n_rep;
        // int32 per bound set and per pulse-time set (none for a model without bands / pulses: the engine has nothing to apply them
        // to), doubles per compact parameter vector (no width for a model without parameters), doubles per box array
        NB2 = a.rows_path() && a.band_bounds ? 2 * (size_t)c->dm.n_band : 0;
        NP = a.rows_path() && a.pulse_times ? (size_t)c->dm.n_pulse : 0;
        NQ = a.fit_split() ? (size_t)N - 1 : 0;
        NX = (size_t)a.n_box * (size_t)N;
    }
    // `n_batch` batches of slots[.] slots, the largest evaluation M points
    void layout(Carver<double>& f, Carver<int32_t>& i, NmBatch* b, const size_t* slots, int n_batch, size_t M) {
        if (a.rows_path()) {
            if (a.per_start()) d_split = f.take(S);
            d_table = f.take(R * 8); d_consts = f.take(R); rjafs = f.take(M * 7);
            if (NQ) nm_per_slot(b, slots, n_batch, &NmBatch::par, f, NQ);
            d_rowof = i.take(S);
            nm_per_slot(b, slots, n_batch, &NmBatch::row, i, 1);
            rstatus = i.take(M);
            if (NB2) { d_bounds = i.take(S * NB2); nm_per_slot(b, slots, n_batch, &NmBatch::bnd, i, NB2); }
            if (NP) { d_pulses = i.take(S * NP); nm_per_slot(b, slots, n_batch, &NmBatch::put, i, NP); }
        }
        if (NX) { d_lo = f.take(NX); d_hi = f.take(NX); }
        if (a.ids) d_ids = f.take(S);                      // uint64 ids: 8-byte words of the double buffer
    }
    // the caller's arrays to the device, and llh_const over the table: once per call, every row
    int upload(misti_ctx* c) const {
        hipStream_t sm = c->stream;
        if (d_split) HIP_TRY(hipMemcpyAsync(d_split, a.split_times, S * sizeof(double), hipMemcpyHostToDevice, sm));
        if (d_rowof) HIP_TRY(hipMemcpyAsync(d_rowof, a.rows, S * sizeof(int32_t), hipMemcpyHostToDevice, sm));
        if (NB2) HIP_TRY(hipMemcpyAsync(d_bounds, a.band_bounds, S * NB2 * sizeof(int32_t), hipMemcpyHostToDevice, sm));
        if (NP) HIP_TRY(hipMemcpyAsync(d_pulses, a.pulse_times, S * NP * sizeof(int32_t), hipMemcpyHostToDevice, sm));
        if (NX) {
            HIP_TRY(hipMemcpyAsync(d_lo, a.box_lo, NX * sizeof(double), hipMemcpyHostToDevice, sm));
            HIP_TRY(hipMemcpyAsync(d_hi, a.box_hi, NX * sizeof(double), hipMemcpyHostToDevice, sm));
        }
        if (d_ids) HIP_TRY(hipMemcpyAsync(d_ids, a.ids, S * sizeof(uint64_t), hipMemcpyHostToDevice, sm));
        if (d_table) {
            HIP_TRY(hipMemcpyAsync(d_table, a.jsfs, R * 8 * sizeof(double), hipMemcpyHostToDevice, sm));
            HIP_TRY(misti::launch_llh_const(a.n_rep, d_table, d_consts, c->unfolded, sm));
        }
        return 0;
    }
    void fill(misti::PointSource& src) const {
        src.N = N; src.split = a.rows_path() ? 0.0 : a.split_time;
        src.split_of = d_split; src.row_of = d_rowof;
        src.bounds_of = d_bounds; src.nb2 = (int)NB2;
        src.pulses_of = d_pulses; src.np = (int)NP;
        src.fit_split = a.fit_split() ? 1 : 0;
        src.box_lo = d_lo; src.box_hi = d_hi; src.box_per_start = a.n_box > 1 ? 1 : 0;
        src.ids = reinterpret_cast<const uint64_t*>(d_ids);
    }
    // One batch of the rows path through the engine: the first n slots of `b` evaluated without replicates into rjafs / rstatus, with
    // each slot's own band bounds and pulse times where the batch carries them, then every point scored against its own row of the
    // table.  With the split as a coordinate the engine reads the batch's compact parameter vectors, not the points (NULL for a model
    // without parameters, as misti_eval_batch allows).  The one hint: integer splits where the caller's are; a fitted split is never
    // known to be whole.  `mask`: the hints a diagnostic run lets through.
    int eval(misti_ctx* c, const NmBatch& b, int64_t n, double* llk, unsigned mask = ~0u) const {
        const unsigned hints = (whole ? RUN_INTEGER_SPLITS : 0u) & mask;
        if (int r = run_dev(c, n, b.split, a.fit_split() ? b.par : b.pts, b.bnd, 0, nullptr, nullptr, rjafs, nullptr, nullptr, rstatus, hints, b.put)) return r;
        HIP_TRY(misti::launch_llk_rows(n, rjafs, rstatus, b.row, d_table, d_consts, llk, c->unfolded, c->stream));
        return 0;
    }
};

// The pinned words the live count of a paced search comes back in (Pacer): made by the context's first paced search, behind the
// carving of its workspace.  `noun`: what the caller's count counts.
inline int live_words(misti_ctx* c, const char* noun) {
    if (c->nm_live_host || hipHostMalloc((void**)&c->nm_live_host, 4 * sizeof(int32_t), hipHostMallocDefault) == hipSuccess) return 0;
    (void)hipGetLastError();
    c->nm_live_host = nullptr;
    return fail(MISTI_E_HIP, "pinned allocation for the live-%s count failed", noun);
}

// A paced search: the host runs at most two iterations ahead of the device.  Before issuing iteration k it waits for the event of
// iteration k - 2 and reads the count of live starts that iteration left in pinned memory (4 bytes; nothing else of the search
// leaves the device).  That count bounds the live starts of iteration k from above - the number only falls - and sizes its
// batches; zero -> stop issuing.
struct Pacer {
    hipStream_t sm;
    volatile int32_t* live;          // the context's pinned words (live_words): [it & 1] the count iteration `it` left
    hipEvent_t ev[2] = {nullptr, nullptr};
    explicit Pacer(misti_ctx* c) : sm(c->stream), live(c->nm_live_host) {}
    Pacer(const Pacer&) = delete;
    ~Pacer() { for (int i = 0; i < 2; ++i) if (ev[i]) (void)hipEventDestroy(ev[i]); }
    // the count the search's set-up left in d_count (stream order): the bound of iteration 0
    int start(const int32_t* d_count, int64_t& bound) {
        for (int i = 0; i < 2; ++i) HIP_TRY(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
        live[0] = live[1] = -1;
        HIP_TRY(hipMemcpyAsync((void*)&live[0], d_count, sizeof(int32_t), hipMemcpyDeviceToHost, sm));
        HIP_TRY(hipEventRecord(ev[0], sm));
        HIP_TRY(hipEventSynchronize(ev[0]));
        bound = live[0];
        return 0;
    }
    // the bound of iteration `it`: lowered to the count iteration it - 2 left
    int bound(int it, int64_t& bound) {
        if (it < 2) return 0;
        HIP_TRY(hipEventSynchronize(ev[it & 1]));
        if (live[it & 1] < bound) bound = live[it & 1];
        return 0;
    }
    int32_t* word(int it) { return (int32_t*)&live[it & 1]; }
    // iteration `it` is issued: its count from d_count, or (NULL) already on its way into word(it) by the iteration's own kernel
    int record(int it, const int32_t* d_count) {
        if (d_count) HIP_TRY(hipMemcpyAsync((void*)word(it), d_count, sizeof(int32_t), hipMemcpyDeviceToHost, sm));
        HIP_TRY(hipEventRecord(ev[it & 1], sm));
        return 0;
    }
};

}  // namespace misti_host
