// Curvature at fitted points (include/misti_hip.h: misti_curvature, misti_curvature_assemble_dev): the stencil laid out on the device,
// its candidates through the batch path (run_dev, misti_api.cpp), the derivatives assembled and contracted there.
#include <cmath>
#include <new>

#include "misti_ctx.h"

using namespace misti_host;

namespace {

// What misti_curvature_assemble_dev and misti_curvature share behind the spectra: derivatives of the class logs, then (with rows) the
// contraction with each point's row.  d_dlog / d_d2log NULL with a contraction wanted: the context's own buffers take their place.
int curv_assemble(misti_ctx* c, int64_t n_point, const double* d_jafs, const int32_t* d_status, const double* d_h, const int32_t* d_slot,
                  const int32_t* d_pre_status, const int32_t* d_rows, const double* d_jsfs, double* d_dlog, double* d_d2log,
                  double* d_grad, double* d_hess, int32_t* d_point_status, const double* d_consts, double* d_llh0) {
    const int D = c->dm.n_param;
    HIP_TRY(misti::launch_curv_assemble(n_point, D, c->unfolded, d_jafs, d_status, d_h, d_slot, d_pre_status, d_dlog, d_d2log, d_point_status, c->stream));
    if (d_rows)
        HIP_TRY(misti::launch_curv_contract(n_point, D, c->unfolded, d_dlog, d_d2log, d_point_status, d_rows, d_jsfs, d_grad, d_hess, d_jafs, d_slot,
                                            d_consts, d_llh0, c->stream));
    return 0;
}

int curvature_impl(misti_ctx* c, int64_t n_point, const double* x, const double* split_times, const int32_t* rows, const int32_t* band_bounds,
                   const int32_t* pulse_times, int64_t n_rep, const double* jsfs, double rel_step, double abs_step, int64_t batch_limit,
                   double* llh0, double* grad, double* hess, double* dlog, int32_t* point_status) {
    // the arguments, before the first HIP call: what does not depend on the context, the context, what needs the model (nm_check's order)
    if (n_point < 0) return fail(MISTI_E_ARG, "negative number of points");
    if (!x || !split_times || !rows || !jsfs || !point_status) return fail(MISTI_E_ARG, "x / split_times / rows / jsfs / point_status is NULL");
    if (n_rep < 1) return fail(MISTI_E_ARG, "n_rep must be >= 1 (got %lld)", (long long)n_rep);
    if (!std::isfinite(rel_step) || !std::isfinite(abs_step) || rel_step < 0.0 || abs_step < 0.0 || !(rel_step > 0.0 || abs_step > 0.0))
        return fail(MISTI_E_ARG, "rel_step and abs_step must be finite and not negative, and one of them positive (got %g, %g)", rel_step, abs_step);
    if (batch_limit < 0) return fail(MISTI_E_ARG, "negative batch_limit");
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    const int D = c->dm.n_param;
    if (D < 1) return fail(MISTI_E_ARG, "the model has no optimised parameter");
    const int64_t M = 1 + 2 * (int64_t)D * D;
    if (batch_limit > 0 && batch_limit < M) return fail(MISTI_E_ARG, "batch_limit = %lld is below the %lld candidates of one point's stencil", (long long)batch_limit, (long long)M);
    if (n_point > INT32_MAX / M) return fail(MISTI_E_LIMIT, "n_point x %lld stencil candidates exceeds INT32_MAX", (long long)M);
    if (n_rep > INT32_MAX) return fail(MISTI_E_LIMIT, "too many replicate rows for one call");
    // the host applies the stencil's boundary rule itself - the same two operations as curv_steps_kernel - to know how many
    // candidates the device will emit; the compacted index itself is built on the device
    bool whole = true;
    int64_t n_live = 0;                                                   // points with a stencil
    for (int64_t p = 0; p < n_point; ++p) {
        if (rows[p] < 0 || rows[p] >= n_rep)
            return fail(MISTI_E_ARG, "rows[%lld] = %d is outside the table (n_rep = %lld)", (long long)p, (int)rows[p], (long long)n_rep);
        if (!std::isfinite(split_times[p])) return fail(MISTI_E_ARG, "split_times[%lld] is not finite", (long long)p);
        if (split_times[p] != std::floor(split_times[p])) whole = false;
        bool boundary = false;
        for (int i = 0; i < D; ++i) {
            const double xi = x[p * D + i];
            if (!std::isfinite(xi)) return fail(MISTI_E_ARG, "x[%lld][%d] is not finite", (long long)p, i);
            const double hi = (xi + std::fmax(rel_step * std::fabs(xi), abs_step)) - xi;
            boundary = boundary || xi - hi < 0.0 || hi == 0.0;
        }
        n_live += boundary ? 0 : 1;
    }
    if (n_point == 0) return 0;
    const size_t P = (size_t)n_point, L = (size_t)n_live, C = L * (size_t)M, R = (size_t)n_rep;
    const size_t NB2 = band_bounds ? 2 * (size_t)c->dm.n_band : 0, NP = pulse_times ? (size_t)c->dm.n_pulse : 0;
    if (batch_limit == 0) batch_limit = M > 16384 ? M : 16384;
    if (batch_limit > INT32_MAX / 8) batch_limit = INT32_MAX / 8;            // one engine call's own limit
    HIP_TRY(hipSetDevice(c->device));
    double *d_x, *d_split, *d_table, *d_consts, *d_h, *c_split, *c_params, *c_jafs, *d_dlog, *d_d2log, *d_grad, *d_hess, *d_llh0;
    int32_t *d_rows, *d_bounds = nullptr, *d_pulses = nullptr, *d_pre, *d_slot, *d_pstatus, *c_bounds = nullptr, *c_pulses = nullptr, *c_status;
    auto layout = [&](Carver<double>& f, Carver<int32_t>& q) {
        d_x = f.take(P * D); d_split = f.take(P); d_table = f.take(R * 8); d_consts = f.take(R); d_h = f.take(P * D);
        c_split = f.take(C); c_params = f.take(C * D); c_jafs = f.take(C * 7);
        d_dlog = f.take(P * D * 7); d_d2log = f.take(P * D * D * 7); d_grad = f.take(P * D); d_hess = f.take(P * D * D); d_llh0 = f.take(P);
        d_rows = q.take(P); d_pre = q.take(P); d_slot = q.take(P); d_pstatus = q.take(P); c_status = q.take(C);
        if (NB2) { d_bounds = q.take(P * NB2); c_bounds = q.take(C * NB2); }
        if (NP) { d_pulses = q.take(P * NP); c_pulses = q.take(C * NP); }
    };
    if (int r = carve(c->curv_f64, c->curv_i32, layout)) return r;
    hipStream_t sm = c->stream;
    HIP_TRY(hipMemcpyAsync(d_x, x, P * D * sizeof(double), hipMemcpyHostToDevice, sm));
    HIP_TRY(hipMemcpyAsync(d_split, split_times, P * sizeof(double), hipMemcpyHostToDevice, sm));
    HIP_TRY(hipMemcpyAsync(d_rows, rows, P * sizeof(int32_t), hipMemcpyHostToDevice, sm));
    HIP_TRY(hipMemcpyAsync(d_table, jsfs, R * 8 * sizeof(double), hipMemcpyHostToDevice, sm));
    if (NB2) HIP_TRY(hipMemcpyAsync(d_bounds, band_bounds, P * NB2 * sizeof(int32_t), hipMemcpyHostToDevice, sm));
    if (NP) HIP_TRY(hipMemcpyAsync(d_pulses, pulse_times, P * NP * sizeof(int32_t), hipMemcpyHostToDevice, sm));
    HIP_TRY(misti::launch_llh_const(n_rep, d_table, d_consts, c->unfolded, sm));
    // a slot the device does not fill (it fills every one: the host's count is the device's) would be an empty slot to the engine
    if (C) HIP_TRY(hipMemsetAsync(c_split, 0xBF, C * sizeof(double), sm));
    HIP_TRY(misti::launch_curv_stencil(n_point, D, d_x, d_split, d_bounds, (int)NB2, d_pulses, (int)NP, rel_step, abs_step, (int64_t)L, d_h, d_pre,
                                       d_slot, c_split, c_params, c_bounds, c_pulses, sm));
    // whole points into engine batches: compacted points [a, b) are candidates [a M, b M)
    const int64_t per_batch = batch_limit / M;
    for (int64_t a = 0; a < (int64_t)L; a += per_batch) {
        const int64_t b = a + per_batch < (int64_t)L ? a + per_batch : (int64_t)L;
        const size_t o = (size_t)(a * M);
        if (int r = run_dev(c, (b - a) * M, c_split + o, c_params + o * D, NB2 ? c_bounds + o * NB2 : nullptr, 0, nullptr, nullptr, c_jafs + o * 7,
                            nullptr, nullptr, c_status + o, whole ? RUN_INTEGER_SPLITS : 0u, NP ? c_pulses + o * NP : nullptr)) return r;
    }
    if (int r = curv_assemble(c, n_point, c_jafs, c_status, d_h, d_slot, d_pre, d_rows, d_table, d_dlog, d_d2log, d_grad, d_hess, d_pstatus, d_consts, d_llh0))
        return r;
    if (llh0) HIP_TRY(hipMemcpyAsync(llh0, d_llh0, P * sizeof(double), hipMemcpyDeviceToHost, sm));
    if (grad) HIP_TRY(hipMemcpyAsync(grad, d_grad, P * D * sizeof(double), hipMemcpyDeviceToHost, sm));
    if (hess) HIP_TRY(hipMemcpyAsync(hess, d_hess, P * D * D * sizeof(double), hipMemcpyDeviceToHost, sm));
    if (dlog) HIP_TRY(hipMemcpyAsync(dlog, d_dlog, P * D * 7 * sizeof(double), hipMemcpyDeviceToHost, sm));
    HIP_TRY(hipMemcpyAsync(point_status, d_pstatus, P * sizeof(int32_t), hipMemcpyDeviceToHost, sm));
    HIP_TRY(hipStreamSynchronize(sm));
    return 0;
}

}  // namespace

extern "C" {

int misti_curvature_assemble_dev(misti_ctx* c, int64_t n_point, const double* d_jafs, const int32_t* d_status, const double* d_h,
                                 const int32_t* d_rows, int64_t n_rep, const double* d_jsfs,
                                 double* d_dlog, double* d_d2log, double* d_grad, double* d_hess, int32_t* d_point_status) {
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    const int D = c->dm.n_param;
    if (D < 1) return fail(MISTI_E_ARG, "the model has no optimised parameter");
    if (n_point < 0) return fail(MISTI_E_ARG, "negative number of points");
    const int64_t M = 1 + 2 * (int64_t)D * D;
    if (n_point > INT32_MAX / M) return fail(MISTI_E_LIMIT, "n_point x %lld stencil candidates exceeds INT32_MAX", (long long)M);
    if (!d_rows && (d_grad || d_hess)) return fail(MISTI_E_ARG, "grad / hess need a row per point: d_rows is NULL");
    if (d_rows && (n_rep < 1 || !d_jsfs)) return fail(MISTI_E_ARG, "d_rows needs the replicate table: n_rep < 1 or d_jsfs is NULL");
    if (n_point == 0) return 0;
    if (!d_jafs || !d_h || !d_point_status) return fail(MISTI_E_ARG, "jafs / h / point_status is NULL");
    HIP_TRY(hipSetDevice(c->device));
    const bool contract = d_rows && (d_grad || d_hess);
    const size_t P = (size_t)n_point;
    if (contract) {
        // the contraction reads both derivative arrays and writes both results: what the caller does not want lives in the context
        const size_t n1 = P * D * 7, n2 = P * D * D * 7, n3 = P * D, n4 = P * D * D;
        HIP_TRY(c->curv_f64.reserve((n1 + n2 + n3 + n4) * sizeof(double)));
        double* w = c->curv_f64.as<double>();
        if (!d_dlog) d_dlog = w;
        if (!d_d2log) d_d2log = w + n1;
        if (!d_grad) d_grad = w + n1 + n2;
        if (!d_hess) d_hess = w + n1 + n2 + n3;
    }
    return curv_assemble(c, n_point, d_jafs, d_status, d_h, nullptr, nullptr, contract ? d_rows : nullptr, d_jsfs, d_dlog, d_d2log, d_grad, d_hess,
                         d_point_status, nullptr, nullptr);
}

int misti_curvature(misti_ctx* c, int64_t n_point, const double* x, const double* split_times, const int32_t* rows,
                    const int32_t* band_bounds, const int32_t* pulse_times, int64_t n_rep, const double* jsfs,
                    double rel_step, double abs_step, int64_t batch_limit,
                    double* llh0, double* grad, double* hess, double* dlog, int32_t* point_status) {
    try {
        // (an error between the first copy and the final wait leaves copies in flight: drained before it is reported)
        return eval_batch_drained(c, curvature_impl(c, n_point, x, split_times, rows, band_bounds && c && c->dm.n_band > 0 ? band_bounds : nullptr,
                                                    pulse_times && c && c->dm.n_pulse > 0 ? pulse_times : nullptr, n_rep, jsfs, rel_step, abs_step,
                                                    batch_limit, llh0, grad, hess, dlog, point_status));
    } catch (const std::bad_alloc&) {
        return eval_batch_drained(c, fail(MISTI_E_NOMEM, "out of host memory for %lld points", (long long)n_point));
    }
}

}  // extern "C"
