// Trajectory bands (include/misti_hip.h: misti_traj_bands_dev, misti_traj_bands, misti_bands_rank): the reduction of the corrected
// rates lc per interval and population (misti_bands.hip), alone on spectra-side outputs that are already in HBM, or behind the batch
// path (run_dev, misti_api.cpp) for points given on the host.
#include <cmath>
#include <new>

#include "misti_bands.h"
#include "misti_ctx.h"

using namespace misti_host;

namespace {

constexpr int64_t BANDS_WORKSPACE = 256ll << 20;           // the default bound of the sort's ping-pong pair
constexpr int64_t BANDS_BATCH = 16384;                     // the default engine batch of misti_traj_bands

// The arguments of misti_traj_bands_dev, before the first HIP call, in the header's order, up to the context (the caller's).
int bands_check(const misti_bands_t* b, int64_t G, int64_t m, bool have_inputs) {
    if (!b) return fail(MISTI_E_ARG, "the bands descriptor is NULL");
    if (b->size != sizeof(misti_bands_t))
        return fail(MISTI_E_ARG, "the bands descriptor's size is %u, this library's misti_bands_t has %u bytes", (unsigned)b->size, (unsigned)sizeof(misti_bands_t));
    if (b->n_prob < 1 || b->n_prob > MISTI_POST_MAX_PROBS) return fail(MISTI_E_ARG, "n_prob must be 1 ... %d (got %d)", MISTI_POST_MAX_PROBS, (int)b->n_prob);
    if (!b->probs) return fail(MISTI_E_ARG, "probs is NULL");
    for (int i = 0; i < b->n_prob; ++i)
        if (!(b->probs[i] >= 0.0 && b->probs[i] <= 1.0)) return fail(MISTI_E_ARG, "probs[%d] = %g is not in [0, 1]", i, b->probs[i]);
    if (b->workspace_bytes < 0 || b->batch_limit < 0)
        return fail(MISTI_E_ARG, "workspace_bytes and batch_limit must not be negative (got %lld, %lld)", (long long)b->workspace_bytes, (long long)b->batch_limit);
    if (G < 0 || m < 1) return fail(MISTI_E_ARG, "negative number of groups, or no sample (G = %lld, m = %lld)", (long long)G, (long long)m);
    if (!have_inputs && G > 0) return fail(MISTI_E_ARG, "the rates (the points) or the split times are NULL");
    return 0;
}

// ... and behind the context: what the launch indices and the engine's candidate index can hold
int bands_limits(const misti_ctx* c, int64_t G, int64_t m) {
    if (m > INT32_MAX / 8) return fail(MISTI_E_LIMIT, "m = %lld samples per group exceed INT32_MAX / 8", (long long)m);
    if (G > (INT32_MAX / 8) / m) return fail(MISTI_E_LIMIT, "G x m = %lld x %lld samples exceed INT32_MAX / 8", (long long)G, (long long)m);
    const int64_t tiles = (m + misti::BANDS_TILE - 1) / misti::BANDS_TILE;
    if (G > INT32_MAX / (2 * (int64_t)c->dm.numT * tiles))
        return fail(MISTI_E_LIMIT, "G x 2 numT x ceil(m / %d) = %lld x %d x %lld exceeds INT32_MAX", misti::BANDS_TILE, (long long)G, 2 * c->dm.numT, (long long)tiles);
    return 0;
}

// the groups of one pass: as many as the bound allows, at least one
int64_t bands_pass(const misti_ctx* c, const misti_bands_t& b, int64_t G, int64_t m) {
    const int64_t bound = b.workspace_bytes ? b.workspace_bytes : BANDS_WORKSPACE;
    const int64_t per_group = 2 * 2 * (int64_t)c->dm.numT * m * (int64_t)sizeof(uint64_t);
    const int64_t fit = bound / per_group;
    return fit < 1 ? 1 : fit < G ? fit : G;
}

// One pass of `g` groups, the first being group `first` of the call: outputs are the call's device arrays [G][numT][2]([n_prob]).
int bands_launch(misti_ctx* c, const misti_bands_t& b, int64_t first, int64_t g, int64_t m, const double* d_lc, const double* d_split,
                 const int32_t* d_status, int32_t* count, double* mean, double* quant, double* lo, double* hi) {
    const size_t C = 2 * (size_t)c->dm.numT, at = (size_t)first * C;
    misti::BandsArgs a{};
    a.G = g; a.m = m; a.numT = c->dm.numT; a.n_prob = b.n_prob;
    a.lc = d_lc; a.split = d_split; a.status = d_status;
    a.ws = c->bands_ws.as<uint64_t>();
    a.count = count ? count + at : nullptr; a.mean = mean ? mean + at : nullptr; a.quant = quant ? quant + at * (size_t)b.n_prob : nullptr;
    a.lo = lo ? lo + at : nullptr; a.hi = hi ? hi + at : nullptr;
    for (int i = 0; i < b.n_prob; ++i) a.probs[i] = b.probs[i];
    HIP_TRY(misti::launch_bands(a, c->stream));
    return 0;
}

hipError_t bands_reserve(misti_ctx* c, int64_t pass, int64_t m) {
    return c->bands_ws.reserve(2 * (size_t)pass * 2 * (size_t)c->dm.numT * (size_t)m * sizeof(uint64_t));
}

int traj_bands_impl(misti_ctx* c, int64_t G, int64_t m, const double* x, const double* split_times, const int32_t* band_bounds,
                    const int32_t* pulse_times, const misti_bands_t* b) {
    // a NULL x is an error only where the model has parameters: without a context that cannot be judged, and the context's refusal follows
    if (int r = bands_check(b, G, m, split_times && (x || !c || c->dm.n_param == 0))) return r;
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    if (int r = bands_limits(c, G, m)) return r;
    if (G == 0 || !(b->count || b->mean || b->quant || b->lo || b->hi)) return 0;
    const int D = c->dm.n_param, T1 = c->dm.numT + 1;
    const size_t C = 2 * (size_t)c->dm.numT, NP = (size_t)b->n_prob;
    const size_t NB2 = band_bounds ? 2 * (size_t)c->dm.n_band : 0, NPU = pulse_times ? (size_t)c->dm.n_pulse : 0;
    const int64_t pass = bands_pass(c, *b, G, m);
    int64_t batch = b->batch_limit ? b->batch_limit : BANDS_BATCH;
    if (batch > INT32_MAX / 8) batch = INT32_MAX / 8;                    // one engine call's own limit
    const size_t P = (size_t)pass * (size_t)m, SG = (size_t)G * C;
    HIP_TRY(hipSetDevice(c->device));
    double *d_x = nullptr, *d_split, *d_lc, *d_mean, *d_quant, *d_lo, *d_hi;
    int32_t *d_bounds = nullptr, *d_pulses = nullptr, *d_status, *d_count;
    auto layout = [&](Carver<double>& f, Carver<int32_t>& q) {
        if (D) d_x = f.take(P * D);
        d_split = f.take(P); d_lc = f.take(P * (size_t)T1 * 2);
        d_mean = f.take(SG); d_quant = f.take(SG * NP); d_lo = f.take(SG); d_hi = f.take(SG);
        d_status = q.take(P); d_count = q.take(SG);
        if (NB2) d_bounds = q.take(P * NB2);
        if (NPU) d_pulses = q.take(P * NPU);
    };
    if (int r = carve(c->bands_f64, c->bands_i32, layout)) return r;
    HIP_TRY(bands_reserve(c, pass, m));
    hipStream_t sm = c->stream;
    for (int64_t first = 0; first < G; first += pass) {
        const int64_t g = first + pass < G ? pass : G - first, n = g * m;
        const size_t o = (size_t)first * (size_t)m;
        // decided per pass, so it varies with workspace_bytes: the hint only spares the launch that fractional splits need and changes no bit
        // of a whole-split candidate's lc (misti_eval_batch decides it per call the same way)
        bool whole = true;
        for (int64_t i = 0; i < n && whole; ++i) whole = split_times[o + i] == std::floor(split_times[o + i]);
        if (D) HIP_TRY(hipMemcpyAsync(d_x, x + o * D, (size_t)n * D * sizeof(double), hipMemcpyHostToDevice, sm));
        HIP_TRY(hipMemcpyAsync(d_split, split_times + o, (size_t)n * sizeof(double), hipMemcpyHostToDevice, sm));
        if (NB2) HIP_TRY(hipMemcpyAsync(d_bounds, band_bounds + o * NB2, (size_t)n * NB2 * sizeof(int32_t), hipMemcpyHostToDevice, sm));
        if (NPU) HIP_TRY(hipMemcpyAsync(d_pulses, pulse_times + o * NPU, (size_t)n * NPU * sizeof(int32_t), hipMemcpyHostToDevice, sm));
        for (int64_t a0 = 0; a0 < n; a0 += batch) {
            const int64_t k = a0 + batch < n ? batch : n - a0;
            if (int r = run_dev(c, k, d_split + a0, D ? d_x + a0 * D : nullptr, NB2 ? d_bounds + a0 * NB2 : nullptr, 0, nullptr, nullptr, nullptr,
                                d_lc + (size_t)a0 * T1 * 2, nullptr, d_status + a0, whole ? RUN_INTEGER_SPLITS : 0u, NPU ? d_pulses + a0 * NPU : nullptr)) return r;
        }
        if (int r = bands_launch(c, *b, first, g, m, d_lc, d_split, d_status, b->count ? d_count : nullptr, b->mean ? d_mean : nullptr,
                                 b->quant ? d_quant : nullptr, b->lo ? d_lo : nullptr, b->hi ? d_hi : nullptr)) return r;
    }
    auto back = [&](void* host, const void* dev, size_t bytes) { return host ? hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, sm) : hipSuccess; };
    HIP_TRY(back(b->count, d_count, SG * sizeof(int32_t)));
    HIP_TRY(back(b->mean, d_mean, SG * sizeof(double)));
    HIP_TRY(back(b->quant, d_quant, SG * NP * sizeof(double)));
    HIP_TRY(back(b->lo, d_lo, SG * sizeof(double)));
    HIP_TRY(back(b->hi, d_hi, SG * sizeof(double)));
    HIP_TRY(hipStreamSynchronize(sm));
    return 0;
}

}  // namespace

extern "C" {

int misti_traj_bands_dev(misti_ctx* c, int64_t G, int64_t m, const double* d_lc, const double* d_split, const int32_t* d_status, const misti_bands_t* b) {
    if (int r = bands_check(b, G, m, d_lc && d_split)) return r;
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    if (int r = bands_limits(c, G, m)) return r;
    if (G == 0 || !(b->count || b->mean || b->quant || b->lo || b->hi)) return 0;     // nothing asked for: nothing launched
    HIP_TRY(hipSetDevice(c->device));
    const int64_t pass = bands_pass(c, *b, G, m);
    HIP_TRY(bands_reserve(c, pass, m));
    const size_t row = 2 * ((size_t)c->dm.numT + 1);
    for (int64_t first = 0; first < G; first += pass) {
        const size_t o = (size_t)first * (size_t)m;
        if (int r = bands_launch(c, *b, first, first + pass < G ? pass : G - first, m, d_lc + o * row, d_split + o, d_status ? d_status + o : nullptr,
                                 b->count, b->mean, b->quant, b->lo, b->hi)) return r;
    }
    return 0;
}

int misti_traj_bands(misti_ctx* c, int64_t G, int64_t m, const double* x, const double* split_times, const int32_t* band_bounds,
                     const int32_t* pulse_times, const misti_bands_t* b) {
    try {
        // (an error between the first copy and the final wait leaves copies in flight: drained before it is reported)
        return eval_batch_drained(c, traj_bands_impl(c, G, m, x, split_times, band_bounds && c && c->dm.n_band > 0 ? band_bounds : nullptr,
                                                     pulse_times && c && c->dm.n_pulse > 0 ? pulse_times : nullptr, b));
    } catch (const std::bad_alloc&) {
        return eval_batch_drained(c, fail(MISTI_E_NOMEM, "out of host memory for %lld x %lld samples", (long long)G, (long long)m));
    }
}

int misti_bands_rank(int64_t n, double p, int64_t* lo, int64_t* hi, double* g) {
    if (!lo || !hi || !g) return fail(MISTI_E_ARG, "lo / hi / g is NULL");
    if (n < 1) return fail(MISTI_E_ARG, "n must be >= 1 (got %lld)", (long long)n);
    if (!(p >= 0.0 && p <= 1.0)) return fail(MISTI_E_ARG, "p = %g is not in [0, 1]", p);
    misti::bands_rank(n, p, lo, hi, g);
    return 0;
}

}  // extern "C"
