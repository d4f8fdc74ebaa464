// The samplers of the C ABI (include/misti_hip.h) over the rows problem (misti_rows.h): ensemble MCMC per search (misti_ens.hip), its
// tempered form per fit (misti_pt.hip), priors and log-scale coordinates (misti_prior.h), the posterior summaries (misti_post.hip) and
// the joint regions of coordinate pairs (misti_joint.hip).
#include <cstdio>

#include "misti_joint.h"
#include "misti_post.h"
#include "misti_prior.h"
#include "misti_rows.h"

using namespace misti_host;

namespace {

// ---- posterior summaries of a chain (misti_post.hip) ---------------------------------------------------------------------------------
// The arguments of misti_ens_summary_dev, before the first HIP call, in the header's order, up to the context (the caller's).
int post_check(const misti_ens_post_t* p, int64_t S, int64_t K, int32_t W, int32_t N, bool have_chain) {
    if (!p) return fail(MISTI_E_ARG, "the summary descriptor is NULL");
    if (p->size != sizeof(misti_ens_post_t))
        return fail(MISTI_E_ARG, "the summary descriptor's size is %u, this library's misti_ens_post_t has %u bytes", (unsigned)p->size, (unsigned)sizeof(misti_ens_post_t));
    if (S < 0 || W < 1 || N < 1) return fail(MISTI_E_ARG, "negative number of searches, or no walker or coordinate (S = %lld, W = %d, N = %d)", (long long)S, (int)W, (int)N);
    if (p->burn < 0 || p->burn >= K) return fail(MISTI_E_ARG, "burn must be 0 ... K - 1 (got %d for %lld kept steps)", (int)p->burn, (long long)K);
    if (p->n_prob < 1 || p->n_prob > MISTI_POST_MAX_PROBS) return fail(MISTI_E_ARG, "n_prob must be 1 ... %d (got %d)", MISTI_POST_MAX_PROBS, (int)p->n_prob);
    if (!p->probs) return fail(MISTI_E_ARG, "probs is NULL");
    for (int i = 0; i < p->n_prob; ++i)
        if (!(p->probs[i] >= 0.0 && p->probs[i] <= 1.0)) return fail(MISTI_E_ARG, "probs[%d] = %g is not in [0, 1]", i, p->probs[i]);
    if (p->max_lag < 0) return fail(MISTI_E_ARG, "max_lag must not be negative (got %d)", (int)p->max_lag);
    if (!std::isfinite(p->c) || !(p->c > 0.0)) return fail(MISTI_E_ARG, "c must be finite and positive (got %g)", p->c);
    if (!have_chain && S > 0) return fail(MISTI_E_ARG, "the chain is NULL");
    if (W > MISTI_ENS_MAX_WALKERS) return fail(MISTI_E_LIMIT, "W = %d exceeds MISTI_ENS_MAX_WALKERS = %d", (int)W, MISTI_ENS_MAX_WALKERS);
    if (N > MISTI_MAX_PARAMS) return fail(MISTI_E_LIMIT, "N = %d exceeds MISTI_MAX_PARAMS = %d", (int)N, MISTI_MAX_PARAMS);
    if ((K - p->burn) > INT32_MAX / W) return fail(MISTI_E_LIMIT, "%lld kept steps x %d walkers exceed INT32_MAX samples per search", (long long)(K - p->burn), (int)W);
    if (S > INT32_MAX) return fail(MISTI_E_LIMIT, "too many searches for one call");
    // the shortest intervals: behind everything older, so that no older refusal changes its text
    if (p->n_mass < 0 || p->n_mass > MISTI_POST_MAX_PROBS) return fail(MISTI_E_ARG, "n_mass must be 0 ... %d (got %d)", MISTI_POST_MAX_PROBS, (int)p->n_mass);
    if (p->n_mass > 0 && !p->masses) return fail(MISTI_E_ARG, "masses is NULL");
    for (int i = 0; i < p->n_mass; ++i)
        if (!(p->masses[i] > 0.0 && p->masses[i] <= 1.0)) return fail(MISTI_E_ARG, "masses[%d] = %g is not in (0, 1]", i, p->masses[i]);
    if (p->n_mass == 0 && (p->hpd || p->hpd_at)) return fail(MISTI_E_ARG, "hpd / hpd_at given with n_mass == 0: a shortest interval needs its mass");
    return 0;
}

// the launch record of a checked descriptor, without its pointers
void post_fill(misti::PostArgs& a, int64_t S, int64_t K, int32_t W, int32_t N, const misti_ens_post_t& p) {
    a.S = S; a.K = K; a.llh_K = K; a.W = W; a.N = N; a.burn = p.burn; a.n = K - p.burn; a.c = p.c;
    a.L = p.max_lag < a.n - 1 ? p.max_lag : a.n - 1;
    a.sel = misti::post_select(a.n * W, p.n_prob, p.probs);
    a.n_mass = p.n_mass;
    for (int i = 0; i < p.n_mass; ++i) a.hpd_k[i] = misti::post_hpd_window(a.n * W, p.masses[i]);
}
// the keys of the sort's ping-pong pair (misti_post.hip) where the descriptor asks for a sorted output, else none
size_t post_sort_keys(const misti_ens_post_t& p, size_t S, int N, const misti::PostArgs& a) {
    return p.hpd || p.hpd_at || p.order ? 2 * S * (size_t)N * (size_t)a.n * (size_t)a.W : 0;
}

// The device side of the summaries of a sampler that keeps its chain (sampler_run): carved behind everything the sampler carves,
// so its layout does not move; an output the caller does not ask for is not carved.  back(): the summaries to post's host buffers.
void post_carve(misti::PostArgs& pa, const misti_ens_post_t& p, size_t S, int N, Carver<double>& f, Carver<int32_t>& i) {
    const size_t SN = S * (size_t)N, NP = (size_t)p.n_prob;
    pa.ws_mean = f.take(SN); pa.ws_y = f.take(SN * (size_t)pa.n);
    pa.mean = p.mean ? f.take(SN) : nullptr; pa.cov = p.cov ? f.take(SN * (size_t)N) : nullptr;
    pa.quant = p.quant ? f.take(SN * NP) : nullptr; pa.tau = p.tau ? f.take(SN) : nullptr;
    pa.best_llh = p.best_llh ? f.take(S) : nullptr; pa.best_x = p.best_x ? f.take(SN) : nullptr;
    pa.window = p.window ? i.take(SN) : nullptr; pa.best_at = p.best_at ? i.take(2 * S) : nullptr;
    const size_t NM = (size_t)p.n_mass, keys = post_sort_keys(p, S, N, pa);
    pa.ws_sort = keys ? reinterpret_cast<uint64_t*>(f.take(keys)) : nullptr;                // 8-byte words of the double buffer
    pa.hpd = p.hpd ? f.take(SN * NM * 2) : nullptr; pa.order = p.order ? f.take(keys / 2) : nullptr;
    pa.hpd_at = p.hpd_at ? i.take(SN * NM) : nullptr;
}
int post_back(const misti::PostArgs& pa, const misti_ens_post_t& p, size_t S, int N, hipStream_t sm) {
    const size_t SN = S * (size_t)N, NP = (size_t)p.n_prob;
    auto back = [&](void* host, const void* dev, size_t bytes) { return host ? hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, sm) : hipSuccess; };
    HIP_TRY(back(p.mean, pa.mean, SN * sizeof(double)));
    HIP_TRY(back(p.cov, pa.cov, SN * N * sizeof(double)));
    HIP_TRY(back(p.quant, pa.quant, SN * NP * sizeof(double)));
    HIP_TRY(back(p.tau, pa.tau, SN * sizeof(double)));
    HIP_TRY(back(p.window, pa.window, SN * sizeof(int32_t)));
    HIP_TRY(back(p.best_llh, pa.best_llh, S * sizeof(double)));
    HIP_TRY(back(p.best_x, pa.best_x, SN * sizeof(double)));
    HIP_TRY(back(p.best_at, pa.best_at, 2 * S * sizeof(int32_t)));
    HIP_TRY(back(p.hpd, pa.hpd, SN * (size_t)p.n_mass * 2 * sizeof(double)));
    HIP_TRY(back(p.hpd_at, pa.hpd_at, SN * (size_t)p.n_mass * sizeof(int32_t)));
    HIP_TRY(back(p.order, pa.order, SN * (size_t)pa.n * (size_t)pa.W * sizeof(double)));
    return 0;
}

// ---- joint regions of coordinate pairs (misti_joint.hip) --------------------------------------------------------------------------------
// The arguments of misti_ens_joint_dev, before the first HIP call, in the header's order, up to the context (the caller's).  The shape
// errors are misti_ens_summary_dev's, worded as there.
int joint_check(const misti_ens_joint_t* j, int64_t S, int64_t K, int32_t W, int32_t N, bool have_chain) {
    if (!j) return fail(MISTI_E_ARG, "the joint descriptor is NULL");
    if (j->size != sizeof(misti_ens_joint_t))
        return fail(MISTI_E_ARG, "the joint descriptor's size is %u, this library's misti_ens_joint_t has %u bytes", (unsigned)j->size, (unsigned)sizeof(misti_ens_joint_t));
    if (S < 0 || W < 1 || N < 1) return fail(MISTI_E_ARG, "negative number of searches, or no walker or coordinate (S = %lld, W = %d, N = %d)", (long long)S, (int)W, (int)N);
    if (j->burn < 0 || j->burn >= K) return fail(MISTI_E_ARG, "burn must be 0 ... K - 1 (got %d for %lld kept steps)", (int)j->burn, (long long)K);
    if (!have_chain && S > 0) return fail(MISTI_E_ARG, "the chain is NULL");
    if (W > MISTI_ENS_MAX_WALKERS) return fail(MISTI_E_LIMIT, "W = %d exceeds MISTI_ENS_MAX_WALKERS = %d", (int)W, MISTI_ENS_MAX_WALKERS);
    if (N > MISTI_MAX_PARAMS) return fail(MISTI_E_LIMIT, "N = %d exceeds MISTI_MAX_PARAMS = %d", (int)N, MISTI_MAX_PARAMS);
    if ((K - j->burn) > INT32_MAX / W) return fail(MISTI_E_LIMIT, "%lld kept steps x %d walkers exceed INT32_MAX samples per search", (long long)(K - j->burn), (int)W);
    if (S > INT32_MAX) return fail(MISTI_E_LIMIT, "too many searches for one call");
    if (j->n_pair < 1 || j->n_pair > MISTI_JOINT_MAX_PAIRS) return fail(MISTI_E_ARG, "n_pair must be 1 ... %d (got %d)", MISTI_JOINT_MAX_PAIRS, (int)j->n_pair);
    if (!j->pairs || !j->bins) return fail(MISTI_E_ARG, "pairs / bins is NULL");
    for (int q = 0; q < j->n_pair; ++q) {
        const int32_t a = j->pairs[2 * q], b = j->pairs[2 * q + 1];
        if (a < 0 || a >= N || b < 0 || b >= N) return fail(MISTI_E_ARG, "pairs[%d] = (%d, %d): a coordinate is outside 0 ... %d", q, (int)a, (int)b, (int)N - 1);
        if (a == b) return fail(MISTI_E_ARG, "pairs[%d] = (%d, %d): a pair needs two distinct coordinates", q, (int)a, (int)b);
    }
    for (int q = 0; q < 2 * j->n_pair; ++q)
        if (j->bins[q] < 1 || j->bins[q] > MISTI_JOINT_MAX_BINS)
            return fail(MISTI_E_ARG, "bins[%d][%d] = %d: a bin count must be 1 ... %d", q / 2, q % 2, (int)j->bins[q], MISTI_JOINT_MAX_BINS);
    if (j->n_mass < 0 || j->n_mass > MISTI_POST_MAX_PROBS) return fail(MISTI_E_ARG, "the joint n_mass must be 0 ... %d (got %d)", MISTI_POST_MAX_PROBS, (int)j->n_mass);
    if (j->n_mass > 0 && !j->masses) return fail(MISTI_E_ARG, "the joint masses is NULL");
    for (int i = 0; i < j->n_mass; ++i)
        if (!(j->masses[i] > 0.0 && j->masses[i] <= 1.0)) return fail(MISTI_E_ARG, "the joint masses[%d] = %g is not in (0, 1]", i, j->masses[i]);
    if (j->n_mass == 0 && (j->level || j->cells || j->held)) return fail(MISTI_E_ARG, "level / cells / held given with n_mass == 0: a region needs its mass");
    return 0;
}

// the launch record of a checked descriptor, without its pointers
void joint_fill(misti::JointArgs& a, int64_t S, int64_t K, int32_t W, int32_t N, const misti_ens_joint_t& j) {
    a.S = S; a.K = K; a.burn = j.burn; a.n = K - j.burn; a.W = W; a.N = N; a.n_pair = j.n_pair; a.n_mass = j.n_mass;
    a.slabs = (int32_t)((a.n * W + misti::JOINT_SLAB - 1) / misti::JOINT_SLAB);
    bool used[MISTI_MAX_PARAMS] = {};
    for (int q = 0; q < j.n_pair; ++q) {
        a.a[q] = (uint8_t)j.pairs[2 * q]; a.b[q] = (uint8_t)j.pairs[2 * q + 1];
        a.Ba[q] = (uint8_t)j.bins[2 * q]; a.Bb[q] = (uint8_t)j.bins[2 * q + 1];
        a.off[q] = (int32_t)a.cells;
        a.cells += (int64_t)j.bins[2 * q] * j.bins[2 * q + 1];
        used[a.a[q]] = used[a.b[q]] = true;
    }
    for (int k = 0; k < N; ++k)
        if (used[k]) a.coord[a.n_coord++] = (uint8_t)k;
    for (int i = 0; i < j.n_mass; ++i) a.mass[i] = j.masses[i];
}
bool joint_levels(const misti_ens_joint_t& j) { return j.inside || j.mode || j.level || j.cells || j.held; }

// The device side of the regions of a sampler that keeps its chain (sampler_run): carved behind everything else, the summaries'
// included, so no older layout moves.  The window is always carved - a given range is uploaded into it -, the histograms where they
// or what is read off them are asked for.  back(): to the descriptor's host buffers.
void joint_carve(misti::JointArgs& ja, const misti_ens_joint_t& j, size_t S, Carver<double>& f, Carver<int32_t>& i) {
    const size_t SP = S * (size_t)j.n_pair, NM = (size_t)j.n_mass;
    double* window = f.take(SP * 4);
    ja.window = window; ja.from_data = j.range ? nullptr : window;
    ja.counts = j.counts || joint_levels(j) ? i.take(S * (size_t)ja.cells) : nullptr;
    ja.inside = j.inside ? i.take(SP) : nullptr; ja.mode = j.mode ? i.take(2 * SP) : nullptr;
    ja.level = j.level ? i.take(SP * NM) : nullptr; ja.n_cells = j.cells ? i.take(SP * NM) : nullptr; ja.held = j.held ? i.take(SP * NM) : nullptr;
}
int joint_back(const misti::JointArgs& ja, const misti_ens_joint_t& j, size_t S, hipStream_t sm) {
    const size_t SP = S * (size_t)j.n_pair, NM = (size_t)j.n_mass;
    auto back = [&](void* host, const void* dev, size_t bytes) { return host && bytes ? hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, sm) : hipSuccess; };
    HIP_TRY(back(j.counts, ja.counts, S * (size_t)ja.cells * sizeof(int32_t)));
    HIP_TRY(back(j.range_out, ja.window, SP * 4 * sizeof(double)));
    HIP_TRY(back(j.inside, ja.inside, SP * sizeof(int32_t)));
    HIP_TRY(back(j.mode, ja.mode, 2 * SP * sizeof(int32_t)));
    HIP_TRY(back(j.level, ja.level, SP * NM * sizeof(int32_t)));
    HIP_TRY(back(j.cells, ja.n_cells, SP * NM * sizeof(int32_t)));
    HIP_TRY(back(j.held, ja.held, SP * NM * sizeof(int32_t)));
    return 0;
}

// ---- priors and log-scale coordinates (misti_prior.h) ----------------------------------------------------------------------------------
// The prior descriptor of the two samplers, or NULL: its shape (behind check_n_box, before the context is looked at) ...
int check_prior_shape(const misti_prior_t* p, int64_t n_start, const char* noun) {
    if (!p) return 0;
    if (p->n_prior != 1 && p->n_prior != n_start)
        return fail(MISTI_E_ARG, "n_prior must be 1 or n_start (got %d for %lld %s)", (int)p->n_prior, (long long)n_start, noun);
    if (!p->scale || !p->kind || !p->p0 || !p->p1) return fail(MISTI_E_ARG, "the prior's scale / kind / p0 / p1 is NULL");
    return 0;
}
// ... one coordinate of search s (p0 / p1 are looked at only where the kind reads them) ...
int check_prior_coord(int64_t s, int k, int32_t scale, int32_t kind, const double* p0, const double* p1, double lo, double hi) {
    if (scale != MISTI_COORD_LINEAR && scale != MISTI_COORD_LOG)
        return fail(MISTI_E_ARG, "prior of search %lld, coordinate %d: the scale %d is neither MISTI_COORD_LINEAR nor MISTI_COORD_LOG", (long long)s, k, (int)scale);
    if (kind != MISTI_PRIOR_FLAT && kind != MISTI_PRIOR_NORMAL && kind != MISTI_PRIOR_EXPONENTIAL)
        return fail(MISTI_E_ARG, "prior of search %lld, coordinate %d: the kind %d is none of MISTI_PRIOR_FLAT / NORMAL / EXPONENTIAL", (long long)s, k, (int)kind);
    if (kind == MISTI_PRIOR_NORMAL && (!std::isfinite(*p1) || !(*p1 > 0.0)))
        return fail(MISTI_E_ARG, "prior of search %lld, coordinate %d: the normal's sd %g is not finite and positive", (long long)s, k, *p1);
    if (kind == MISTI_PRIOR_EXPONENTIAL && (!std::isfinite(*p0) || !(*p0 > 0.0)))
        return fail(MISTI_E_ARG, "prior of search %lld, coordinate %d: the exponential's scale %g is not finite and positive", (long long)s, k, *p0);
    if (kind == MISTI_PRIOR_NORMAL && !std::isfinite(*p0))
        return fail(MISTI_E_ARG, "prior of search %lld, coordinate %d: the normal's mean is not finite", (long long)s, k);
    if (scale == MISTI_COORD_LOG && (hi > 709.0 || lo < -745.0))
        return fail(MISTI_E_ARG, "prior of search %lld, coordinate %d: the log-scale box [%g, %g] leaves [-745, 709] - its natural value would leave the doubles",
                    (long long)s, k, lo, hi);
    return 0;
}
// ... and every coordinate against its search's box (behind check_box: N comes from the context).
int check_prior(const misti_prior_t* p, const RowsArgs& a, int N) {
    if (!p || p->n_prior < 1 || a.n_box < 1) return 0;
    const int64_t n = p->n_prior > a.n_box ? p->n_prior : a.n_box;
    for (int64_t s = 0; s < n; ++s)
        for (int k = 0; k < N; ++k) {
            const int64_t q = (p->n_prior > 1 ? s : 0) * N + k, o = (a.n_box > 1 ? s : 0) * N + k;
            if (int r = check_prior_coord(s, k, p->scale[q], p->kind[q], p->p0 + q, p->p1 + q, a.box_lo[o], a.box_hi[o])) return r;
        }
    return 0;
}

// The device side of a checked prior: carved and uploaded only where a coordinate is not LINEAR and FLAT - a prior that says nothing
// takes the prior-less path.  `slots`: the proposals of a half-step.
struct PriorProblem {
    const misti_prior_t* p = nullptr;
    size_t n = 0, ny = 0;            // n_prior x N; slots x N.  n == 0: no prior
    int32_t *d_scale = nullptr, *d_kind = nullptr;
    double *d_p0 = nullptr, *d_p1 = nullptr, *d_y = nullptr;
    PriorProblem(const misti_prior_t* p_, int N, size_t slots) {
        if (!p_) return;
        const size_t all = (size_t)p_->n_prior * (size_t)N;
        bool says = false;
        for (size_t q = 0; q < all; ++q) says = says || p_->scale[q] != MISTI_COORD_LINEAR || p_->kind[q] != MISTI_PRIOR_FLAT;
        if (says) { p = p_; n = all; ny = slots * (size_t)N; }
    }
    void layout(Carver<double>& f, Carver<int32_t>& i) {
        if (!n) return;
        d_p0 = f.take(n); d_p1 = f.take(n); d_y = f.take(ny);
        d_scale = i.take(n); d_kind = i.take(n);
    }
    int upload(hipStream_t sm) const {
        if (!n) return 0;
        HIP_TRY(hipMemcpyAsync(d_scale, p->scale, n * sizeof(int32_t), hipMemcpyHostToDevice, sm));
        HIP_TRY(hipMemcpyAsync(d_kind, p->kind, n * sizeof(int32_t), hipMemcpyHostToDevice, sm));
        HIP_TRY(hipMemcpyAsync(d_p0, p->p0, n * sizeof(double), hipMemcpyHostToDevice, sm));
        HIP_TRY(hipMemcpyAsync(d_p1, p->p1, n * sizeof(double), hipMemcpyHostToDevice, sm));
        return 0;
    }
    void fill(misti::EnsPrior& pr) const {
        pr.scale = d_scale; pr.kind = d_kind; pr.p0 = d_p0; pr.p1 = d_p1; pr.per_start = n && p->n_prior > 1 ? 1 : 0; pr.y = d_y;
    }
};

// ---- the samplers: ensemble MCMC per search (misti_ens.hip) and its tempered form per fit (misti_pt.hip) ---------------------------
// What a sampler call is: the rows problem, n_rung ensembles of `walkers` walkers per start at temperatures of their own, the steps,
// and where the results go.  misti_ensemble_sample is the call of ONE rung (EnsState::L = 1) without swap rounds and without the
// reduction.  A per-sampler field is added HERE, to sampler_check and sampler_run below and to EnsState (misti_device.h) - nowhere
// else.  The two public descriptors lay these fields out differently: one sampler_args() each.
struct SamplerArgs {
    RowsArgs rows;
    const double* init;              // [n_start][n_rung][walkers][N]
    int32_t walkers, n_rung;         // n_rung: 1 at the plain door
    bool tempered;                   // misti_tempered_sample: a ladder, swap rounds and the reduction - also where n_rung == 1
    int32_t n_temp;                  // 1 or n_start: temp is [n_temp][n_rung]
    const double* temp;
    int32_t n_step, thin;
    double a;
    uint64_t seed;
    int32_t swap_every, burn;        // the tempered door's; 0 at the plain door
    bool keep_x, keep_llh;           // the chain of the cold rung / of every rung's values is kept on the device
    double *chain, *chain_llh;       // what is copied back: NULL, not copied.  rung_llh, logz and the swap counters: NULL at the plain door
    int32_t *accepted, *swap_proposed, *swap_accepted;
    double *last, *last_llh, *rung_llh, *logz;
    int64_t* n_points;
    const char *noun, *per, *kept;   // the words the doors' texts differ in: "searches" | "fits"; what the limits count; "device " chain
};
// the plain door keeps both chains or none: where the caller or a reduction (`post`: a summary or a joint descriptor) asks for one
SamplerArgs sampler_args(const misti_ens_t& q, const void* post) {
    const bool keep = q.chain || q.chain_llh || post;
    return {rows_args(q), q.init, q.walkers, 1, false, q.n_temp, q.temperature, q.n_step, q.thin, q.a, q.seed, 0, 0, keep, keep,
            q.chain, q.chain_llh, q.accepted, nullptr, nullptr, q.last, q.last_llh, nullptr, nullptr, q.n_points,
            "searches", "searches x walkers", post ? "device " : ""};
}
// the tempered door always keeps the values of every rung (the reduction reads them), the cold rung's coordinates where they are wanted
SamplerArgs sampler_args(const misti_pt_t& q, const void* post) {
    return {rows_args(q), q.init, q.walkers, q.n_rung, true, q.n_ladder, q.ladder, q.n_step, q.thin, q.a, q.seed, q.swap_every, q.burn,
            q.chain || post, true, q.chain, q.chain_llh, q.accepted, q.swap_proposed, q.swap_accepted, q.last, q.last_llh, q.rung_llh, q.logz,
            q.n_points, "fits", "fits x rungs x walkers", ""};
}

// The arguments of a sampler call, before the first HIP call, in the order of its door's header.  The two orders are one order: where
// misti_ensemble_sample has n_temp and temperature, misti_tempered_sample has n_rung, n_ladder, the ladder, swap_every and burn.  Leaves
// the number of coordinates in N and whether every split time is an integer in `whole`.
int sampler_check(const misti_ctx* c, const SamplerArgs& q, const misti_prior_t* prior, int& N, bool& whole) {
    const RowsArgs& a = q.rows;
    const bool pt = q.tempered;
    if (a.n_start < 0) return fail(MISTI_E_ARG, "negative number of %s", q.noun);
    if (!q.init || !a.rows || !a.jsfs || !a.box_lo || !a.box_hi || !q.temp || !q.last || !q.last_llh || (pt && (!q.rung_llh || !q.logz)) || (a.per_start() && !a.split_times))
        return fail(MISTI_E_ARG, "init / rows / jsfs / box_lo / box_hi / %s / last / last_llh%s%s is NULL", pt ? "ladder" : "temperature",
                    pt ? " / rung_llh / logz" : "", a.per_start() ? " / split_times" : "");
    if (a.n_rep < 1) return fail(MISTI_E_ARG, "n_rep must be >= 1 (got %lld)", (long long)a.n_rep);
    if (q.walkers < 4 || (q.walkers & 1)) return fail(MISTI_E_ARG, "walkers must be even and >= 4 (got %d)", (int)q.walkers);
    if (q.walkers > MISTI_ENS_MAX_WALKERS) return fail(MISTI_E_LIMIT, "walkers = %d exceeds MISTI_ENS_MAX_WALKERS = %d", (int)q.walkers, MISTI_ENS_MAX_WALKERS);
    if (q.n_step < 0) return fail(MISTI_E_ARG, "n_step must not be negative");
    if (q.thin < 1) return fail(MISTI_E_ARG, "thin must be >= 1");
    if (!std::isfinite(q.a) || !(q.a > 1.0)) return fail(MISTI_E_ARG, "a must be finite and > 1 (got %g)", q.a);
    // the temperatures: n_temp / temperature | n_rung / n_ladder / ladder / swap_every / burn
    if (pt && q.n_rung < 1) return fail(MISTI_E_ARG, "n_rung must be >= 1 (got %d)", (int)q.n_rung);
    if (pt && q.n_rung > MISTI_PT_MAX_RUNGS) return fail(MISTI_E_LIMIT, "n_rung = %d exceeds MISTI_PT_MAX_RUNGS = %d", (int)q.n_rung, MISTI_PT_MAX_RUNGS);
    if (q.n_temp != 1 && q.n_temp != a.n_start)
        return fail(MISTI_E_ARG, "%s must be 1 or n_start (got %d for %lld %s)", pt ? "n_ladder" : "n_temp", (int)q.n_temp, (long long)a.n_start, q.noun);
    for (int64_t s = 0; s < q.n_temp; ++s)
        for (int l = 0; l < q.n_rung; ++l) {
            const double T = q.temp[s * q.n_rung + l];
            if (!std::isfinite(T) || !(T > 0.0))
                return pt ? fail(MISTI_E_ARG, "ladder[%lld][%d] = %g is not finite and positive", (long long)s, l, T)
                          : fail(MISTI_E_ARG, "temperature[%lld] = %g is not finite and positive", (long long)s, T);
            if (l && !(T > q.temp[s * q.n_rung + l - 1]))
                return fail(MISTI_E_ARG, "ladder[%lld][%d] = %g is not above ladder[%lld][%d] = %g: a ladder is strictly increasing", (long long)s, l, T,
                            (long long)s, l - 1, q.temp[s * q.n_rung + l - 1]);
        }
    const int64_t K = q.n_step / q.thin;
    if (pt && q.swap_every < 0) return fail(MISTI_E_ARG, "swap_every must not be negative (got %d)", (int)q.swap_every);
    if (pt && K > 0 && (q.burn < 0 || q.burn >= K)) return fail(MISTI_E_ARG, "burn must be 0 ... K - 1 (got %d for %lld kept steps)", (int)q.burn, (long long)K);
    // the rows problem and the prior's shape; then the context and what needs the model
    if (int r = check_n_box(a, q.noun)) return r;
    if (int r = check_prior_shape(prior, a.n_start, q.noun)) return r;
    if (int r = check_rows(a, whole)) return r;
    const int64_t per = (int64_t)q.walkers * q.n_rung;
    if (int r = check_limits(c, a, per, q.per, N)) return r;
    if ((q.keep_x || q.keep_llh) && a.n_start > 0 && K > INT32_MAX / 8 / N / per / a.n_start) {
        char rungs[32] = "";
        if (pt) snprintf(rungs, sizeof(rungs), " x %d rungs", (int)q.n_rung);
        return fail(MISTI_E_LIMIT, "the %schain of %lld %s%s x %lld kept steps x %d walkers x %d coordinates exceeds INT32_MAX / 8 elements (raise thin)", q.kept,
                    (long long)a.n_start, q.noun, rungs, (long long)K, (int)q.walkers, N);
    }
    for (int64_t b = 0; b < a.n_box; ++b) {
        if (int r = check_box(a, N, b, "the sampler's prior is uniform on a finite box")) return r;
        int n_free = 0;
        for (int k = 0; k < N; ++k) n_free += a.box_lo[b * N + k] != a.box_hi[b * N + k] ? 1 : 0;
        if (n_free == 0) return fail(MISTI_E_ARG, "box %lld: every coordinate is fixed", (long long)b);
    }
    if (int r = check_prior(prior, a, N)) return r;
    for (int64_t s = 0; s < a.n_start; ++s)
        for (int l = 0; l < q.n_rung; ++l)
            for (int i = 0; i < q.walkers; ++i)
                for (int k = 0; k < N; ++k) {
                    const double v = q.init[((s * q.n_rung + l) * q.walkers + i) * N + k];
                    const int64_t o = (a.n_box > 1 ? s : 0) * N + k;
                    if (std::isfinite(v) && v >= a.box_lo[o] && v <= a.box_hi[o]) continue;
                    char at[80];                           // the walker: the plain door names no rung
                    if (pt) snprintf(at, sizeof(at), "init[%lld][%d][%d][%d]", (long long)s, l, i, k);
                    else snprintf(at, sizeof(at), "init[%lld][%d][%d]", (long long)s, i, k);
                    if (!std::isfinite(v)) return fail(MISTI_E_ARG, "%s is not finite", at);
                    return fail(MISTI_E_ARG, "%s = %g is outside its box [%g, %g]", at, v, a.box_lo[o], a.box_hi[o]);
                }
    return 0;
}

// A checked call with n_start >= 1: n_start x n_rung searches of the device's one sampler (EnsState::L).  One batch record of
// n_start x n_rung x walkers slots serves the initial ensembles and every half-step (which fills the first half of it); the state and
// the chains lie in the search buffers of the context, and nothing is read back before the end.  A tempered call adds a swap launch
// behind the steps that have a round, the reduction at the end, and their four arrays; a plain call issues neither launch and carves
// none of them.  With `post` (checked: post_check) the summary kernels run on the cold chain where it lies and the summaries come back
// with the rest; the series workspace and the summaries' device side are carved with the chain.  With `joint` (checked: joint_check)
// the kernels of misti_joint.hip follow on the same chain, their device side carved behind the summaries'.
int sampler_run(misti_ctx* c, const SamplerArgs& q, int N, bool whole, const misti_ens_post_t* post, const misti_prior_t* prior, const misti_ens_joint_t* joint) {
    using namespace misti;
    HIP_TRY(hipSetDevice(c->device));
    const size_t F = (size_t)q.rows.n_start, L = (size_t)q.n_rung, S = F * L, W = (size_t)q.walkers, H = W / 2, M = S * W, NT = (size_t)q.n_temp * L;
    const size_t K = (q.keep_x || q.keep_llh) ? (size_t)(q.n_step / q.thin) : 0, P = F * (L - 1);
    PostArgs pa{};
    if (post) post_fill(pa, q.rows.n_start, (int64_t)K, q.walkers, N, *post);
    JointArgs ja{};
    if (joint) joint_fill(ja, q.rows.n_start, (int64_t)K, q.walkers, N, *joint);
    RowsProblem rows(c, q.rows, N, whole);
    PriorProblem pri(prior, N, S * H);
    EnsState st{};
    st.S = (int64_t)S; st.L = q.n_rung; st.N = N; st.W = q.walkers; st.thin = q.thin; st.a = q.a; st.am1 = q.a - 1.0; st.seed = q.seed;
    st.temp_per_start = q.n_temp > 1 ? 1 : 0;
    st.n_keep = (int64_t)K;
    PtState pt{};
    double *llk = nullptr, *d_init = nullptr, *d_temp = nullptr, *d_points = nullptr, *d_rung = nullptr, *d_logz = nullptr;
    auto layout = [&](Carver<double>& f, Carver<int32_t>& i) {
        st.b.pts = f.take(M * N); st.x = f.take(M * N); st.llh = f.take(M); st.b.split = f.take(M); llk = f.take(M);
        st.z = f.take(S * H); st.u_acc = f.take(S * H);
        d_init = f.take(M * N); d_temp = f.take(NT);
        d_points = f.take(S);                              // int64 per search: 8-byte words of the double buffer
        if (q.keep_x && K) st.chain = f.take(F * K * W * (size_t)N);
        if (q.keep_llh && K) st.chain_llh = f.take(S * K * W);
        st.accepted = i.take(M); st.submitted = i.take(M);
        if (q.tempered) {
            d_rung = f.take(S); d_logz = f.take(F);
            pt.swap_proposed = i.take(P); pt.swap_accepted = i.take(P);
        }
        rows.layout(f, i, &st.b, &M, 1, M);
        pri.layout(f, i);
        if (post) post_carve(pa, *post, F, N, f, i);
        if (joint) joint_carve(ja, *joint, F, f, i);
    };
    if (int r = carve(c->nm_f64, c->nm_i32, layout)) return r;
    rows.fill(st.src);
    pri.fill(st.prior);
    st.temp = d_temp;
    st.points = reinterpret_cast<long long*>(d_points);
    hipStream_t sm = c->stream;
    HIP_TRY(hipMemcpyAsync(d_init, q.init, M * N * sizeof(double), hipMemcpyHostToDevice, sm));
    HIP_TRY(hipMemcpyAsync(d_temp, q.temp, NT * sizeof(double), hipMemcpyHostToDevice, sm));
    if (P) HIP_TRY(hipMemsetAsync(pt.swap_proposed, 0, 2 * P * sizeof(int32_t), sm));     // the two counters lie back to back
    if (int r = rows.upload(c)) return r;
    if (int r = pri.upload(sm)) return r;
    c->nm_iterations = c->nm_slots = c->nm_spec_iterations = 0;
    HIP_TRY(launch_ens_init(st, d_init, sm));
    if (int r = rows.eval(c, st.b, (int64_t)M, llk)) return r;
    HIP_TRY(launch_ens_accept(st, 0, -1, llk, sm));
    for (int64_t step = 1; step <= q.n_step; ++step) {
        for (int half = 0; half < 2; ++half) {
            HIP_TRY(launch_ens_propose(st, step, half, sm));
            if (int r = rows.eval(c, st.b, (int64_t)(S * H), llk)) return r;
            HIP_TRY(launch_ens_accept(st, step, half, llk, sm));
        }
        if (q.swap_every >= 1 && step % q.swap_every == 0) {
            const int first = (int)((step / q.swap_every - 1) & 1);
            if (first + 1 < q.n_rung) HIP_TRY(launch_pt_swap(st, pt, step, first, sm));
        }
    }
    c->nm_iterations = 2 * (int64_t)q.n_step;
    c->nm_slots = 2 * (int64_t)q.n_step * (int64_t)(S * H);
    HIP_TRY(launch_ens_result(st, sm));
    if (q.tempered) HIP_TRY(launch_pt_reduce(st, K ? q.burn : 0, d_rung, d_logz, sm));
    if (post) {
        pa.chain = st.chain; pa.chain_llh = st.chain_llh; pa.llh_K = (int64_t)(L * K);     // rung 0 of fit s: the first K rows of its L K
        HIP_TRY(launch_post(pa, sm));
        if (int r = post_back(pa, *post, F, N, sm)) return r;
    }
    if (joint) {
        ja.chain = st.chain;
        if (joint->range) HIP_TRY(hipMemcpyAsync(const_cast<double*>(ja.window), joint->range, F * (size_t)joint->n_pair * 4 * sizeof(double), hipMemcpyHostToDevice, sm));
        HIP_TRY(launch_joint(ja, sm));
        if (int r = joint_back(ja, *joint, F, sm)) return r;
    }
    auto back = [&](void* host, const void* dev, size_t bytes) { return host && bytes ? hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, sm) : hipSuccess; };
    HIP_TRY(back(q.last, st.x, M * N * sizeof(double)));
    HIP_TRY(back(q.last_llh, st.llh, M * sizeof(double)));
    HIP_TRY(back(q.rung_llh, d_rung, S * sizeof(double)));
    HIP_TRY(back(q.logz, d_logz, F * sizeof(double)));
    HIP_TRY(back(q.accepted, st.accepted, M * sizeof(int32_t)));
    HIP_TRY(back(q.swap_proposed, pt.swap_proposed, P * sizeof(int32_t)));
    HIP_TRY(back(q.swap_accepted, pt.swap_accepted, P * sizeof(int32_t)));
    HIP_TRY(back(q.chain, st.chain, F * K * W * N * sizeof(double)));
    HIP_TRY(back(q.chain_llh, st.chain_llh, S * K * W * sizeof(double)));
    std::vector<int64_t> per_search;
    if (q.n_points) {
        per_search.resize(S);
        HIP_TRY(hipMemcpyAsync(per_search.data(), d_points, S * sizeof(int64_t), hipMemcpyDeviceToHost, sm));
    }
    HIP_TRY(hipStreamSynchronize(sm));
    if (q.n_points) {
        int64_t n = 0;
        for (int64_t v : per_search) n += v;
        *q.n_points = n;
    }
    return 0;
}

// The one door behind the five sampling entry points, entered once the sampler descriptor's own size is known to be this library's
// (sampler_size: nothing else of a descriptor is read before).  `need_post`: a summary there must be (misti_ensemble_posterior).
int sampler_size(const void* q, uint32_t size, uint32_t want, const char* type) {
    if (!q) return fail(MISTI_E_ARG, "the sampler descriptor is NULL");
    if (size != want) return fail(MISTI_E_ARG, "the sampler descriptor's size is %u, this library's %s has %u bytes", (unsigned)size, type, (unsigned)want);
    return 0;
}
int sampler_door(misti_ctx* c, const SamplerArgs& q, const misti_ens_post_t* p, const misti_prior_t* pr, bool need_post, const misti_ens_joint_t* j) {
    if (need_post && !p) return fail(MISTI_E_ARG, "the summary descriptor is NULL");
    if (p && p->size != sizeof(misti_ens_post_t))
        return fail(MISTI_E_ARG, "the summary descriptor's size is %u, this library's misti_ens_post_t has %u bytes", (unsigned)p->size, (unsigned)sizeof(misti_ens_post_t));
    if (pr && pr->size != sizeof(misti_prior_t))
        return fail(MISTI_E_ARG, "the prior descriptor's size is %u, this library's misti_prior_t has %u bytes", (unsigned)pr->size, (unsigned)sizeof(misti_prior_t));
    if (j && j->size != sizeof(misti_ens_joint_t))
        return fail(MISTI_E_ARG, "the joint descriptor's size is %u, this library's misti_ens_joint_t has %u bytes", (unsigned)j->size, (unsigned)sizeof(misti_ens_joint_t));
    if (q.rows.split != MISTI_SPLIT_PER_START && q.rows.split != MISTI_SPLIT_FITTED)
        return fail(MISTI_E_ARG, "the sampler descriptor's split mode %d is neither MISTI_SPLIT_PER_START nor MISTI_SPLIT_FITTED", (int)q.rows.split);
    int N = 0;
    bool whole = false;
    if (int r = sampler_check(c, q, pr, N, whole)) return r;
    if (p) if (int r = post_check(p, q.rows.n_start, q.n_step / q.thin, q.walkers, N, true)) return r;
    if (j) if (int r = joint_check(j, q.rows.n_start, q.n_step / q.thin, q.walkers, N, true)) return r;
    if (q.rows.n_start == 0) return 0;
    return sampler_run(c, q, N, whole, p, pr, j);
}
const void* reduced(const misti_ens_post_t* p, const misti_ens_joint_t* j) { return p ? static_cast<const void*>(p) : static_cast<const void*>(j); }
int ens_door(misti_ctx* c, const misti_ens_t* q, const misti_ens_post_t* p, const misti_prior_t* pr, bool need_post, const misti_ens_joint_t* j = nullptr) {
    if (int r = sampler_size(q, q ? q->size : 0, sizeof(misti_ens_t), "misti_ens_t")) return r;
    return sampler_door(c, sampler_args(*q, reduced(p, j)), p, pr, need_post, j);
}
int pt_door(misti_ctx* c, const misti_pt_t* q, const misti_ens_post_t* p, const misti_prior_t* pr, const misti_ens_joint_t* j) {
    if (int r = sampler_size(q, q ? q->size : 0, sizeof(misti_pt_t), "misti_pt_t")) return r;
    return sampler_door(c, sampler_args(*q, reduced(p, j)), p, pr, false, j);
}

}  // namespace

extern "C" {

int misti_ensemble_sample(misti_ctx* c, const misti_ens_t* q) { return ens_door(c, q, nullptr, nullptr, false); }

int misti_ensemble_posterior(misti_ctx* c, const misti_ens_t* q, const misti_ens_post_t* p) { return ens_door(c, q, p, nullptr, true); }

int misti_ensemble_sample_prior(misti_ctx* c, const misti_ens_t* q, const misti_ens_post_t* p, const misti_prior_t* pr) { return ens_door(c, q, p, pr, false); }

int misti_tempered_sample_prior(misti_ctx* c, const misti_pt_t* q, const misti_ens_post_t* p, const misti_prior_t* pr) { return pt_door(c, q, p, pr, nullptr); }

int misti_ensemble_sample_joint(misti_ctx* c, const misti_ens_t* q, const misti_ens_post_t* p, const misti_prior_t* pr, const misti_ens_joint_t* j) {
    return ens_door(c, q, p, pr, false, j);
}

int misti_tempered_sample_joint(misti_ctx* c, const misti_pt_t* q, const misti_ens_post_t* p, const misti_prior_t* pr, const misti_ens_joint_t* j) {
    return pt_door(c, q, p, pr, j);
}

int misti_tempered_sample(misti_ctx* c, const misti_pt_t* q, const misti_ens_post_t* p) { return misti_tempered_sample_prior(c, q, p, nullptr); }

int misti_ens_log_prior(int32_t N, const int32_t* scale, const int32_t* kind, const double* p0, const double* p1, const double* lo, const double* hi,
                        const double* y, double* lp, double* natural) {
    if (N < 1 || N > MISTI_MAX_PARAMS) return fail(MISTI_E_ARG, "N must be 1 ... %d (got %d)", MISTI_MAX_PARAMS, (int)N);
    if (!scale || !kind || !p0 || !p1 || !lo || !hi || !y || !lp) return fail(MISTI_E_ARG, "scale / kind / p0 / p1 / lo / hi / y / lp is NULL");
    for (int k = 0; k < N; ++k)
        if (int r = check_prior_coord(0, k, scale[k], kind[k], p0 + k, p1 + k, lo[k], hi[k])) return r;
    *lp = misti::ens_log_prior(N, kind, p0, p1, lo, hi, y);
    for (int k = 0; natural && k < N; ++k) natural[k] = misti::ens_natural(scale[k], y[k]);
    return 0;
}

int misti_ens_accept_prior(double z, int32_t d, double llk_old, double llk_new, double T, double lp_old, double lp_new, double u_acc, int32_t* accept) {
    if (!accept) return fail(MISTI_E_ARG, "accept is NULL");
    if (d < 0 || d >= MISTI_MAX_PARAMS) return fail(MISTI_E_ARG, "d must be 0 ... MISTI_MAX_PARAMS - 1");
    if (!(T > 0.0) || !std::isfinite(T)) return fail(MISTI_E_ARG, "the temperature must be finite and positive");
    *accept = misti::ens_decide_prior(z, d, llk_old, llk_new, T, lp_old, lp_new, u_acc) ? 1 : 0;
    return 0;
}

int misti_ens_summary_dev(misti_ctx* c, int64_t S, int64_t K, int32_t W, int32_t N, const double* d_chain, const double* d_chain_llh, const misti_ens_post_t* p) {
    if (int r = post_check(p, S, K, W, N, d_chain != nullptr)) return r;
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    if (S == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    misti::PostArgs a{};
    post_fill(a, S, K, W, N, *p);
    const size_t SN = (size_t)S * (size_t)N;
    const size_t keys = post_sort_keys(*p, (size_t)S, N, a);
    HIP_TRY(c->post_ws.reserve((SN * (size_t)(a.n + 1) + keys) * sizeof(double)));
    a.ws_mean = c->post_ws.as<double>(); a.ws_y = a.ws_mean + SN;
    a.ws_sort = keys ? reinterpret_cast<uint64_t*>(a.ws_y + SN * (size_t)a.n) : nullptr;
    a.chain = d_chain; a.chain_llh = d_chain_llh;
    a.mean = p->mean; a.cov = p->cov; a.quant = p->quant; a.tau = p->tau; a.window = p->window;
    a.best_llh = p->best_llh; a.best_x = p->best_x; a.best_at = p->best_at;
    a.hpd = p->hpd; a.hpd_at = p->hpd_at; a.order = p->order;
    HIP_TRY(misti::launch_post(a, c->stream));
    return 0;
}

int misti_ens_joint_dev(misti_ctx* c, int64_t S, int64_t K, int32_t W, int32_t N, const double* d_chain, const misti_ens_joint_t* j) {
    if (int r = joint_check(j, S, K, W, N, d_chain != nullptr)) return r;
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    if (S == 0 || !(j->counts || j->range_out || joint_levels(*j))) return 0;   // nothing asked for: nothing launched
    HIP_TRY(hipSetDevice(c->device));
    misti::JointArgs a{};
    joint_fill(a, S, K, W, N, *j);
    // the context's workspace: the window where the data gives it and the caller does not take it | the histograms where only what is
    // read off them is asked for.  Doubles first: both parts stay aligned.
    const size_t window = !j->range && !j->range_out ? (size_t)S * (size_t)j->n_pair * 4 : 0;
    const size_t counts = !j->counts && joint_levels(*j) ? (size_t)S * (size_t)a.cells : 0;
    if (window || counts) HIP_TRY(c->joint_ws.reserve(window * sizeof(double) + counts * sizeof(int32_t)));
    a.chain = d_chain;
    a.from_data = j->range ? nullptr : window ? c->joint_ws.as<double>() : j->range_out;
    a.window = j->range ? j->range : a.from_data;
    a.counts = j->counts ? j->counts : counts ? reinterpret_cast<int32_t*>(c->joint_ws.as<double>() + window) : nullptr;
    a.inside = j->inside; a.mode = j->mode; a.level = j->level; a.n_cells = j->cells; a.held = j->held;
    if (j->range && j->range_out)
        HIP_TRY(hipMemcpyAsync(j->range_out, j->range, (size_t)S * (size_t)j->n_pair * 4 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if (!a.counts && !a.from_data) return 0;                                    // only range_out of a given range: the copy above
    HIP_TRY(misti::launch_joint(a, c->stream));
    return 0;
}

}  // extern "C"
