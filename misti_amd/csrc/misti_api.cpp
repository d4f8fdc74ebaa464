// C-ABI host layer of libmisti_hip.so (see include/misti_hip.h).
//
// Replaces, for a batch, what the reference does once per Python object:
//   MigrationInference.__init__ / SetModel   MigrationInference.py:41-289   -> misti_create
//   JAFSLikelihood                           MigrationInference.py:566-614  -> misti_eval_batch*
// No CPU fallback: every compute entry point needs a HIP device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <chrono>
#include <complex>
#include <thread>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "misti_ctx.h"
#include "misti_tables.hpp"

using namespace misti_host;

namespace {

thread_local std::string g_err;

const misti::HostTables& host_tables() {
    static const misti::HostTables t = misti::build_tables();
    return t;
}

constexpr size_t PIN_STAGE_MAX = (size_t)256 << 20;    // beyond this the host-buffer calls copy straight from / to the caller's memory

// Every live context of the process, so that a batch can tell whether the device is busy with other contexts' batches (the
// launch shape of mid-sized batches depends on it: latency when alone, throughput when not - misti_consts.h FOLLOW_BUSY_*).
std::mutex g_ctx_mu;
std::vector<misti_ctx*> g_ctxs;
// the device-wide table of chain waves per (compute unit, SIMD) (correct_follow_kernel's role choice): one per device, zeroed once
int32_t* g_pair_table[16] = {};
int32_t* pair_table(int device) {
    if (device < 0 || device >= 16) return nullptr;
    std::lock_guard<std::mutex> lock(g_ctx_mu);
    if (!g_pair_table[device]) {
        void* p = nullptr;
        if (hipMalloc(&p, misti::PAIR_TABLE * sizeof(int32_t)) != hipSuccess) return nullptr;
        if (hipMemset(p, 0, misti::PAIR_TABLE * sizeof(int32_t)) != hipSuccess) { (void)hipFree(p); return nullptr; }
        g_pair_table[device] = (int32_t*)p;
    }
    return g_pair_table[device];
}

int other_contexts_busy(const misti_ctx* self) {
    int busy = 0;
    std::lock_guard<std::mutex> lock(g_ctx_mu);
    for (misti_ctx* o : g_ctxs)
        if (o != self && o->device == self->device && o->last_ev_set && hipEventQuery(o->last_ev) == hipErrorNotReady) ++busy;
    (void)hipGetLastError();                       // "not ready" is an answer, not an error to be found by the next launch check
    return busy;
}

// Greedy runs of (numerically) constant lh, exactly as SmoothConst scans them
// (MigrationInference.py:387-405): a run starts at k and takes every j with
// |lh[j] - lh[k]| < 1e-10 while j < numT-1.
void smoothing_runs(const double* lh, int numT, int k, std::vector<int>& rs, std::vector<int>& re) {
    rs.assign(numT, 0);
    re.assign(numT, 0);
    int i = 0;
    while (i < numT) {
        int j = i;
        double lam = lh[2 * i + k];
        while (j < numT - 1 && std::fabs(lh[2 * j + k] - lam) < 1e-10) ++j;
        if (j == i) j = i + 1;                 // index numT-1: a run of its own (never smoothed: t < split <= numT-1)
        for (int t = i; t < j; ++t) { rs[t] = i; re[t] = j; }
        i = j;
    }
}

int validate_model(const misti_model_t* m) {
    if (!m) return fail(MISTI_E_ARG, "model is NULL");
    if (m->numT < 2) return fail(MISTI_E_ARG, "numT must be >= 2 (got %d)", m->numT);
    if (m->numT > MISTI_MAX_NUMT) return fail(MISTI_E_LIMIT, "numT %d exceeds MISTI_MAX_NUMT %d", m->numT, MISTI_MAX_NUMT);
    if (!m->times || !m->lh) return fail(MISTI_E_ARG, "times / lh is NULL");
    if (m->n_band < 0 || m->n_band > MISTI_MAX_BANDS) return fail(MISTI_E_LIMIT, "n_band %d out of range", m->n_band);
    if (m->n_pulse < 0 || m->n_pulse > MISTI_MAX_PULSES) return fail(MISTI_E_LIMIT, "n_pulse %d out of range", m->n_pulse);
    if (m->n_param < 0 || m->n_param > MISTI_MAX_PARAMS) return fail(MISTI_E_LIMIT, "n_param %d out of range", m->n_param);
    if ((m->n_band && !m->bands) || (m->n_pulse && !m->pulses)) return fail(MISTI_E_ARG, "bands / pulses is NULL");
    if (m->sample_date < 0 || m->sample_date >= m->numT) return fail(MISTI_E_ARG, "sample_date %d out of range", m->sample_date);
    for (int t = 0; t < m->numT - 1; ++t)
        if (!(m->times[t] >= 0) || !std::isfinite(m->times[t])) return fail(MISTI_E_ARG, "times[%d] is negative or not finite", t);
    for (int t = 0; t < 2 * m->numT; ++t)
        if (!(m->lh[t] > 0) || !std::isfinite(m->lh[t])) return fail(MISTI_E_ARG, "lh[%d] must be positive and finite", t);
    for (int b = 0; b < m->n_band; ++b) {
        const misti_band_t& B = m->bands[b];
        // SetModel, MigrationInference.py:237-247
        if (B.pop != 0 && B.pop != 1) return fail(MISTI_E_ARG, "band %d: population index should be 1 or 2", b);
        if (B.start < m->sample_date) return fail(MISTI_E_ARG, "band %d: migration start (%d) should be >= sample date (%d)", b, B.start, m->sample_date);
        if (B.end != -1 && B.end <= B.start) return fail(MISTI_E_ARG, "band %d: migration start (%d) should be strictly less than migration end (%d)", b, B.start, B.end);
        if (B.end > m->numT + 1) return fail(MISTI_E_ARG, "band %d: end %d beyond the grid", b, B.end);
        if (B.param < -1 || B.param >= m->n_param) return fail(MISTI_E_ARG, "band %d: param index %d out of range", b, B.param);
        if (B.param < 0 && !(B.value >= 0)) return fail(MISTI_E_ARG, "band %d: fixed rate must be >= 0", b);
        for (int c = 0; c < b; ++c) {                                   // :254-255 overlap
            const misti_band_t& C = m->bands[c];
            if (C.pop != B.pop) continue;
            int be = B.end < 0 ? INT32_MAX : B.end, ce = C.end < 0 ? INT32_MAX : C.end;
            if (B.start < ce && C.start < be) return fail(MISTI_E_ARG, "bands %d and %d: migration rate intervals should not overlap", c, b);
        }
    }
    for (int p = 0; p < m->n_pulse; ++p) {
        const misti_pulse_t& P = m->pulses[p];
        // :260-277
        if (P.pop != 0 && P.pop != 1) return fail(MISTI_E_ARG, "pulse %d: population index should be 1 or 2", p);
        if (P.time < m->sample_date) return fail(MISTI_E_ARG, "pulse %d: time (%d) should be >= sample date (%d)", p, P.time, m->sample_date);
        if (P.time >= m->numT + 1) return fail(MISTI_E_ARG, "pulse %d: time %d beyond the grid", p, P.time);
        if (P.param < -1 || P.param >= m->n_param) return fail(MISTI_E_ARG, "pulse %d: param index %d out of range", p, P.param);
        if (P.param < 0 && !(P.value >= 0 && P.value <= 1)) return fail(MISTI_E_ARG, "pulse %d: pulse migration rate should be between 0 and 1", p);
        for (int c = 0; c < p; ++c)
            if (m->pulses[c].time == P.time) return fail(MISTI_E_ARG, "pulses %d and %d: only single-direction pulse migration at a time", c, p);
    }
    return 0;
}

// Fold the finished event pairs of one stage into its totals (all of them when `all`, else only while more than
// `keep` are pending: a caller that enables timing and never reads it must not accumulate events without bound).
int drain_pending(misti_ctx* c, int which, bool all, size_t keep = 256) {
    auto& v = c->pending[which];
    size_t done = 0;
    while (done < v.size() && (all || v.size() - done > keep)) {
        HIP_TRY(hipEventSynchronize(v[done].second));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, v[done].first, v[done].second));
        c->ms[which] += t;
        (void)hipEventDestroy(v[done].first);
        (void)hipEventDestroy(v[done].second);
        ++done;
    }
    v.erase(v.begin(), v.begin() + (long)done);
    return 0;
}
int record_begin(misti_ctx* c, int which, hipEvent_t* a, hipEvent_t* b) {
    *a = *b = nullptr;
    if (!c->timing) return 0;
    if (int r = drain_pending(c, which, false)) return r;
    hipError_t e = hipEventCreate(a);
    if (e == hipSuccess) e = hipEventCreate(b);
    if (e == hipSuccess) e = hipEventRecord(*a, c->stream);
    if (e != hipSuccess) {
        if (*a) (void)hipEventDestroy(*a);
        if (*b) (void)hipEventDestroy(*b);
        *a = *b = nullptr;
        return fail(MISTI_E_HIP, "timing events: %s", hipGetErrorString(e));
    }
    return 0;
}
// which < 0: the stage failed - drop the pair
int record_end(misti_ctx* c, int which, hipEvent_t a, hipEvent_t b) {
    if (!a) return 0;
    hipError_t e = which >= 0 ? hipEventRecord(b, c->stream) : hipErrorUnknown;
    if (e != hipSuccess) {
        (void)hipEventDestroy(a);
        (void)hipEventDestroy(b);
        return which >= 0 ? fail(MISTI_E_HIP, "hipEventRecord: %s", hipGetErrorString(e)) : 0;
    }
    c->pending[which].push_back({a, b});
    return 0;
}
// a launch between record_begin and record_end failed: release the pair, keep the error
#define HIP_TRY_EV(expr, a, b)                                                            \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) { (void)record_end(c, -1, a, b); return fail(MISTI_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); } \
    } while (0)

// (hints: the RUN_* bits of misti_ctx.h)
int run_dev_impl(misti_ctx* c, int64_t n_cand, const double* d_split, const double* d_params, const int32_t* d_bounds, int64_t n_rep, const double* d_jsfs,
                 double* d_llk, double* d_jafs, double* d_lc, double* d_pr, int32_t* d_status, unsigned hints, const int32_t* d_pulses) {
    if (n_cand < 0 || n_rep < 0) return fail(MISTI_E_ARG, "negative batch size");
    if (n_cand == 0) return 0;
    if (!d_split) return fail(MISTI_E_ARG, "split_time is NULL");
    if (c->hints & MISTI_HINT_INTEGER_SPLITS) hints |= RUN_INTEGER_SPLITS;           // the caller's word (verified on the device: spectrum_kernel)
    if (c->dm.n_param > 0 && !d_params) return fail(MISTI_E_ARG, "params is NULL but the model has %d parameters", c->dm.n_param);
    if (n_rep > 0 && (!d_jsfs || !d_llk)) return fail(MISTI_E_ARG, "jsfs / llk is NULL with n_rep > 0");
    HIP_TRY(hipSetDevice(c->device));
    if (!d_jafs) { HIP_TRY(c->ws_jafs.reserve((size_t)n_cand * 7 * sizeof(double))); d_jafs = c->ws_jafs.as<double>(); }
    if (!d_status) { HIP_TRY(c->ws_status.reserve((size_t)n_cand * sizeof(int32_t))); d_status = c->ws_status.as<int32_t>(); }
    if (n_cand > INT32_MAX / 8) return fail(MISTI_E_LIMIT, "n_cand too large for one call");
    const size_t nc = (size_t)n_cand, numT = (size_t)c->dm.numT;
    // chain machinery: one allocation per type, carved below
    const size_t tsize = misti::chain_table_size(n_cand);
    const int64_t follow_max_h = c->tune.follow_max > 0 ? c->tune.follow_max : misti::FOLLOW_MAX_CHAINS;
    const size_t ntr = ((hints & RUN_UNSHARED) && n_cand > follow_max_h) ? 0 : (size_t)misti::trunk_capacity(n_cand, c->tune);
    const size_t f64_n = nc * numT * 2 + nc * (numT + 1) * 6 + nc * 6 + nc * 2 + nc * 6;
    // chain tables: TWO sets {n_chains[2], table, slot_chain, slot_len} used alternately - a batch clears the other set for its successor
    const size_t set_n = 4 + 4 * tsize;                     // counters [4] | table | slot_chain | slot_len | slot_keep
    const size_t i32_n = 2 * set_n + 10 * nc + ntr;         // two table sets | slot_of, of, chain_slot, rep, fail_t, fail_status, tail_status, chain_order, resume_t, resume_list | trunk_ok
    HIP_TRY(c->ws_chain_f64.reserve(f64_n * sizeof(double)));
    {
        void* before = c->ws_chain_i32.p;
        HIP_TRY(c->ws_chain_i32.reserve(i32_n * sizeof(int32_t)));
        if (c->ws_chain_i32.p != before) c->table_clean[0] = c->table_clean[1] = 0;      // a new allocation: nothing is clean
    }
    HIP_TRY(c->ws_order.reserve(nc * sizeof(int32_t)));
    if (ntr) HIP_TRY(c->ws_trunk.reserve(ntr * numT * misti::TRUNK_REC * sizeof(double)));
    if (n_rep > 0) HIP_TRY(c->consts.reserve((size_t)n_rep * sizeof(double)));
    c->batches_begun += 1;                          // from here on the batch puts work into the stream
    misti::ChainBufs cb;
    {
        double* d = c->ws_chain_f64.as<double>();
        cb.lc = d; d += nc * numT * 2;
        cb.trace = d; d += nc * (numT + 1) * 6;
        cb.work = d; d += nc * 6;
        cb.tail_lc = d; d += nc * 2;
        cb.tail_state = d;
        int32_t* q = c->ws_chain_i32.as<int32_t>();
        const int cur = c->table_cur;
        int32_t* set[2] = {q, q + set_n};
        q += 2 * set_n;
        // a set is clean for this batch if the previous batch cleared it for exactly this table size (same layout)
        if (c->table_clean[cur] != tsize) HIP_TRY(hipMemsetAsync(set[cur], 0, set_n * sizeof(int32_t), c->stream));
        c->table_clean[cur] = 0;                    // about to be used
        c->table_clean[cur ^ 1] = 0;                // until the setup launch below is in the stream
        cb.n_chains = set[cur]; cb.table = set[cur] + 4; cb.slot_chain = cb.table + tsize; cb.slot_len = cb.slot_chain + tsize;
        cb.slot_keep = cb.slot_len + tsize;
        cb.z_n_chains = set[cur ^ 1]; cb.z_table = set[cur ^ 1] + 4; cb.z_slot_len = cb.z_table + 2 * tsize; cb.z_slot_keep = cb.z_slot_len + tsize;
        cb.slot_of = q; q += nc; cb.of = q; q += nc; cb.chain_slot = q; q += nc; cb.rep = q; q += nc;
        cb.fail_t = q; q += nc; cb.fail_status = q; q += nc; cb.tail_status = q; q += nc; cb.chain_order = q; q += nc; cb.resume_t = q; q += nc; cb.resume_list = q; q += nc;
        cb.trunk_ok = q;
        cb.tmask = (uint32_t)(tsize - 1);
        cb.trunk = ntr ? c->ws_trunk.as<double>() : nullptr;
        cb.trunk_cap = (int64_t)ntr;
        cb.hint = c->hint_dev;
        cb.simd_load = c->tune.pairing ? pair_table(c->device) : nullptr;
        cb.bounds = c->dm.n_band > 0 ? d_bounds : nullptr;
        cb.pulse_times = c->dm.n_pulse > 0 ? d_pulses : nullptr;
        cb.integer_splits = (hints & RUN_INTEGER_SPLITS) ? 1 : 0;
        cb.post_lam = nullptr;
        cb.post_word = nullptr;
        if (!(c->dm.flags & MISTI_CPFIT)) {
            HIP_TRY(c->ws_post.reserve(nc * (numT + 1) * (sizeof(double) + sizeof(int32_t))));
            cb.post_lam = c->ws_post.as<double>();
            if (c->trace) cb.post_word = reinterpret_cast<int32_t*>(cb.post_lam + nc * (numT + 1));
        }
        cb.solver = cb.tail_solver = cb.cand_solver = nullptr;
        cb.iters = nullptr;
        cb.iter_cap = 0;
        c->trace_n = 0;
        c->trace_iter_cap = 0;
        if (c->trace) {
            HIP_TRY(c->ws_solver.reserve((nc * numT + nc + nc * (numT + 1)) * sizeof(int32_t)));
            HIP_TRY(hipMemsetAsync(c->ws_solver.p, 0, (nc * numT + nc + nc * (numT + 1)) * sizeof(int32_t), c->stream));
            cb.solver = c->ws_solver.as<int32_t>();
            cb.tail_solver = cb.solver + nc * numT;
            cb.cand_solver = cb.tail_solver + nc;
            c->trace_n = n_cand;
            c->trace_of = cb.of;
            if (n_cand <= MISTI_TRACE_MAX_CAND) {
                const size_t it_n = nc * numT * MISTI_TRACE_MAX_ITER * 2;
                HIP_TRY(c->ws_iters.reserve(it_n * sizeof(double)));
                HIP_TRY(hipMemsetAsync(c->ws_iters.p, 0xff, it_n * sizeof(double), c->stream));      // all-ones = NaN: "no such iterate"
                cb.iters = c->ws_iters.as<double>();
                cb.iter_cap = n_cand;
                c->trace_iter_cap = n_cand;
            }
        }
    }
    // Launch shape of kernel 1 depends on the number of chains, which lives on the device: setup_kernel drops
    // {chains, candidates, batch tag} into pinned memory.  A batch of the same size as the previous one on this
    // context uses that one's count (no waiting; a stale value costs speed only); otherwise the host waits for
    // this batch's own count - bounded, a few microseconds after the launch.
    c->batch_seq += 1;
    cb.seq = c->batch_seq;
    cb.unsorted = (hints & RUN_ONE_LENGTH) ? 3 : 0;          // bit 0: candidates in their own order, bit 1: chains in order of arrival
    int64_t est_chains = -1;
    const volatile int32_t* hint = c->hint_host;
    if (hint && hint[1] == (int32_t)n_cand && hint[0] > 0 && hint[0] <= n_cand) est_chains = hint[0];
    // chains per wavefront: packed (up to 8) when the batch is large - fewer instructions in total, which is what
    // counts when batches overlap - unless it is known to collapse into a few long chains (pure latency: one chain
    // per wave and the trunk following it)
    int busy_seen = -1;                                      // other contexts with a batch in flight (looked up at most once per batch)
    auto busy = [&]() { if (busy_seen < 0) busy_seen = other_contexts_busy(c); return busy_seen; };
    auto shape = [&](int64_t est, int& cpw, bool& follow) {
        int64_t follow_max = c->tune.follow_max > 0 ? c->tune.follow_max : misti::FOLLOW_MAX_CHAINS;
        // mid-sized batches: one chain per wave is the latency shape (a 1 024-chain batch then occupies every wave slot of the chip);
        // when other contexts have batches in flight the caller is after throughput and the packed shape carries ten chains per
        // instruction stream (up to 1.9 x the rate).  Looked at only where it matters; the result never depends on it.
        const int busy_from = c->tune.busy_contexts >= 0 ? c->tune.busy_contexts : misti::FOLLOW_BUSY_CONTEXTS;
        if (c->tune.follow_max <= 0 && busy_from > 0 && est > misti::FOLLOW_BUSY_CHAINS && est <= follow_max && busy() >= busy_from)
            follow_max = misti::FOLLOW_BUSY_CHAINS;
        cpw = (est >= 0 && est <= follow_max) ? 1 : misti::correct_cands_per_wave(n_cand, c->tune);
        // The default fit's one-chain-per-wave kernel holds ONE wave per SIMD (512 registers): with its trunk wave beside it a 64-chain batch
        // takes 128 of the chip's 1 024 wave slots and eight batches fill it, where --cpfit fits sixteen.  With other contexts' batches in
        // flight a small default-fit batch therefore packs two chains per wave (trunks in the next launch): measured on the headline grid
        // with 20 batches in flight 2.03 -> 2.62e7 evals/s (4 per wave 2.39, 8: 1.94, 10: 2.11; trunks after the chains but one chain
        // per wave 2.46); alone it keeps the latency shape (1.73 ms against 2.54).  The result never depends on it.
        if (!(c->dm.flags & MISTI_CPFIT) && cpw == 1 && est >= 0 && est <= misti::FOLLOW_BUSY_CHAINS && busy_from > 0 && c->tune.follow_max <= 0 &&
            busy() >= busy_from)
            cpw = 2;
        const int f = c->tune.chains_per_wave;                       // diagnostic override (scratch experiments, tests)
        if (f == 1 || f == 2 || f == 4 || f == 8 || f == 10) cpw = f;
        follow = misti::trunk_follows(cpw, (int64_t)ntr, c->tune);
    };
    // a batch is four launches (+1 for the default fit, +1 with more than LLK_INLINE_MAX replicates): setup | chains |
    // trunks + tails | candidates (+ replicate epilogue) - three where the trunk follows its chain inside the chain launch
    // (the headline grid: setup | chains with their trunks and tails | candidates).  Few launches matter when many batches are in flight.
    int32_t* d_order = c->ws_order.as<int32_t>();
    double* d_consts = n_rep > 0 ? c->consts.as<double>() : nullptr;
    const bool llk_inline = n_rep > 0 && n_rep <= misti::LLK_INLINE_MAX;
    hipEvent_t a = nullptr, b = nullptr;
    if (int r = record_begin(c, 0, &a, &b)) return r;
    HIP_TRY_EV(misti::launch_setup(c->dm, n_cand, d_params, d_split, cb, d_order, n_rep, d_jsfs, d_consts, c->unfolded, c->stream), a, b);
    c->table_clean[c->table_cur ^ 1] = tsize;       // setup_kernel clears the other set (table, slot_len, counters) for this table size
    c->table_cur ^= 1;
    if (est_chains < 0 && hint && misti::correct_cands_per_wave(n_cand, c->tune) > 1) {
        const auto t0 = std::chrono::steady_clock::now();
        while (hint[2] != cb.seq && std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(500)) std::this_thread::yield();
        if (hint[2] == cb.seq && hint[1] == (int32_t)n_cand) est_chains = hint[0];
    }
    int cpw_chains = 1;
    bool follow = false;
    shape(est_chains, cpw_chains, follow);
    // Packed launches let a chain whose solve runs away yield to a second launch, one chain per wave (latency: a packed launch ends
    // with its few long chains) - unless other contexts keep the device busy, where the packed shape's throughput is what counts.
    // --cpfit only by default: the default fit's one-per-wave kernel holds one wave per SIMD, half the resume launch's parallelism, and
    // its solves are short (bounded 2-D fits) - measured on 16 384 chains 3.59 ms without yielding, 4.39 with (MISTI_YIELD_NFEV forces it).
    int yield_nfev = 0;
    if (cpw_chains > 1) {
        yield_nfev = c->tune.yield_nfev >= 0 ? c->tune.yield_nfev : ((c->dm.flags & MISTI_CPFIT) ? misti::YIELD_NFEV : 0);
        const int busy_from = c->tune.busy_contexts >= 0 ? c->tune.busy_contexts : misti::FOLLOW_BUSY_CONTEXTS;
        if (yield_nfev > 0 && busy_from > 0 && busy() >= busy_from) yield_nfev = 0;
    }
    // Two phases behind a packed launch that lets chains yield (--cpfit; misti_chain.h: wrong_phase): what waits for the chains that launch
    // completed - trunks, tails, the candidate kernel of their members: 91 % of BASELINE config 3 - runs on a second stream BESIDE the resume
    // launch, which is one chain latency long and leaves most of the chip idle; the members of the chains that yielded follow behind it on the
    // batch's own stream, which then waits for the second one.  MISTI_TWO_PHASE=0 keeps everything on one stream.
    // Only while NO other context of the process has a batch in flight: the second stream is one more hardware queue (a process gets 24, and
    // twenty contexts with a second stream each collapse the overlapped rate: config 5 4.5e7 -> 2.9e7 evals/s measured), and beside other contexts'
    // batches there is no idle chip to fill.
    const bool two_phase = yield_nfev > 0 && (c->dm.flags & MISTI_CPFIT) && c->tune.two_phase && busy() == 0;
    if (two_phase) {
        if (!c->side_stream) HIP_TRY_EV(hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking), a, b);
        if (!c->packed_ev) HIP_TRY_EV(hipEventCreateWithFlags(&c->packed_ev, hipEventDisableTiming), a, b);
        if (!c->side_ev) HIP_TRY_EV(hipEventCreateWithFlags(&c->side_ev, hipEventDisableTiming), a, b);
    }
    HIP_TRY_EV(misti::launch_correct(c->dm, n_cand, cb, d_split, d_params, cpw_chains, follow, est_chains, c->tune, yield_nfev, c->stream,
                                     two_phase ? c->packed_ev : nullptr), a, b);
    // Kernel 2 in single-wave workgroups (they slip into any free wave slot while other batches' chain kernels are resident: +21 % on
    // the headline grid with 20 batches in flight) - except behind a chip-filling one-chain-per-wave launch of this context's own:
    // there the next such launch was measured 18 % slower after single-wave workgroups (1.66 -> 1.96 ms on 1 024 chains; the placement
    // of its chain and trunk waves on the SIMDs follows where the previous kernel's workgroups ended), and such a batch runs alone -
    // with other contexts busy it would have taken the packed shape.
    const bool single_waves = c->tune.k2_single_waves >= 0 ? c->tune.k2_single_waves != 0 : !(follow && est_chains > 256);
    if (int r = record_end(c, 0, a, b)) return r;
    if (c->timing) c->launches[0] += 1;
    HIP_TRY(c->ws_diag.reserve(nc * sizeof(double)));
    c->diag_n = n_cand;
    if (int r = record_begin(c, 1, &a, &b)) return r;
    const bool skip_post = (hints & RUN_INTEGER_SPLITS) && (follow || ntr == 0);
    if (two_phase) {
        HIP_TRY_EV(hipStreamWaitEvent(c->side_stream, c->packed_ev, 0), a, b);
        HIP_TRY_EV(misti::launch_spectrum(c->dm, n_cand, d_order, d_split, d_params, cb, d_lc, d_pr, d_jafs, d_status, c->ws_diag.as<double>(),
                                          n_rep, d_jsfs, d_consts, d_llk, follow, skip_post, single_waves, c->tune, c->side_stream, 1), a, b);
        HIP_TRY_EV(hipEventRecord(c->side_ev, c->side_stream), a, b);
    }
    HIP_TRY_EV(misti::launch_spectrum(c->dm, n_cand, d_order, d_split, d_params, cb, d_lc, d_pr, d_jafs, d_status, c->ws_diag.as<double>(),
                                      n_rep, d_jsfs, d_consts, d_llk, follow, skip_post, single_waves, c->tune, c->stream, two_phase ? 2 : 0), a, b);
    if (two_phase) HIP_TRY_EV(hipStreamWaitEvent(c->stream, c->side_ev, 0), a, b);            // the batch's stream is behind both phases from here on
    if (int r = record_end(c, 1, a, b)) return r;
    if (c->timing) c->launches[1] += 1;
    if (n_rep > 0 && !llk_inline) {
        if (int r = record_begin(c, 2, &a, &b)) return r;
        HIP_TRY_EV(misti::launch_llk(n_cand, d_jafs, d_status, n_rep, d_jsfs, d_consts, d_llk, c->unfolded, c->stream), a, b);
        if (int r = record_end(c, 2, a, b)) return r;
        if (c->timing) c->launches[2] += 1;
    }
    if (c->last_ev) {                              // behind the batch: other contexts read it (other_contexts_busy), and so does the context's lane (misti_lanes.cpp)
        std::lock_guard<std::mutex> lock(g_ctx_mu);
        HIP_TRY(hipEventRecord(c->last_ev, c->stream));
        c->last_ev_set = true;
        c->batches_recorded += 1;
    }
    return 0;
}

}  // namespace

// A two-phase batch joins its side stream to the batch's stream with its LAST wait; a failure anywhere between the phase-1 launch and
// that wait would return with phase-1 kernels in flight on a stream nothing else waits for (misti_sync and the host-buffer drain
// know the batch's stream) while the next batch's set-up rewrites the chain buffers they read.  So: on any failure the side stream is
// drained before the error is reported.
int misti_host::run_dev(misti_ctx* c, int64_t n_cand, const double* d_split, const double* d_params, const int32_t* d_bounds, int64_t n_rep,
                        const double* d_jsfs, double* d_llk, double* d_jafs, double* d_lc, double* d_pr, int32_t* d_status, unsigned hints,
                        const int32_t* d_pulses) {
    const int r = run_dev_impl(c, n_cand, d_split, d_params, d_bounds, n_rep, d_jsfs, d_llk, d_jafs, d_lc, d_pr, d_status, hints, d_pulses);
    if (r != 0 && c->side_stream) {
        const std::string why = g_err;
        (void)hipStreamSynchronize(c->side_stream);
        (void)hipGetLastError();
        g_err = why;
    }
    return r;
}

extern "C" {

int misti_abi_version(void) { return MISTI_ABI_VERSION; }
#ifndef MISTI_BUILD_ID
#define MISTI_BUILD_ID "unknown"
#endif
const char* misti_build_id(void) { return MISTI_BUILD_ID; }

const char* misti_last_error(void) { return g_err.c_str(); }

// internal (misti_fail.h): make `msg` the calling thread's last error; returns `code`
int misti_set_error_(int code, const char* msg) { g_err = msg ? msg : ""; return code; }

int misti_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(MISTI_E_NODEV, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    return n;
}

int misti_tables(int32_t* gen, int32_t* jaf) {
    try {
        const misti::HostTables& t = host_tables();
        if (gen)
            for (int k = 0; k < 4; ++k) for (int d = 0; d < misti::NS2; ++d) for (int s = 0; s < misti::NS2; ++s)
                gen[(k * misti::NS2 + d) * misti::NS2 + s] = t.gen[k][d][s];
        if (jaf)
            for (int s = 0; s < misti::NS2; ++s) for (int c = 0; c < 7; ++c) jaf[s * 7 + c] = t.jaf[s][c];
    } catch (const std::exception& e) {
        return fail(MISTI_E_ARG, "table construction failed: %s", e.what());
    }
    return 0;
}

// internal (misti_lanes.cpp): misti_create with the context's own stream on a stream priority of the caller's choice (a value of
// hipDeviceGetStreamPriorityRange; 0 is the default).  The runtime keeps one pool of hardware queues per priority, which is how a lane
// pool reaches more queues than GPU_MAX_HW_QUEUES.  The side stream of two-phase batches is created at the default priority as before.
int misti_create_prio_(const misti_model_t* model, int device, int priority, misti_ctx** out) {
    if (!out) return fail(MISTI_E_ARG, "out is NULL");
    *out = nullptr;
    if (int r = validate_model(model)) return r;
    int ndev = misti_device_count();
    if (ndev <= 0) return fail(MISTI_E_NODEV, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(MISTI_E_ARG, "device %d out of range (0..%d)", device, ndev - 1);
    misti_ctx* c = nullptr;
    // every failure after `new` releases what the context already owns (stream, pinned hint, device buffers)
    struct Guard { misti_ctx*& c; bool keep = false; ~Guard() { if (!keep && c) { misti_destroy(c); c = nullptr; } } } guard{c};
    try {
        c = new misti_ctx();
        c->tune = misti::read_tuning();
        const misti::HostTables& t = host_tables();
        c->device = device;
        HIP_TRY(hipSetDevice(device));
        // constant tables (per device; idempotent)
        misti::DevTables dt{};
        std::memcpy(dt.src, t.src, sizeof dt.src);
        std::memcpy(dt.kind, t.kind, sizeof dt.kind);
        std::memcpy(dt.mult, t.mult, sizeof dt.mult);
        std::memcpy(dt.dcnt, t.dcnt, sizeof dt.dcnt);
        for (int cl = 0; cl < 7; ++cl) {
            for (int s = 0; s < 64; ++s) dt.jaf[cl][s] = s < misti::NS2 ? t.jaf[s][cl] : 0;
            for (int s = 0; s < misti::NS1; ++s) dt.jaf1[cl][s] = t.jaf1[s][cl];
            for (int s = 0; s < misti::NS2; ++s) {
                const int wgt = t.jaf[s][cl];
                if (wgt < 0 || wgt > 7) throw std::runtime_error("spectrum weight out of range");
                for (int b = 0; b < 3; ++b) if ((wgt >> b) & 1) dt.jaf_bits[cl][b] |= 1ull << s;
            }
            for (int s = 0; s < misti::NS1; ++s) {
                const int wgt = t.jaf1[s][cl];
                if (wgt < 0 || wgt > 7) throw std::runtime_error("spectrum weight out of range");
                dt.jaf1_bits[cl] |= (unsigned)wgt << (3 * s);
            }
        }
        std::memcpy(dt.grp_lo, t.grp_lo, sizeof dt.grp_lo);
        std::memcpy(dt.grp_hi, t.grp_hi, sizeof dt.grp_hi);
        std::memcpy(dt.anc_n, t.anc_n, sizeof dt.anc_n);
        std::memcpy(dt.anc_dst, t.anc_dst, sizeof dt.anc_dst);
        std::memcpy(dt.anc_src, t.anc_src, sizeof dt.anc_src);
        std::memcpy(dt.pulse_n, t.pulse_n, sizeof dt.pulse_n);
        std::memcpy(dt.pulse_src, t.pulse_src, sizeof dt.pulse_src);
        std::memcpy(dt.pulse_ab, t.pulse_ab, sizeof dt.pulse_ab);
        {   // modified Talbot contour z(th) = N[-0.6122 + 0.5017 th cot(0.6407 th) + 0.2645 i th]
            // (Trefethen, Weideman, Schmelzer 2006), midpoint nodes th_k = -pi + (2k-1) pi/N, upper half
            const int N = misti::TALBOT_N;
            const double PI = 3.14159265358979323846;
            for (int j = 0; j < misti::TALBOT_HALF; ++j) {
                int k = N / 2 + 1 + j;
                double th = -PI + (2.0 * k - 1.0) * PI / N;
                double a = 0.6407 * th;
                std::complex<double> z(N * (-0.6122 + 0.5017 * th / std::tan(a)), N * 0.2645 * th);
                std::complex<double> dz(N * (0.5017 / std::tan(a) - 0.5017 * 0.6407 * th / (std::sin(a) * std::sin(a))), N * 0.2645);
                std::complex<double> cw = std::complex<double>(0.0, 1.0 / N) * std::exp(z) * dz;
                dt.tal_zr[j] = z.real(); dt.tal_zi[j] = z.imag(); dt.tal_cr[j] = cw.real(); dt.tal_ci[j] = cw.imag();
            }
        }
        HIP_TRY(misti::upload_tables(dt));
        // the closed form after the split assumes this one-population generator
        static const int want1[8][8] = {{-6, 0, 0, 0, 0, 0, 0, 0}, {1, -3, 0, 0, 0, 0, 0, 0}, {4, 0, -3, 0, 0, 0, 0, 0}, {1, 0, 0, -3, 0, 0, 0, 0},
                                        {0, 2, 1, 0, -1, 0, 0, 0}, {0, 0, 1, 2, 0, -1, 0, 0}, {0, 1, 0, 1, 0, 0, -1, 0}, {0, 0, 1, 0, 0, 0, 0, -1}};
        for (int i = 0; i < 8; ++i) for (int j = 0; j < 8; ++j)
            if (t.gen1[i][j] != want1[i][j]) return fail(MISTI_E_ARG, "one-population generator mismatch at (%d,%d)", i, j);

        const int numT = model->numT;
        if (priority == 0) HIP_TRY(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
        else HIP_TRY(hipStreamCreateWithPriority(&c->own_stream, hipStreamNonBlocking, priority));
        if (hipHostMalloc((void**)&c->hint_host, 4 * sizeof(int32_t), hipHostMallocMapped) == hipSuccess) {
            c->hint_host[0] = c->hint_host[1] = c->hint_host[2] = 0;
            if (hipHostGetDevicePointer((void**)&c->hint_dev, c->hint_host, 0) != hipSuccess) c->hint_dev = nullptr;
        } else { (void)hipGetLastError(); c->hint_host = nullptr; }
        c->stream = c->own_stream;
        std::vector<double> f64((size_t)(numT - 1) + 2 * (size_t)numT);
        std::memcpy(f64.data(), model->times, sizeof(double) * (numT - 1));
        std::memcpy(f64.data() + (numT - 1), model->lh, sizeof(double) * 2 * numT);
        HIP_TRY(c->model_f64.reserve(f64.size() * sizeof(double)));
        HIP_TRY(hipMemcpy(c->model_f64.p, f64.data(), f64.size() * sizeof(double), hipMemcpyHostToDevice));
        std::vector<int> runs(4 * (size_t)numT), rs, re;
        for (int k = 0; k < 2; ++k) {
            smoothing_runs(model->lh, numT, k, rs, re);
            std::memcpy(runs.data() + k * numT, rs.data(), sizeof(int) * numT);
            std::memcpy(runs.data() + (2 + k) * numT, re.data(), sizeof(int) * numT);
        }
        {
            // Where can a candidate leave its chain's trunk?  (trunk_leave in misti_model.h, for every split an integer or a
            // fractional split time can produce.)  A function of the smoothing runs alone: the trunk stores records only there.
            const int* rs0 = runs.data(), *rs1 = runs.data() + numT, *re0 = runs.data() + 2 * numT, *re1 = runs.data() + 3 * numT;
            std::vector<int> ok((size_t)numT, 0);
            const bool smooth = (model->flags & MISTI_SMOOTH) != 0;
            for (int s = 0; s < numT; ++s) {
                int frac_own = s, int_own = s;
                if (smooth) {
                    frac_own = rs0[s] < rs1[s] ? rs0[s] : rs1[s];               // the interval s is split in two
                    if (s > 0) {
                        if (re0[s - 1] > s && rs0[s - 1] < int_own) int_own = rs0[s - 1];
                        if (re1[s - 1] > s && rs1[s - 1] < int_own) int_own = rs1[s - 1];
                    }
                }
                ok[(size_t)frac_own] = 1;
                ok[(size_t)int_own] = 1;
            }
            runs.insert(runs.end(), ok.begin(), ok.end());
        }
        HIP_TRY(c->model_i32.reserve(runs.size() * sizeof(int)));
        HIP_TRY(hipMemcpy(c->model_i32.p, runs.data(), runs.size() * sizeof(int), hipMemcpyHostToDevice));
        misti::DevModel& d = c->dm;
        d.numT = numT;
        d.sample_date = model->sample_date;
        d.flags = model->flags;
        d.n_band = model->n_band; d.n_pulse = model->n_pulse; d.n_param = model->n_param;
        d.mixture_th = model->mixture_th;
        d.times = c->model_f64.as<double>();
        d.lh = d.times + (numT - 1);
        d.run_start = c->model_i32.as<int>();
        d.run_end = d.run_start + 2 * numT;
        d.leave_ok = d.run_start + 4 * numT;
        for (int b = 0; b < model->n_band; ++b) d.bands[b] = model->bands[b];
        for (int p = 0; p < model->n_pulse; ++p) d.pulses[p] = model->pulses[p];
        c->unfolded = (model->flags & MISTI_UNFOLDED) ? 1 : 0;
    } catch (const std::exception& e) {
        return fail(MISTI_E_ARG, "misti_create: %s", e.what());
    }
    if (hipEventCreateWithFlags(&c->last_ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); c->last_ev = nullptr; }
    {
        std::lock_guard<std::mutex> lock(g_ctx_mu);
        g_ctxs.push_back(c);
    }
    guard.keep = true;
    *out = c;
    return 0;
}

int misti_create(const misti_model_t* model, int device, misti_ctx** out) { return misti_create_prio_(model, device, 0, out); }

// internal (misti_lanes.cpp): the event the context records behind every batch (NULL: it has none), how many batches have recorded it and
// how many have put work into the stream.  A lane reads the counters around a batch: the first moved - the context's record, on the
// lane's stream, stands behind that batch and the lane needs none of its own; only the second moved - the batch failed with work in flight.
void* misti_batch_event_(misti_ctx* c, int64_t* recorded, int64_t* begun) {
    if (!c) return nullptr;
    if (recorded) *recorded = c->batches_recorded;
    if (begun) *begun = c->batches_begun;
    return static_cast<void*>(c->last_ev);
}

int misti_destroy(misti_ctx* c) {
    if (!c) return 0;
    {
        std::lock_guard<std::mutex> lock(g_ctx_mu);
        for (size_t i = 0; i < g_ctxs.size(); ++i) if (g_ctxs[i] == c) { g_ctxs.erase(g_ctxs.begin() + (long)i); break; }
    }
    (void)hipSetDevice(c->device);
    // EVERYTHING the context ever issued is finished before anything it owns is released: the stream batches are issued on (the
    // caller's, after misti_set_stream), the context's own stream (work issued before a misti_set_stream is ordered before its
    // successor by an event, which this wait does not rely on) and the side stream of two-phase batches.  Only then buffers, the
    // mapped hint word the set-up kernel writes, events, and last the streams themselves.
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->own_stream && c->own_stream != c->stream) (void)hipStreamSynchronize(c->own_stream);
    if (c->side_stream) (void)hipStreamSynchronize(c->side_stream);
    (void)hipGetLastError();
    for (auto* b : {&c->model_f64, &c->model_i32, &c->consts, &c->ws_jafs, &c->ws_status, &c->ws_chain_f64, &c->ws_chain_i32, &c->ws_order, &c->ws_diag, &c->ws_trunk, &c->ws_solver, &c->ws_iters, &c->ws_post,
                    &c->st_split, &c->st_params, &c->st_bounds, &c->st_pulses, &c->st_jsfs, &c->st_llk, &c->st_jafs, &c->st_lc, &c->st_pr, &c->st_status, &c->nm_f64, &c->nm_i32, &c->scan_v, &c->scan_i, &c->prof_v, &c->prof_i, &c->prof_idx, &c->curv_f64, &c->curv_i32, &c->boot_chunks, &c->param_totals, &c->post_ws, &c->joint_ws, &c->bands_ws, &c->bands_f64, &c->bands_i32})
        b->release();
    c->pin_in.release();
    c->pin_out.release();
    if (c->nm_live_host) (void)hipHostFree(c->nm_live_host);
    if (c->hint_host) (void)hipHostFree(c->hint_host);
    for (int w = 0; w < 3; ++w)
        for (auto& pr : c->pending[w]) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (hipEvent_t e : {c->order_ev, c->last_ev, c->packed_ev, c->side_ev}) if (e) (void)hipEventDestroy(e);
    if (c->side_stream) (void)hipStreamDestroy(c->side_stream);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    (void)hipGetLastError();
    delete c;
    return 0;
}

int misti_set_stream(misti_ctx* c, void* s) {
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    hipStream_t next = s ? static_cast<hipStream_t>(s) : c->own_stream;
    if (next == c->stream) return 0;
    // All batches of a context share its workspaces (chain table, rates, trunk records, the pinned hint) and the
    // *_dev calls are asynchronous: what was issued on the old stream must finish before anything issued on the new
    // one starts, or batch N+1 overwrites what batch N is still reading.
    HIP_TRY(hipSetDevice(c->device));
    if (!c->order_ev) HIP_TRY(hipEventCreateWithFlags(&c->order_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c->order_ev, c->stream));
    HIP_TRY(hipStreamWaitEvent(next, c->order_ev, 0));
    c->stream = next;
    return 0;
}

int misti_set_hints(misti_ctx* c, uint32_t hints) {
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    if (hints & ~MISTI_HINT_INTEGER_SPLITS) return fail(MISTI_E_ARG, "unknown hint bits 0x%x", (unsigned)(hints & ~MISTI_HINT_INTEGER_SPLITS));
    c->hints = hints;
    return 0;
}

int misti_get_stream(misti_ctx* c, void** s) {
    if (!c || !s) return fail(MISTI_E_ARG, "ctx / output is NULL");
    *s = static_cast<void*>(c->stream);
    return 0;
}

int misti_sync(misti_ctx* c) {
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->side_stream) HIP_TRY(hipStreamSynchronize(c->side_stream));      // joined to the stream by every batch that used it; a failed one may not have got that far
    return 0;
}

int misti_eval_batch_dev(misti_ctx* c, int64_t n_cand, const double* d_split, const double* d_params, const int32_t* d_bounds, int64_t n_rep,
                         const double* d_jsfs, double* d_llk, double* d_jafs, double* d_lc, double* d_pr, int32_t* d_status) {
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    return run_dev(c, n_cand, d_split, d_params, d_bounds, n_rep, d_jsfs, d_llk, d_jafs, d_lc, d_pr, d_status);
}

int misti_eval_batch_pulses_dev(misti_ctx* c, int64_t n_cand, const double* d_split, const double* d_params, const int32_t* d_bounds,
                                const int32_t* d_pulse_times, int64_t n_rep, const double* d_jsfs, double* d_llk, double* d_jafs, double* d_lc,
                                double* d_pr, int32_t* d_status) {
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    return run_dev(c, n_cand, d_split, d_params, d_bounds, n_rep, d_jsfs, d_llk, d_jafs, d_lc, d_pr, d_status, 0u, d_pulse_times);
}

int misti_llk_dev(misti_ctx* c, int64_t n_cand, const double* d_jafs, const int32_t* d_status, int64_t n_rep, const double* d_jsfs, double* d_llk) {
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    if (n_cand < 0 || n_rep < 0) return fail(MISTI_E_ARG, "negative batch size");
    if (n_cand == 0 || n_rep == 0) return 0;
    if (!d_jafs || !d_jsfs || !d_llk) return fail(MISTI_E_ARG, "jafs / jsfs / llk is NULL");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->consts.reserve((size_t)n_rep * sizeof(double)));
    HIP_TRY(misti::launch_llh_const(n_rep, d_jsfs, c->consts.as<double>(), c->unfolded, c->stream));
    hipEvent_t a = nullptr, b = nullptr;
    if (int r = record_begin(c, 2, &a, &b)) return r;
    HIP_TRY_EV(misti::launch_llk(n_cand, d_jafs, d_status, n_rep, d_jsfs, c->consts.as<double>(), d_llk, c->unfolded, c->stream), a, b);
    if (int r = record_end(c, 2, a, b)) return r;
    if (c->timing) c->launches[2] += 1;
    return 0;
}

int misti_argmax_dev(misti_ctx* c, int64_t n_cand, int64_t n_rep, const double* d_llk, int32_t* d_best, double* d_best_llk) {
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    if (n_cand < 0 || n_rep < 0) return fail(MISTI_E_ARG, "negative batch size");
    if (n_rep == 0) return 0;
    if (!d_best || (n_cand > 0 && !d_llk)) return fail(MISTI_E_ARG, "llk / best is NULL");
    if (n_cand > INT32_MAX) return fail(MISTI_E_LIMIT, "n_cand too large");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(misti::launch_argmax(n_cand, n_rep, d_llk, d_best, d_best_llk, c->stream));
    return 0;
}

int misti_scan_best_dev(misti_ctx* c, int64_t n_cand, const double* d_jafs, const int32_t* d_status, int64_t n_rep, const double* d_jsfs, int32_t k,
                        int32_t* d_best, double* d_best_llk) {
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    if (k < 1 || k > MISTI_SCAN_MAX_BEST) return fail(MISTI_E_ARG, "k must be 1 ... %d (got %d)", MISTI_SCAN_MAX_BEST, (int)k);
    if (n_cand < 0 || n_rep < 0) return fail(MISTI_E_ARG, "negative batch size");
    if (n_rep == 0) return 0;
    if (!d_best || (n_cand > 0 && (!d_jafs || !d_jsfs))) return fail(MISTI_E_ARG, "jafs / jsfs / best is NULL");
    if (n_cand > INT32_MAX) return fail(MISTI_E_LIMIT, "n_cand too large");
    HIP_TRY(hipSetDevice(c->device));
    const int64_t slices = misti::scan_best_slices(n_cand, n_rep, c->tune);
    const size_t part = (size_t)slices * (size_t)misti::scan_best_width(k) * (size_t)n_rep;
    if (n_cand > 0) {
        HIP_TRY(c->consts.reserve((size_t)n_rep * sizeof(double)));
        HIP_TRY(c->scan_v.reserve(part * sizeof(double)));
        HIP_TRY(c->scan_i.reserve(part * sizeof(int32_t)));
        HIP_TRY(misti::launch_llh_const(n_rep, d_jsfs, c->consts.as<double>(), c->unfolded, c->stream));
    }
    HIP_TRY(misti::launch_scan_best(n_cand, d_jafs, d_status, n_rep, d_jsfs, c->consts.as<double>(), k, d_best, d_best_llk, slices,
                                    c->scan_v.as<double>(), c->scan_i.as<int32_t>(), c->unfolded, c->stream));
    return 0;
}

int misti_scan_profile_dev(misti_ctx* c, int64_t n_cand, const double* d_jafs, const int32_t* d_status, const int32_t* d_group, int32_t n_group,
                           int64_t n_rep, const double* d_jsfs, double* d_prof_llk, int32_t* d_prof_best) {
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    if (n_group < 1) return fail(MISTI_E_ARG, "n_group must be at least 1 (got %d)", (int)n_group);
    if (n_cand < 0 || n_rep < 0) return fail(MISTI_E_ARG, "negative batch size");
    if (n_group > MISTI_SCAN_MAX_GROUPS) return fail(MISTI_E_LIMIT, "n_group beyond MISTI_SCAN_MAX_GROUPS = %d (got %d)", MISTI_SCAN_MAX_GROUPS, (int)n_group);
    if (n_cand > INT32_MAX) return fail(MISTI_E_LIMIT, "n_cand too large");
    if (n_rep == 0) return 0;
    if (!d_prof_llk || (n_cand > 0 && (!d_jafs || !d_jsfs || !d_group))) return fail(MISTI_E_ARG, "jafs / jsfs / group / prof_llk is NULL");
    HIP_TRY(hipSetDevice(c->device));
    const int64_t slices = misti::scan_profile_slices(n_cand, n_group, n_rep, c->tune);
    if (n_cand > 0) {
        const size_t part = (size_t)slices * (size_t)n_group * (size_t)n_rep;
        HIP_TRY(c->consts.reserve((size_t)n_rep * sizeof(double)));
        HIP_TRY(c->prof_v.reserve(part * sizeof(double)));
        HIP_TRY(c->prof_i.reserve(part * sizeof(int32_t)));
        HIP_TRY(c->prof_idx.reserve(misti::scan_profile_index_size(n_cand, n_group) * sizeof(int32_t)));
        HIP_TRY(misti::launch_llh_const(n_rep, d_jsfs, c->consts.as<double>(), c->unfolded, c->stream));
    }
    // (the buffers are passed as they are: without candidates they may be NULL, and no address is derived from them here)
    HIP_TRY(misti::launch_scan_profile(n_cand, d_jafs, d_status, d_group, n_group, n_rep, d_jsfs, c->consts.as<double>(), d_prof_llk, d_prof_best, slices,
                                       c->prof_idx.as<int32_t>(), c->prof_v.as<double>(), c->prof_i.as<int32_t>(), c->unfolded, c->stream));
    return 0;
}

}  // extern "C"

namespace {
int eval_batch_host(misti_ctx* c, int64_t n_cand, const double* split, const double* params, const int32_t* band_bounds, int64_t n_rep, const double* jsfs,
                    double* llk, double* jafs, double* lc, double* pr, int32_t* status, const int64_t* idx = nullptr,
                    const int32_t* pulse_times = nullptr);
}

int misti_host::eval_batch_drained(misti_ctx* c, int r) {
    // An error between the first asynchronous copy and the final wait leaves DMAs reading the context's pinned input block or
    // writing its pinned output block: the next call would overwrite what they read.  Drain the stream before reporting.
    if (r != 0 && c) {
        const std::string why = g_err;
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        if (c->side_stream) (void)hipStreamSynchronize(c->side_stream);
        (void)hipGetLastError();
        g_err = why;
    }
    return r;
}

extern "C" {

int misti_eval_batch(misti_ctx* c, int64_t n_cand, const double* split, const double* params, const int32_t* band_bounds, int64_t n_rep, const double* jsfs,
                     double* llk, double* jafs, double* lc, double* pr, int32_t* status) {
    return eval_batch_drained(c, eval_batch_host(c, n_cand, split, params, band_bounds, n_rep, jsfs, llk, jafs, lc, pr, status));
}

// misti_eval_batch with a time per candidate for every pulse of the model; NULL (or a model without pulses) is misti_eval_batch.
int misti_eval_batch_pulses(misti_ctx* c, int64_t n_cand, const double* split, const double* params, const int32_t* band_bounds,
                            const int32_t* pulse_times, int64_t n_rep, const double* jsfs, double* llk, double* jafs, double* lc, double* pr,
                            int32_t* status) {
    return eval_batch_drained(c, eval_batch_host(c, n_cand, split, params, band_bounds, n_rep, jsfs, llk, jafs, lc, pr, status, nullptr, pulse_times));
}

// misti_eval_batch on the rows idx[0 .. n) of the caller's arrays: inputs are GATHERED from those rows into the context's staging
// block and every output row i is SCATTERED to row idx[i] - what a context of misti_multi_eval_batch does with its shard of a
// batch (misti_multi.cpp), without a staging copy of the shard in between.  jsfs is shared (not indexed).  Not part of the public ABI.
int misti_eval_batch_indexed_(misti_ctx* c, int64_t n, const int64_t* idx, const double* split, const double* params, const int32_t* band_bounds,
                              int64_t n_rep, const double* jsfs, double* llk, double* jafs, double* lc, double* pr, int32_t* status) {
    if (!idx) return fail(MISTI_E_ARG, "idx is NULL");
    try {
        return eval_batch_drained(c, eval_batch_host(c, n, split, params, band_bounds, n_rep, jsfs, llk, jafs, lc, pr, status, idx));
    } catch (const std::bad_alloc&) {
        return eval_batch_drained(c, fail(MISTI_E_NOMEM, "out of host memory staging %lld candidates", (long long)n));
    } catch (const std::exception& e) {
        return eval_batch_drained(c, fail(MISTI_E_ARG, "%s", e.what()));
    }
}

}  // extern "C"

namespace {

int eval_batch_host(misti_ctx* c, int64_t n_cand, const double* split, const double* params, const int32_t* band_bounds, int64_t n_rep, const double* jsfs,
                    double* llk, double* jafs, double* lc, double* pr, int32_t* status, const int64_t* idx, const int32_t* pulse_times) {
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    if (n_cand < 0 || n_rep < 0) return fail(MISTI_E_ARG, "negative batch size");
    if (n_cand == 0) return 0;
    if (!split) return fail(MISTI_E_ARG, "split_time is NULL");
    const int P = c->dm.n_param, numT = c->dm.numT;
    if (P > 0 && !params) return fail(MISTI_E_ARG, "params is NULL but the model has %d parameters", P);
    if (n_rep > 0 && (!jsfs || !llk)) return fail(MISTI_E_ARG, "jsfs / llk is NULL with n_rep > 0");
    HIP_TRY(hipSetDevice(c->device));
    const size_t nc = (size_t)n_cand, nr = (size_t)n_rep;
    const bool with_bounds = band_bounds && c->dm.n_band > 0;
    const bool with_pulses = pulse_times && c->dm.n_pulse > 0;
    const size_t b_pulses = with_pulses ? nc * (size_t)c->dm.n_pulse * sizeof(int32_t) : 0;
    const size_t b_split = nc * sizeof(double), b_par = P > 0 ? nc * P * sizeof(double) : 0;
    const size_t b_bounds = with_bounds ? nc * 2 * (size_t)c->dm.n_band * sizeof(int32_t) : 0, b_jsfs = nr * 8 * sizeof(double);
    const size_t lc_n = nc * (size_t)(numT + 1) * 2, pr_n = nc * (size_t)(numT + 2) * 6;
    const size_t b_llk = nr ? nc * nr * sizeof(double) : 0, b_jafs = jafs ? nc * 7 * sizeof(double) : 0, b_lc = lc ? lc_n * sizeof(double) : 0;
    const size_t b_pr = pr ? pr_n * sizeof(double) : 0, b_status = status ? nc * sizeof(int32_t) : 0;
    const size_t in_bytes = b_split + b_par + b_bounds + b_pulses + b_jsfs, out_bytes = b_llk + b_jafs + b_lc + b_pr + b_status;
    // The caller's buffers are pageable: inputs are packed into ONE pinned block (a CPU memcpy of tens of KB), copied by truly
    // asynchronous DMAs; outputs come back into one pinned block and are handed over after the single wait at the end.
    const bool pinned = in_bytes <= PIN_STAGE_MAX && out_bytes <= PIN_STAGE_MAX &&
                        c->pin_in.reserve(in_bytes) == hipSuccess && c->pin_out.reserve(out_bytes ? out_bytes : 8) == hipSuccess;
    if (!pinned) (void)hipGetLastError();
    // Indexed form (idx: rows of the caller's arrays, misti_eval_batch_indexed_): rows are gathered on the way in and scattered on the
    // way out; beyond the pinned block's limit the gather goes through pageable heap blocks (std::bad_alloc is the caller's to catch).
    // They belong to the context: an error return leaves copies in flight until misti_eval_batch's drain, which comes AFTER this
    // function's locals are gone.
    std::vector<char>& heap_in = c->heap_in;
    std::vector<char>& heap_out = c->heap_out;
    if (idx && !pinned) { heap_in.resize(in_bytes); heap_out.resize(out_bytes ? out_bytes : 8); }
    char* hin = pinned ? static_cast<char*>(c->pin_in.p) : (idx ? heap_in.data() : nullptr);
    const bool staged = pinned || idx;
    // row = bytes per candidate of this array (0: not per candidate - the replicate table)
    auto h2d = [&](DevBuf& dst, const void* src, size_t bytes, size_t row, size_t& off) -> int {
        if (!bytes) return 0;
        HIP_TRY(dst.reserve(bytes));
        const void* from = src;
        if (staged) {
            if (idx && row) for (size_t i = 0; i < nc; ++i) std::memcpy(hin + off + i * row, static_cast<const char*>(src) + (size_t)idx[i] * row, row);
            else std::memcpy(hin + off, src, bytes);
            from = hin + off; off += bytes;
        }
        HIP_TRY(hipMemcpyAsync(dst.p, from, bytes, hipMemcpyHostToDevice, c->stream));
        return 0;
    };
    size_t off = 0;
    if (int r = h2d(c->st_split, split, b_split, sizeof(double), off)) return r;
    if (int r = h2d(c->st_params, params, b_par, (size_t)P * sizeof(double), off)) return r;
    if (int r = h2d(c->st_bounds, band_bounds, b_bounds, 2 * (size_t)c->dm.n_band * sizeof(int32_t), off)) return r;
    if (int r = h2d(c->st_jsfs, jsfs, b_jsfs, 0, off)) return r;
    // last: its size need not be a multiple of 8, and nothing behind it is read as doubles
    if (int r = h2d(c->st_pulses, pulse_times, b_pulses, (size_t)c->dm.n_pulse * sizeof(int32_t), off)) return r;
    if (nr) HIP_TRY(c->st_llk.reserve(nc * nr * sizeof(double)));
    HIP_TRY(c->st_jafs.reserve(nc * 7 * sizeof(double)));
    HIP_TRY(c->st_status.reserve(nc * sizeof(int32_t)));
    if (lc) HIP_TRY(c->st_lc.reserve(lc_n * sizeof(double)));
    if (pr) {
        HIP_TRY(c->st_pr.reserve(pr_n * sizeof(double)));
        HIP_TRY(hipMemsetAsync(c->st_pr.p, 0, pr_n * sizeof(double), c->stream));
    }
    // the split times are in host memory here: whether any has a fractional part is a glance (the device-buffer form needs misti_set_hints)
    bool whole = true;
    for (size_t i = 0; i < nc && whole; ++i) { const double st = split[idx ? (size_t)idx[i] : i]; whole = st == std::floor(st); }
    int r = run_dev(c, n_cand, c->st_split.as<double>(), P > 0 ? c->st_params.as<double>() : nullptr,
                    with_bounds ? c->st_bounds.as<int32_t>() : nullptr, n_rep,
                    nr ? c->st_jsfs.as<double>() : nullptr, nr ? c->st_llk.as<double>() : nullptr, c->st_jafs.as<double>(),
                    lc ? c->st_lc.as<double>() : nullptr, pr ? c->st_pr.as<double>() : nullptr, c->st_status.as<int32_t>(), whole ? RUN_INTEGER_SPLITS : 0u,
                    with_pulses ? c->st_pulses.as<int32_t>() : nullptr);
    if (r) return r;
    char* hout = pinned ? static_cast<char*>(c->pin_out.p) : (idx ? heap_out.data() : nullptr);
    struct Back { void* user; size_t off, bytes, row; };
    Back back[5];
    int n_back = 0;
    size_t ooff = 0;
    auto d2h = [&](void* user, const void* src, size_t bytes, size_t row) -> int {
        if (!bytes) return 0;
        void* to = user;
        if (staged) { to = hout + ooff; back[n_back++] = {user, ooff, bytes, row}; ooff += bytes; }
        HIP_TRY(hipMemcpyAsync(to, src, bytes, hipMemcpyDeviceToHost, c->stream));
        return 0;
    };
    if (int q = d2h(llk, c->st_llk.p, b_llk, nr * sizeof(double))) return q;
    if (int q = d2h(jafs, c->st_jafs.p, b_jafs, 7 * sizeof(double))) return q;
    if (int q = d2h(lc, c->st_lc.p, b_lc, (size_t)(numT + 1) * 2 * sizeof(double))) return q;
    if (int q = d2h(pr, c->st_pr.p, b_pr, (size_t)(numT + 2) * 6 * sizeof(double))) return q;
    if (int q = d2h(status, c->st_status.p, b_status, sizeof(int32_t))) return q;
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n_back; ++i) {
        if (idx) for (size_t k = 0; k < nc; ++k) std::memcpy(static_cast<char*>(back[i].user) + (size_t)idx[k] * back[i].row, hout + back[i].off + k * back[i].row, back[i].row);
        else std::memcpy(back[i].user, hout + back[i].off, back[i].bytes);
    }
    return 0;
}

}  // namespace

extern "C" {

int misti_forward_rates_dev(misti_ctx* c, int64_t n_cand, const double* d_split, const double* d_params, int hold_mu,
                            double* d_lh, double* d_pr, int32_t* d_status) {
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    if (n_cand < 0) return fail(MISTI_E_ARG, "negative batch size");
    if (n_cand == 0) return 0;
    if (!d_split || !d_lh) return fail(MISTI_E_ARG, "split_time / lh is NULL");
    if (c->dm.n_param > 0 && !d_params) return fail(MISTI_E_ARG, "params is NULL but the model has %d parameters", c->dm.n_param);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(misti::launch_forward(c->dm, n_cand, d_split, d_params, hold_mu != 0, d_lh, d_pr, d_status, c->stream));
    return 0;
}

int misti_forward_rates(misti_ctx* c, int64_t n_cand, const double* split, const double* params, int hold_mu,
                        double* lh, double* pr, int32_t* status) {
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    if (n_cand < 0) return fail(MISTI_E_ARG, "negative batch size");
    if (n_cand == 0) return 0;
    if (!split || !lh) return fail(MISTI_E_ARG, "split_time / lh is NULL");
    const int P = c->dm.n_param, numT = c->dm.numT;
    if (P > 0 && !params) return fail(MISTI_E_ARG, "params is NULL but the model has %d parameters", P);
    HIP_TRY(hipSetDevice(c->device));
    const size_t nc = (size_t)n_cand;
    const size_t lh_n = nc * (size_t)(numT + 1) * 2, pr_n = nc * (size_t)(numT + 2) * 6;
    HIP_TRY(c->st_split.reserve(nc * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(c->st_split.p, split, nc * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (P > 0) {
        HIP_TRY(c->st_params.reserve(nc * P * sizeof(double)));
        HIP_TRY(hipMemcpyAsync(c->st_params.p, params, nc * P * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c->st_lc.reserve(lh_n * sizeof(double)));
    HIP_TRY(c->st_status.reserve(nc * sizeof(int32_t)));
    if (pr) HIP_TRY(c->st_pr.reserve(pr_n * sizeof(double)));
    int r = misti_forward_rates_dev(c, n_cand, c->st_split.as<double>(), P > 0 ? c->st_params.as<double>() : nullptr, hold_mu,
                                    c->st_lc.as<double>(), pr ? c->st_pr.as<double>() : nullptr, c->st_status.as<int32_t>());
    if (r) return r;
    HIP_TRY(hipMemcpyAsync(lh, c->st_lc.p, lh_n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (pr) HIP_TRY(hipMemcpyAsync(pr, c->st_pr.p, pr_n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (status) HIP_TRY(hipMemcpyAsync(status, c->st_status.p, nc * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int misti_pair_residuals(misti_ctx* c, int cpfit, int64_t n, const double* problems, double* out) {
    // everything that can be said about the arguments is said before the context is looked at
    if (cpfit != 0 && cpfit != 1) return fail(MISTI_E_ARG, "cpfit must be 0 or 1 (got %d)", cpfit);
    if (n < 0) return fail(MISTI_E_ARG, "negative number of problems");
    if (n > MISTI_PAIR_MAX_PROBLEMS) return fail(MISTI_E_LIMIT, "n beyond MISTI_PAIR_MAX_PROBLEMS = %d (got %lld)", (int)MISTI_PAIR_MAX_PROBLEMS, (long long)n);
    if (n > 0 && (!problems || !out)) return fail(MISTI_E_ARG, "problems / out is NULL");
    for (int64_t i = 0; i < n; ++i) {
        const double* p = problems + i * 10;
        for (int k = 0; k < 6; ++k)
            if (!std::isfinite(p[k])) return fail(MISTI_E_ARG, "problems[%lld][%d] is not finite (only the point may be)", (long long)i, k);
        if (p[0] < 0.0 || p[1] < 0.0) return fail(MISTI_E_ARG, "problems[%lld]: a migration rate must not be negative", (long long)i);
        const double role = p[8], red = p[9];
        if (!(role == 0.0 || role == 1.0 || role == 2.0 || role == 3.0 || role == 4.0 || role == 5.0))
            return fail(MISTI_E_ARG, "problems[%lld]: role %g is not one of 0..5", (long long)i, role);
        if (!(red == 0.0 || red == 1.0 || red == 2.0)) return fail(MISTI_E_ARG, "problems[%lld]: red %g is not one of 0..2", (long long)i, red);
        if (red != 0.0) {
            if (!cpfit) return fail(MISTI_E_ARG, "problems[%lld]: red = %g without cpfit (the default fit has no reduced form)", (long long)i, red);
            const int k = red == 1.0 ? 0 : 1;            // the state that is empty and unfed: mu of the OTHER population is zero
            if (p[1 - k] != 0.0 || p[2 + k] != 0.0)
                return fail(MISTI_E_ARG, "problems[%lld]: red = %g needs mu%d == 0 and P[%d] == 0 exactly", (long long)i, red, 1 - k, k);
        }
    }
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    const size_t nn = (size_t)n;
    HIP_TRY(c->st_params.reserve(nn * 10 * sizeof(double)));
    HIP_TRY(c->st_lc.reserve(nn * 4 * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(c->st_params.p, problems, nn * 10 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(misti::launch_pair_residuals(cpfit != 0, n, c->st_params.as<double>(), c->st_lc.as<double>(), c->stream));
    HIP_TRY(hipMemcpyAsync(out, c->st_lc.p, nn * 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int misti_lsq_probe(misti_ctx* c, int kind, int64_t n, const double* problems, double* out) {
    // everything that can be said about the arguments is said before the context is looked at
    if (kind < 0 || kind >= MISTI_LSQ_KINDS) return fail(MISTI_E_ARG, "kind must be one of 0..%d (got %d)", (int)MISTI_LSQ_KINDS - 1, kind);
    if (n < 0) return fail(MISTI_E_ARG, "negative number of problems");
    if (n > MISTI_LSQ_MAX_PROBLEMS) return fail(MISTI_E_LIMIT, "n beyond MISTI_LSQ_MAX_PROBLEMS = %d (got %lld)", (int)MISTI_LSQ_MAX_PROBLEMS, (long long)n);
    if (n > 0 && (!problems || !out)) return fail(MISTI_E_ARG, "problems / out is NULL");
    const int n_at = kind == MISTI_LSQ_SVD4 || kind == MISTI_LSQ_STEPN ? 12 : kind == MISTI_LSQ_SELECT ? 19 : -1;
    for (int64_t i = 0; i < n; ++i) {
        const double* p = problems + i * MISTI_LSQ_IN;
        if (n_at >= 0 && !(p[n_at] == 1.0 || p[n_at] == 2.0))
            return fail(MISTI_E_ARG, "problems[%lld]: N %g is not 1 or 2", (long long)i, p[n_at]);
        if (kind == MISTI_LSQ_UPDATE && !(p[0] == 0.0 || p[0] == 1.0))
            return fail(MISTI_E_ARG, "problems[%lld]: finite %g is not 0 or 1", (long long)i, p[0]);
    }
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    const size_t nn = (size_t)n;
    HIP_TRY(c->st_params.reserve(nn * MISTI_LSQ_IN * sizeof(double)));
    HIP_TRY(c->st_lc.reserve(nn * MISTI_LSQ_OUT * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(c->st_params.p, problems, nn * MISTI_LSQ_IN * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(misti::launch_lsq_probe(kind, n, c->st_params.as<double>(), c->st_lc.as<double>(), c->stream));
    HIP_TRY(hipMemcpyAsync(out, c->st_lc.p, nn * MISTI_LSQ_OUT * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int misti_last_diag(misti_ctx* c, int64_t n_cand, double* max_rate_x_len) {
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    if (!max_rate_x_len) return fail(MISTI_E_ARG, "output is NULL");
    if (n_cand != c->diag_n) return fail(MISTI_E_ARG, "the last batch had %lld candidates, not %lld", (long long)c->diag_n, (long long)n_cand);
    if (n_cand == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(max_rate_x_len, c->ws_diag.p, (size_t)n_cand * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int misti_enable_solver_trace(misti_ctx* c, int on) {
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    c->trace = on != 0;
    if (!c->trace) { c->trace_n = 0; c->trace_iter_cap = 0; }
    return 0;
}

int misti_last_solver_trace(misti_ctx* c, int64_t n_cand, int32_t* trace, int64_t cand, double* iterates) {
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    if (!c->trace || c->trace_n == 0) return fail(MISTI_E_ARG, "no solver trace: enable it before the batch (misti_enable_solver_trace)");
    if (n_cand != c->trace_n) return fail(MISTI_E_ARG, "the traced batch had %lld candidates, not %lld", (long long)c->trace_n, (long long)n_cand);
    HIP_TRY(hipSetDevice(c->device));
    const size_t nc = (size_t)n_cand, numT = (size_t)c->dm.numT;
    if (trace) {
        const int32_t* src = c->ws_solver.as<int32_t>() + nc * numT + nc;
        HIP_TRY(hipMemcpyAsync(trace, src, nc * (numT + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    }
    if (iterates) {
        if (c->trace_iter_cap == 0) return fail(MISTI_E_LIMIT, "iterates are recorded for batches of at most %d candidates", MISTI_TRACE_MAX_CAND);
        if (cand < 0 || cand >= n_cand) return fail(MISTI_E_ARG, "candidate %lld out of range", (long long)cand);
        int32_t ch = -1;
        HIP_TRY(hipMemcpyAsync(&ch, c->trace_of + cand, sizeof ch, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (ch < 0 || ch >= c->trace_iter_cap) return fail(MISTI_E_ARG, "candidate %lld has no chain", (long long)cand);
        const size_t per = numT * MISTI_TRACE_MAX_ITER * 2;
        HIP_TRY(hipMemcpyAsync(iterates, c->ws_iters.as<double>() + (size_t)ch * per, per * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int misti_enable_timing(misti_ctx* c, int on) {
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    c->timing = on != 0;
    return 0;
}

int misti_kernel_times(misti_ctx* c, double ms[3], int64_t launches[3], int reset) {
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    for (int w = 0; w < 3; ++w) {
        if (int r = drain_pending(c, w, true)) return r;
        if (ms) ms[w] = c->ms[w];
        if (launches) launches[w] = c->launches[w];
        if (reset) { c->ms[w] = 0; c->launches[w] = 0; }
    }
    return 0;
}

}  // extern "C"
