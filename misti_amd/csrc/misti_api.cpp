// C-ABI host layer of libmisti_hip.so (see include/misti_hip.h).
//
// Replaces, for a batch, what the reference does once per Python object:
//   MigrationInference.__init__ / SetModel   MigrationInference.py:41-289   -> misti_create
//   JAFSLikelihood                           MigrationInference.py:566-614  -> misti_eval_batch*
// No CPU fallback: every compute entry point needs a HIP device.
#include <cassert>
#include <hip/hip_runtime.h>

#include <cmath>
#include <chrono>
#include <complex>
#include <thread>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "misti_device.h"
#include "misti_post.h"
#include "misti_prior.h"
#include "misti_tables.hpp"

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) return fail(MISTI_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

const misti::HostTables& host_tables() {
    static const misti::HostTables t = misti::build_tables();
    return t;
}

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() { return static_cast<T*>(p); }
};

// Host-pinned staging of the host-buffer entry points: a copy from / to pageable memory makes the runtime stage the bytes itself
// and wait; from pinned memory hipMemcpyAsync is a DMA the stream orders like a kernel.
struct PinBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipHostFree(p); if (e != hipSuccess) return e; p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 4 + 4096;
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};
constexpr size_t PIN_STAGE_MAX = (size_t)256 << 20;    // beyond this the host-buffer calls copy straight from / to the caller's memory

}  // namespace

struct misti_ctx {
    int device = 0;
    misti::DevModel dm{};
    int unfolded = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    DevBuf model_f64, model_i32;        // times | lh ; run_start | run_end
    DevBuf consts;                      // llh_const per replicate
    DevBuf scan_v, scan_i;              // misti_scan_best_dev: the slices' lists [slices][width][n_rep], values and indices
    DevBuf prof_v, prof_i, prof_idx;    // misti_scan_profile_dev: the slices' pairs [slices][n_group][n_rep]; first [n_group + 1] | cursor [n_group] | members [n_cand]
    DevBuf ws_jafs, ws_status;          // spectra / status when the caller passes NULL
    DevBuf ws_order;                    // dispatch order (heaviest candidates first)
    DevBuf ws_diag;                     // per candidate: largest corrected rate x interval length of the last batch
    int64_t diag_n = 0;
    int32_t* hint_host = nullptr;       // pinned, device-visible: {chains, candidates} of the last batch (a launch-shape hint only)
    int32_t* hint_dev = nullptr;
    int32_t batch_seq = 0;
    misti::Tuning tune;                 // diagnostic launch-shape overrides, read from the environment once (misti_create)
    int table_cur = 0;                  // which of the two chain-table sets the next batch uses
    size_t table_clean[2] = {0, 0};     // table size each set is known to be clean for (0: not clean)
    DevBuf ws_trunk;                    // per chain: 44-state records before every interval (trunk kernel -> kernel 2)
    DevBuf ws_chain_f64, ws_chain_i32;  // chain buffers (kernel 1 -> kernel 2) and the chain table
    DevBuf st_split, st_params, st_bounds, st_pulses, st_jsfs, st_llk, st_jafs, st_lc, st_pr, st_status;   // staging for the host-buffer form
    PinBuf pin_in, pin_out;             // pinned staging of misti_eval_batch: inputs packed, outputs packed
    std::vector<char> heap_in, heap_out;   // pageable staging of the indexed form beyond PIN_STAGE_MAX (kept here: they outlive an error return's drain)
    bool trace = false;                 // solver trace (misti_enable_solver_trace)
    DevBuf ws_solver, ws_iters;         // per chain / per candidate solver words; trial points of small batches
    DevBuf ws_post;                     // default fit: rates after the split per candidate and interval (+ their solver words)
    int64_t trace_n = 0, trace_iter_cap = 0;   // candidates / chains covered by the trace of the last batch
    const int32_t* trace_of = nullptr;  // candidate -> chain of the last batch (device)
    hipEvent_t order_ev = nullptr;      // orders a replaced stream before its successor (misti_set_stream)
    hipEvent_t last_ev = nullptr;       // recorded behind every batch: lets OTHER contexts see whether this one has work in flight
    bool last_ev_set = false;
    int64_t batches_begun = 0, batches_recorded = 0;   // batches that reached their first stream operation / that recorded last_ev behind them (misti_batch_event_)
    unsigned hints = 0;                 // misti_set_hints: what the caller knows about its batches (MISTI_HINT_INTEGER_SPLITS)
    hipStream_t side_stream = nullptr;  // phase 1 of a two-phase batch (run_dev): what follows the chains a packed launch completed, beside its resume launch
    hipEvent_t packed_ev = nullptr, side_ev = nullptr;
    DevBuf nm_f64, nm_i32;              // batched Nelder-Mead: simplices, points, counters (misti_nm_solve)
    DevBuf curv_f64, curv_i32;          // misti_curvature: points, stencil candidates, their spectra, derivatives | rows, slots, statuses
    DevBuf boot_chunks;                 // misti_bootstrap_rows_dev: the chunk table [n_chunk][8]
    DevBuf param_totals;                // misti_parametric_rows_dev: the draw counts of one slice of replicates, [n][6] uint64
    DevBuf post_ws;                     // misti_ens_summary_dev: means [S][N] | the centred ensemble-mean series [S][N][n]
    int32_t* nm_live_host = nullptr;    // pinned: live starts after the last two finished iterations
    int64_t nm_iterations = 0;          // iterations issued by the last misti_nm_solve
    int64_t nm_slots = 0;               // and the batch slots they had in total (live starts + the stale-count slack)
    int64_t nm_spec_iterations = 0;     // how many of those iterations were speculative (all points of a start in one batch)
    bool timing = false;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    double ms[3] = {0, 0, 0};
    int64_t launches[3] = {0, 0, 0};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending[3];
};

namespace {

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

// hints (what an internal caller knows about its own batch; 0 from the ABI's entry points, whose split times live on the device):
//   RUN_INTEGER_SPLITS  no split time has a fractional part (or is negative: an empty slot) - no tail for the post launch
//   RUN_UNSHARED        every candidate has its own parameter vector: no trunk for a batch too large for one chain per wave
//   RUN_ONE_LENGTH      every chain has the same number of intervals: the chains need no sorting by length
enum : unsigned { RUN_INTEGER_SPLITS = 1u, RUN_UNSHARED = 2u, RUN_ONE_LENGTH = 4u };
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
    // Two phases behind a packed launch that lets chains yield (--cpfit; misti_kernels.hip: wrong_phase): what waits for the chains that launch
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

// A two-phase batch joins its side stream to the batch's stream with its LAST wait; a failure anywhere between the phase-1 launch and
// that wait would return with phase-1 kernels in flight on a stream nothing else waits for (misti_sync and the host-buffer drain
// know the batch's stream) while the next batch's set-up rewrites the chain buffers they read.  So: on any failure the side stream is
// drained before the error is reported.
int run_dev(misti_ctx* c, int64_t n_cand, const double* d_split, const double* d_params, const int32_t* d_bounds, int64_t n_rep, const double* d_jsfs,
            double* d_llk, double* d_jafs, double* d_lc, double* d_pr, int32_t* d_status, unsigned hints = 0, const int32_t* d_pulses = nullptr) {
    const int r = run_dev_impl(c, n_cand, d_split, d_params, d_bounds, n_rep, d_jsfs, d_llk, d_jafs, d_lc, d_pr, d_status, hints, d_pulses);
    if (r != 0 && c->side_stream) {
        const std::string why = g_err;
        (void)hipStreamSynchronize(c->side_stream);
        (void)hipGetLastError();
        g_err = why;
    }
    return r;
}

}  // namespace

extern "C" {

int misti_abi_version(void) { return MISTI_ABI_VERSION; }
#ifndef MISTI_BUILD_ID
#define MISTI_BUILD_ID "unknown"
#endif
const char* misti_build_id(void) { return MISTI_BUILD_ID; }

const char* misti_last_error(void) { return g_err.c_str(); }

// internal (misti_multi.cpp): make `msg` the calling thread's last error; returns `code`
int misti_set_error_(int code, const char* msg) { return fail(code, "%s", msg ? msg : ""); }

// internal (misti_boot.hip): make the context's device current; its stream, and its buffer for the chunk table grown to `bytes`.  A
// table that grows frees the old buffer, which waits for the device: no kernel of an earlier call still reads it.
int misti_boot_ctx_(misti_ctx* c, size_t bytes, void** stream, void** d_chunks) {
    if (!c || !stream || !d_chunks) return fail(MISTI_E_ARG, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->boot_chunks.reserve(bytes));
    *stream = static_cast<void*>(c->stream);
    *d_chunks = c->boot_chunks.p;
    return 0;
}

// internal (misti_parametric.hip): make the context's device current; its stream, and its buffer for the draw counts grown to `bytes`.
// A buffer that grows frees the old one, which waits for the device: no kernel of an earlier call still adds to it.
int misti_param_ctx_(misti_ctx* c, size_t bytes, void** stream, void** d_totals) {
    if (!c || !stream || !d_totals) return fail(MISTI_E_ARG, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->param_totals.reserve(bytes));
    *stream = static_cast<void*>(c->stream);
    *d_totals = c->param_totals.p;
    return 0;
}

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
            // Where can a candidate leave its chain's trunk?  (trunk_leave in misti_kernels.hip, for every split an integer or a
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
                    &c->st_split, &c->st_params, &c->st_bounds, &c->st_pulses, &c->st_jsfs, &c->st_llk, &c->st_jafs, &c->st_lc, &c->st_pr, &c->st_status, &c->nm_f64, &c->nm_i32, &c->scan_v, &c->scan_i, &c->prof_v, &c->prof_i, &c->prof_idx, &c->curv_f64, &c->curv_i32, &c->boot_chunks, &c->param_totals, &c->post_ws})
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
int eval_batch_drained(misti_ctx* c, int r) {
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

}  // extern "C"

namespace {

using misti::NmBatch;
using misti::NM_BATCHES;

// Bump allocation over one buffer.  A workspace's layout is ONE sequence of take() calls, run twice: over a null base to learn the
// size, then over the buffer to assign the pointers - size and layout cannot disagree.
template <class T>
struct Carver {
    T* base = nullptr;
    size_t n = 0;
    T* take(size_t k) { T* p = base ? base + n : nullptr; n += k; return p; }
};

// A workspace in the context's search buffers (one allocation per type: doubles | int32): `layout` run twice, as Carver says, and
// the pinned words the live count of a paced search comes back in (Pacer).  `noun`: what the caller's count counts.
template <class Layout>
int carve(misti_ctx* c, const char* noun, Layout&& layout) {
    Carver<double> f;
    Carver<int32_t> q;
    layout(f, q);
    HIP_TRY(c->nm_f64.reserve(f.n * sizeof(double)));
    HIP_TRY(c->nm_i32.reserve(q.n * sizeof(int32_t)));
    if (!c->nm_live_host) {
        if (hipHostMalloc((void**)&c->nm_live_host, 4 * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            c->nm_live_host = nullptr;
            return fail(MISTI_E_HIP, "pinned allocation for the live-%s count failed", noun);
        }
    }
    f = Carver<double>{c->nm_f64.as<double>()};
    q = Carver<int32_t>{c->nm_i32.as<int32_t>()};
    layout(f, q);
    return 0;
}

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
RowsArgs rows_args(const misti_search_t& q) {
    return {q.split, q.split_time, q.split_times, q.n_start, q.rows, q.n_rep, q.jsfs, q.band_bounds, q.pulse_times, q.n_box, q.box_lo, q.box_hi, nullptr};
}
RowsArgs rows_args(const misti_de_t& q) {
    return {q.split, 0.0, q.split_times, q.n_start, q.rows, q.n_rep, q.jsfs, q.band_bounds, q.pulse_times, q.n_box, q.box_lo, q.box_hi, q.ids};
}
RowsArgs rows_args(const misti_ens_t& q) {
    return {q.split, 0.0, q.split_times, q.n_start, q.rows, q.n_rep, q.jsfs, q.band_bounds, q.pulse_times, q.n_box, q.box_lo, q.box_hi, q.ids};
}
RowsArgs rows_args(const misti_pt_t& q) {
    return {q.split, 0.0, q.split_times, q.n_start, q.rows, q.n_rep, q.jsfs, q.band_bounds, q.pulse_times, q.n_box, q.box_lo, q.box_hi, q.ids};
}

// The checks the three doors share.  Each door calls them where its header's order of refusals puts them (nm_check, de_check,
// sampler_check); `noun` is what the door calls its n_start.
int check_n_box(const RowsArgs& a, const char* noun) {
    if (a.n_box != 1 && a.n_box != a.n_start)
        return fail(MISTI_E_ARG, "n_box must be 1 or n_start (got %lld for %lld %s)", (long long)a.n_box, (long long)a.n_start, noun);
    return 0;
}
// every row inside the table, every split time of MISTI_SPLIT_PER_START finite; `whole`: every such split time is an integer (a
// fitted split is whole by accident only: never the integer-splits hint)
int check_rows(const RowsArgs& a, bool& whole) {
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
int check_limits(const misti_ctx* c, const RowsArgs& a, int64_t per, const char* noun, int& N) {
    if (!c) return fail(MISTI_E_ARG, "ctx is NULL");
    N = c->dm.n_param + (a.fit_split() ? 1 : 0);
    if (N < 1) return fail(MISTI_E_ARG, "the model has no optimised parameter");
    // the sort's local arrays hold MISTI_MAX_PARAMS + 1 vertices (misti_nm.hip: sort_simplex)
    if (N > MISTI_MAX_PARAMS) return fail(MISTI_E_LIMIT, "the split as a coordinate needs n_param + 1 <= %d (n_param = %d)", MISTI_MAX_PARAMS, c->dm.n_param);
    if (a.n_start > INT32_MAX / 8 / (N + 1) / per) return fail(MISTI_E_LIMIT, "too many %s for one call", noun);
    if (a.n_rep > INT32_MAX) return fail(MISTI_E_LIMIT, "too many replicate rows for one call");
    return 0;
}
int check_finite(const double* starts, int64_t n_start, int N) {
    for (int64_t s = 0; s < n_start; ++s)
        for (int k = 0; k < N; ++k)
            if (!std::isfinite(starts[s * N + k])) return fail(MISTI_E_ARG, "starts[%lld][%d] is not finite", (long long)s, k);
    return 0;
}
// box b of the call: neither bound NaN, lo <= hi (lo == hi holds a coordinate fixed).  `finite`: why the door needs a finite box -
// then an infinite bound or width is refused as well; NULL: +-inf leaves a side open.
int check_box(const RowsArgs& a, int N, int64_t b, const char* finite) {
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

// A paced search: the host runs at most two iterations ahead of the device.  Before issuing iteration k it waits for the event of
// iteration k - 2 and reads the count of live starts that iteration left in pinned memory (4 bytes; nothing else of the search
// leaves the device).  That count bounds the live starts of iteration k from above - the number only falls - and sizes its
// batches; zero -> stop issuing.
struct Pacer {
    hipStream_t sm;
    volatile int32_t* live;          // the context's pinned words (carve): [it & 1] the count iteration `it` left
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
    if (int r = carve(c, "start", layout)) return r;
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
    if (int r = carve(c, "search", layout)) return r;
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
    return 0;
}

// the launch record of a checked descriptor, without its pointers
void post_fill(misti::PostArgs& a, int64_t S, int64_t K, int32_t W, int32_t N, const misti_ens_post_t& p) {
    a.S = S; a.K = K; a.llh_K = K; a.W = W; a.N = N; a.burn = p.burn; a.n = K - p.burn; a.c = p.c;
    a.L = p.max_lag < a.n - 1 ? p.max_lag : a.n - 1;
    a.sel = misti::post_select(a.n * W, p.n_prob, p.probs);
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
// the plain door keeps both chains or none: where the caller or a summary (`post`) asks for one
SamplerArgs sampler_args(const misti_ens_t& q, const misti_ens_post_t* post) {
    const bool keep = q.chain || q.chain_llh || post;
    return {rows_args(q), q.init, q.walkers, 1, false, q.n_temp, q.temperature, q.n_step, q.thin, q.a, q.seed, 0, 0, keep, keep,
            q.chain, q.chain_llh, q.accepted, nullptr, nullptr, q.last, q.last_llh, nullptr, nullptr, q.n_points,
            "searches", "searches x walkers", post ? "device " : ""};
}
// the tempered door always keeps the values of every rung (the reduction reads them), the cold rung's coordinates where they are wanted
SamplerArgs sampler_args(const misti_pt_t& q, const misti_ens_post_t* post) {
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
// with the rest; the series workspace and the summaries' device side are carved with the chain.
int sampler_run(misti_ctx* c, const SamplerArgs& q, int N, bool whole, const misti_ens_post_t* post, const misti_prior_t* prior) {
    using namespace misti;
    HIP_TRY(hipSetDevice(c->device));
    const size_t F = (size_t)q.rows.n_start, L = (size_t)q.n_rung, S = F * L, W = (size_t)q.walkers, H = W / 2, M = S * W, NT = (size_t)q.n_temp * L;
    const size_t K = (q.keep_x || q.keep_llh) ? (size_t)(q.n_step / q.thin) : 0, P = F * (L - 1);
    PostArgs pa{};
    if (post) post_fill(pa, q.rows.n_start, (int64_t)K, q.walkers, N, *post);
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
    };
    if (int r = carve(c, "search", layout)) return r;
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
int sampler_door(misti_ctx* c, const SamplerArgs& q, const misti_ens_post_t* p, const misti_prior_t* pr, bool need_post) {
    if (need_post && !p) return fail(MISTI_E_ARG, "the summary descriptor is NULL");
    if (p && p->size != sizeof(misti_ens_post_t))
        return fail(MISTI_E_ARG, "the summary descriptor's size is %u, this library's misti_ens_post_t has %u bytes", (unsigned)p->size, (unsigned)sizeof(misti_ens_post_t));
    if (pr && pr->size != sizeof(misti_prior_t))
        return fail(MISTI_E_ARG, "the prior descriptor's size is %u, this library's misti_prior_t has %u bytes", (unsigned)pr->size, (unsigned)sizeof(misti_prior_t));
    if (q.rows.split != MISTI_SPLIT_PER_START && q.rows.split != MISTI_SPLIT_FITTED)
        return fail(MISTI_E_ARG, "the sampler descriptor's split mode %d is neither MISTI_SPLIT_PER_START nor MISTI_SPLIT_FITTED", (int)q.rows.split);
    int N = 0;
    bool whole = false;
    if (int r = sampler_check(c, q, pr, N, whole)) return r;
    if (p) if (int r = post_check(p, q.rows.n_start, q.n_step / q.thin, q.walkers, N, true)) return r;
    if (q.rows.n_start == 0) return 0;
    return sampler_run(c, q, N, whole, p, pr);
}
int ens_door(misti_ctx* c, const misti_ens_t* q, const misti_ens_post_t* p, const misti_prior_t* pr, bool need_post) {
    if (int r = sampler_size(q, q ? q->size : 0, sizeof(misti_ens_t), "misti_ens_t")) return r;
    return sampler_door(c, sampler_args(*q, p), p, pr, need_post);
}

}  // namespace

extern "C" {

int misti_ensemble_sample(misti_ctx* c, const misti_ens_t* q) { return ens_door(c, q, nullptr, nullptr, false); }

int misti_ensemble_posterior(misti_ctx* c, const misti_ens_t* q, const misti_ens_post_t* p) { return ens_door(c, q, p, nullptr, true); }

int misti_ensemble_sample_prior(misti_ctx* c, const misti_ens_t* q, const misti_ens_post_t* p, const misti_prior_t* pr) { return ens_door(c, q, p, pr, false); }

int misti_tempered_sample_prior(misti_ctx* c, const misti_pt_t* q, const misti_ens_post_t* p, const misti_prior_t* pr) {
    if (int r = sampler_size(q, q ? q->size : 0, sizeof(misti_pt_t), "misti_pt_t")) return r;
    return sampler_door(c, sampler_args(*q, p), p, pr, false);
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
    HIP_TRY(c->post_ws.reserve(SN * (size_t)(a.n + 1) * sizeof(double)));
    a.ws_mean = c->post_ws.as<double>(); a.ws_y = a.ws_mean + SN;
    a.chain = d_chain; a.chain_llh = d_chain_llh;
    a.mean = p->mean; a.cov = p->cov; a.quant = p->quant; a.tau = p->tau; a.window = p->window;
    a.best_llh = p->best_llh; a.best_x = p->best_x; a.best_at = p->best_at;
    HIP_TRY(misti::launch_post(a, c->stream));
    return 0;
}

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

}  // extern "C"

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
    Carver<double> f;
    Carver<int32_t> q;
    layout(f, q);
    HIP_TRY(c->curv_f64.reserve(f.n * sizeof(double)));
    HIP_TRY(c->curv_i32.reserve(q.n * sizeof(int32_t)));
    f = Carver<double>{c->curv_f64.as<double>()};
    q = Carver<int32_t>{c->curv_i32.as<int32_t>()};
    layout(f, q);
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
