// The context of the C ABI (include/misti_hip.h: misti_ctx) and what the host layer's translation units share around it: its buffers,
// the HIP error check, the batch path (run_dev, misti_api.cpp) and the carving of a workspace.  Internal: never installed, and not
// included by misti_multi.cpp and misti_lanes.cpp, which know the public entry points alone.  Everything shared lies in misti_host,
// hidden: nothing of it is exported from the library.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

#include "misti_device.h"
#include "misti_fail.h"

#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) return misti_host::fail(MISTI_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

namespace misti_host __attribute__((visibility("hidden"))) {

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

}  // namespace misti_host

using misti_host::DevBuf;
using misti_host::PinBuf;

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
    DevBuf post_ws;                     // misti_ens_summary_dev: means [S][N] | the centred ensemble-mean series [S][N][n] | the sort's keys [2][S][N][m] (hpd / order)
    DevBuf joint_ws;                    // misti_ens_joint_dev: the windows [S][n_pair][2][2] | the histograms [S][cells], each only where the caller gives no buffer of its own
    DevBuf bands_ws;                    // misti_traj_bands_dev: the sort's keys [2][groups of a pass][numT][2][m]
    DevBuf bands_f64, bands_i32;        // misti_traj_bands: a pass's points, splits and rates, the call's outputs | statuses, bounds, pulse times, counts
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

namespace misti_host __attribute__((visibility("hidden"))) {

// hints (what an internal caller knows about its own batch; 0 from the ABI's entry points, whose split times live on the device):
//   RUN_INTEGER_SPLITS  no split time has a fractional part (or is negative: an empty slot) - no tail for the post launch
//   RUN_UNSHARED        every candidate has its own parameter vector: no trunk for a batch too large for one chain per wave
//   RUN_ONE_LENGTH      every chain has the same number of intervals: the chains need no sorting by length
enum : unsigned { RUN_INTEGER_SPLITS = 1u, RUN_UNSHARED = 2u, RUN_ONE_LENGTH = 4u };

// The batch path (misti_api.cpp): one batch of candidates through the engine, on the context's stream.
int run_dev(misti_ctx* c, int64_t n_cand, const double* d_split, const double* d_params, const int32_t* d_bounds, int64_t n_rep, const double* d_jsfs,
            double* d_llk, double* d_jafs, double* d_lc, double* d_pr, int32_t* d_status, unsigned hints = 0, const int32_t* d_pulses = nullptr);
// What a host-buffer entry point returns through (misti_api.cpp): on an error the context's streams are drained before it is reported.
int eval_batch_drained(misti_ctx* c, int r);

// Bump allocation over one buffer.  A workspace's layout is ONE sequence of take() calls, run twice: over a null base to learn the
// size, then over the buffer to assign the pointers - size and layout cannot disagree.
template <class T>
struct Carver {
    T* base = nullptr;
    size_t n = 0;
    T* take(size_t k) { T* p = base ? base + n : nullptr; n += k; return p; }
};

// A workspace in two of the context's buffers (one allocation per type: doubles | int32): `layout` run twice, as Carver says.
template <class Layout>
int carve(DevBuf& f64, DevBuf& i32, Layout&& layout) {
    Carver<double> f;
    Carver<int32_t> q;
    layout(f, q);
    HIP_TRY(f64.reserve(f.n * sizeof(double)));
    HIP_TRY(i32.reserve(q.n * sizeof(int32_t)));
    f = Carver<double>{f64.as<double>()};
    q = Carver<int32_t>{i32.as<int32_t>()};
    layout(f, q);
    return 0;
}

}  // namespace misti_host
