// Lanes (include/misti_hip.h, "lanes: many batches in flight on ONE device"): n engine contexts of one model on one device, each with
// its own non-blocking stream, behind one object - the overlapped rate of the headline benchmark for a caller of the C ABI (VERDICT r5
// item 5; until round 6 the pool lived in Python, misti_amd/lanes.py).  The reference's counterpart: one MigrationInference object per
// process, as many processes as cores (/root/reference/MiSTI.py:213-214 under `parallel -j 20`, README.md:110-115).
// Built on the public single-context entry points; no C++ exception leaves this file.
#include <cstdlib>
#include <exception>
#include <new>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/misti_hip.h"
#include "misti_fail.h"

// misti_api.cpp: misti_create on a stream priority.  This and the runtime's priority range are the only things here beyond the public
// single-context entry points and the event calls, and both are WEAK references: the library always has them; the host-only build of
// this file against stand-ins (tests/multi_host) has not, and is then a pool on one level made by misti_create, as before the plan.
extern "C" int misti_create_prio_(const misti_model_t* model, int device, int priority, misti_ctx** out) __attribute__((weak));
extern "C" hipError_t hipDeviceGetStreamPriorityRange(int* least, int* greatest) __attribute__((weak));
// misti_api.cpp: the event a context records behind every batch of its own, with its counters (weak for the same reason: without it a
// lane records its own event behind every batch, as before)
extern "C" void* misti_batch_event_(misti_ctx* c, int64_t* recorded, int64_t* begun) __attribute__((weak));

using misti_host::fail;

namespace {

// A hardware queue per lane where the runtime grants one.  The HIP runtime keeps one pool of hardware queues PER STREAM PRIORITY and
// opens at most GPU_MAX_HW_QUEUES queues in each (default 4; it says so itself at AMD_LOG_LEVEL=3: "Number of allocated hardware queues
// with low priority: 4, with normal priority: 4, with high priority: 4, maximum per priority is: 4").  It reads the variable when it
// initialises - at the process's first HIP call, which for a C caller comes after this library was loaded - so the constructor below
// asks for 22 where the environment names nothing.  Never overrides a value the user has set; MISTI_KEEP_HW_QUEUES=1 leaves the
// environment alone.
// Where the limit is smaller than the pool (a GPU_MAX_HW_QUEUES inherited from the caller, or a runtime that was up before this
// library was loaded), streams that share a queue are serialised packet by packet: twenty lanes on four queues run four batches at a
// time.  lane_plan() below then deals the lanes over the priority levels the device reports - three levels of four queues are twelve
// queues, twelve long kernels beside each other where there were four (tools/ub/queue_burst.hip, profiles/lane_priorities_queue_burst.txt;
// a kernel on the low level starts as soon and takes as long as one on the high level while the chip has room).
// MISTI_LANE_PRIORITIES=0 keeps every lane on the default level.
// 22, not "as many as possible": the device runs 23 queues beside each other, and with a 24th ACTIVE one a burst of batches takes 10 ms
// instead of 2.7 (the scheduler starts time-slicing the queues; measured round 6, profiles/r06_hw_queue_cliff.txt: 22 lanes + the null
// stream 2.9 ms, 23 lanes 10.4 ms when the runtime may open 32).  Capped at 22 the runtime never opens the 24th: streams beyond the cap
// SHARE queues (24 lanes: 4.3 ms) - and what else a process creates (the null stream, RCCL's and PyTorch's own streams) cannot push a
// lane pool over the edge.  The plan keeps the same cap over all levels together.
constexpr int POOL_MAX_QUEUES = 22;
constexpr int HIP_DEFAULT_HW_QUEUES = 4;

__attribute__((constructor)) void misti_lanes_queue_env() {
    const char* keep = std::getenv("MISTI_KEEP_HW_QUEUES");
    if (keep && keep[0] && keep[0] != '0') return;
    (void)setenv("GPU_MAX_HW_QUEUES", "22", 0);
}

// Which priority level each of `n_lanes` lanes goes on: level 0 is the default priority, `q` the runtime's queue limit per level,
// `n_levels` what the device reports, `cap` the most distinct queues the pool may occupy.  A level with n lanes occupies min(n, q)
// queues (the runtime deals a level's streams over its queues).  Pure: no HIP call, no environment, the same answer every time.
//  - n_lanes + 1 <= q (a queue for every lane beside the null stream) or one level: every lane on the default level.
//  - else the levels are given queues in order, the default level first, q each until min(n_lanes, cap) are dealt; each queue gets one
//    lane; lanes beyond the queues go to the levels that have all q queues (a level with fewer must not grow: every further lane there
//    would open a further queue), evenly, the default level last - its queues also carry the process's null stream.
//    So no queue carries more than ceil(n_lanes / queues) lanes - except where the cap leaves a level with fewer than q queues: that
//    level keeps one lane per queue and the full levels carry the rest.
//  - consecutive lanes go on different levels, so that a caller who issues round-robin reaches every queue early.
void lane_plan(int n_lanes, int q, int n_levels, int cap, std::vector<int>& level) {
    level.assign((size_t)n_lanes, 0);
    if (q < 1) q = 1;
    if (n_levels <= 1 || n_lanes + 1 <= q) return;
    std::vector<int> lanes_on((size_t)n_levels, 0);
    int queues = n_lanes < cap ? n_lanes : cap, full = 0;
    for (int l = 0; l < n_levels && queues > 0; ++l) {
        lanes_on[(size_t)l] = queues < q ? queues : q;
        queues -= lanes_on[(size_t)l];
        full += lanes_on[(size_t)l] == q;
    }
    int placed = 0;
    for (int n : lanes_on) placed += n;
    if (full == 0) { lanes_on[0] += n_lanes - placed; placed = n_lanes; }        // cap < q: one level, as without a plan
    for (int l = full - 1; placed < n_lanes; l = l > 0 ? l - 1 : full - 1) { ++lanes_on[(size_t)l]; ++placed; }
    int l = 0;
    for (int i = 0; i < n_lanes; ++i) {
        while (lanes_on[(size_t)l] == 0) l = (l + 1) % n_levels;
        level[(size_t)i] = l;
        --lanes_on[(size_t)l];
        l = (l + 1) % n_levels;
    }
}

// The plan of a pool that is created now: the queue limit as the environment names it (else HIP's own), MISTI_LANE_PRIORITIES=0.
void lane_levels(int n_lanes, int n_levels, std::vector<int>& level) {
    const char* e = std::getenv("GPU_MAX_HW_QUEUES");
    int q = e ? std::atoi(e) : 0;
    if (q < 1) q = HIP_DEFAULT_HW_QUEUES;
    const char* p = std::getenv("MISTI_LANE_PRIORITIES");
    if (p && p[0] == '0' && !p[1]) n_levels = 1;
    lane_plan(n_lanes, q, n_levels, POOL_MAX_QUEUES, level);
}

// Level 0 is the default priority (0), levels 1, 2, ... the lower priorities (larger numbers) down to `least`, then the higher ones.
int level_priority(int level, int least) { return level <= least ? level : least - level; }

}  // namespace

struct misti_lanes {
    int device = 0;
    std::vector<misti_ctx*> ctx;
    std::vector<int> level;               // each lane's priority level (lane_plan)
    std::vector<hipStream_t> stream;      // each context's own stream (misti_get_stream at creation)
    std::vector<hipEvent_t> done;         // the lane's own event: recorded behind a batch only where the context recorded none behind it
    std::vector<hipEvent_t> last;         // the event behind the lane's last batch - the context's or done[i]; NULL: no batch yet.
                                          // "Nothing in flight" is a query of it
    int next = 0;                         // round-robin position of MISTI_LANE_ANY
};

namespace {

template <class F>
int guarded(const char* where, F&& fn) noexcept {
    try {
        return fn();
    } catch (const std::bad_alloc&) {
        return fail(MISTI_E_NOMEM, "%s: out of host memory", where);
    } catch (const std::exception& e) {
        return fail(MISTI_E_ARG, "%s: %s", where, e.what());
    } catch (...) {
        return fail(MISTI_E_ARG, "%s: unknown C++ exception", where);
    }
}

// 1 busy, 0 idle, < 0 error
int lane_busy(misti_lanes* L, int i) {
    if (!L->last[(size_t)i]) return 0;
    const hipError_t e = hipEventQuery(L->last[(size_t)i]);
    if (e == hipSuccess) return 0;
    (void)hipGetLastError();
    if (e == hipErrorNotReady) return 1;
    return fail(MISTI_E_HIP, "hipEventQuery on lane %d: %s", i, hipGetErrorString(e));
}

void release(misti_lanes* L) {
    for (misti_ctx* c : L->ctx) (void)misti_destroy(c);          // waits for the context's streams before releasing (misti_api.cpp)
    (void)hipSetDevice(L->device);
    for (hipEvent_t e : L->done) if (e) (void)hipEventDestroy(e);
    (void)hipGetLastError();
    delete L;
}

}  // namespace

extern "C" {

int misti_create_lanes(const misti_model_t* model, int device, int n_lanes, misti_lanes** out) {
    if (!out) return fail(MISTI_E_ARG, "out is NULL");
    *out = nullptr;
    if (n_lanes < 1 || n_lanes > MISTI_MAX_LANES) return fail(MISTI_E_LIMIT, "n_lanes %d out of range (1..%d)", n_lanes, MISTI_MAX_LANES);
    misti_lanes* L = nullptr;
    const int r = guarded("misti_create_lanes", [&]() -> int {
        L = new misti_lanes;
        L->device = device;
        // the levels the device has (least = the lowest priority = the largest number); a device that cannot be asked has one, and the
        // first context reports what is wrong with it
        int least = 0, greatest = 0;
        if (!misti_create_prio_ || !hipDeviceGetStreamPriorityRange || hipSetDevice(device) != hipSuccess ||
            hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { (void)hipGetLastError(); least = greatest = 0; }
        if (least < 0) least = 0;
        if (greatest > 0) greatest = 0;
        lane_levels(n_lanes, least - greatest + 1, L->level);
        for (int i = 0; i < n_lanes; ++i) {
            misti_ctx* c = nullptr;
            const int lv = L->level[(size_t)i];
            if (int q = lv ? misti_create_prio_(model, device, level_priority(lv, least), &c) : misti_create(model, device, &c)) return q;   // the message is the context's
            L->ctx.push_back(c);
            void* s = nullptr;
            if (int q = misti_get_stream(c, &s)) return q;
            L->stream.push_back(static_cast<hipStream_t>(s));
            hipEvent_t e = nullptr;
            const hipError_t he = hipEventCreateWithFlags(&e, hipEventDisableTiming);
            if (he != hipSuccess) return fail(MISTI_E_HIP, "hipEventCreateWithFlags: %s", hipGetErrorString(he));
            L->done.push_back(e);
            L->last.push_back(nullptr);
        }
        return 0;
    });
    if (r != 0) {
        if (L) { const std::string why = misti_last_error(); release(L); return fail(r, "%s", why.c_str()); }
        return r;
    }
    *out = L;
    return 0;
}

int misti_destroy_lanes(misti_lanes* L) {
    if (!L) return 0;
    release(L);
    return 0;
}

// internal (tests): the plan without a device.  `queues_per_level` > 0: lane_plan itself with that limit and `max_queues`;
// 0: what misti_create_lanes would do in this environment on a device with `n_levels` levels.  levels[n_lanes] receives each lane's level.
int misti_lane_plan_(int n_lanes, int queues_per_level, int n_levels, int max_queues, int* levels) {
    if (n_lanes < 1 || n_lanes > MISTI_MAX_LANES || n_levels < 1 || !levels) return fail(MISTI_E_ARG, "misti_lane_plan_: bad argument");
    return guarded("misti_lane_plan_", [&]() -> int {
        std::vector<int> level;
        if (queues_per_level > 0) lane_plan(n_lanes, queues_per_level, n_levels, max_queues, level);
        else lane_levels(n_lanes, n_levels, level);
        for (int i = 0; i < n_lanes; ++i) levels[i] = level[(size_t)i];
        return 0;
    });
}

// internal (tests): the priority level lane i's stream was created on (0: the default level); < 0: no such lane
int misti_lanes_level_(misti_lanes* L, int i) {
    if (!L || i < 0 || i >= (int)L->level.size()) return fail(MISTI_E_ARG, "no such lane");
    return L->level[(size_t)i];
}

int misti_lanes_size(misti_lanes* L) { return L ? (int)L->ctx.size() : 0; }

int misti_lanes_context(misti_lanes* L, int i, misti_ctx** ctx) {
    if (!L || !ctx || i < 0 || i >= (int)L->ctx.size()) return fail(MISTI_E_ARG, "no such lane");
    *ctx = L->ctx[(size_t)i];
    return 0;
}

int misti_lanes_set_hints(misti_lanes* L, uint32_t hints) {
    if (!L) return fail(MISTI_E_ARG, "lanes is NULL");
    for (misti_ctx* c : L->ctx) if (int r = misti_set_hints(c, hints)) return r;
    return 0;
}

int misti_lanes_busy(misti_lanes* L, int lane) {
    if (!L || lane < 0 || lane >= (int)L->ctx.size()) return fail(MISTI_E_ARG, "no such lane");
    return lane_busy(L, lane);
}

int misti_lanes_eval_batch_dev(misti_lanes* L, int lane, int64_t n_cand, const double* d_split, const double* d_params, const int32_t* d_bounds,
                               int64_t n_rep, const double* d_jsfs, double* d_llk, double* d_jafs, double* d_lc, double* d_pr, int32_t* d_status, int* lane_used) {
    if (!L) return fail(MISTI_E_ARG, "lanes is NULL");
    const int n = (int)L->ctx.size();
    if (lane != MISTI_LANE_ANY && (lane < 0 || lane >= n)) return fail(MISTI_E_ARG, "lane %d out of range (0..%d, or MISTI_LANE_ANY)", lane, n - 1);
    if (lane == MISTI_LANE_ANY) {
        // a lane with nothing in flight, looked for from the round-robin position on; if every lane is busy, the round-robin one
        lane = L->next;
        for (int k = 0; k < n; ++k) {
            const int i = (L->next + k) % n;
            const int b = lane_busy(L, i);
            if (b < 0) return b;
            if (b == 0) { lane = i; break; }
        }
        L->next = (lane + 1) % n;
    }
    // One event per batch: the context records its own behind every batch, on this lane's stream (misti_api.cpp: last_ev).  A second
    // record straight behind it would be one more packet for the queue to hand over, and streams that share a hardware queue are
    // served packet by packet.  So the lane records its own event only where the context's does not stand behind the batch: a context
    // without one, a batch that put nothing into the stream (n_cand == 0), and a batch that failed with work already in flight - which
    // stays waitable.  A batch that failed before its first stream operation leaves the lane as it was.
    misti_ctx* const c = L->ctx[(size_t)lane];
    int64_t rec0 = 0, rec1 = 0, beg0 = 0, beg1 = 0;
    void* const ctx_ev = misti_batch_event_ ? misti_batch_event_(c, &rec0, &beg0) : nullptr;
    const int r = misti_eval_batch_dev(c, n_cand, d_split, d_params, d_bounds, n_rep, d_jsfs, d_llk, d_jafs, d_lc, d_pr, d_status);
    if (ctx_ev) (void)misti_batch_event_(c, &rec1, &beg1);
    if (ctx_ev && rec1 != rec0) {
        L->last[(size_t)lane] = static_cast<hipEvent_t>(ctx_ev);
    } else if (r == 0 || beg1 != beg0) {
        const hipError_t e = hipEventRecord(L->done[(size_t)lane], L->stream[(size_t)lane]);
        if (e == hipSuccess) L->last[(size_t)lane] = L->done[(size_t)lane];
        else if (r == 0) return fail(MISTI_E_HIP, "hipEventRecord on lane %d: %s", lane, hipGetErrorString(e));
        else (void)hipGetLastError();                    // the batch's own error is the one to report
    }
    if (r != 0) return r;
    if (lane_used) *lane_used = lane;
    return 0;
}

// Waiting for a lane = waiting for the EVENT recorded behind its last batch when that batch was issued, then misti_sync.  The event is
// what makes the difference with many lanes: asked whether a stream is finished (hipStreamSynchronize, hipStreamQuery,
// hipDeviceSynchronize) the runtime first has to put a marker of its own behind the stream's last kernel and wait for it to come back -
// one round trip per hardware queue, one queue after the other, 0.02 ms each: twenty lanes report complete 0.25 - 0.36 ms after their
// last kernel ended.  The event's marker is already in the queue behind the batch; its signal fires when the batch ends, and the
// stream synchronisation after it finds the queue's last command complete (tools/ub/queue_burst.hip, wait modes 0 / 5 / 3: a burst
// of twenty batch-shaped streams WITHOUT events 2.09 / 2.03 ms, with them 1.87 ms; profiles/r06_queue_burst.txt).  Every batch of a
// context has had such an event behind it since round 3 (misti_api.cpp: last_ev), which is why the bench's device-wide fence never paid
// that price: the bench gains nothing from waiting here first (2.73 against 2.76 - 2.81 ms, run-to-run spread), a caller that
// waits lane by lane does.
static int wait_done(misti_lanes* L, size_t i) {
    if (!L->last[i]) return 0;
    const hipError_t e = hipEventSynchronize(L->last[i]);
    if (e != hipSuccess) return fail(MISTI_E_HIP, "hipEventSynchronize on lane %d: %s", (int)i, hipGetErrorString(e));
    return 0;
}

int misti_lanes_wait(misti_lanes* L, int lane) {
    if (!L || lane < 0 || lane >= (int)L->ctx.size()) return fail(MISTI_E_ARG, "no such lane");
    if (int r = wait_done(L, (size_t)lane)) return r;
    return misti_sync(L->ctx[(size_t)lane]);
}

int misti_lanes_sync(misti_lanes* L) {
    if (!L) return fail(MISTI_E_ARG, "lanes is NULL");
    (void)hipSetDevice(L->device);
    for (size_t i = 0; i < L->ctx.size(); ++i)
        if (int r = wait_done(L, i)) return r;
    for (size_t i = 0; i < L->ctx.size(); ++i)
        if (int r = misti_sync(L->ctx[i])) { const std::string why = misti_last_error(); return fail(r, "lane %d: %s", (int)i, why.c_str()); }
    return 0;
}

}  // extern "C"
