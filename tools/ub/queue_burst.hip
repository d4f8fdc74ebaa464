// How a burst of batches on many streams starts from an idle device: N streams, each given `pre` short kernels, one long kernel (spins
// `long_us`, 20 workgroups of 128 threads - the shape of the follow kernel on config 2) and `post` short dependent kernels.
// Prints, per (N, pre, post): the burst's wall time and when each stream's long kernel started and ended (device clock, relative to the first).
// hipcc --offload-arch=gfx950 -O2 -o queue_burst queue_burst.hip && ./queue_burst
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdio>
#include <vector>
#include <algorithm>

__global__ void spin_kernel(long long ticks, long long* stamp) {
    const long long t0 = wall_clock64();
    if (blockIdx.x == 0 && threadIdx.x == 0 && stamp) stamp[0] = t0;
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
    if (blockIdx.x == 0 && threadIdx.x == 0 && stamp) stamp[1] = wall_clock64();
}

__global__ void short_kernel(double* x) { x[blockIdx.x * blockDim.x + threadIdx.x] += 1.0; }

int main(int argc, char** argv) {
    const double long_us = argc > 1 ? atof(argv[1]) : 1400.0;
    const long long ticks = (long long)(long_us * 100.0);        // wall_clock64: 100 MHz
    double* x;
    hipMalloc(&x, 256 * 128 * sizeof(double));
    hipMemset(x, 0, 256 * 128 * sizeof(double));
    long long* stamps;
    hipHostMalloc(&stamps, 64 * 2 * sizeof(long long));
    const int shapes[][2] = {{0, 0}, {1, 1}, {1, 2}};
    // how the burst is waited for: 0 hipDeviceSynchronize; 1 poll hipStreamQuery on every stream, then hipDeviceSynchronize;
    // 2 an event per stream joined on one stream (device-side waits), hipStreamSynchronize of that one, then hipDeviceSynchronize
    // 3 an event recorded behind each stream's launches AT ISSUE, hipEventSynchronize of every one, then hipDeviceSynchronize
    // 4 the same events, polled with hipEventQuery;  5 hipStreamSynchronize of every stream, then hipDeviceSynchronize
    const int wait_mode = argc > 2 ? atoi(argv[2]) : 0;
    if (argc > 3) hipSetDeviceFlags(atoi(argv[3]) ? hipDeviceScheduleSpin : hipDeviceScheduleBlockingSync);
    const int use_graph = argc > 4 ? atoi(argv[4]) : 0;      // 1: the launches of a stream are ONE captured graph (hipGraphLaunch per stream)
    // argv[6]: how the streams are created.  0 hipStreamCreateWithFlags (the default level);  1 hipStreamCreateWithPriority, every stream on
    // the default level;  2 hipStreamCreateWithPriority, stream i on level i % (number of levels hipDeviceGetStreamPriorityRange reports) -
    // the runtime keeps one pool of GPU_MAX_HW_QUEUES hardware queues PER LEVEL.  With 1 or 2 every line is followed by the number of long
    // kernels that ran beside each other (from the stamps) and, per level, when its long kernels started and how long they took start to end.
    const int prio_mode = argc > 6 ? atoi(argv[6]) : 0;
    int prio_least = 0, prio_greatest = 0;                   // least = lowest priority = the LARGEST number
    hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    const int n_levels = prio_least - prio_greatest + 1;
    if (prio_mode) printf("stream priorities %d (greatest) .. %d (least): %d levels; streams %s\n", prio_greatest, prio_least, n_levels,
                          prio_mode == 2 ? "dealt over the levels" : "all on level 0");
    // level 0 is the default priority (0), then the lower ones, then the higher ones
    auto level_priority = [&](int level) {
        std::vector<int> order{0};
        for (int p = 1; p <= prio_least; ++p) order.push_back(p);
        for (int p = -1; p >= prio_greatest; --p) order.push_back(p);
        return order[(size_t)level % order.size()];
    };
    hipStream_t join;
    hipStreamCreateWithFlags(&join, hipStreamNonBlocking);
    std::vector<hipEvent_t> evs(32);
    for (auto& e : evs) hipEventCreateWithFlags(&e, hipEventDisableTiming);
    for (int N : {4, 12, 20}) {
        std::vector<hipStream_t> st(N);
        std::vector<int> prio(N, 0);
        for (int i = 0; i < N; ++i) {
            if (!prio_mode) { hipStreamCreateWithFlags(&st[i], hipStreamNonBlocking); continue; }
            prio[i] = prio_mode == 2 ? level_priority(i % n_levels) : 0;
            hipStreamCreateWithPriority(&st[i], hipStreamNonBlocking, prio[i]);
        }
        for (auto& sh : shapes) {
            std::vector<hipGraphExec_t> gx(N, nullptr);
            if (use_graph) {
                for (int i = 0; i < N; ++i) {
                    hipGraph_t g;
                    hipStreamBeginCapture(st[i], hipStreamCaptureModeThreadLocal);
                    for (int k = 0; k < sh[0]; ++k) short_kernel<<<256, 128, 0, st[i]>>>(x);
                    spin_kernel<<<20, 128, 0, st[i]>>>(ticks, stamps + 2 * i);
                    for (int k = 0; k < sh[1]; ++k) short_kernel<<<256, 128, 0, st[i]>>>(x);
                    hipStreamEndCapture(st[i], &g);
                    hipGraphInstantiate(&gx[i], g, nullptr, nullptr, 0);
                    hipGraphDestroy(g);
                    hipGraphLaunch(gx[i], st[i]);            // first launch uploads
                }
                hipDeviceSynchronize();
            }
            double best = 1e30;
            std::vector<double> starts, ends;
            for (int rep = 0; rep < 5; ++rep) {
                hipDeviceSynchronize();
                const auto t0 = std::chrono::steady_clock::now();
                for (int i = 0; i < N; ++i) {
                    if (use_graph) { hipGraphLaunch(gx[i], st[i]); continue; }
                    for (int k = 0; k < sh[0]; ++k) short_kernel<<<256, 128, 0, st[i]>>>(x);
                    spin_kernel<<<20, 128, 0, st[i]>>>(ticks, stamps + 2 * i);
                    for (int k = 0; k < sh[1]; ++k) short_kernel<<<256, 128, 0, st[i]>>>(x);
                    if (wait_mode == 3 || wait_mode == 4) hipEventRecord(evs[i], st[i]);
                }
                const auto t1 = std::chrono::steady_clock::now();
                if (wait_mode == 3) for (int i = 0; i < N; ++i) hipEventSynchronize(evs[i]);
                if (wait_mode == 4) for (int i = 0; i < N; ++i) while (hipEventQuery(evs[i]) == hipErrorNotReady) {}
                if (wait_mode == 5) for (int i = 0; i < N; ++i) hipStreamSynchronize(st[i]);
                if (wait_mode == 1) {
                    for (int i = 0; i < N; ++i) while (hipStreamQuery(st[i]) == hipErrorNotReady) {}
                } else if (wait_mode == 2) {
                    for (int i = 0; i < N; ++i) { hipEventRecord(evs[i], st[i]); hipStreamWaitEvent(join, evs[i], 0); }
                    hipStreamSynchronize(join);
                }
                const auto t1b = std::chrono::steady_clock::now();
                hipDeviceSynchronize();
                const auto t2 = std::chrono::steady_clock::now();
                const double ms = std::chrono::duration<double, std::milli>(t2 - t0).count();
                if (ms < best) {
                    best = ms;
                    starts.clear();
                    ends.clear();
                    long long first = stamps[0];
                    for (int i = 0; i < N; ++i) first = std::min(first, stamps[2 * i]);
                    for (int i = 0; i < N; ++i) starts.push_back((stamps[2 * i] - first) / 100.0);
                    for (int i = 0; i < N; ++i) ends.push_back((stamps[2 * i + 1] - first) / 100.0);
                    long long last = 0;
                    for (int i = 0; i < N; ++i) last = std::max(last, stamps[2 * i + 1]);
                    starts.push_back((last - first) / 100.0);
                    starts.push_back(std::chrono::duration<double, std::micro>(t2 - t1b).count());
                    starts.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
                }
            }
            for (auto g : gx) if (g) hipGraphExecDestroy(g);
            printf("N=%2d pre=%d post=%d  burst %.3f ms (issue %.0f us; last long kernel ends at %.0f us; final hipDeviceSynchronize %.0f us)",
                   N, sh[0], sh[1], best, starts[N + 2], starts[N], starts[N + 1]);
            if (argc > 5) { printf("  long-kernel starts [us]:"); for (int i = 0; i < N; ++i) printf(" %.0f", starts[i]); }
            printf("\n");
            if (prio_mode) {
                int beside = 0;                              // the most long kernels running at one moment: counted at every start
                for (int i = 0; i < N; ++i) {
                    int n = 0;
                    for (int j = 0; j < N; ++j) n += starts[j] <= starts[i] && starts[i] < ends[j];
                    beside = std::max(beside, n);
                }
                printf("    long kernels beside each other: %d of %d;", beside, N);
                for (int p = prio_greatest; p <= prio_least; ++p) {
                    int n = 0;
                    double s0 = 1e30, s1 = 0, dur = 0, dmax = 0;
                    for (int i = 0; i < N; ++i) if (prio[i] == p) {
                        ++n; s0 = std::min(s0, starts[i]); s1 = std::max(s1, starts[i]);
                        dur += ends[i] - starts[i]; dmax = std::max(dmax, ends[i] - starts[i]);
                    }
                    if (n) printf("  priority %d: %d streams, starts %.0f .. %.0f us, start to end mean %.0f max %.0f us;", p, n, s0, s1, dur / n, dmax);
                }
                printf("\n");
            }
        }
        for (auto& s : st) hipStreamDestroy(s);
    }
    return 0;
}
