// Compile-time sizes shared by the table builder, the kernels and the C-ABI layer.
#pragma once
namespace misti {
constexpr int NS2 = 44;               // two-population states
constexpr int NS1 = 8;                // one-population states
constexpr int MAXNZ = 4;              // off-diagonal entries per generator row
constexpr int MAXPULSE = 12;          // entries per row of the pulse operator
#ifndef MISTI_WAVES_PER_BLOCK
#define MISTI_WAVES_PER_BLOCK 4
#endif
// Issue priority (s_setprio) in a one-chain-per-wave launch of at most 256 chains (correct_follow_kernel; the ladder of larger launches
// is not touched): 0 none; 1 the chain wave runs at priority 3 and returns to 0 before it pulls the next chain; 2 as 1, and the trunk
// wave sets priority 0 explicitly.  Shipped: 1 (measured against 0 and 2: DESIGN.md section 6).
#ifndef MISTI_SMALL_LAUNCH_PRIO
#define MISTI_SMALL_LAUNCH_PRIO 1
#endif
// Defaults of the other build switches that take a value (misti_kernels.hip and its headers; the ones that are only defined or not -
// MISTI_STAMP, MISTI_STAMP2, MISTI_TREE_STATS, MISTI_NO_STALL_RULE, MISTI_NO_NOISE_RULE - have none):
#ifndef MISTI_WORK_COUNTERS
#define MISTI_WORK_COUNTERS 0         // 1: diagnostic build that also counts the per-lane work of a chain (Diag, misti_model.h)
#endif
#ifndef MISTI_NOISE_PROBE
#define MISTI_NOISE_PROBE 1           // 0: diagnostic build, the default fit's noise rule from its width model alone (correct_body, misti_chain.h)
#endif
#ifndef MISTI_DEFAULT_FIT_WAVES
#define MISTI_DEFAULT_FIT_WAVES 1     // waves per SIMD of the default fit's packed chain kernel (correct_kernel)
#endif
#ifndef MISTI_FOLLOW_WAVES
#define MISTI_FOLLOW_WAVES 2          // waves per SIMD of the --cpfit one-chain-per-wave kernels (correct_follow_kernel, correct_resume_kernel)
#endif
constexpr int WAVES_PER_BLOCK = MISTI_WAVES_PER_BLOCK;    // candidates per workgroup of kernel 2 (one wavefront each)
constexpr int TALBOT_N = 28;           // nodes of the Talbot contour (conjugate pairs folded: TALBOT_HALF solves)
constexpr int TALBOT_HALF = TALBOT_N / 2;
constexpr int INV_TABLE = 1024;         // reciprocal table for the series (also the cap on terms per series)
constexpr int TRUNK_REC = 3 * NS2;    // doubles per trunk record: state vector | occupation integral before | from the sample date
constexpr int TRUNK_MAX_CHAINS = 8192; // trunk buffer bound: 8 192 chains x numT records x 1 056 B (1.1 GB at numT = 128)
constexpr int TRUNK_MIN_SHARE = 8;    // the trunk runs when a chain has on average at least this many candidates
constexpr int FOLLOW_MAX_CHAINS = 1024; // up to this many chains a batch runs one chain per wave (speculation, trunk wave following), workgroups
                                        // pulling chains longest-first from a queue; beyond it chains are packed 10 per wave.  1 024 two-wave
                                        // workgroups are resident at 2 waves per SIMD: one round.  Measured (MI355X): 1 024 chains 1.68 ms
                                        // against 2.71 ms packed; 2 048 chains (config 5) 5.07 against 5.50 ms alone, and with 20 batches in
                                        // flight 1.7e7 against 4.1e7 evals/s - a packed wave carries ten chains per instruction stream
constexpr int FOLLOW_BUSY_CHAINS = 128; // ... but only up to this many while the device is busy with OTHER contexts' batches (FOLLOW_BUSY_CONTEXTS of them or
                                        // more have a batch in flight): one chain per wave buys latency with the whole chip, and a caller who
                                        // overlaps batches wants throughput.  Measured, 20 batches in flight: 128 chains 3.3e7 evals/s either way;
                                        // 256 chains 3.7e7 one per wave, 4.7e7 packed; 512: 4.0e7 / 6.3e7; 1 024 (config2x16): 4.2e7 / 7.7e7
constexpr int FOLLOW_BUSY_CONTEXTS = 3;
constexpr int YIELD_NFEV = 8;           // packed launches: a solve still running after this many evaluations hands its chain to the resume launch
constexpr int PAIR_TABLE = 8 * 8 * 2 * 16 * 4;   // XCC x SE x SH x CU x SIMD counters of the placement-aware role choice (correct_follow_kernel)
constexpr int FOLLOW_MIN_BLOCKS = 256;   // workgroups of the one-chain-per-wave launch whatever the (possibly stale) chain-count hint says
constexpr int SMOOTH_REPS = 4;        // numT <= 64 * SMOOTH_REPS (smoothing pass keeps runs in registers)
}  // namespace misti
