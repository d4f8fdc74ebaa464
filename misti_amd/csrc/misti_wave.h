// Wave and LDS helpers of the chain kernels: lane broadcasts, the LDS hand-over words between the two waves of a workgroup, scalar
// branch conditions.  No entry of its own: every kernel of misti_kernels.hip reaches it, and the suite holds it through them.
#pragma once
#include <hip/hip_runtime.h>

namespace misti {

// ---------------------------------------------------------------- helpers ----
__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// broadcast from a WAVE-UNIFORM source lane: scalar readlane, no LDS crossbar round trip
__device__ __forceinline__ double bcast(double v, int src_lane) {
    int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
    return __hiloint2double(hi, lo);
}

// The correction kernel packs GROUP (8, 16, 32 or 64) lanes per candidate, 6 of which carry the
// residual evaluations (3 forward-difference points x 2 genomes): 8 ... 1 candidates per wavefront,
// chosen at launch from the batch size (few candidates per wave while the chip is not full).
// Everything "uniform" is uniform within a group; cross-lane traffic never leaves a group.
template <int GROUP>
__device__ __forceinline__ double gbcast(double v, int j) {
    if (GROUP == 64) {                       // one candidate per wave: scalar broadcast (j wave-uniform), no LDS crossbar round trip
        const int ju = __builtin_amdgcn_readfirstlane(j);
        int lo = __builtin_amdgcn_readlane(__double2loint(v), ju);
        int hi = __builtin_amdgcn_readlane(__double2hiint(v), ju);
        return __hiloint2double(hi, lo);
    }
    return __shfl(v, (lane_id() - lane_id() % GROUP) + j, 64);     // GROUP = 6: ten items per wave, lanes 60-63 idle
}

// Hand-over words in LDS between the two waves of a workgroup (correct_follow_kernel).  The pointers reach the
// device functions as generic pointers and a volatile access through a generic pointer is a FLAT instruction with
// system-scope cache bits followed by a wait for every outstanding global store; through an LDS-typed pointer it is a
// plain ds_read / ds_write.  Ordering between the two waves ("data, then count" on the writer's side, "count, then data" on the
// reader's) is a workgroup-scope release / acquire fence restricted to the LDS address space: it compiles to s_waitcnt lgkmcnt(0)
// - no wait for the outstanding global stores of the chain - and is what the AMDGPU memory model asks for between waves (a
// wavefront-scope fence orders nothing across waves and merely happened to work; the build never uses -mtgsplit).
typedef __attribute__((address_space(3))) int lds_i32_t;
__device__ __forceinline__ void lds_put(volatile int* p, int v) { *(volatile lds_i32_t*)(lds_i32_t*)p = v; }
__device__ __forceinline__ int lds_get(const volatile int* p) { return *(const volatile lds_i32_t*)(lds_i32_t*)p; }
__device__ __forceinline__ void lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// A branch condition that is the same in every lane - everything of a chain is, when the chain has the wave to itself
// (GROUP == 64) - handed to the compiler as a SCALAR: it then branches with s_cbranch_scc instead of masking lanes off
// (s_and_saveexec / s_or exec around every block, and copies of all loop-carried state at every divergent loop edge:
// that plumbing was about a fifth of the correction kernel's instructions).  With several chains per wave the condition
// really differs between lanes and is left alone.
template <int GROUP>
__device__ __forceinline__ bool uni(bool c) { return GROUP == 64 ? (bool)__builtin_amdgcn_readfirstlane((int)c) : c; }

__device__ __forceinline__ void lds_fence() {
    // one wave owns its LDS slice: ordering only has to be kept by the compiler
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace misti
