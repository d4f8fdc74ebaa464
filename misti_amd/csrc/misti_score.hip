// MI355X (gfx950) kernels behind a batch (misti_kernels.hip), on its finished spectra jafs[n_cand][7] / status[n_cand]: llh_const_kernel,
// llk_kernel + argmax_kernel (the table and its reduction), the scans without the table (scan_best, scan_profile), llk_rows_kernel (one row
// per candidate) and the curvature at a point (curv_*_kernel).  The expressions every path shares are in misti_score.h, once.
#include "misti_score.h"

namespace misti {

// ------------------------------------------------------- replicate epilogue --
// llh_const of SetJAFS (MigrationInference.py:217-227): one thread per replicate (misti_llk_dev).
__global__ __launch_bounds__(256) void llh_const_kernel(int64_t n_rep, const double* __restrict__ jsfs, double* __restrict__ consts, int unfolded) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rep) return;
    consts[r] = llh_const_of(jsfs + r * 8, unfolded);
}
hipError_t launch_llh_const(int64_t n_rep, const double* jsfs, double* consts, int unfolded, hipStream_t stream) {
    if (n_rep <= 0) return hipSuccess;
    hipLaunchKernelGGL(llh_const_kernel, dim3((unsigned)((n_rep + 255) / 256)), dim3(256), 0, stream, n_rep, jsfs, consts, unfolded);
    return hipGetLastError();
}

// llk[c][r] = const[r] + sum_i data[r][i] log JAFS[c][i]  (folded: pairs 0+6, 1+5, 2+4, 3)
// MigrationInference.py:600-609.  The one HBM-WRITE-bound kernel of the path: 8 bytes out per value, 56 bytes of
// spectrum in per CANDIDATE and 72 bytes of data in per REPLICATE.  So the replicate is what a thread keeps: thread = two adjacent
// replicates (their class counts and constants in registers, read once), block = 512 replicates x a CHUNK of candidates whose
// class logs the block computes once into LDS; per value that leaves 4 (folded) or 7 fused multiply-adds and one half of a
// 16-byte store, 1 KB contiguous per wave-instruction, streamed past the caches (nontemporal: nothing reads llk in this kernel).
// Round 4's kernel gave every value its own 64-byte read of the replicate row - 4.7 GB through L2 for 0.5 GB written.
// Same expressions as llk_of / log_class (the inline epilogue of spectrum_kernel): the same bits.
template <bool UNFOLDED>
__global__ __launch_bounds__(256)
void llk_kernel(int64_t n_cand, int chunk, const double* __restrict__ jafs, const int32_t* __restrict__ status,
                int64_t n_rep, const double* __restrict__ jsfs, const double* __restrict__ consts,
                double* __restrict__ llk) {
    __shared__ double lj[SCORE_CHUNK][8];
    const int64_t c0 = (int64_t)blockIdx.y * chunk;
    const int nc = (int)(n_cand - c0 < chunk ? n_cand - c0 : chunk);
    stage_class_logs<UNFOLDED>(lj, nc, jafs, status, [&](int c) { return c0 + c; });
    // this thread's two replicates: class counts (folded: the four sums) and constants
    const int64_t r0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
    const RowCounts<UNFOLDED> row0(jsfs, consts, r0 < n_rep ? r0 : n_rep - 1);          // a lane beyond the table repeats the last row (never stored)
    const RowCounts<UNFOLDED> row1(jsfs, consts, r0 + 1 < n_rep ? r0 + 1 : n_rep - 1);
    __syncthreads();
    if (r0 >= n_rep) return;
    const bool pair = r0 + 1 < n_rep && (n_rep & 1) == 0;                  // both in range and every row 16-byte aligned
    double* out = llk + c0 * n_rep + r0;
    for (int c = 0; c < nc; ++c, out += n_rep) {
        const double a0 = score(row0, lj[c]), a1 = score(row1, lj[c]);
        if (pair) {
            typedef double d2 __attribute__((ext_vector_type(2)));
            d2 v; v.x = a0; v.y = a1;
            __builtin_nontemporal_store(v, (d2*)out);
        } else {
            __builtin_nontemporal_store(a0, out);
            if (r0 + 1 < n_rep) __builtin_nontemporal_store(a1, out + 1);
        }
    }
}

// Bootstrap reduction (test.bs/bs_conf_int.ipynb: per replicate the split value with the largest
// likelihood): thread = replicate, coalesced reads along the replicate axis; -inf / NaN are skipped,
// ties go to the lowest candidate index (numpy.argmax), -1 when no candidate has a value.
__global__ __launch_bounds__(256)
void argmax_kernel(int64_t n_cand, int64_t n_rep, const double* __restrict__ llk, int32_t* __restrict__ best, double* __restrict__ best_llk) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rep) return;
    double bv = -INFINITY;
    int32_t bi = -1;
    for (int64_t c = 0; c < n_cand; ++c) {
        const double v = llk[c * n_rep + r];
        if (v > bv) { bv = v; bi = (int32_t)c; }           // false for NaN and for -inf
    }
    best[r] = bi;
    if (best_llk) best_llk[r] = bv;
}

hipError_t launch_argmax(int64_t n_cand, int64_t n_rep, const double* llk, int32_t* best, double* best_llk, hipStream_t stream) {
    if (n_rep <= 0) return hipSuccess;
    hipLaunchKernelGGL(argmax_kernel, dim3((unsigned)((n_rep + 255) / 256)), dim3(256), 0, stream, n_cand, n_rep, llk, best, best_llk);
    return hipGetLastError();
}

// The K best candidates per replicate WITHOUT the table (misti_scan_best_dev): llk_kernel's values - the same expressions, the same
// bits - compared where they are computed and never stored.  Order: value descending, candidate index ascending on equal values;
// only v > -inf qualifies (false for NaN: argmax_kernel's rule).  That is a total order, so the result does not depend on how the
// candidates are cut into slices.
// One place of a sorted K-list: `v` goes in front of every entry it beats, the entries behind it move down one place and the last
// one leaves.  K is a compile-time constant and every index below is one too: the list is 3 K registers, not an indexed local array.
template <int K>
__device__ __forceinline__ void best_insert(double (&bv)[K], int32_t (&bi)[K], double v, int32_t c) {
#pragma unroll
    for (int j = K - 1; j >= 1; --j) {
        const bool here = v > bv[j], above = v > bv[j - 1];
        bv[j] = above ? bv[j - 1] : (here ? v : bv[j]);
        bi[j] = above ? bi[j - 1] : (here ? c : bi[j]);
    }
    if (v > bv[0]) { bv[0] = v; bi[0] = c; }
}

// thread = one replicate (class counts, constant and K-list in registers); blockIdx.y = a SLICE of `per_slice` consecutive candidates,
// walked in chunks of SCORE_CHUNK whose class logs and no-value flags the block stages in LDS as llk_kernel does.  A slice walks its
// candidates in index order and takes a value only where it is strictly larger, so equal values stay in index order.  Each slice
// leaves its list in part_v / part_i [slice][K][n_rep] (the replicate innermost: coalesced here and in the merge).
template <bool UNFOLDED, int K>
__global__ __launch_bounds__(256)
void scan_best_kernel(int64_t n_cand, int64_t per_slice, const double* __restrict__ jafs, const int32_t* __restrict__ status,
                      int64_t n_rep, const double* __restrict__ jsfs, const double* __restrict__ consts,
                      double* __restrict__ part_v, int32_t* __restrict__ part_i) {
    __shared__ double lj[SCORE_CHUNK][8];
    const int64_t s0 = (int64_t)blockIdx.y * per_slice;
    const int64_t s1 = s0 + per_slice < n_cand ? s0 + per_slice : n_cand;
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const RowCounts<UNFOLDED> row(jsfs, consts, r < n_rep ? r : n_rep - 1);       // a lane beyond the table repeats the last row (never stored)
    double bv[K];
    int32_t bi[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { bv[j] = -INFINITY; bi[j] = -1; }
    for (int64_t c0 = s0; c0 < s1; c0 += SCORE_CHUNK) {
        const int nc = (int)(s1 - c0 < SCORE_CHUNK ? s1 - c0 : SCORE_CHUNK);
        __syncthreads();                              // the previous chunk has been walked by every wave
        stage_class_logs<UNFOLDED>(lj, nc, jafs, status, [&](int c) { return c0 + c; });
        __syncthreads();
        for (int c = 0; c < nc; ++c) {
            const double a = score(row, lj[c]);
            if (a > bv[K - 1]) best_insert<K>(bv, bi, a, (int32_t)(c0 + c));      // false for NaN and for -inf
        }
    }
    if (r >= n_rep) return;
    const int64_t base = (int64_t)blockIdx.y * K * n_rep + r;
#pragma unroll
    for (int j = 0; j < K; ++j) { part_v[base + j * n_rep] = bv[j]; part_i[base + j * n_rep] = bi[j]; }
}

// thread = one replicate: folds the slices' lists together in slice order (ascending candidate indices, so again a value is taken
// only where it is strictly larger) and writes the first k places as best[r][k] / best_llk[r][k]; no slice at all: -1 / -inf.
template <int K>
__global__ __launch_bounds__(256)
void scan_merge_kernel(int slices, int64_t n_rep, const double* __restrict__ part_v, const int32_t* __restrict__ part_i, int k,
                       int32_t* __restrict__ best, double* __restrict__ best_llk) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rep) return;
    double bv[K];
    int32_t bi[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { bv[j] = -INFINITY; bi[j] = -1; }
    for (int s = 0; s < slices; ++s) {
        const int64_t base = (int64_t)s * K * n_rep + r;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double v = part_v[base + j * n_rep];
            if (v > bv[K - 1]) best_insert<K>(bv, bi, v, part_i[base + j * n_rep]);
        }
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (j < k) {
            best[r * k + j] = bi[j];
            if (best_llk) best_llk[r * k + j] = bv[j];
        }
}

int scan_best_width(int k) { return k <= 1 ? 1 : (k <= 2 ? 2 : (k <= 4 ? 4 : 8)); }

// Slices of a scan: as many as give the chip about a thousand workgroups (four per compute unit) together with the replicate
// blocks - one when the replicates alone do - and no slice shorter than a quarter chunk (a slice's list costs a merge step).
int64_t scan_best_slices(int64_t n_cand, int64_t n_rep, const Tuning& tn) {
    if (n_cand <= 0 || n_rep <= 0) return 0;
    const int64_t rep_blocks = (n_rep + 255) / 256;
    int64_t slices = tn.scan_slices > 0 ? tn.scan_slices : (1024 + rep_blocks - 1) / rep_blocks;
    const int64_t most = tn.scan_slices > 0 ? n_cand : (n_cand + SCORE_CHUNK / 4 - 1) / (SCORE_CHUNK / 4);
    if (slices > most) slices = most;
    if (slices > 65535) slices = 65535;                                     // gridDim.y limit
    const int64_t per_slice = (n_cand + slices - 1) / slices;
    return (n_cand + per_slice - 1) / per_slice;                            // no empty slice behind the last candidate
}

template <int K>
static void launch_scan_best_t(int64_t n_cand, const double* jafs, const int32_t* status, int64_t n_rep, const double* jsfs, const double* consts,
                               int k, int32_t* best, double* best_llk, int64_t slices, double* part_v, int32_t* part_i, int unfolded, hipStream_t stream) {
    const unsigned rep_blocks = (unsigned)((n_rep + 255) / 256);
    if (slices > 0) {
        const int64_t per_slice = (n_cand + slices - 1) / slices;
        const dim3 grid(rep_blocks, (unsigned)slices);
        with_fold(unfolded, [&](auto U) { hipLaunchKernelGGL((scan_best_kernel<decltype(U)::value, K>), grid, dim3(256), 0, stream,
                                                             n_cand, per_slice, jafs, status, n_rep, jsfs, consts, part_v, part_i); });
    }
    hipLaunchKernelGGL(scan_merge_kernel<K>, dim3(rep_blocks), dim3(256), 0, stream, (int)slices, n_rep, part_v, part_i, k, best, best_llk);
}

hipError_t launch_scan_best(int64_t n_cand, const double* jafs, const int32_t* status, int64_t n_rep, const double* jsfs, const double* consts,
                            int k, int32_t* best, double* best_llk, int64_t slices, double* part_v, int32_t* part_i, int unfolded, hipStream_t stream) {
    if (n_rep <= 0) return hipSuccess;
    switch (scan_best_width(k)) {
        case 1: launch_scan_best_t<1>(n_cand, jafs, status, n_rep, jsfs, consts, k, best, best_llk, slices, part_v, part_i, unfolded, stream); break;
        case 2: launch_scan_best_t<2>(n_cand, jafs, status, n_rep, jsfs, consts, k, best, best_llk, slices, part_v, part_i, unfolded, stream); break;
        case 4: launch_scan_best_t<4>(n_cand, jafs, status, n_rep, jsfs, consts, k, best, best_llk, slices, part_v, part_i, unfolded, stream); break;
        default: launch_scan_best_t<8>(n_cand, jafs, status, n_rep, jsfs, consts, k, best, best_llk, slices, part_v, part_i, unfolded, stream); break;
    }
    return hipGetLastError();
}

// The PROFILE per group and replicate WITHOUT the table (misti_scan_profile_dev): every candidate carries a group label, and per
// (replicate, group) the best candidate of that group is kept - a segmented form of the scan above, llk_kernel's values again (the
// same expressions, the same bits).  Order: value descending, candidate index ascending on equal values, only v > -inf qualifies.
// Three small index kernels bucket the candidates by label on the device (no host synchronisation): a count per group, an
// exclusive scan over the groups, a scatter into a member list.  The scatter order inside a group is whatever order the atomics
// arrive in, so the reduction compares (value, index) pairs as a total order and never relies on the order of the walk.
// count[g] = members of group g; a label outside 0 ... n_group - 1 is in no group.
__global__ __launch_bounds__(256)
void profile_count_kernel(int64_t n_cand, const int32_t* __restrict__ group, int32_t n_group, int32_t* __restrict__ count) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cand) return;
    const int32_t g = group[c];
    if (g >= 0 && g < n_group) atomicAdd(&count[g], 1);
}

// One workgroup: first[0 ... n_group] = the exclusive scan of count[0 ... n_group), and count[g] = first[g] (the scatter's cursor).
// A thread sums a contiguous run of groups, the 256 run sums are scanned (block_exclusive_scan_256), then every thread walks its run again.
__global__ __launch_bounds__(256)
void profile_offsets_kernel(int32_t n_group, int32_t* __restrict__ count, int32_t* __restrict__ first) {
    __shared__ int32_t run[256];
    const int per = (n_group + 255) / 256;
    const int g0 = (int)threadIdx.x * per;
    const int g1 = g0 + per < n_group ? g0 + per : n_group;
    int32_t sum = 0;
    for (int g = g0; g < g1; ++g) sum += count[g];
    int32_t acc = block_exclusive_scan_256(run, sum);  // members of every group in front of this run
    for (int g = g0; g < g1; ++g) {
        const int32_t n = count[g];
        first[g] = acc;
        count[g] = acc;
        acc += n;
    }
    if (threadIdx.x == 255) first[n_group] = run[255];
}

// members[first[g] ... first[g + 1]) = the candidates of group g, in the order their atomics arrive.
__global__ __launch_bounds__(256)
void profile_scatter_kernel(int64_t n_cand, const int32_t* __restrict__ group, int32_t n_group, int32_t* __restrict__ cursor,
                            int32_t* __restrict__ members) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cand) return;
    const int32_t g = group[c];
    if (g >= 0 && g < n_group) members[atomicAdd(&cursor[g], 1)] = (int32_t)c;
}

// thread = one replicate (class counts, constant and ONE (best value, best index) pair in registers); blockIdx.y = a group,
// blockIdx.z = a SLICE of that group's member list (slice s of a list of n walks members s * per ... with per = ceil(n / slices)),
// walked in chunks of SCORE_CHUNK whose class logs, no-value flags and candidate indices the block gathers into LDS through the member
// list.  Each (slice, group) leaves its pair in part_v / part_i [slice][group][n_rep] (the replicate innermost: coalesced here and in
// the merge); a slice of an empty group, or beyond a short list, leaves -inf / -1.  Replicate blocks beyond gridDim.x are walked by
// the same workgroup (a launch never exceeds the grid limits however many rows there are).
template <bool UNFOLDED>
__global__ __launch_bounds__(256)
void scan_profile_kernel(int32_t n_group, const int32_t* __restrict__ first, const int32_t* __restrict__ members,
                         const double* __restrict__ jafs, const int32_t* __restrict__ status,
                         int64_t n_rep, const double* __restrict__ jsfs, const double* __restrict__ consts,
                         double* __restrict__ part_v, int32_t* __restrict__ part_i) {
    __shared__ double lj[SCORE_CHUNK][8];
    __shared__ int32_t lc[SCORE_CHUNK];               // the candidate's index
    const int32_t g = (int32_t)blockIdx.y;
    const int64_t m0 = first[g];
    const int64_t n_mem = first[g + 1] - m0;
    const int64_t per = (n_mem + gridDim.z - 1) / gridDim.z;
    const int64_t s0 = (int64_t)blockIdx.z * per < n_mem ? (int64_t)blockIdx.z * per : n_mem;
    const int64_t s1 = s0 + per < n_mem ? s0 + per : n_mem;
    const int64_t rep_blocks = (n_rep + 255) / 256;
    for (int64_t rb = blockIdx.x; rb < rep_blocks; rb += gridDim.x) {
        const int64_t r = rb * 256 + threadIdx.x;
        const RowCounts<UNFOLDED> row(jsfs, consts, r < n_rep ? r : n_rep - 1);       // a lane beyond the table repeats the last row (never stored)
        double bv = -INFINITY;
        int32_t bi = -1;
        for (int64_t c0 = s0; c0 < s1; c0 += SCORE_CHUNK) {
            const int nc = (int)(s1 - c0 < SCORE_CHUNK ? s1 - c0 : SCORE_CHUNK);
            __syncthreads();                          // the previous chunk has been walked by every wave
            stage_class_logs<UNFOLDED>(lj, nc, jafs, status, [&](int c) { return (int64_t)members[m0 + c0 + c]; }, lc);
            __syncthreads();
            for (int c = 0; c < nc; ++c) {
                const double a = score(row, lj[c]);
                const int32_t ci = lc[c];
                if (a > bv || (a == bv && ci < bi)) { bv = a; bi = ci; }      // false for NaN; -inf equals only the empty pair, whose -1 no index is below
            }
        }
        if (r < n_rep) {
            const int64_t at = ((int64_t)blockIdx.z * n_group + g) * n_rep + r;
            part_v[at] = bv;
            part_i[at] = bi;
        }
    }
}

// A tile of 32 replicates x 32 groups per pass: the slices' pairs are read with the replicate innermost and folded under the same
// total order, turned through LDS and written with the group innermost as prof_llk[n_rep][n_group] / prof_best (NULL: not wanted).
// No slice at all (no candidate): -inf / -1.  Tiles beyond the grid are walked by the same workgroup.
__global__ __launch_bounds__(256)
void profile_merge_kernel(int slices, int32_t n_group, int64_t n_rep, const double* __restrict__ part_v, const int32_t* __restrict__ part_i,
                          double* __restrict__ prof_llk, int32_t* __restrict__ prof_best) {
    __shared__ double tv[32][33];
    __shared__ int32_t ti[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;                  // 32 x 8
    const int64_t rep_tiles = (n_rep + 31) / 32;
    const int64_t g0 = (int64_t)blockIdx.y * 32;
    for (int64_t rt = blockIdx.x; rt < rep_tiles; rt += gridDim.x) {
        const int64_t r0 = rt * 32;
        __syncthreads();                              // the previous tile has been written out
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t g = g0 + ty + 8 * j, r = r0 + tx;
            double bv = -INFINITY;
            int32_t bi = -1;
            if (g < n_group && r < n_rep)
                for (int s = 0; s < slices; ++s) {
                    const int64_t at = ((int64_t)s * n_group + g) * n_rep + r;
                    const double v = part_v[at];
                    const int32_t ci = part_i[at];
                    if (v > bv || (v == bv && ci < bi)) { bv = v; bi = ci; }
                }
            tv[ty + 8 * j][tx] = bv;
            ti[ty + 8 * j][tx] = bi;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t g = g0 + tx, r = r0 + ty + 8 * j;
            if (g < n_group && r < n_rep) {
                prof_llk[r * n_group + g] = tv[tx][ty + 8 * j];
                if (prof_best) prof_best[r * n_group + g] = ti[tx][ty + 8 * j];
            }
        }
    }
}

// Slices of a profile: as many as give the chip about a thousand workgroups together with the replicate blocks and the groups - one
// when those alone do - and no slice shorter than a quarter chunk of the AVERAGE group (the groups' sizes are known on the device
// only; a slice beyond a short list costs one merge step).  MISTI_SCAN_SLICES forces the number as it does for the scan.
constexpr int64_t PROFILE_MOST_BLOCKS = (int64_t)1 << 22;                  // workgroups of one launch at most: 2^30 threads
int64_t scan_profile_slices(int64_t n_cand, int64_t n_group, int64_t n_rep, const Tuning& tn) {
    if (n_cand <= 0 || n_rep <= 0 || n_group <= 0) return 0;
    const int64_t blocks = (n_rep + 255) / 256 * n_group;
    int64_t slices = tn.scan_slices > 0 ? tn.scan_slices : (1024 + blocks - 1) / blocks;
    const int64_t average = (n_cand + n_group - 1) / n_group;
    const int64_t most = tn.scan_slices > 0 ? n_cand : (average + SCORE_CHUNK / 4 - 1) / (SCORE_CHUNK / 4);
    if (slices > most) slices = most;
    if (slices > 65535) slices = 65535;                                     // gridDim.z limit
    if (slices > PROFILE_MOST_BLOCKS / n_group) slices = PROFILE_MOST_BLOCKS / n_group;      // (groups x slices) fit one launch
    return slices;
}

// first [n_group + 1] | cursor [n_group] | members [n_cand]
size_t scan_profile_index_size(int64_t n_cand, int64_t n_group) { return 2 * (size_t)n_group + 1 + (size_t)n_cand; }

hipError_t launch_scan_profile(int64_t n_cand, const double* jafs, const int32_t* status, const int32_t* group, int32_t n_group,
                               int64_t n_rep, const double* jsfs, const double* consts, double* prof_llk, int32_t* prof_best,
                               int64_t slices, int32_t* index, double* part_v, int32_t* part_i, int unfolded, hipStream_t stream) {
    if (n_rep <= 0) return hipSuccess;
    if (slices > 0) {                                 // there are candidates, and `index` is a buffer: only here are addresses derived from it
        int32_t* first = index;
        int32_t* cursor = first + n_group + 1;
        int32_t* members = cursor + n_group;
        hipError_t e = hipMemsetAsync(cursor, 0, (size_t)n_group * sizeof(int32_t), stream);
        if (e != hipSuccess) return e;
        const dim3 cand_grid((unsigned)((n_cand + 255) / 256));
        hipLaunchKernelGGL(profile_count_kernel, cand_grid, dim3(256), 0, stream, n_cand, group, n_group, cursor);
        hipLaunchKernelGGL(profile_offsets_kernel, dim3(1), dim3(256), 0, stream, n_group, cursor, first);
        hipLaunchKernelGGL(profile_scatter_kernel, cand_grid, dim3(256), 0, stream, n_cand, group, n_group, cursor, members);
        const int64_t rep_blocks = (n_rep + 255) / 256, most = PROFILE_MOST_BLOCKS / ((int64_t)n_group * slices);
        const dim3 grid((unsigned)(rep_blocks < most ? rep_blocks : (most > 1 ? most : 1)), (unsigned)n_group, (unsigned)slices);
        with_fold(unfolded, [&](auto U) { hipLaunchKernelGGL(scan_profile_kernel<decltype(U)::value>, grid, dim3(256), 0, stream,
                                                             n_group, first, members, jafs, status, n_rep, jsfs, consts, part_v, part_i); });
    }
    const int64_t rep_tiles = (n_rep + 31) / 32, group_tiles = ((int64_t)n_group + 31) / 32, room = PROFILE_MOST_BLOCKS / group_tiles;
    hipLaunchKernelGGL(profile_merge_kernel, dim3((unsigned)(rep_tiles < room ? rep_tiles : room), (unsigned)group_tiles), dim3(256), 0, stream,
                       (int)slices, n_group, n_rep, part_v, part_i, prof_llk, prof_best);
    return hipGetLastError();
}

// One replicate per candidate (misti_nm_solve_rows: every start of the batched search has its own bootstrap row): thread = candidate,
// llk[c] = llk_of(row[c]) from log_class of its own spectrum.  Same expressions as llk_of / log_class (the inline epilogue of
// spectrum_kernel and llk_kernel): the same bits as the single-row search's values.  A candidate without a value (status != OK;
// empty slots carry row 0) reads no row.
__global__ __launch_bounds__(256)
void llk_rows_kernel(int64_t n, const double* __restrict__ jafs, const int32_t* __restrict__ status, const int32_t* __restrict__ row,
                     const double* __restrict__ jsfs, const double* __restrict__ consts, double* __restrict__ llk, int unfolded) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    if (status[c] != MISTI_OK) { llk[c] = -INFINITY; return; }
    const int64_t r = row[c];
    double lj[7];
    for (int i = 0; i < 7; ++i) lj[i] = log_class(jafs + c * 7, i, unfolded);
    llk[c] = llk_of(jsfs + r * 8, consts[r], lj, unfolded);
}

hipError_t launch_llk_rows(int64_t n, const double* jafs, const int32_t* status, const int32_t* row, const double* jsfs,
                           const double* consts, double* llk, int unfolded, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(llk_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, jafs, status, row, jsfs, consts, llk, unfolded);
    return hipGetLastError();
}

hipError_t launch_llk(int64_t n_cand, const double* jafs, const int32_t* status, int64_t n_rep, const double* jsfs,
                      const double* consts, double* llk, int unfolded, hipStream_t stream) {
    if (n_cand <= 0 || n_rep <= 0) return hipSuccess;
    // block = 512 replicates x `chunk` candidates: as large a chunk as still leaves the chip a few thousand blocks (a block's
    // set-up - the class logs of its chunk, the rows of its replicates - is paid once per chunk)
    const int64_t tiles = (n_rep + 511) / 512;
    int64_t chunk = n_cand * tiles / 4096;
    chunk = chunk < 4 ? 4 : (chunk > SCORE_CHUNK ? SCORE_CHUNK : chunk);
    const int64_t per_launch = 65535 * chunk;                               // gridDim.y limit
    for (int64_t c0 = 0; c0 < n_cand; c0 += per_launch) {
        const int64_t nc = n_cand - c0 < per_launch ? n_cand - c0 : per_launch;
        const dim3 grid((unsigned)tiles, (unsigned)((nc + chunk - 1) / chunk));
        with_fold(unfolded, [&](auto U) { hipLaunchKernelGGL(llk_kernel<decltype(U)::value>, grid, dim3(256), 0, stream, nc, (int)chunk,
                                                             jafs + c0 * 7, status ? status + c0 : nullptr, n_rep, jsfs, consts, llk + c0 * n_rep); });
    }
    return hipGetLastError();
}

// ------------------------------------------------------- curvature at a point --
// Hessians of the log-likelihood by central differences of L_k = log S_k over a fixed stencil (misti_curvature,
// misti_curvature_assemble_dev; the rule is optimize.curvature_stencil / optimize.curvature_from_spectra, operation for operation).
// A point has D parameters and M = 1 + 2 D^2 stencil candidates: 0 the centre, 1 + 2i / 2 + 2i the steps +h_i / -h_i, and for the
// q-th pair i < j (lexicographic) 1 + 2D + 4q + {0, 1, 2, 3} the steps (+,+), (+,-), (-,+), (-,-).
__host__ __device__ __forceinline__ int curv_pair_rank(int i, int j, int D) { return i * D - i * (i + 1) / 2 + (j - i - 1); }

// thread = point: h[p][i] = (x_i + max(rel |x_i|, abs)) - x_i, the step the doubles realise; a point with a step that leaves the positive half-line (x_i - h_i < 0), or with no
// step at all (h_i == 0: a rate of 0 under a purely relative step), has no two-sided stencil: MISTI_CURV_BOUNDARY.
__global__ __launch_bounds__(256)
void curv_steps_kernel(int64_t n_point, int D, const double* __restrict__ x, double rel_step, double abs_step,
                       double* __restrict__ h, int32_t* __restrict__ point_status) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_point) return;
    bool boundary = false;
    for (int i = 0; i < D; ++i) {
        const double xi = x[p * D + i];
        const double hi = (xi + fmax(rel_step * fabs(xi), abs_step)) - xi;    // the realised step: xi + hi and (for hi <= xi; else boundary) xi - hi are exact
        h[p * D + i] = hi;
        boundary = boundary || xi - hi < 0.0 || hi == 0.0;
    }
    point_status[p] = boundary ? MISTI_CURV_BOUNDARY : MISTI_OK;
}

// One workgroup: slot[p] = the number of points in front of p that have a stencil (their rank in the compacted candidate arrays),
// -1 for a boundary point.  A thread sums a contiguous run of points, the 256 run sums are scanned in LDS, then every thread walks
// its run again.
__global__ __launch_bounds__(256)
void curv_slots_kernel(int64_t n_point, const int32_t* __restrict__ point_status, int32_t* __restrict__ slot) {
    __shared__ int32_t run[256];
    const int64_t per = (n_point + 255) / 256;
    const int64_t p0 = (int64_t)threadIdx.x * per < n_point ? (int64_t)threadIdx.x * per : n_point;
    const int64_t p1 = p0 + per < n_point ? p0 + per : n_point;
    int32_t sum = 0;
    for (int64_t p = p0; p < p1; ++p) sum += point_status[p] == MISTI_OK ? 1 : 0;
    int32_t acc = block_exclusive_scan_256(run, sum);
    for (int64_t p = p0; p < p1; ++p) {
        const bool live = point_status[p] == MISTI_OK;
        slot[p] = live ? acc : -1;
        acc += live ? 1 : 0;
    }
}

// thread = (point, stencil index): candidate slot[p] * M + m of the compacted arrays gets the point's split, bounds and pulse times
// and its parameters moved by the stencil's steps.  A boundary point emits nothing; `cap` (the host's own count of points with a
// stencil) bounds every write.
__global__ __launch_bounds__(256)
void curv_stencil_kernel(int64_t n_point, int D, int M, const double* __restrict__ x, const double* __restrict__ split,
                         const int32_t* __restrict__ bounds, int nb2, const int32_t* __restrict__ pulses, int np,
                         const double* __restrict__ h, const int32_t* __restrict__ slot, int64_t cap,
                         double* __restrict__ c_split, double* __restrict__ c_params, int32_t* __restrict__ c_bounds,
                         int32_t* __restrict__ c_pulses) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_point * M) return;
    const int64_t p = t / M;
    const int m = (int)(t - p * M);
    const int64_t s = slot[p];
    if (s < 0 || s >= cap) return;
    // which coordinates move, and in which direction
    int a = -1, b = -1;
    double sa = 0.0, sb = 0.0;
    if (m >= 1 && m < 1 + 2 * D) { a = (m - 1) >> 1; sa = ((m - 1) & 1) ? -1.0 : 1.0; }
    else if (m >= 1 + 2 * D) {
        const int q = (m - 1 - 2 * D) >> 2, w = (m - 1 - 2 * D) & 3;
        int i = 0, left = q;
        while (left >= D - 1 - i) { left -= D - 1 - i; ++i; }
        a = i; b = i + 1 + left;
        sa = (w & 2) ? -1.0 : 1.0;
        sb = (w & 1) ? -1.0 : 1.0;
    }
    const int64_t c = s * M + m;
    c_split[c] = split[p];
    for (int i = 0; i < D; ++i) {
        const double xi = x[p * D + i], hi = h[p * D + i];
        double v = xi;
        if (i == a) v = sa > 0.0 ? xi + hi : xi - hi;
        if (i == b) v = sb > 0.0 ? xi + hi : xi - hi;
        c_params[c * D + i] = v;
    }
    for (int i = 0; i < nb2; ++i) c_bounds[c * nb2 + i] = bounds[p * nb2 + i];
    for (int i = 0; i < np; ++i) c_pulses[c * np + i] = pulses[p * np + i];
}

// One wave per point (workgroup = one wave; points beyond the grid are walked by the same wave).  The wave reads the point's M
// spectra - contiguous, lanes over (candidate, class) - and leaves the logs of the K class values in LDS (K = 4 folded, 7 unfolded;
// log_class's expression); a candidate without a value (status != 0, or a class value that is not positive and finite) makes the
// point fail with the status of the FIRST such candidate in stencil order (MISTI_NUMERIC where that candidate's status was 0).  Then
// lanes over (i, k) write dlog[p][i][k] and lanes over (i, j >= i, k) write d2log[p][i][j][k] and d2log[p][j][i][k] from one value.
// Entries K ... 6 are 0; every output of a failed point is NaN.  slot (may be NULL: point p's spectra are rows p M ... of jafs)
// names the point's place in compacted arrays, -1 where it has none: its status is then pre_status[p] (MISTI_CURV_BOUNDARY).
// dlog / d2log may be NULL (not wanted).  LDS: M x K doubles.
__global__ __launch_bounds__(64)
void curv_assemble_kernel(int64_t n_point, int D, int M, int unfolded, const double* __restrict__ jafs, const int32_t* __restrict__ status,
                          const double* __restrict__ h, const int32_t* __restrict__ slot, const int32_t* __restrict__ pre_status,
                          double* __restrict__ dlog, double* __restrict__ d2log, int32_t* __restrict__ point_status) {
    extern __shared__ double curv_L[];
    const int K = unfolded ? 7 : 4;
    const int lane = threadIdx.x;
    for (int64_t p = blockIdx.x; p < n_point; p += gridDim.x) {
        const int64_t s = slot ? (int64_t)slot[p] : p;
        int st = MISTI_OK;
        __syncthreads();                              // the previous point's logs have been read by every lane
        if (s < 0) st = pre_status[p];
        else {
            const double* J = jafs + s * M * 7;
            const int32_t* cs = status ? status + s * M : nullptr;
            int first = INT_MAX;                      // the first candidate without a value this lane has seen
            for (int idx = lane; idx < M * K; idx += 64) {
                const int m = idx / K, k = idx - m * K;
                const double S = class_value(J + m * 7, k, unfolded);
                const bool ok = S > 0.0 && isfinite(S) && !(cs && cs[m] != MISTI_OK);
                if (!ok && m < first) first = m;
                curv_L[idx] = log(S);
            }
            for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(first, d, 64); first = o < first ? o : first; }
            if (first != INT_MAX) st = (cs && cs[first] != MISTI_OK) ? cs[first] : MISTI_NUMERIC;
        }
        __syncthreads();
        if (lane == 0) point_status[p] = st;
        const double* hp = h + p * D;
        if (dlog) {
            double* out = dlog + p * D * 7;
            for (int idx = lane; idx < D * 7; idx += 64) {
                const int i = idx / 7, k = idx - i * 7;
                double v = 0.0;
                if (st != MISTI_OK) v = NAN;
                else if (k < K) v = (curv_L[(1 + 2 * i) * K + k] - curv_L[(2 + 2 * i) * K + k]) / (2.0 * hp[i]);
                out[idx] = v;
            }
        }
        if (d2log) {
            double* out = d2log + p * D * D * 7;
            for (int idx = lane; idx < D * D * 7; idx += 64) {
                const int ij = idx / 7, k = idx - ij * 7;
                const int i = ij / D, j = ij - i * D;
                if (j < i) continue;                  // written by the lane that has (j, i)
                double v = 0.0;
                if (st != MISTI_OK) v = NAN;
                else if (k < K) {
                    if (i == j) {
                        const double lp = curv_L[(1 + 2 * i) * K + k], l0 = curv_L[k], lm = curv_L[(2 + 2 * i) * K + k];
                        v = ((lp - 2.0 * l0) + lm) / (hp[i] * hp[i]);
                    } else {
                        const int c = 1 + 2 * D + 4 * curv_pair_rank(i, j, D);
                        const double lpp = curv_L[c * K + k], lpm = curv_L[(c + 1) * K + k], lmp = curv_L[(c + 2) * K + k], lmm = curv_L[(c + 3) * K + k];
                        v = (((lpp - lpm) - lmp) + lmm) / ((4.0 * hp[i]) * hp[j]);
                    }
                }
                out[(i * D + j) * 7 + k] = v;
                out[(j * D + i) * 7 + k] = v;
            }
        }
    }
}

// thread = one entry of (grad[p][D], hess[p][D][D]): the sum over the classes, ascending, of the row's class counts - formed as the
// replicate epilogue forms them (llk_of) - times dlog / d2log; products and sums are rounded one by one (no fused multiply-add: the
// rule in optimize.curvature_contract is written without one).  NaN for a point without a value.  With llh0 given the thread of
// entry 0 also writes the log-likelihood of the point's centre against its row: llk_rows_kernel's expressions (the same bits as
// misti_eval_batch's), NaN for a point without a value.
__global__ __launch_bounds__(256)
void curv_contract_kernel(int64_t n_point, int D, int unfolded, const double* __restrict__ dlog, const double* __restrict__ d2log,
                          const int32_t* __restrict__ point_status, const int32_t* __restrict__ row, const double* __restrict__ jsfs,
                          double* __restrict__ grad, double* __restrict__ hess,
                          const double* __restrict__ jafs, const int32_t* __restrict__ slot, int M, const double* __restrict__ consts,
                          double* __restrict__ llh0) {
    const int E = D + D * D;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_point * E) return;
    const int64_t p = t / E;
    const int e = (int)(t - p * E);
    const bool ok = point_status[p] == MISTI_OK;
    double f[7];
    const int K = unfolded ? 7 : 4;
    if (unfolded) row_counts<true>(jsfs + (int64_t)row[p] * 8, f); else row_counts<false>(jsfs + (int64_t)row[p] * 8, f);
    const double* v = e < D ? dlog + (p * D + e) * 7 : d2log + (p * D * D + (e - D)) * 7;
    double acc = 0.0;
    for (int k = 0; k < K; ++k) acc = __dadd_rn(acc, __dmul_rn(f[k], v[k]));
    if (!ok) acc = NAN;
    if (e < D) grad[p * D + e] = acc;
    else hess[p * D * D + (e - D)] = acc;
    if (e == 0 && llh0) {
        double l = NAN;
        if (ok) {
            const double* J = jafs + (int64_t)slot[p] * M * 7;
            double lj[7];
            for (int i = 0; i < 7; ++i) lj[i] = log_class(J, i, unfolded);
            l = llk_of(jsfs + (int64_t)row[p] * 8, consts[row[p]], lj, unfolded);
        }
        llh0[p] = l;
    }
}

hipError_t launch_curv_stencil(int64_t n_point, int D, const double* x, const double* split, const int32_t* bounds, int nb2,
                               const int32_t* pulses, int np, double rel_step, double abs_step, int64_t cap, double* h, int32_t* point_status,
                               int32_t* slot, double* c_split, double* c_params, int32_t* c_bounds, int32_t* c_pulses, hipStream_t stream) {
    if (n_point <= 0) return hipSuccess;
    const int M = 1 + 2 * D * D;
    hipLaunchKernelGGL(curv_steps_kernel, dim3((unsigned)((n_point + 255) / 256)), dim3(256), 0, stream, n_point, D, x, rel_step, abs_step, h, point_status);
    hipLaunchKernelGGL(curv_slots_kernel, dim3(1), dim3(256), 0, stream, n_point, point_status, slot);
    if (cap > 0)
        hipLaunchKernelGGL(curv_stencil_kernel, dim3((unsigned)((n_point * M + 255) / 256)), dim3(256), 0, stream, n_point, D, M, x, split, bounds, nb2,
                           pulses, np, h, slot, cap, c_split, c_params, c_bounds, c_pulses);
    return hipGetLastError();
}

hipError_t launch_curv_assemble(int64_t n_point, int D, int unfolded, const double* jafs, const int32_t* status, const double* h,
                                const int32_t* slot, const int32_t* pre_status, double* dlog, double* d2log, int32_t* point_status,
                                hipStream_t stream) {
    if (n_point <= 0) return hipSuccess;
    const int M = 1 + 2 * D * D;
    const size_t lds = (size_t)M * (unfolded ? 7 : 4) * sizeof(double);           // at most 513 x 7 doubles (D = MISTI_MAX_PARAMS): 28 KB
    const int64_t blocks = n_point < 65536 ? n_point : 65536;
    hipLaunchKernelGGL(curv_assemble_kernel, dim3((unsigned)blocks), dim3(64), lds, stream, n_point, D, M, unfolded, jafs, status, h, slot, pre_status,
                       dlog, d2log, point_status);
    return hipGetLastError();
}

hipError_t launch_curv_contract(int64_t n_point, int D, int unfolded, const double* dlog, const double* d2log, const int32_t* point_status,
                                const int32_t* row, const double* jsfs, double* grad, double* hess, const double* jafs, const int32_t* slot,
                                const double* consts, double* llh0, hipStream_t stream) {
    if (n_point <= 0) return hipSuccess;
    const int64_t threads = n_point * (D + D * D);
    hipLaunchKernelGGL(curv_contract_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, n_point, D, unfolded, dlog, d2log,
                       point_status, row, jsfs, grad, hess, jafs, slot, 1 + 2 * D * D, consts, llh0);
    return hipGetLastError();
}

}  // namespace misti
