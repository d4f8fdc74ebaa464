// The replicate scoring, each piece written once, for misti_kernels.hip (setup_kernel, the inline epilogue of spectrum_kernel) and
// misti_score.hip: every path that scores a spectrum against a replicate row evaluates the same expressions in the same order - the same bits.
#pragma once
#include <type_traits>

#include "misti_device.h"

namespace misti {

// The class counts of one replicate row (row[0] is the row's total, the seven counts follow): all seven, or folded the sums 0+6, 1+5, 2+4, 3.
template <bool UNFOLDED> __device__ __forceinline__ void row_counts(const double* __restrict__ row, double* f) {
    const double* d = row + 1;
    if (UNFOLDED) { for (int i = 0; i < 7; ++i) f[i] = d[i]; }
    else { f[0] = d[0] + d[6]; f[1] = d[1] + d[5]; f[2] = d[2] + d[4]; f[3] = d[3]; }
}
// Row r of a table as a kernel that walks candidates keeps it in registers: the class counts and the row's constant.
template <bool UNFOLDED> struct RowCounts {
    static constexpr int NF = UNFOLDED ? 7 : 4;
    double f[NF], cst;
    __device__ __forceinline__ RowCounts(const double* __restrict__ jsfs, const double* __restrict__ consts, int64_t r) : cst(consts[r]) { row_counts<UNFOLDED>(jsfs + r * 8, f); }
};

// llh_const of SetJAFS (MigrationInference.py:217-227) for one replicate
__device__ __forceinline__ double llh_const_of(const double* __restrict__ row, int unfolded) {
    const double* d = row + 1;
    double snps = 0.0;
    for (int i = 0; i < 7; ++i) snps += d[i];
    double c = lgamma(snps + 1.0);
    if (unfolded) { for (int i = 0; i < 7; ++i) c -= lgamma(d[i] + 1.0); }
    else {
        double f[4];
        row_counts<false>(row, f);
        c -= lgamma(f[0] + 1.0);
        c -= lgamma(f[1] + 1.0);
        c -= lgamma(f[2] + 1.0);
        c -= lgamma(f[3] + 1.0);
    }
    return c;
}

// Class k of a spectrum (folded: classes 0+6, 1+5, 2+4, 3; k > 3 is no class) and its log.
__device__ __forceinline__ double class_value(const double* J, int k, int unfolded) { return (unfolded || k == 3) ? J[k] : J[k] + J[6 - k]; }
__device__ __forceinline__ double log_class(const double* J, int k, int unfolded) { return (unfolded || k <= 3) ? log(class_value(J, k, unfolded)) : 0.0; }

// Multinomial log-likelihood of one replicate (MigrationInference.py:600-609) from the logs of the spectrum classes.  The epilogue of the
// spectrum kernel calls this one: the body is the one written there (row_counts' sums restated), which keeps that kernel's instructions.
__device__ __forceinline__ double llk_of(const double* __restrict__ row, double cst, const double* lj, int unfolded) {
    const double* d = row + 1;
    double a = cst;
    if (unfolded) { for (int i = 0; i < 7; ++i) a = fma(d[i], lj[i], a); }
    else {
        a = fma(d[0] + d[6], lj[0], a);
        a = fma(d[1] + d[5], lj[1], a);
        a = fma(d[2] + d[4], lj[2], a);
        a = fma(d[3], lj[3], a);
    }
    return a;
}

// Whether a candidate of this status has a value: the one predicate of every path that scores a spectrum or draws from one.
__host__ __device__ __forceinline__ bool status_has_value(int32_t st) { return st == MISTI_OK; }

// A chunk of at most SCORE_CHUNK candidates staged in LDS for the kernels that walk candidates per row: lj[c][0..6] = the class logs of
// the chunk's c-th candidate, lj[c][7] = 1.0 where it has no value (status != OK), else 0.0.  The block fills lj[0 .. nc): cand_of(c) is
// the candidate's index in jafs / status, also left in lc[c] where lc is given.
constexpr int SCORE_CHUNK = 64;
template <bool UNFOLDED, class CandOf> __device__ __forceinline__
void stage_class_logs(double (*lj)[8], int nc, const double* __restrict__ jafs, const int32_t* __restrict__ status, CandOf cand_of, int32_t* lc = nullptr) {
    for (int i = threadIdx.x; i < nc * 8; i += blockDim.x) {
        const int c = i >> 3, k = i & 7;
        const int64_t cand = cand_of(c);
        double v;
        if (k < 7) v = log_class(jafs + cand * 7, k, UNFOLDED ? 1 : 0);
        else { v = (status && !status_has_value(status[cand])) ? 1.0 : 0.0; if (lc) lc[c] = (int32_t)cand; }
        lj[c][k] = v;
    }
}
// The value of a staged candidate for a row - llk_of's chain on the row's counts - and -inf where the candidate has none.
template <bool UNFOLDED> __device__ __forceinline__ double score(const RowCounts<UNFOLDED>& row, const double* lj_c) {
    double a = row.cst;
#pragma unroll
    for (int i = 0; i < row.NF; ++i) a = fma(row.f[i], lj_c[i], a);
    return lj_c[7] != 0.0 ? -INFINITY : a;
}

// Exclusive scan over the 256 threads of a workgroup through run[256] (LDS): the sum of `sum` over the threads in front of this one; run[255] = the total.
__device__ __forceinline__ int32_t block_exclusive_scan_256(int32_t* run, int32_t sum) {
    run[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int32_t below = (int)threadIdx.x >= d ? run[threadIdx.x - d] : 0;
        __syncthreads();
        run[threadIdx.x] += below;
        __syncthreads();
    }
    return run[threadIdx.x] - sum;
}

// Host: f(std::true_type) for unfolded data, f(std::false_type) for folded - the launch of a kernel templated on the fold.
template <class F> static inline void with_fold(int unfolded, F f) { if (unfolded) f(std::true_type{}); else f(std::false_type{}); }

}  // namespace misti
