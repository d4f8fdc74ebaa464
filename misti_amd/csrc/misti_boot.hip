// Block bootstrap on the device (include/misti_hip.h, "block bootstrap"): replicate rows of a chunked JSFS, one replicate per lane.
// The rule is optimize.block_bootstrap, restated here operation for operation: the same draws (misti_boot.h), the same float64
// additions in the same order - the same bits.  The reference's counterpart is migrationIO.BootstrapJAFS
// (migrationIO.py:506-524) once per replicate under Python's Mersenne Twister, a sequential stream; the stream here
// is the project's own, counter-based: replicate r is a function of (seed, r) and of nothing else.
#include <hip/hip_runtime.h>

#include <cmath>

#include "misti_boot.h"
#include "misti_ctx.h"

namespace misti {

// Chunk tables up to this many rows are staged in LDS (64 B a row: 64 KiB, two workgroups per compute unit); beyond it every draw
// reads its row from global memory (4 MiB at MISTI_BOOT_MAX_CHUNKS: the table stays in L2).
constexpr int BOOT_STAGED_MAX_CHUNKS = 1024;

// lane = replicate first_rep + r.  While the row's total is below the genome length: draw a chunk, add its 8 columns - each column in
// draw order, one addition per draw.  One Philox block serves four draws; a lane that needs fewer leaves the rest unused (draw j is
// element j of the replicate's stream whatever the lane's neighbours do).  Lanes of a wave end after different numbers of draws:
// behind the staging barrier nothing is shared, a finished lane just idles until its wave ends.  The loop is bounded by max_draws
// (the host's MISTI_BOOT_MAX_DRAWS) besides: a table that passed the host's checks never gets there.
template <bool STAGED> __global__ __launch_bounds__(256)
void bootstrap_rows_kernel(int n_chunk, const double* __restrict__ chunks, double genome, double seg, uint64_t seed, int64_t first_rep,
                           int64_t n_rep, int normalize, int max_draws, double* __restrict__ rows, int32_t* __restrict__ draws) {
    extern __shared__ double boot_tab[];
    if (STAGED) {
        for (int i = threadIdx.x; i < n_chunk * 8; i += blockDim.x) boot_tab[i] = chunks[i];
        __syncthreads();
    }
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rep) return;
    const double* tab = STAGED ? boot_tab : chunks;
    const uint64_t rep = (uint64_t)(first_rep + r);
    double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int n = 0;
    for (uint64_t block = 0; s[0] < genome && n < max_draws; ++block) {
        uint64_t raw[4];
        philox4x64_10_block(seed, rep, block, raw);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (s[0] < genome && n < max_draws) {
                const double* row = tab + boot_index(raw[j], n_chunk) * 8;
#pragma unroll
                for (int k = 0; k < 8; ++k) s[k] += row[k];
                ++n;
            }
        }
    }
    if (normalize) {                                  // the reference's normalize=True: every entry times seg / seg_bs - the division first
        const double seg_bs = (((((s[1] + s[2]) + s[3]) + s[4]) + s[5]) + s[6]) + s[7];
        const double scale = seg / seg_bs;
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] = s[k] * scale;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) rows[r * 8 + k] = s[k];
    if (draws) draws[r] = n;
}

}  // namespace misti

using namespace misti_host;

int misti_host::chunk_entries(int64_t n_chunk, const double* chunks, double* genome, double* seg, double* shortest_out) {
    double g = 0.0, sg = 0.0, shortest = INFINITY;
    for (int64_t i = 0; i < n_chunk; ++i) {
        const double* c = chunks + i * 8;
        for (int k = 0; k < 8; ++k)
            if (!std::isfinite(c[k])) return fail(MISTI_E_ARG, "chunks[%lld][%d] is not finite", (long long)i, k);
        if (!(c[0] > 0.0)) return fail(MISTI_E_ARG, "chunks[%lld][0] = %g: a chunk's length must be > 0", (long long)i, c[0]);
        for (int k = 1; k < 8; ++k)
            if (c[k] < 0.0) return fail(MISTI_E_ARG, "chunks[%lld][%d] = %g: a count must not be negative", (long long)i, k, c[k]);
        g += c[0];
        sg += (((((c[1] + c[2]) + c[3]) + c[4]) + c[5]) + c[6]) + c[7];
        shortest = c[0] < shortest ? c[0] : shortest;
    }
    if (!std::isfinite(g) || !std::isfinite(sg)) return fail(MISTI_E_ARG, "the chunk lengths or counts do not sum to a finite number");
    *genome = g;
    *seg = sg;
    *shortest_out = shortest;
    return 0;
}

// A table that grows frees the old buffer, which waits for the device: no kernel of an earlier call still reads it.
int misti_host::upload_chunks(misti_ctx* c, size_t bytes, const double* chunks) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->boot_chunks.reserve(bytes));
    // (the caller's table is pageable host memory: the runtime has taken its bytes when this returns)
    hipError_t e = hipMemcpyAsync(c->boot_chunks.p, chunks, bytes, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return fail(MISTI_E_HIP, "hipMemcpyAsync of the chunk table: %s", hipGetErrorString(e));
    return 0;
}

namespace {

// What a chunk table must be for the loop to end, and the two sums of the rule: genome = the lengths added in chunk order, seg = the
// running sum over the chunks of ((c1 + c2) + ... + c7).
int check_chunks(int64_t n_chunk, const double* chunks, double* genome, double* seg) {
    double shortest = INFINITY;
    if (int r = chunk_entries(n_chunk, chunks, genome, seg, &shortest)) return r;
    const double g = *genome;
    // the most draws a replicate can need; the comparison is made in floating point, where an infinite quotient is simply too large
    if (!(std::ceil(g / shortest) <= (double)MISTI_BOOT_MAX_DRAWS))
        return fail(MISTI_E_LIMIT, "a replicate may need ceil(%g / %g) draws, beyond MISTI_BOOT_MAX_DRAWS = %d", g, shortest, (int)MISTI_BOOT_MAX_DRAWS);
    return 0;
}

}  // namespace

extern "C" {

int misti_bootstrap_rows_dev(misti_ctx* ctx, int64_t n_chunk, const double* chunks, uint64_t seed, int64_t first_rep, int64_t n_rep, uint32_t flags,
                             double* d_rows, int32_t* d_draws) {
    // everything that can be said about the arguments is said before the context is looked at
    if (n_chunk < 1) return fail(MISTI_E_ARG, "n_chunk must be at least 1 (got %lld)", (long long)n_chunk);
    if (n_rep < 0 || first_rep < 0) return fail(MISTI_E_ARG, "negative n_rep or first_rep");
    if (flags & ~MISTI_BOOT_NORMALIZE) return fail(MISTI_E_ARG, "unknown flag bits 0x%x", (unsigned)(flags & ~MISTI_BOOT_NORMALIZE));
    if (n_chunk > MISTI_BOOT_MAX_CHUNKS) return fail(MISTI_E_LIMIT, "n_chunk beyond MISTI_BOOT_MAX_CHUNKS = %d (got %lld)", (int)MISTI_BOOT_MAX_CHUNKS, (long long)n_chunk);
    if (n_rep > INT32_MAX || first_rep > INT64_MAX - n_rep) return fail(MISTI_E_LIMIT, "too many replicates for one call");
    if (n_rep > 0 && (!chunks || !d_rows)) return fail(MISTI_E_ARG, "chunks / rows is NULL");
    double genome = 0.0, seg = 0.0;
    if (chunks)
        if (int r = check_chunks(n_chunk, chunks, &genome, &seg)) return r;
    if (!ctx) return fail(MISTI_E_ARG, "ctx is NULL");
    if (n_rep == 0) return 0;
    const size_t bytes = (size_t)n_chunk * 8 * sizeof(double);
    if (int r = upload_chunks(ctx, bytes, chunks)) return r;
    hipStream_t s = ctx->stream;
    const double* d_chunks = ctx->boot_chunks.as<double>();
    const dim3 grid((unsigned)((n_rep + 255) / 256)), block(256);
    const int normalize = (flags & MISTI_BOOT_NORMALIZE) ? 1 : 0;
    if (n_chunk <= misti::BOOT_STAGED_MAX_CHUNKS)
        hipLaunchKernelGGL(misti::bootstrap_rows_kernel<true>, grid, block, bytes, s, (int)n_chunk, d_chunks, genome, seg, seed,
                           first_rep, n_rep, normalize, (int)MISTI_BOOT_MAX_DRAWS, d_rows, d_draws);
    else
        hipLaunchKernelGGL(misti::bootstrap_rows_kernel<false>, grid, block, 0, s, (int)n_chunk, d_chunks, genome, seg, seed,
                           first_rep, n_rep, normalize, (int)MISTI_BOOT_MAX_DRAWS, d_rows, d_draws);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MISTI_E_HIP, "bootstrap_rows_kernel: %s", hipGetErrorString(e));
    return 0;
}

int misti_bootstrap_draws(uint64_t seed, int64_t rep, int64_t n_chunk, int64_t n, int64_t* idx) {
    if (rep < 0 || n < 0) return fail(MISTI_E_ARG, "negative rep or n");
    if (n_chunk < 1) return fail(MISTI_E_ARG, "n_chunk must be at least 1 (got %lld)", (long long)n_chunk);
    if (n_chunk > MISTI_BOOT_MAX_CHUNKS) return fail(MISTI_E_LIMIT, "n_chunk beyond MISTI_BOOT_MAX_CHUNKS = %d (got %lld)", (int)MISTI_BOOT_MAX_CHUNKS, (long long)n_chunk);
    if (n > MISTI_BOOT_MAX_DRAWS) return fail(MISTI_E_LIMIT, "n beyond MISTI_BOOT_MAX_DRAWS = %d (got %lld)", (int)MISTI_BOOT_MAX_DRAWS, (long long)n);
    if (n > 0 && !idx) return fail(MISTI_E_ARG, "idx is NULL");
    for (int64_t j = 0; j < n; j += 4) {
        uint64_t raw[4];
        misti::philox4x64_10_block(seed, (uint64_t)rep, (uint64_t)(j >> 2), raw);
        for (int k = 0; k < 4 && j + k < n; ++k) idx[j + k] = misti::boot_index(raw[k], n_chunk);
    }
    return 0;
}

}  // extern "C"
