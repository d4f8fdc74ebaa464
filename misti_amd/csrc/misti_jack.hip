// Delete-m block jackknife on the device (include/misti_hip.h, "block jackknife"): the leave-out rows of a chunked JSFS, one group per
// lane.  The rule is optimize.jackknife_rows, restated here operation for operation: row g is the chunks OUTSIDE group g added in
// chunk order from zero, one float64 addition per column per chunk - the same bits.  Nothing is drawn: there is no stream and no seed.
// The reference has no counterpart (its confidence statement is the bootstrap's t-interval, test.bs/bs_conf_int.ipynb).
#include <hip/hip_runtime.h>

#include "misti_boot.h"
#include "misti_ctx.h"

namespace misti {

// The tile: 1 024 chunk rows of 64 B = 64 KiB of the compute unit's 160 KiB LDS, so two workgroups fit a compute unit (a table of
// fewer rows asks for its own size only).  ONE tile is staged per pair of barriers: the 1 024 x 8 predicated additions a lane makes per
// tile dwarf the two barriers and the 32 doubles each lane copies, so a second buffer would buy nothing but occupancy lost.  Tables
// beyond one tile walk the tiles in chunk order - the additions of a row are the same ones in the same order whatever the tile.
constexpr int JACK_TILE_CHUNKS = 1024;
constexpr int JACK_THREADS = 256;

// lane = group first_group + r, which leaves out chunks lo ... hi - 1 (lo = g m, hi = min(lo + m, n_chunk)).  Every lane of the
// workgroup walks ALL chunks in chunk order and adds the chunk's 8 columns unless the chunk is its own: at step i every lane reads the
// same 64 B of LDS - a broadcast, no bank conflict - where the bootstrap's lanes gather 64 different rows.  A lane beyond n_group
// stages and waits at the barriers like the others (lo = hi = 0: it adds everything) and writes nothing.  The loop is bounded by
// n_chunk <= MISTI_BOOT_MAX_CHUNKS; g m < 2^32 fits the 64-bit product with room.
__global__ __launch_bounds__(JACK_THREADS)
void jackknife_rows_kernel(int n_chunk, const double* __restrict__ chunks, int m, int64_t first_group, int64_t n_group, double* __restrict__ rows) {
    extern __shared__ __align__(16) double jack_tab[];
    const int64_t r = (int64_t)blockIdx.x * JACK_THREADS + threadIdx.x;
    const bool live = r < n_group;
    int lo = 0, hi = 0;
    if (live) {
        const int64_t start = (first_group + r) * (int64_t)m, end = start + m;
        lo = (int)start;
        hi = (int)(end < n_chunk ? end : n_chunk);
    }
    double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int t0 = 0; t0 < n_chunk; t0 += JACK_TILE_CHUNKS) {
        const int nt = n_chunk - t0 < JACK_TILE_CHUNKS ? n_chunk - t0 : JACK_TILE_CHUNKS;
        if (t0) __syncthreads();                      // every lane is done with the tile before
        for (int i = threadIdx.x; i < nt * 8; i += JACK_THREADS) jack_tab[i] = chunks[t0 * 8 + i];
        __syncthreads();
        for (int i = 0; i < nt; ++i) {
            const int c = t0 + i;
            if (c < lo || c >= hi) {                  // a chunk of the lane's own group is skipped - not added as zero
                const double* row = jack_tab + i * 8;
#pragma unroll
                for (int k = 0; k < 8; ++k) s[k] += row[k];
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int k = 0; k < 8; ++k) rows[r * 8 + k] = s[k];
}

}  // namespace misti

using namespace misti_host;

namespace {

// What both entry points say about (n_chunk, m): 0 and *G = ceil(n_chunk / m), or the code.
int check_groups(int64_t n_chunk, int64_t m, int64_t* G) {
    if (n_chunk < 2) return fail(MISTI_E_ARG, "n_chunk must be at least 2 (got %lld): one chunk leaves nothing behind", (long long)n_chunk);
    if (m < 1) return fail(MISTI_E_ARG, "m must be at least 1 (got %lld)", (long long)m);
    if (m >= n_chunk) return fail(MISTI_E_ARG, "m = %lld of n_chunk = %lld: a single group would leave nothing behind", (long long)m, (long long)n_chunk);
    if (n_chunk > MISTI_BOOT_MAX_CHUNKS) return fail(MISTI_E_LIMIT, "n_chunk beyond MISTI_BOOT_MAX_CHUNKS = %d (got %lld)", (int)MISTI_BOOT_MAX_CHUNKS, (long long)n_chunk);
    *G = (n_chunk + m - 1) / m;
    return 0;
}

}  // namespace

extern "C" {

int misti_jackknife_rows_dev(misti_ctx* ctx, int64_t n_chunk, const double* chunks, int64_t m, int64_t first_group, int64_t n_group, uint32_t flags,
                             double* d_rows) {
    // everything that can be said about the arguments is said before the context is looked at
    int64_t G = 0;
    if (int r = check_groups(n_chunk, m, &G)) return r;
    if (n_group < 0 || first_group < 0) return fail(MISTI_E_ARG, "negative n_group or first_group");
    if (first_group > G || n_group > G - first_group)
        return fail(MISTI_E_ARG, "groups %lld ... %lld of G = %lld", (long long)first_group, (long long)first_group + (long long)n_group - 1, (long long)G);
    if (flags) return fail(MISTI_E_ARG, "unknown flag bits 0x%x", (unsigned)flags);
    if (n_group > 0 && (!chunks || !d_rows)) return fail(MISTI_E_ARG, "chunks / rows is NULL");
    if (chunks) {
        double genome = 0.0, seg = 0.0, shortest = 0.0;   // (the bootstrap's draw limit has no meaning here: nothing is drawn)
        if (int r = chunk_entries(n_chunk, chunks, &genome, &seg, &shortest)) return r;   // (with the bootstrap's messages)
    }
    if (!ctx) return fail(MISTI_E_ARG, "ctx is NULL");
    if (n_group == 0) return 0;
    const size_t bytes = (size_t)n_chunk * 8 * sizeof(double);
    if (int r = upload_chunks(ctx, bytes, chunks)) return r;
    const int64_t tile = n_chunk < misti::JACK_TILE_CHUNKS ? n_chunk : misti::JACK_TILE_CHUNKS;
    const dim3 grid((unsigned)((n_group + misti::JACK_THREADS - 1) / misti::JACK_THREADS)), block(misti::JACK_THREADS);
    hipLaunchKernelGGL(misti::jackknife_rows_kernel, grid, block, (size_t)tile * 8 * sizeof(double), ctx->stream, (int)n_chunk,
                       ctx->boot_chunks.as<const double>(), (int)m, first_group, n_group, d_rows);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MISTI_E_HIP, "jackknife_rows_kernel: %s", hipGetErrorString(e));
    return 0;
}

int misti_jackknife_geometry(int64_t n_chunk, int64_t m, int64_t* n_group) {
    int64_t G = 0;
    if (int r = check_groups(n_chunk, m, &G)) return r;
    if (!n_group) return fail(MISTI_E_ARG, "n_group is NULL");
    *n_group = G;
    return 0;
}

}  // extern "C"
