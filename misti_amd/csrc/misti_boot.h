// The generator of the block bootstrap (misti_bootstrap_rows_dev, misti_bootstrap_draws; the rule is optimize.philox_draws /
// optimize.block_bootstrap, operation for operation): Philox4x64-10 as numpy.random.Philox(key=[seed, rep]) runs it, and the
// index rule.  Host and device call the same functions: what the CPU suite checks through misti_bootstrap_draws is what the kernel draws.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace misti {

// 64 x 64 -> the high 64 bits of the 128-bit product
__host__ __device__ __forceinline__ uint64_t boot_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}

// Block `block` (0, 1, ...) of the stream of numpy.random.Philox(key=[key0, key1]): the generator starts at counter 0 and advances
// the counter BEFORE every block, so block b is the ten rounds applied to the counter (b + 1, 0, 0, 0); random_raw hands out
// out[0], out[1], out[2], out[3] of block 0, then block 1's.  (A stream is at most MISTI_BOOT_MAX_DRAWS / 4 blocks here: the
// counter's first word never carries.)
__host__ __device__ __forceinline__ void philox4x64_10_block(uint64_t key0, uint64_t key1, uint64_t block, uint64_t out[4]) {
    constexpr uint64_t M0 = 0xD2E7470EE14C6C93ull, M1 = 0xCA5A826395121157ull;      // the multipliers (Random123, philox.h)
    constexpr uint64_t W0 = 0x9E3779B97F4A7C15ull, W1 = 0xBB67AE8584CAA73Bull;      // the key schedule's Weyl increments
    uint64_t c0 = block + 1, c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t hi0 = boot_mulhi(M0, c0), lo0 = M0 * c0;
        const uint64_t hi1 = boot_mulhi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ key0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ key1;
        c3 = lo0;
        key0 += W0;                                   // (the bump behind the last round is dead code)
        key1 += W1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// The chunk a raw value picks: floor(raw n_chunk / 2^64).  No rejection step - one raw value per draw, whatever it is; a chunk is
// picked with probability within n_chunk / 2^64 of 1 / n_chunk.
__host__ __device__ __forceinline__ int64_t boot_index(uint64_t raw, int64_t n_chunk) { return (int64_t)boot_mulhi(raw, (uint64_t)n_chunk); }

}  // namespace misti

// ---- the host part (misti_boot.hip), shared with the jackknife (misti_jack.hip) ----------------------------------------------------------
struct misti_ctx;
namespace misti_host __attribute__((visibility("hidden"))) {
// What every entry of a chunk table must be, whoever resamples it - finite, a length > 0, no negative count, sums that stay finite -
// and the sums themselves with the shortest length.  The bootstrap's draw limit is not part of it.
int chunk_entries(int64_t n_chunk, const double* chunks, double* genome, double* seg, double* shortest);
// The table of `bytes` bytes into the context's chunk buffer (c->boot_chunks), on its stream and with its device current.
int upload_chunks(misti_ctx* c, size_t bytes, const double* chunks);
}  // namespace misti_host
