// kt_sort.hip - (key, count) pairs in device memory into ascending key order: a plain least-significant-digit radix sort,
// 8-bit digits, hand-written (no hipcub / rocprim in this library).  Used by kt_ctr_setop's sorted output, whose result is
// compact in device memory already and usually far smaller than either table: simple and correct before fast.
//
// A pass = three launches.  The array is cut into WAVE TILES of 4096 consecutive pairs, one wave each (a wave never talks
// to another, so there is no barrier in the loops):
//   sort_hist_kernel     tile t's count of every digit value d -> hist[d * T + t]            (T tiles; digit-major)
//   sort_scan_kernel     workgroup d: exclusive prefix of row d in place, its sum -> totals[d]
//   sort_scatter_kernel  every pair to digit_base[d] + hist[d * T + t] + its rank among the tile's earlier pairs of digit d
// Stable: inside a tile pairs are taken 64 at a time in array order, and the lanes of one step that share a digit find
// each other with 8 ballots (one per digit bit) - the rank is the number of lower lanes among them, the lowest one moves
// the tile's running offset of that digit on.  No LDS atomics, so a digit that is the same for every key (the top bits of
// short k-mers) costs what any other does.  The passes ping-pong between the caller's arrays and one scratch pair of the
// context; their number is made even, so the result ends where it started.
#include "kt_device.hpp"
#include "kt_internal.hpp"

namespace {

constexpr int BLOCK = 256, WAVES = BLOCK / 64;
constexpr uint32_t STEPS = 64, WTILE = 64 * STEPS, LOADS = 8;  // pairs per wave tile; loads in flight per lane in the scatter

// the lanes of this step that hold digit d (valid lanes only)
__device__ __forceinline__ uint64_t digit_peers(uint32_t d, bool valid) {
    uint64_t m = __ballot(valid);
#pragma unroll
    for (uint32_t b = 0; b < 8; b++) {
        const bool bit = (d >> b) & 1u;
        const uint64_t v = __ballot(bit);
        m &= bit ? v : ~v;
    }
    return m;
}

__global__ __launch_bounds__(BLOCK) void sort_hist_kernel(const uint64_t *__restrict__ keys, uint64_t n, uint32_t shift, uint64_t T,
                                                          uint64_t *__restrict__ hist) {
    __shared__ uint32_t cnt[WAVES][256];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t t = (uint64_t)blockIdx.x * WAVES + wave;
    for (uint32_t d = lane; d < 256u; d += 64u) cnt[wave][d] = 0u;
    ktd::lds_barrier();
    if (t < T) {
        const uint64_t base = t * WTILE;
        for (uint32_t r = 0; r < STEPS && base + r * 64u < n; r++) {
            const uint64_t i = base + r * 64u + lane;
            const bool valid = i < n;
            const uint32_t d = valid ? (uint32_t)(keys[i] >> shift) & 255u : 0u;
            const uint64_t peers = digit_peers(d, valid);
            if (valid && (peers & ((1ull << lane) - 1ull)) == 0) cnt[wave][d] += (uint32_t)__popcll(peers);
        }
    }
    ktd::lds_barrier();
    if (t < T)
        for (uint32_t d = lane; d < 256u; d += 64u) hist[(uint64_t)d * T + t] = cnt[wave][d];
}

__global__ __launch_bounds__(BLOCK) void sort_scan_kernel(uint64_t *__restrict__ hist, uint64_t T, uint64_t *__restrict__ totals) {
    __shared__ uint64_t wsum[WAVES];
    uint64_t *row = hist + (uint64_t)blockIdx.x * T;
    uint64_t carry = 0;
    for (uint64_t c0 = 0; c0 < T; c0 += BLOCK) {
        const uint64_t i = c0 + threadIdx.x;
        const uint64_t v = i < T ? row[i] : 0;
        uint64_t tot;
        const uint64_t pre = ktd::block_excl_scan<WAVES>(v, wsum, &tot);
        if (i < T) row[i] = carry + pre;
        carry += tot;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

__global__ __launch_bounds__(BLOCK) void sort_scatter_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ counts,
                                                             uint64_t n, uint32_t shift, uint64_t T,
                                                             const uint64_t *__restrict__ hist, const uint64_t *__restrict__ totals,
                                                             uint64_t *__restrict__ out_keys, uint32_t *__restrict__ out_counts) {
    __shared__ uint64_t wsum[WAVES];
    __shared__ uint64_t run[WAVES][256];  // where the tile's next pair of digit d goes
    __shared__ uint64_t dbase[256];       // pairs with a smaller digit
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t t = (uint64_t)blockIdx.x * WAVES + wave;
    {
        dbase[threadIdx.x] = ktd::block_excl_scan<WAVES>(totals[threadIdx.x], wsum);
    }
    ktd::lds_barrier();
    if (t < T)
        for (uint32_t d = lane; d < 256u; d += 64u) run[wave][d] = dbase[d] + hist[(uint64_t)d * T + t];
    ktd::lds_barrier();
    if (t >= T) return;
    const uint64_t base = t * WTILE;
    for (uint32_t r0 = 0; r0 < STEPS && base + r0 * 64u < n; r0 += LOADS) {
        uint64_t k[LOADS];
        uint32_t c[LOADS];
#pragma unroll
        for (uint32_t j = 0; j < LOADS; j++) {
            const uint64_t i = base + (r0 + j) * 64u + lane;
            k[j] = i < n ? keys[i] : 0;
            c[j] = i < n ? counts[i] : 0u;
        }
#pragma unroll
        for (uint32_t j = 0; j < LOADS; j++) {
            const uint64_t i = base + (r0 + j) * 64u + lane;
            const bool valid = i < n;
            const uint32_t d = (uint32_t)(k[j] >> shift) & 255u;
            const uint64_t peers = digit_peers(d, valid);
            const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
            if (valid) {
                const uint64_t pos = run[wave][d] + rank;
                if (pos < n) {  // (always: the offsets are the histogram's)
                    out_keys[pos] = k[j];
                    out_counts[pos] = c[j];
                }
            }
            // every lane has read its offset (one LDS instruction of the wave, in order) before the lowest peer moves it on
            if (valid && rank == 0u) run[wave][d] += (uint64_t)__popcll(peers);
        }
    }
}

}  // namespace

// keys[0, n) / counts[0, n) (device) into ascending key order, on the context's stream; key_bits = the bits a key can
// have set.  Scratch: the context's OUT (a second pair) and AUX0 (the digit histograms).
int kt_sort_pairs(kt_ctx *ctx, uint64_t *keys, uint32_t *counts, uint64_t n, uint32_t key_bits) {
    if (n < 2) return KT_OK;
    if (int rc = ctx->use()) return rc;
    uint32_t passes = (key_bits + 7u) / 8u;
    passes += passes & 1u;  // (even: the pairs end where they started)
    const uint64_t T = (n + WTILE - 1) / WTILE;
    uint64_t *hist = nullptr, *k_dst = nullptr;
    if (int rc = ctx->claim(kt::OUT, n * 12, "kt_sort_pairs", &k_dst)) return rc;
    if (int rc = ctx->claim(kt::AUX0, (256 * T + 256) * 8, "kt_sort_pairs", &hist)) return rc;
    uint64_t *totals = hist + 256 * T, *k_src = keys;
    uint32_t *c_src = counts, *c_dst = (uint32_t *)(k_dst + n);
    const dim3 grid((uint32_t)((T + WAVES - 1) / WAVES)), block(BLOCK);
    for (uint32_t p = 0; p < passes; p++) {
        const uint32_t shift = 8u * p;
        hipLaunchKernelGGL(sort_hist_kernel, grid, block, 0, ctx->stream, (const uint64_t *)k_src, n, shift, T, hist);
        hipLaunchKernelGGL(sort_scan_kernel, dim3(256), block, 0, ctx->stream, hist, T, totals);
        hipLaunchKernelGGL(sort_scatter_kernel, grid, block, 0, ctx->stream, (const uint64_t *)k_src, (const uint32_t *)c_src, n,
                           shift, T, (const uint64_t *)hist, (const uint64_t *)totals, k_dst, c_dst);
        KT_HIP(hipGetLastError());
        uint64_t *tk = k_src;
        k_src = k_dst, k_dst = tk;
        uint32_t *tc = c_src;
        c_src = c_dst, c_dst = tc;
    }
    return KT_OK;
}
