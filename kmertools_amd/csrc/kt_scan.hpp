// kt_scan.hpp - the exclusive scan over n items, two u64 sums at once, written once over a functor F (kt_unitig.hip's
// stages d and g, kt_tablefile.hip's escape ranks, kt_thread.hip's run numbering, kt_component.hip's component numbering): word(i) is item i's one u32, add(word, a, b) what it contributes to the
// two sums (word 0, the filler past n, contributes nothing), put(i, a, b) takes the sums over the items before i, total()
// is thread 0's after the last put.  Three launches: the tiles' sums (scan2_tile_sum_kernel), one workgroup over those
// (scan2_tile_scan_kernel, which also leaves the two totals), and the tiles again (scan2_apply_kernel).
// The kernels sit in an unnamed namespace: every translation unit that includes this gets its own copy of them in the
// code object (five today - kt_unitig.hip, kt_tablefile.hip, kt_thread.hip, kt_component.hip, kt_scaled.hip; only scan2_tile_scan_kernel is no template and so
// truly repeated: tolerable; a user that needs more of it should move them into a translation unit of their own).
#pragma once
#include "kt_device.hpp"

namespace {

constexpr int SCAN_BLOCK = 256, SCAN_WAVES = SCAN_BLOCK / 64;
constexpr uint32_t SCAN_ITEMS = 4, SCAN_TILE = SCAN_BLOCK * SCAN_ITEMS;

// inclusive prefix sums of a and b over the workgroup's threads; *ta, *tb = the sums
__device__ __forceinline__ void block_scan2(uint64_t &a, uint64_t &b, uint64_t (*wsum)[2], uint64_t *ta, uint64_t *tb) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t ua = __shfl_up(a, off, 64), ub = __shfl_up(b, off, 64);
        if (lane >= (uint32_t)off) a += ua, b += ub;
    }
    if (lane == 63u) wsum[wave][0] = a, wsum[wave][1] = b;
    ktd::lds_barrier();
    uint64_t pa = 0, pb = 0, sa = 0, sb = 0;
#pragma unroll
    for (uint32_t x = 0; x < (uint32_t)SCAN_WAVES; x++) {
        const uint64_t xa = wsum[x][0], xb = wsum[x][1];
        if (x < wave) pa += xa, pb += xb;
        sa += xa, sb += xb;
    }
    ktd::lds_barrier();  // (wsum is rewritten by the next call)
    a += pa, b += pb;
    *ta = sa, *tb = sb;
}

// tile t (SCAN_TILE items) -> tiles[2t], tiles[2t + 1] = its two sums
template <class F>
__global__ __launch_bounds__(SCAN_BLOCK) void scan2_tile_sum_kernel(F f, uint64_t n, uint64_t *__restrict__ tiles) {
    __shared__ uint64_t wsum[SCAN_WAVES][2];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
    uint64_t a = 0, b = 0, ta, tb;
#pragma unroll
    for (uint32_t j = 0; j < SCAN_ITEMS; j++) f.add(base + j < n ? f.word(base + j) : 0u, a, b);
    block_scan2(a, b, wsum, &ta, &tb);
    if (threadIdx.x == 0) tiles[2ull * blockIdx.x] = ta, tiles[2ull * blockIdx.x + 1] = tb;
}

// one workgroup: the tiles' sums into their exclusive prefixes, the totals into *sum_a and *sum_b
__global__ __launch_bounds__(SCAN_BLOCK) void scan2_tile_scan_kernel(uint64_t *__restrict__ tiles, uint64_t T,
                                                                      unsigned long long *__restrict__ sum_a,
                                                                      unsigned long long *__restrict__ sum_b) {
    __shared__ uint64_t wsum[SCAN_WAVES][2];
    uint64_t ca = 0, cb = 0;
    for (uint64_t c0 = 0; c0 < T; c0 += SCAN_BLOCK) {
        const uint64_t t = c0 + threadIdx.x;
        const uint64_t va = t < T ? tiles[2 * t] : 0, vb = t < T ? tiles[2 * t + 1] : 0;
        uint64_t a = va, b = vb, ta, tb;
        block_scan2(a, b, wsum, &ta, &tb);
        if (t < T) tiles[2 * t] = ca + a - va, tiles[2 * t + 1] = cb + b - vb;
        ca += ta, cb += tb;
    }
    if (threadIdx.x == 0) *sum_a = ca, *sum_b = cb;
}

// every item's put(), from its tile's exclusive prefix in `tiles`
template <class F>
__global__ __launch_bounds__(SCAN_BLOCK) void scan2_apply_kernel(F f, uint64_t n, const uint64_t *__restrict__ tiles) {
    __shared__ uint64_t wsum[SCAN_WAVES][2];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
    uint32_t v[SCAN_ITEMS];
    uint64_t a = 0, b = 0, ta, tb;
#pragma unroll
    for (uint32_t j = 0; j < SCAN_ITEMS; j++) {
        v[j] = base + j < n ? f.word(base + j) : 0u;
        f.add(v[j], a, b);
    }
    const uint64_t own_a = a, own_b = b;
    block_scan2(a, b, wsum, &ta, &tb);
    uint64_t ra = tiles[2ull * blockIdx.x] + a - own_a, rb = tiles[2ull * blockIdx.x + 1] + b - own_b;
#pragma unroll
    for (uint32_t j = 0; j < SCAN_ITEMS; j++) {
        if (base + j < n) f.put(base + j, ra, rb);
        f.add(v[j], ra, rb);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) f.total();
}

}  // namespace
