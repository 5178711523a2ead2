// kt_scan.hpp - the exclusive scan over n items, two u64 sums at once, written once over a functor F: word(i) is item i's
// one u32, add(word, a, b) what it contributes to the two sums (word 0, the filler past n, contributes nothing),
// put(i, a, b) takes the sums over the items before i, total() is thread 0's after the last put.  Three launches, in two
// calls on the host - callers read the totals back and size their outputs between them:
//   scan2_sums   the tiles' sums (scan2_tile_sum_kernel), then one workgroup over those (scan2_tile_scan_kernel), which
//                also leaves the two totals where the caller wants them;
//   scan2_apply  the tiles again (scan2_apply_kernel): every item's put().
// `tiles` is 2 * scan2_tiles(n) u64 of device memory that lives from the one call to the other.
// Users: kt_unitig.hip's stages d and g, kt_tablefile.hip's escape ranks, kt_thread.hip's run numbering, kt_component.hip's
// component numbering, kt_scaled.hip's segment bases and merged rows.
// Everything sits in an unnamed namespace: every translation unit that includes this gets its own copy of the kernels in
// the code object (only scan2_tile_scan_kernel is no template and so truly repeated: tolerable; a user that needs more of
// it should move them into a translation unit of their own).
#pragma once
#include "kt_device.hpp"
#include "kt_internal.hpp"

namespace {

constexpr int SCAN_BLOCK = 256, SCAN_WAVES = SCAN_BLOCK / 64;
constexpr uint32_t SCAN_ITEMS = 4, SCAN_TILE = SCAN_BLOCK * SCAN_ITEMS;
using ktd::sum2;

// tile t (SCAN_TILE items) -> tiles[2t], tiles[2t + 1] = its two sums
template <class F>
__global__ __launch_bounds__(SCAN_BLOCK) void scan2_tile_sum_kernel(F f, uint64_t n, uint64_t *__restrict__ tiles) {
    __shared__ sum2 wsum[SCAN_WAVES];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
    sum2 v{0, 0}, t;
#pragma unroll
    for (uint32_t j = 0; j < SCAN_ITEMS; j++) f.add(base + j < n ? f.word(base + j) : 0u, v.a, v.b);
    ktd::block_excl_scan<SCAN_WAVES>(v, wsum, &t);
    if (threadIdx.x == 0) tiles[2ull * blockIdx.x] = t.a, tiles[2ull * blockIdx.x + 1] = t.b;
}

// one workgroup: the tiles' sums into their exclusive prefixes, the totals into *sum_a and *sum_b
__global__ __launch_bounds__(SCAN_BLOCK) void scan2_tile_scan_kernel(uint64_t *__restrict__ tiles, uint64_t T,
                                                                      unsigned long long *__restrict__ sum_a,
                                                                      unsigned long long *__restrict__ sum_b) {
    __shared__ sum2 wsum[SCAN_WAVES];
    sum2 c{0, 0};
    for (uint64_t c0 = 0; c0 < T; c0 += SCAN_BLOCK) {
        const uint64_t t = c0 + threadIdx.x;
        const sum2 v{t < T ? tiles[2 * t] : 0, t < T ? tiles[2 * t + 1] : 0};
        sum2 tot;
        const sum2 pre = c + ktd::block_excl_scan<SCAN_WAVES>(v, wsum, &tot);
        if (t < T) tiles[2 * t] = pre.a, tiles[2 * t + 1] = pre.b;
        c = c + tot;
    }
    if (threadIdx.x == 0) *sum_a = c.a, *sum_b = c.b;
}

// every item's put(), from its tile's exclusive prefix in `tiles`
template <class F>
__global__ __launch_bounds__(SCAN_BLOCK) void scan2_apply_kernel(F f, uint64_t n, const uint64_t *__restrict__ tiles) {
    __shared__ sum2 wsum[SCAN_WAVES];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
    uint32_t v[SCAN_ITEMS];
    sum2 own{0, 0};
#pragma unroll
    for (uint32_t j = 0; j < SCAN_ITEMS; j++) {
        v[j] = base + j < n ? f.word(base + j) : 0u;
        f.add(v[j], own.a, own.b);
    }
    const sum2 pre = ktd::block_excl_scan<SCAN_WAVES>(own, wsum);
    uint64_t ra = tiles[2ull * blockIdx.x] + pre.a, rb = tiles[2ull * blockIdx.x + 1] + pre.b;
#pragma unroll
    for (uint32_t j = 0; j < SCAN_ITEMS; j++) {
        if (base + j < n) f.put(base + j, ra, rb);
        f.add(v[j], ra, rb);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) f.total();
}

// the host half: the launches, on `stream`.  sum_a and sum_b: device memory, 8 bytes each, for the two totals
uint64_t scan2_tiles(uint64_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }

template <class F, class S>
int scan2_sums(hipStream_t stream, const F &f, uint64_t n, uint64_t *tiles, S *sum_a, S *sum_b) {
    static_assert(sizeof(S) == 8, "the totals are 64-bit words");
    const uint64_t T = scan2_tiles(n);
    hipLaunchKernelGGL(scan2_tile_sum_kernel<F>, dim3((uint32_t)T), dim3(SCAN_BLOCK), 0, stream, f, n, tiles);
    hipLaunchKernelGGL(scan2_tile_scan_kernel, dim3(1), dim3(SCAN_BLOCK), 0, stream, tiles, T, (unsigned long long *)sum_a,
                       (unsigned long long *)sum_b);
    KT_HIP(hipGetLastError());
    return KT_OK;
}

template <class F>
int scan2_apply(hipStream_t stream, const F &f, uint64_t n, const uint64_t *tiles) {
    hipLaunchKernelGGL(scan2_apply_kernel<F>, dim3((uint32_t)scan2_tiles(n)), dim3(SCAN_BLOCK), 0, stream, f, n, tiles);
    KT_HIP(hipGetLastError());
    return KT_OK;
}

}  // namespace
