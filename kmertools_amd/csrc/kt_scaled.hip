// kt_scaled.hip - scaled (FracMinHash) sketches: every distinct k-mer hash of a read at or below 2^64 / scaled, with its
// abundance (kt_scaled_batch), unions of such sketches with the abundances summed (kt_scaled_merge), the shared hashes of
// every pair of two sets of sketches (kt_scaled_pairs), and the routine that kt_ctr_scaled (kt_ctr.hip) shares with the
// first two: kt::scaled_finish.
//
// A window's hash is mix64(canonical k-mer ^ seed), kt_sketch_batch's; it is KEPT when hash <= max_hash(scaled).  A sketch
// is variable in length, so sketches lie CSR: hashes[row_offsets[i] .. row_offsets[i + 1]), abundances beside them.
//
//   select_count_kernel   the ktseg front end, a persistent grid over the 8192-base segments: kept windows per segment.
//   (kt_scan.hpp)         the segments' counts into their exclusive prefix: where a segment's kept windows go, and how
//                         many there are in all - read back, it sizes everything behind.
//   select_emit_kernel    the same walk again: a segment's kept windows, in batch order (a prefix sum over the workgroup's
//                         threads), as (hash, read) elements; the reads' windows with multiplicity are counted here, one
//                         integer atomic per piece of a read inside a thread's 32 window starts.
//   kt::scaled_finish     elements -> sketches, whatever made the elements.  Sort by hash with the element's index as the
//                         payload (kt_sort_pairs, 8 digit passes); with more than one row the rows are gathered through
//                         the permutation and sorted, stably, over the bits of n_rows, and the hashes gathered behind
//                         them: the elements are now in (row, hash) order.  An element is a HEAD when its (row, hash)
//                         differs from its predecessor's; a scan numbers the heads (that number is read back: *n_out), a
//                         second one - only when abundances were given, else an element's index is that sum - gives the
//                         abundances in front of every element, a head's abundance is the difference of two of those sums
//                         (saturating at 2^32 - 1), and row r starts at the number of heads in front of the first element
//                         of a row >= r.  One row skips the second sort and everything that has to do with rows.
//   scaled_pairs_kernel   a tile of a row of A in LDS (16384 hashes, 128 KiB), a wave per row of B, a lane per lower
//                         bound, matches counted by ballot - sketch_pairs_kernel's walk.  A row of A longer than a tile
//                         goes tile by tile, every wave adding to the cells it wrote for the tile before, and reads of a
//                         row of B only what lies between the tile's first and last hash.
// Integer atomics only (window counts); every output is a function of the inputs alone.
#include <math.h>

#include "kt_internal.hpp"
#include "kt_launch.hpp"
#include "kt_scan.hpp"

namespace {

using ktseg::SEG;
using ktseg::SegArgs;
using ktseg::SegShared;
constexpr uint32_t BLOCK = ktseg::BLOCK;
constexpr uint32_t WAVE = 64, WAVES = BLOCK / WAVE;
constexpr uint32_t PAIR_TILE = 16384;  // hashes of a row of A in LDS

// ---- select ----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(BLOCK) void select_count_kernel(SegArgs a, uint64_t seed, uint64_t max_hash, uint32_t *__restrict__ seg_cnt) {
    __shared__ SegShared sm;
    __shared__ uint32_t wsum[WAVES];
    const uint32_t tid = threadIdx.x;
    for (uint64_t g = blockIdx.x; g < a.n_seg; g += gridDim.x) {
        uint32_t mine = 0;
        ktseg::for_each_kmer(a, g, sm, [&](uint64_t f, uint64_t r, uint64_t) {
            mine += ktd::mix64((f < r ? f : r) ^ seed) <= max_hash ? 1u : 0u;
        });
        mine = ktd::wave_sum(mine);
        if ((tid & (WAVE - 1)) == 0) wsum[tid / WAVE] = mine;
        ktd::lds_barrier();
        if (tid == 0) {
            uint32_t s = 0;
#pragma unroll
            for (uint32_t w = 0; w < WAVES; w++) s += wsum[w];
            seg_cnt[g] = s;
        }
        // (wsum is written again behind the barriers of the next segment's staging, which thread 0 reaches after this read)
    }
}

// the scan over the segments' counts: sum a = the kept windows in front of a segment
struct SegScan {
    const uint32_t *cnt;
    uint64_t *base;
    __device__ __forceinline__ uint32_t word(uint64_t g) const { return cnt[g]; }
    __device__ __forceinline__ void add(uint32_t w, uint64_t &a, uint64_t &) const { a += w; }
    __device__ __forceinline__ void put(uint64_t g, uint64_t a, uint64_t) const { base[g] = a; }
    __device__ __forceinline__ void total() const {}
};

// n_el: the room of hashes / rows (the scan's total; no store goes past it); n_kmers: null or zeroed
__global__ __launch_bounds__(BLOCK) void select_emit_kernel(SegArgs a, uint64_t seed, uint64_t max_hash, const uint64_t *__restrict__ seg_base,
                                                            uint64_t n_el, uint64_t *__restrict__ hashes, uint64_t *__restrict__ rows,
                                                            uint32_t *__restrict__ n_kmers) {
    __shared__ SegShared sm;
    __shared__ uint32_t wsum[WAVES];
    const uint32_t tid = threadIdx.x;
    const uint64_t total = a.offsets[a.n_reads];
    for (uint64_t g = blockIdx.x; g < a.n_seg; g += gridDim.x) {
        const uint64_t B0 = g * SEG;
        uint64_t keys[ktseg::PER_THREAD];
        uint32_t ok;
        ktseg::collect_kmers(a, g, sm, keys, ok);  // (the staged masks stay until the next segment is staged)
        uint32_t km = 0;  // bit j: window start 32 tid + j is kept
#pragma unroll
        for (uint32_t j = 0; j < ktseg::PER_THREAD; j++) {
            keys[j] = ktd::mix64(keys[j] ^ seed);
            km |= (((ok >> j) & 1u) && keys[j] <= max_hash ? 1u : 0u) << j;
        }
        const uint64_t at = seg_base[g] + ktd::block_excl_scan<WAVES>((uint32_t)__popc(km), wsum);
#pragma unroll
        for (uint32_t j = 0; j < ktseg::PER_THREAD; j++) {
            if (!((km >> j) & 1u)) continue;
            const uint64_t pos = at + (uint32_t)__popc(km & ((1u << j) - 1u));
            if (pos < n_el) hashes[pos] = keys[j];
        }
        // the reads of the thread's window starts: the starts are cut into pieces by the read starts among them
        const uint32_t lim = total - B0 < SEG ? (uint32_t)(total - B0) : SEG;  // positions of the segment that hold a base
        const uint32_t p0 = 32u * tid;
        if (p0 < lim && (km || (n_kmers && ok))) {
            uint32_t bw = sm.bnd[tid] & ~1u;  // read starts behind the thread's first position
            if (lim - p0 < 32u) bw &= (1u << (lim - p0)) - 1u;
            ktseg::ReadCursor cur(a.offsets, a.seg_first, g, B0 + p0);
            uint32_t lo = 0;
            while (true) {
                const uint32_t hi = bw ? (uint32_t)__ffs((int)bw) - 1u : 32u;
                const uint32_t mask = (hi < 32u ? (1u << hi) - 1u : 0xFFFFFFFFu) & ~((1u << lo) - 1u);
                if (n_kmers)
                    if (const uint32_t c = (uint32_t)__popc(ok & mask)) atomicAdd(&n_kmers[cur.rid], c);
                for (uint32_t kp = km & mask; kp; kp &= kp - 1u) {
                    const uint32_t j = (uint32_t)__ffs((int)kp) - 1u;
                    const uint64_t pos = at + (uint32_t)__popc(km & ((1u << j) - 1u));
                    if (pos < n_el) rows[pos] = cur.rid;
                }
                if (hi >= 32u) break;
                cur.advance(B0 + p0 + hi);
                lo = hi;
                bw &= bw - 1u;
            }
        }
        ktd::lds_barrier();  // the staged masks are replaced by the next segment
    }
}

// ---- elements -> sketches ----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(BLOCK) void iota_kernel(uint32_t *__restrict__ v, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLOCK) v[i] = (uint32_t)i;
}

// out[i] = src[perm[i]]
__global__ __launch_bounds__(BLOCK) void gather64_kernel(const uint64_t *__restrict__ src, const uint32_t *__restrict__ perm, uint64_t n,
                                                         uint64_t *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLOCK) out[i] = src[perm[i]];
}

// the abundances in front of every element of the sorted order
struct AbundScan {
    const uint32_t *abunds, *perm;
    uint64_t *pre;
    __device__ __forceinline__ uint32_t word(uint64_t i) const { return abunds[perm[i]]; }
    __device__ __forceinline__ void add(uint32_t w, uint64_t &a, uint64_t &) const { a += w; }
    __device__ __forceinline__ void put(uint64_t i, uint64_t a, uint64_t) const { pre[i] = a; }
    __device__ __forceinline__ void total() const {}
};

// The heads among the sorted elements, numbered.  put: pos[i] (null: one row) = the heads in front of element i; a head h
// leaves its hash in out_h[h] and the abundances in front of it in bstart[h] (both null: a call that only counts).
struct HeadScan {
    const uint64_t *keys, *rows;  // sorted by (row, key); rows null: one row
    const uint64_t *pre;          // AbundScan's sums, or null: every abundance is 1
    const uint64_t *sum_ab;       // ... and their total
    uint64_t n, n_heads;          // (n_heads: known to put and total only)
    uint32_t *pos;
    uint64_t *out_h, *bstart;
    __device__ __forceinline__ uint32_t word(uint64_t i) const {
        return i == 0 || keys[i] != keys[i - 1] || (rows && rows[i] != rows[i - 1]) ? 1u : 0u;
    }
    __device__ __forceinline__ void add(uint32_t w, uint64_t &a, uint64_t &) const { a += w; }
    __device__ __forceinline__ void put(uint64_t i, uint64_t a, uint64_t) const {
        if (pos) pos[i] = (uint32_t)a;
        if (!out_h || !word(i) || a >= n_heads) return;
        out_h[a] = keys[i];
        bstart[a] = pre ? pre[i] : i;
    }
    __device__ __forceinline__ void total() const {
        if (bstart) bstart[n_heads] = pre ? *sum_ab : n;
    }
};

__global__ __launch_bounds__(BLOCK) void head_abund_kernel(const uint64_t *__restrict__ bstart, uint64_t n_heads, uint32_t *__restrict__ out) {
    for (uint64_t h = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; h < n_heads; h += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t s = bstart[h + 1] - bstart[h];
        out[h] = s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s;
    }
}

// row_offsets[r] = the heads in front of the first element of a row >= r, r = 0 .. n_rows
__global__ __launch_bounds__(BLOCK) void row_offsets_kernel(const uint64_t *__restrict__ rows, const uint32_t *__restrict__ pos, uint64_t n,
                                                            uint64_t n_heads, uint64_t n_rows, uint64_t *__restrict__ row_offsets) {
    for (uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; r <= n_rows; r += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t lo = ktd::lower_bound(rows, n, r);
        row_offsets[r] = lo < n ? pos[lo] : n_heads;
    }
}

// ---- merge --------------------------------------------------------------------------------------------------------------------

// group_offsets[0 .. n_groups] must not decrease and must end at or below n_rows: *bad = 1 otherwise; el_offsets[g] = where
// group g's elements start = row_offsets[group_offsets[g]]
__global__ __launch_bounds__(BLOCK) void group_elems_kernel(const uint64_t *__restrict__ go, uint64_t n_groups, uint64_t n_rows,
                                                            const uint64_t *__restrict__ row_offsets, uint64_t *__restrict__ el_offsets,
                                                            uint32_t *bad) {
    for (uint64_t g = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; g <= n_groups; g += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t lo = go[g];
        if (lo > n_rows || (g < n_groups && go[g + 1] < lo)) *bad = 1u;
        el_offsets[g] = row_offsets[lo > n_rows ? n_rows : lo];
    }
}

// rows[i] = the group of element e0 + i: the last g with el_offsets[g] <= e0 + i (empty groups in front of it share its start)
__global__ __launch_bounds__(BLOCK) void elem_groups_kernel(const uint64_t *__restrict__ el_offsets, uint64_t n_groups, uint64_t e0, uint64_t n,
                                                            uint64_t *__restrict__ rows) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLOCK) {
        uint64_t lo = 0, hi = n_groups;  // el_offsets[lo] <= e0 + i < el_offsets[hi]
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (el_offsets[mid] <= e0 + i) lo = mid; else hi = mid;
        }
        rows[i] = lo;
    }
}

// ---- pairs --------------------------------------------------------------------------------------------------------------------

// *max_len = the longest of the n rows of `offsets`
__global__ __launch_bounds__(BLOCK) void max_row_kernel(const uint64_t *__restrict__ offsets, uint64_t n, uint64_t *max_len) {
    uint64_t m = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t lo = offsets[i], hi = offsets[i + 1];
        const uint64_t len = hi < lo ? ~0ull : hi - lo;  // (offsets that decrease are refused with the long rows)
        m = len > m ? len : m;
    }
    if (m) atomicMax((unsigned long long *)max_len, (unsigned long long)m);
}

__global__ __launch_bounds__(BLOCK) void scaled_pairs_kernel(const uint64_t *__restrict__ A, const uint64_t *__restrict__ aoff, uint64_t n_a,
                                                             const uint64_t *__restrict__ B, const uint64_t *__restrict__ boff, uint64_t n_b,
                                                             uint32_t *shared) {
    __shared__ uint64_t arow[PAIR_TILE];
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    for (uint64_t i = blockIdx.x; i < n_a; i += gridDim.x) {
        const uint64_t a0 = aoff[i];
        const uint32_t na = (uint32_t)(aoff[i + 1] - a0);
        const uint32_t tiles = na ? (na + PAIR_TILE - 1) / PAIR_TILE : 1u;  // (an empty row writes its zeros in one round)
        for (uint32_t t = 0; t < tiles; t++) {
            const uint32_t t0 = t * PAIR_TILE, tn = na - t0 < PAIR_TILE ? na - t0 : PAIR_TILE;
            for (uint32_t e = tid; e < tn; e += BLOCK) arow[e] = A[a0 + t0 + e];
            ktd::lds_barrier();
            for (uint64_t j = (uint64_t)blockIdx.y * WAVES + wave; j < n_b; j += (uint64_t)gridDim.y * WAVES) {
                const uint64_t *brow = B + boff[j];
                const uint32_t nb = (uint32_t)(boff[j + 1] - boff[j]);
                uint32_t s = 0, e1 = tn ? nb : 0u;
                if (tiles > 1 && e1) {  // what of B's row lies between the tile's ends
                    const uint64_t first = arow[0], last = arow[tn - 1];
                    s = ktd::lower_bound(brow, nb, first);
                    e1 = ktd::lower_bound(brow, nb, last);
                    if (e1 < nb && brow[e1] == last) e1++;
                }
                uint32_t cnt = 0;
                for (uint32_t c0 = s; c0 < e1; c0 += WAVE) {  // (the same trip count for every lane: the ballot wants them all)
                    const uint32_t e = c0 + lane;
                    bool m = false;
                    if (e < e1) {
                        const uint64_t y = brow[e];
                        const uint32_t lb = ktd::lower_bound(arow, tn, y);
                        m = lb < tn && arow[lb] == y;
                    }
                    cnt += (uint32_t)__popcll(__ballot(m));
                }
                if (lane == 0) {  // (the same wave has this cell in every tile's round)
                    uint32_t *cell = shared + i * n_b + j;
                    *cell = t ? *cell + cnt : cnt;
                }
            }
            ktd::lds_barrier();  // the tile is replaced
        }
    }
}

dim3 flat_grid(const kt_ctx *ctx, uint64_t n) { return dim3(ktl::grid_for(ctx, (n + BLOCK - 1) / BLOCK, 8)); }

// n elements of `src` (device) into the caller's `dst` in `mem`, on the stream
template <class T>
int deliver(kt_ctx *ctx, int mem, T *dst, const T *src, uint64_t n) {
    if (dst && n)
        KT_HIP(hipMemcpyAsync(dst, src, n * sizeof(T), mem == KT_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
    return KT_OK;
}

}  // namespace

using namespace ktl;

int kt::scaled_finish(kt_ctx *ctx, const char *who, const ScaledElems &e, const ScaledOut &o) {
    const uint64_t n = e.n;
    const bool multi = e.rows && e.n_rows > 1;
    const bool emit = o.max_out != 0;
    if (n >= (1ull << 32)) return kt::fail(KT_ERR_ARG, std::string(who) + ": 2^32 elements or more");
    uint32_t *perm = nullptr, *pos = nullptr, *out_a = nullptr;
    uint64_t *rows2 = nullptr, *keys0 = nullptr, *pre = nullptr, *out_h = nullptr, *bstart = nullptr, *roff = nullptr, *tiles = nullptr,
             *sums = nullptr;
    {
        uint8_t *b = nullptr;
        auto parts = [&](uint8_t *at) {
            return carve_parts<16>(at, &perm, n, &rows2, multi ? n : 0, &keys0, multi ? n : 0, &pre, e.abunds ? n : 0, &pos, multi ? n : 0,
                                   &out_h, n, &out_a, n, &bstart, n + 1, &roff, e.n_rows + 1, &tiles, 2 * scan2_tiles(n) + 2, &sums,
                                   (uint64_t)4);
        };
        if (int rc = ctx->claim(kt::AUX2, parts(nullptr), who, &b)) return rc;
        parts(b);
    }
    if (n == 0) {
        *o.n_out = 0;
        KT_HIP(hipMemsetAsync(roff, 0, (e.n_rows + 1) * 8, ctx->stream));
        return deliver(ctx, o.mem, o.row_offsets, (const uint64_t *)roff, e.n_rows + 1);
    }
    const dim3 grid = flat_grid(ctx, n), block(BLOCK);
    hipLaunchKernelGGL(iota_kernel, grid, block, 0, ctx->stream, perm, n);
    KT_HIP(hipGetLastError());
    if (multi) KT_HIP(hipMemcpyAsync(keys0, e.keys, n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (int rc = kt_sort_pairs(ctx, e.keys, perm, n, 64)) return rc;
    if (multi) {
        ctx->unclaim(kt::OUT), ctx->unclaim(kt::AUX0);  // (the second sort's, queued behind the first)
        uint32_t bits = 1;
        while (bits < 64 && ((e.n_rows - 1) >> bits)) bits++;
        hipLaunchKernelGGL(gather64_kernel, grid, block, 0, ctx->stream, e.rows, (const uint32_t *)perm, n, rows2);
        KT_HIP(hipGetLastError());
        if (int rc = kt_sort_pairs(ctx, rows2, perm, n, bits)) return rc;
        hipLaunchKernelGGL(gather64_kernel, grid, block, 0, ctx->stream, (const uint64_t *)keys0, (const uint32_t *)perm, n, e.keys);
        KT_HIP(hipGetLastError());
    }
    if (e.abunds)
        if (int rc = scan2_sums(ctx->stream, AbundScan{e.abunds, perm, pre}, n, tiles, sums + 2, sums + 3)) return rc;
    if (e.abunds)
        if (int rc = scan2_apply(ctx->stream, AbundScan{e.abunds, perm, pre}, n, tiles)) return rc;
    HeadScan hs{e.keys, multi ? rows2 : nullptr, e.abunds ? pre : nullptr, sums + 2, n, 0, nullptr, nullptr, nullptr};
    if (int rc = scan2_sums(ctx->stream, hs, n, tiles, sums, sums + 1)) return rc;
    uint64_t n_heads = 0;
    KT_HIP(hipMemcpyAsync(&n_heads, sums, 8, hipMemcpyDeviceToHost, ctx->stream));
    KT_HIP(hipStreamSynchronize(ctx->stream));
    *o.n_out = n_heads;
    if (emit && n_heads > o.max_out) return kt::fail(KT_ERR_ARG, std::string(who) + ": max_out smaller than the result (*n_out hashes)");
    hs.n_heads = n_heads;
    hs.pos = multi ? pos : nullptr;
    if (emit) hs.out_h = out_h, hs.bstart = bstart;
    if (emit || multi)
        if (int rc = scan2_apply(ctx->stream, hs, n, tiles)) return rc;
    if (emit && o.abunds) {
        hipLaunchKernelGGL(head_abund_kernel, flat_grid(ctx, n_heads), block, 0, ctx->stream, (const uint64_t *)bstart, n_heads, out_a);
        KT_HIP(hipGetLastError());
    }
    if (o.row_offsets) {
        if (multi) {
            hipLaunchKernelGGL(row_offsets_kernel, flat_grid(ctx, e.n_rows + 1), block, 0, ctx->stream, (const uint64_t *)rows2,
                               (const uint32_t *)pos, n, n_heads, e.n_rows, roff);
            KT_HIP(hipGetLastError());
        } else {
            KT_HIP(hipMemsetAsync(roff, 0, 8, ctx->stream));
            KT_HIP(hipMemcpyAsync(roff + 1, sums, 8, hipMemcpyDeviceToDevice, ctx->stream));  // (the heads' total)
        }
        if (int rc = deliver(ctx, o.mem, o.row_offsets, (const uint64_t *)roff, e.n_rows + 1)) return rc;
    }
    if (emit) {
        if (int rc = deliver(ctx, o.mem, o.hashes, (const uint64_t *)out_h, n_heads)) return rc;
        if (int rc = deliver(ctx, o.mem, o.abunds, (const uint32_t *)out_a, n_heads)) return rc;
    }
    return KT_OK;
}

extern "C" uint64_t kt_scaled_max_hash(uint64_t scaled) { return scaled ? 0xFFFFFFFFFFFFFFFFull / scaled : 0; }

extern "C" double kt_containment_ani(uint64_t shared, uint64_t size, int k) {
    if (shared == 0 || size == 0 || k < 1) return 0.0;
    if (shared >= size) return 1.0;
    return pow((double)shared / (double)size, 1.0 / (double)k);
}

extern "C" int kt_scaled_batch(kt_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int k, uint64_t scaled,
                               uint64_t seed, uint64_t *hashes, uint32_t *abunds, uint64_t max_out, uint64_t *row_offsets,
                               uint32_t *n_kmers, uint64_t *n_out, int mem) {
    if (!ctx) return kt::fail(KT_ERR_ARG, "kt_scaled_batch: null ctx");
    if (k < 1 || k > 31) return kt::fail(KT_ERR_ARG, "kt_scaled_batch: k must be in 1..31");
    if (scaled == 0) return kt::fail(KT_ERR_ARG, "kt_scaled_batch: scaled must be >= 1");
    Call call(ctx, mem, "kt_scaled_batch");
    if (int rc = call.enter()) return rc;
    if (!n_out) return call.fail("null n_out");
    if (n_reads == 0) {
        *n_out = 0;
        return KT_OK;
    }
    if (!offsets || !row_offsets || (max_out && !hashes)) return call.fail("null buffer");
    if (int rc = call.batch(bases, offsets, n_reads)) return rc;
    if (int rc = call.refuse_long_reads("the walk's positions in a read are u32")) return rc;
    if (int rc = call.stage()) return rc;
    const uint64_t max_hash = kt_scaled_max_hash(scaled);

    uint64_t n_el = 0;
    SegArgs a{};
    uint64_t *seg_base = nullptr;
    if (call.total) {
        if (int rc = make_seg_args(ctx, call.bases, call.offsets, n_reads, call.total, k, &a)) return rc;
        uint32_t *seg_cnt = nullptr;
        uint64_t *tiles = nullptr, *sums = nullptr;
        if (int rc = carve(call, kt::AUX2, &seg_base, a.n_seg, &seg_cnt, a.n_seg, &tiles, 2 * scan2_tiles(a.n_seg) + 2, &sums, (uint64_t)2))
            return rc;
        if (int rc = launch(select_count_kernel, dim3(grid_for(ctx, a.n_seg, 8)), dim3(BLOCK), 0, ctx->stream, a, seed, max_hash, seg_cnt))
            return rc;
        const SegScan scan{seg_cnt, seg_base};
        if (int rc = scan2_sums(ctx->stream, scan, a.n_seg, tiles, sums, sums + 1)) return rc;
        if (int rc = scan2_apply(ctx->stream, scan, a.n_seg, tiles)) return rc;
        KT_HIP(hipMemcpyAsync(&n_el, sums, 8, hipMemcpyDeviceToHost, ctx->stream));
        KT_HIP(hipStreamSynchronize(ctx->stream));
        if (n_el >= (1ull << 32)) return call.fail("2^32 kept windows or more in one batch (give it in pieces and merge)");
    }
    // the elements and the reads' window counts
    uint64_t *el_h = nullptr, *el_r = nullptr;
    uint32_t *d_nk = nullptr;
    if (int rc = carve(call, kt::AUX1, &el_h, n_el, &el_r, n_el, &d_nk, n_kmers ? n_reads : 0)) return rc;
    if (!n_kmers) d_nk = nullptr;
    if (d_nk) KT_HIP(hipMemsetAsync(d_nk, 0, n_reads * 4, ctx->stream));
    if (call.total && (n_el || d_nk))
        if (int rc = launch(select_emit_kernel, dim3(grid_for(ctx, a.n_seg, 8)), dim3(BLOCK), 0, ctx->stream, a, seed, max_hash,
                            (const uint64_t *)seg_base, n_el, el_h, el_r, d_nk))
            return rc;
    ctx->unclaim(kt::AUX0), ctx->unclaim(kt::AUX2);  // (the segment index and the segments' sums: the emit is queued in front of their next use)
    const kt::ScaledElems e{el_h, nullptr, el_r, n_el, n_reads};
    const kt::ScaledOut o{hashes, abunds, max_out, row_offsets, n_out, mem};
    if (int rc = kt::scaled_finish(ctx, "kt_scaled_batch", e, o)) return rc;
    if (int rc = deliver(ctx, mem, n_kmers, (const uint32_t *)d_nk, n_reads)) return rc;
    return call.finish();
}

extern "C" int kt_scaled_merge(kt_ctx *ctx, const uint64_t *hashes, const uint32_t *abunds, const uint64_t *row_offsets, uint64_t n_rows,
                               const uint64_t *group_offsets, uint64_t n_groups, uint64_t *out_hashes, uint32_t *out_abunds,
                               uint64_t max_out, uint64_t *out_offsets, uint64_t *n_out, int mem) {
    if (!ctx) return kt::fail(KT_ERR_ARG, "kt_scaled_merge: null ctx");
    Call call(ctx, mem, "kt_scaled_merge");
    if (int rc = call.enter()) return rc;
    if (!n_out) return call.fail("null n_out");
    if (n_groups == 0) {
        *n_out = 0;
        return KT_OK;
    }
    if (!group_offsets || !out_offsets || !row_offsets || (max_out && !out_hashes)) return call.fail("null buffer");
    const char *bad_groups = "group_offsets must not decrease and must end at or below n_rows";
    const char *too_many = "2^32 elements or more in the groups (merge them in pieces)";
    uint64_t e0 = 0, n = 0;
    uint64_t *el_h = nullptr, *el_r = nullptr, *el_off = nullptr;
    uint32_t *el_a = nullptr;
    if (call.host()) {
        for (uint64_t r = 0; r < n_rows; r++)
            if (row_offsets[r + 1] < row_offsets[r]) return call.fail("row_offsets decrease");
        for (uint64_t g = 0; g <= n_groups; g++)
            if (group_offsets[g] > n_rows || (g < n_groups && group_offsets[g + 1] < group_offsets[g])) return call.fail(bad_groups);
        e0 = row_offsets[group_offsets[0]];
        n = row_offsets[group_offsets[n_groups]] - e0;
        if (n >= (1ull << 32)) return call.fail(too_many);
        if (n && !hashes) return call.fail("null buffer");
        if (int rc = carve(call, kt::AUX1, &el_h, n, &el_r, n, &el_off, n_groups + 1, &el_a, abunds ? n : 0)) return rc;
        std::unique_ptr<uint64_t[]> h_off(new (std::nothrow) uint64_t[n_groups + 1]);
        if (!h_off) return kt::fail(KT_ERR_NOMEM, "kt_scaled_merge: host alloc");
        for (uint64_t g = 0; g <= n_groups; g++) h_off[g] = row_offsets[group_offsets[g]];
        KT_HIP(hipMemcpyAsync(el_off, h_off.get(), (n_groups + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        if (int rc = call.up(el_h, hashes + e0, n)) return rc;
        if (abunds)
            if (int rc = call.up(el_a, abunds + e0, n)) return rc;
        KT_HIP(hipStreamSynchronize(ctx->stream));  // (h_off goes out of scope)
    } else {
        uint32_t *d_bad = nullptr;
        uint64_t *el_off0 = nullptr;
        if (int rc = carve(call, kt::BASES, &el_off0, n_groups + 1, &d_bad, (uint64_t)4)) return rc;
        KT_HIP(hipMemsetAsync(d_bad, 0, 4, ctx->stream));
        if (int rc = launch(group_elems_kernel, flat_grid(ctx, n_groups + 1), dim3(BLOCK), 0, ctx->stream, group_offsets, n_groups, n_rows,
                            row_offsets, el_off0, d_bad))
            return rc;
        uint64_t ends[2] = {0, 0};
        uint32_t bad = 0;
        KT_HIP(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, ctx->stream));
        KT_HIP(hipMemcpyAsync(&ends[0], el_off0, 8, hipMemcpyDeviceToHost, ctx->stream));
        KT_HIP(hipMemcpyAsync(&ends[1], el_off0 + n_groups, 8, hipMemcpyDeviceToHost, ctx->stream));
        KT_HIP(hipStreamSynchronize(ctx->stream));
        if (bad) return call.fail(bad_groups);
        if (ends[1] < ends[0]) return call.fail("row_offsets decrease");
        e0 = ends[0], n = ends[1] - ends[0];
        if (n >= (1ull << 32)) return call.fail(too_many);
        if (n && !hashes) return call.fail("null buffer");
        if (int rc = carve(call, kt::AUX1, &el_h, n, &el_r, n)) return rc;
        el_off = el_off0;
        if (n) KT_HIP(hipMemcpyAsync(el_h, hashes + e0, n * 8, hipMemcpyDeviceToDevice, ctx->stream));
        el_a = const_cast<uint32_t *>(abunds ? abunds + e0 : nullptr);
    }
    if (n)
        if (int rc = launch(elem_groups_kernel, flat_grid(ctx, n), dim3(BLOCK), 0, ctx->stream, (const uint64_t *)el_off, n_groups, e0, n, el_r))
            return rc;
    const kt::ScaledElems e{el_h, abunds ? el_a : nullptr, el_r, n, n_groups};
    const kt::ScaledOut o{out_hashes, out_abunds, max_out, out_offsets, n_out, mem};
    if (int rc = kt::scaled_finish(ctx, "kt_scaled_merge", e, o)) return rc;
    return call.finish();
}

extern "C" int kt_scaled_pairs(kt_ctx *ctx, const uint64_t *a_hashes, const uint64_t *a_offsets, uint64_t n_a, const uint64_t *b_hashes,
                               const uint64_t *b_offsets, uint64_t n_b, uint32_t *shared, int mem) {
    if (!ctx) return kt::fail(KT_ERR_ARG, "kt_scaled_pairs: null ctx");
    Call call(ctx, mem, "kt_scaled_pairs");
    if (int rc = call.enter()) return rc;
    if (n_a == 0 || n_b == 0) return KT_OK;
    if (!a_offsets || !b_offsets || !shared) return call.fail("null buffer");
    const char *long_row = "a row of 2^32 hashes or more (or offsets that decrease)";
    const bool same = a_hashes == b_hashes && a_offsets == b_offsets && n_a == n_b;
    const uint64_t *d_a = a_hashes, *d_b = b_hashes, *d_ao = a_offsets, *d_bo = b_offsets;
    uint32_t *d_sh = shared;
    const uint64_t cells = n_a * n_b;
    if (call.host()) {
        for (uint64_t i = 0; i < n_a; i++)
            if (a_offsets[i + 1] < a_offsets[i] || a_offsets[i + 1] - a_offsets[i] >= (1ull << 32)) return call.fail(long_row);
        for (uint64_t j = 0; j < n_b; j++)
            if (b_offsets[j + 1] < b_offsets[j] || b_offsets[j + 1] - b_offsets[j] >= (1ull << 32)) return call.fail(long_row);
        // the hashes a's rows and b's rows cover: [a_offsets[0], a_offsets[n_a]) - the copies keep the offsets' origin
        const uint64_t a_lo = a_offsets[0], a_n = a_offsets[n_a] - a_lo, b_lo = b_offsets[0], b_n = same ? 0 : b_offsets[n_b] - b_lo;
        if ((a_n && !a_hashes) || (b_n && !b_hashes)) return call.fail("null buffer");
        uint64_t *h = nullptr, *off = nullptr;
        if (int rc = call.scratch(kt::BASES, (a_n + b_n) * 8 + 8, &h)) return rc;
        if (int rc = call.scratch(kt::OFFSETS, (n_a + n_b + 2) * 8, &off)) return rc;
        if (int rc = call.scratch(kt::AUX1, cells * 4, &d_sh)) return rc;
        if (int rc = call.up(h, a_hashes + a_lo, a_n)) return rc;
        if (int rc = call.up(off, a_offsets, n_a + 1)) return rc;
        d_a = h - a_lo, d_ao = off;  // (only rows' elements, at or behind a_lo, are read)
        d_b = d_a, d_bo = d_ao;
        if (!same) {
            if (int rc = call.up(h + a_n, b_hashes + b_lo, b_n)) return rc;
            if (int rc = call.up(off + n_a + 1, b_offsets, n_b + 1)) return rc;
            d_b = h + a_n - b_lo, d_bo = off + n_a + 1;
        }
    } else {
        uint64_t *d_max = nullptr, max_len = 0;
        if (int rc = call.scratch(kt::AUX2, 8, &d_max)) return rc;
        KT_HIP(hipMemsetAsync(d_max, 0, 8, ctx->stream));
        if (int rc = launch(max_row_kernel, flat_grid(ctx, n_a), dim3(BLOCK), 0, ctx->stream, a_offsets, n_a, d_max)) return rc;
        if (!same)
            if (int rc = launch(max_row_kernel, flat_grid(ctx, n_b), dim3(BLOCK), 0, ctx->stream, b_offsets, n_b, d_max)) return rc;
        KT_HIP(hipMemcpyAsync(&max_len, d_max, 8, hipMemcpyDeviceToHost, ctx->stream));
        KT_HIP(hipStreamSynchronize(ctx->stream));
        if (max_len >= (1ull << 32)) return call.fail(long_row);
        if (max_len && (!a_hashes || !b_hashes)) return call.fail("null buffer");
    }
    if (int rc = launch(scaled_pairs_kernel, ktl::pairs_grid(ctx, n_a, n_b, WAVES), dim3(BLOCK), 0, ctx->stream, d_a, d_ao, n_a, d_b, d_bo, n_b, d_sh))
        return rc;
    call.back(shared, (const uint32_t *)d_sh, cells);
    return call.finish();
}
