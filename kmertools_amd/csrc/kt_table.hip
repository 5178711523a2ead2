// kt_table.hip - the k-mer table (kt_ctr) as an object: its lifetime, the form it is in and the transitions between the
// forms (kt::TableForm, kt_internal.hpp), the two gates everything else enters a table by (ktl::table_ready for readers,
// ktl::table_write for probing writers), and the one export by form behind kt_ctr_export, kt_ctr_export_stage[_range] and
// kt_ctr_export_fetch - with the kernels only these launch.  The counting entry points, erase and the walkers are
// kt_ctr.hip's; the partition passes, the range builds and the bulk job kt_bulk.hip's.
#include "kt_internal.hpp"
#include "kt_launch.hpp"
#include "kt_table.hpp"

namespace {

using kt::TableForm;
using kttab::BUILD_T;
using kttab::Slot;
using kttab::TileShared;
using kttab::XPT;
using kttab::XTILE;

constexpr int BLOCK = kttab::BLOCK;
constexpr uint32_t S = kttab::RANGE_FULL;  // hash positions per range

__global__ __launch_bounds__(BLOCK) void table_clear_kernel(Slot *__restrict__ slots, uint64_t cap) {
    const uint4 empty = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < cap; i += (uint64_t)gridDim.x * BLOCK)
        reinterpret_cast<uint4 *>(slots)[i] = empty;
}

// stream the table, compact occupied slots.  A workgroup takes tiles of 4096 slots (16 coalesced 16-byte loads per
// thread, all in flight at once), ballots every load, scans the 64 (wave, load) popcounts and reserves the tile's
// output range with ONE cursor atomic; every store instruction then writes one contiguous run.  (The first version
// took one atomic per wave and 64 slots: 100 M atomics on one address for a 6.4 G-slot table = 1.2 s.)
#ifndef KT_EXPORT_NT
#define KT_EXPORT_NT 0  // bit 0: non-temporal loads of the slots, bit 1: non-temporal stores of the pairs (measured, see DESIGN)
#endif

// FILTER (kt_ctr_export_stage_range): only the slots whose occurrences lie in [lo, hi] are in the ballot
template <bool FILTER = false>
__global__ __launch_bounds__(BLOCK) void table_export_kernel(const Slot *__restrict__ slots, uint64_t cap,
                                                             uint64_t *__restrict__ out_keys,
                                                             uint32_t *__restrict__ out_counts, uint64_t max_out,
                                                             uint64_t *__restrict__ cursor, uint32_t lo,
                                                             uint32_t hi) {
    __shared__ TileShared sm;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint64_t n_tiles = (cap + XTILE - 1) / XTILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint4 v[XPT];
#pragma unroll
        for (uint32_t j = 0; j < XPT; j++) {
            const uint64_t i = tile * XTILE + (uint64_t)j * BLOCK + tid;
#if KT_EXPORT_NT & 1
            typedef uint32_t raw4 __attribute__((ext_vector_type(4)));
            if (i < cap) {
                const raw4 r = __builtin_nontemporal_load(reinterpret_cast<const raw4 *>(slots) + i);
                v[j] = make_uint4(r.x, r.y, r.z, r.w);
            } else {
                v[j] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);
            }
#else
            v[j] = i < cap ? reinterpret_cast<const uint4 *>(slots)[i] : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);
#endif
        }
        uint64_t bal[XPT];
#pragma unroll
        for (uint32_t j = 0; j < XPT; j++) {
            if constexpr (FILTER) {
                const uint32_t occ = v[j].z + 1u;
                bal[j] = __ballot((v[j].x & v[j].y) != 0xFFFFFFFFu && occ >= lo && occ <= hi);
            } else {
                bal[j] = __ballot((v[j].x & v[j].y) != 0xFFFFFFFFu);  // key != KT_EMPTY_KEY
            }
        }
        const uint64_t base = sm.reserve(bal, cursor);
#pragma unroll
        for (uint32_t j = 0; j < XPT; j++) {
            if ((bal[j] >> lane) & 1ull) {
                const uint64_t pos = sm.pos(base, bal[j], j);
                if (pos < max_out) {
#if KT_EXPORT_NT & 2
                    __builtin_nontemporal_store(((uint64_t)v[j].y << 32) | v[j].x, out_keys + pos);
                    __builtin_nontemporal_store(v[j].z + 1u, out_counts + pos);
#else
                    out_keys[pos] = ((uint64_t)v[j].y << 32) | v[j].x;
                    out_counts[pos] = v[j].z + 1u;  // stored value is occurrences - 1
#endif
                }
            }
        }
        ktd::lds_barrier();  // the reservation's LDS is rewritten by the next tile
    }
}

// (key, occurrences) pairs -> the entries with lo <= occurrences <= hi, compacted (kt_ctr_export_stage_range over a table
// whose entries are an export target's arrays).  The tiles of table_export_kernel over 4-byte counts; a key is read only
// for an entry that is kept and fits: with max_out = 0 the kernel only counts, and reads the counts alone.
__global__ __launch_bounds__(BLOCK) void pairs_filter_kernel(const uint64_t *__restrict__ keys,
                                                             const uint32_t *__restrict__ counts, uint64_t n,
                                                             uint32_t lo, uint32_t hi, uint64_t *__restrict__ out_keys,
                                                             uint32_t *__restrict__ out_counts, uint64_t max_out,
                                                             uint64_t *__restrict__ cursor) {
    __shared__ TileShared sm;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint64_t n_tiles = (n + XTILE - 1) / XTILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint32_t c[XPT];
#pragma unroll
        for (uint32_t j = 0; j < XPT; j++) {
            const uint64_t i = tile * XTILE + (uint64_t)j * BLOCK + tid;
            c[j] = i < n ? counts[i] : 0u;
        }
        uint64_t bal[XPT];
#pragma unroll
        for (uint32_t j = 0; j < XPT; j++) {
            const uint64_t i = tile * XTILE + (uint64_t)j * BLOCK + tid;
            bal[j] = __ballot(i < n && c[j] >= lo && c[j] <= hi);
        }
        const uint64_t base = sm.reserve(bal, cursor);
#pragma unroll
        for (uint32_t j = 0; j < XPT; j++) {
            if ((bal[j] >> lane) & 1ull) {
                const uint64_t pos = sm.pos(base, bal[j], j);
                if (pos < max_out) {
                    out_keys[pos] = keys[tile * XTILE + (uint64_t)j * BLOCK + tid];
                    out_counts[pos] = c[j];
                }
            }
        }
        ktd::lds_barrier();
    }
}

// dense -> image, in place: one workgroup per range reads the range's packed entries, inserts them into the LDS image
// (distinct keys: plain CAS probing, counts carried along) and writes the whole range
__global__ __launch_bounds__(BUILD_T) void materialize_kernel(Slot *__restrict__ slots, uint32_t RS, uint64_t n_ranges,
                                                              uint32_t shift, uint32_t m8, uint32_t kbits,
                                                              const uint32_t *__restrict__ range_counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    unsigned long long *const skeys = reinterpret_cast<unsigned long long *>(smem_raw);
    uint32_t *const scounts = reinterpret_cast<uint32_t *>(smem_raw + (size_t)RS * 8);
    const uint32_t tid = threadIdx.x;
    for (uint64_t r = blockIdx.x; r < n_ranges; r += gridDim.x) {
        for (uint32_t i = tid; i < RS; i += BUILD_T) {
            skeys[i] = KT_EMPTY_KEY;
            scounts[i] = 0;
        }
        ktd::lds_barrier();
        const uint32_t D = range_counts[r];
        uint4 *rs = reinterpret_cast<uint4 *>(slots + r * RS);
        const uint64_t *dkeys = reinterpret_cast<const uint64_t *>(rs);  // the dense layout: keys[D], counts[D] at 8 * RS
        const uint32_t *dcounts = reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(rs) + (size_t)RS * 8);
        for (uint32_t i = tid; i < D; i += BUILD_T) {
            const uint64_t key = dkeys[i];
            const uint32_t cnt = dcounts[i];
            uint32_t s = (((uint32_t)(ktd::khash_k(key, kbits) >> shift) & (S - 1)) * m8) >> 3;
            while (atomicCAS(&skeys[s], (unsigned long long)KT_EMPTY_KEY, (unsigned long long)key) != KT_EMPTY_KEY)
                s = s + 1 == RS ? 0 : s + 1;  // (D <= RS: a free slot exists)
            scounts[s] = cnt;
        }
        ktd::lds_barrier();  // (the image below overwrites what was just read: everything is in LDS by now)
        for (uint32_t i = tid; i < RS; i += BUILD_T) {
            const uint64_t key = skeys[i];
            typedef uint32_t raw4 __attribute__((ext_vector_type(4)));
            const raw4 raw = {(uint32_t)key, (uint32_t)(key >> 32), scounts[i], 0u};
            __builtin_nontemporal_store(raw, reinterpret_cast<raw4 *>(rs + i));
        }
        ktd::lds_barrier();
    }
}

// ---- dense table -> (keys, counts) ----------------------------------------------------------------------------
// Ranges are taken in tiles of 256: tile sums (coalesced), a one-workgroup scan of the tile sums, and the copy kernel
// scans the 256 counts of its tile itself - every read and write coalesced, no atomics, output in range order.
constexpr uint32_t XT = 256;
__global__ __launch_bounds__(XT) void tile_sums_kernel(const uint32_t *__restrict__ counts, uint64_t n,
                                                       uint64_t *__restrict__ tile_sums) {
    __shared__ uint32_t part[XT / 64];
    const uint64_t i = (uint64_t)blockIdx.x * XT + threadIdx.x;
    const uint32_t v = ktd::wave_sum(i < n ? counts[i] : 0u);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = (uint64_t)part[0] + part[1] + part[2] + part[3];
}
// tile_sums[t] -> exclusive prefix; tile_sums[n_tiles] = total.  One workgroup, tiles in chunks of 1024.
__global__ __launch_bounds__(1024) void tile_scan_kernel(uint64_t *__restrict__ tile_sums, uint64_t n_tiles) {
    __shared__ uint64_t wtot[16];
    __shared__ uint64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint64_t c0 = 0; c0 < n_tiles; c0 += 1024) {
        const uint64_t i = c0 + threadIdx.x;
        const uint64_t v = i < n_tiles ? tile_sums[i] : 0;
        const uint64_t inc = ktd::wave_prefix(v);
        if ((threadIdx.x & 63) == 63) wtot[threadIdx.x >> 6] = inc;
        __syncthreads();
        uint64_t base = carry;
        for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) base += wtot[w];
        if (i < n_tiles) tile_sums[i] = base + inc - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = base + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) tile_sums[n_tiles] = carry;
}
// the counting pass of a filtered export (export_entries over a Dense table): kept[r] = entries of range r with lo <= occurrences
// <= hi, tile_sums[tile] = their sum over the tile's 256 ranges.  A wave per range, four 16-byte loads of counts in
// flight per lane.
__global__ __launch_bounds__(XT) void dense_kept_kernel(const Slot *__restrict__ slots, uint32_t RS, uint64_t n_ranges,
                                                        const uint32_t *__restrict__ range_counts, uint32_t lo, uint32_t hi,
                                                        uint32_t *__restrict__ kept, uint64_t *__restrict__ tile_sums) {
    __shared__ uint32_t wsum[XT / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t r0 = (uint64_t)blockIdx.x * XT;
    uint32_t mine = 0;
    for (uint32_t r = wave; r < XT && r0 + r < n_ranges; r += XT / 64) {
        const uint32_t D = range_counts[r0 + r], nq = (D + 3u) / 4u;
        const uint4 *q = reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(slots + (r0 + r) * RS) + (size_t)RS * 8);
        uint32_t k = 0;
        for (uint32_t q0 = 0; q0 < nq; q0 += 256) {
            uint4 v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t qi = q0 + 64u * u + lane;
                v[u] = qi < nq ? q[qi] : make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t e = (q0 + 64u * u + lane) * 4u;
                const uint32_t c0 = v[u].x + 1u, c1 = v[u].y + 1u, c2 = v[u].z + 1u, c3 = v[u].w + 1u;  // occurrences
                k += (e < D && c0 >= lo && c0 <= hi) + (e + 1u < D && c1 >= lo && c1 <= hi) +
                     (e + 2u < D && c2 >= lo && c2 <= hi) + (e + 3u < D && c3 >= lo && c3 <= hi);
            }
        }
        k = ktd::wave_sum(k);
        if (lane == 0) kept[r0 + r] = k;
        mine += k;  // (lane 0's sum is the wave's)
    }
    if (lane == 0) wsum[wave] = mine;
    __syncthreads();
    if (tid == 0) tile_sums[blockIdx.x] = (uint64_t)wsum[0] + wsum[1] + wsum[2] + wsum[3];
}
// FILTER: the ranges' offsets come from kept[] (dense_kept_kernel) and only the entries with lo <= occurrences <= hi are
// copied (a ballot per 64 entries, in the range's order)
template <bool FILTER>
__global__ __launch_bounds__(XT) void dense_export_kernel(const Slot *__restrict__ slots, uint32_t RS, uint64_t n_ranges,
                                                          const uint32_t *__restrict__ range_counts,
                                                          const uint64_t *__restrict__ tile_offsets,
                                                          uint64_t *__restrict__ out_keys,
                                                          uint32_t *__restrict__ out_counts, uint64_t max_out,
                                                          const uint32_t *__restrict__ kept, uint32_t lo, uint32_t hi) {
    __shared__ uint32_t offs[XT + 1], cnt[XT], wt[XT / 64];
    const uint32_t tid = threadIdx.x;
    const uint64_t r0 = (uint64_t)blockIdx.x * XT;
    const uint32_t c = r0 + tid < n_ranges ? (FILTER ? kept : range_counts)[r0 + tid] : 0u;
    const uint32_t inc = ktd::wave_prefix(c);
    if ((tid & 63) == 63) wt[tid >> 6] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t w = 0; w < (tid >> 6); w++) base += wt[w];
    offs[tid] = base + inc - c;
    cnt[tid] = c;
    __syncthreads();
    const uint64_t t0 = tile_offsets[blockIdx.x];
    if constexpr (FILTER) {
        const uint32_t lane = tid & 63u;
        for (uint32_t r = tid >> 6; r < XT && r0 + r < n_ranges; r += XT / 64) {
            const uint32_t D = range_counts[r0 + r];
            uint64_t o = t0 + offs[r];
            const char *rs = reinterpret_cast<const char *>(slots + (r0 + r) * RS);
            const uint64_t *dkeys = reinterpret_cast<const uint64_t *>(rs);
            const uint32_t *dcounts = reinterpret_cast<const uint32_t *>(rs + (size_t)RS * 8);
            for (uint32_t i0 = 0; i0 < D; i0 += 256) {
                uint32_t vc[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const uint32_t i = i0 + 64u * u + lane;
                    vc[u] = i < D ? dcounts[i] + 1u : 0u;  // occurrences (0: beyond the range's entries)
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const uint32_t i = i0 + 64u * u + lane;
                    const bool keep = i < D && vc[u] >= lo && vc[u] <= hi;
                    const uint64_t bal = __ballot(keep);
                    if (keep) {
                        const uint64_t at = o + __popcll(bal & ((1ull << lane) - 1ull));
                        if (at < max_out) {
                            out_keys[at] = dkeys[i];
                            out_counts[at] = vc[u];
                        }
                    }
                    o += __popcll(bal);
                }
            }
        }
        return;
    }
    // every wave copies ranges of its own (no workgroup barrier in the loop), four loads in flight per lane
    for (uint32_t r = tid >> 6; r < XT && r0 + r < n_ranges; r += XT / 64) {
        const uint32_t D = cnt[r];
        const uint64_t o = t0 + offs[r];
        const char *rs = reinterpret_cast<const char *>(slots + (r0 + r) * RS);
        const uint64_t *dkeys = reinterpret_cast<const uint64_t *>(rs);
        const uint32_t *dcounts = reinterpret_cast<const uint32_t *>(rs + (size_t)RS * 8);
        for (uint32_t i0 = tid & 63u; i0 < D; i0 += 256) {
            uint64_t vk[4];
            uint32_t vc[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t i = i0 + 64u * u;
                vk[u] = i < D ? dkeys[i] : 0;
                vc[u] = i < D ? dcounts[i] : 0;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t i = i0 + 64u * u;
                if (i < D && o + i < max_out) {
                    out_keys[o + i] = vk[u];
                    out_counts[o + i] = vc[u] + 1u;  // stored value is occurrences - 1
                }
            }
        }
    }
}

// flag 2 / any other flag of the table: the export target was too small / a range was full
int check_overflow(kt_ctr *ctr) {
    uint32_t flag = 0;
    KT_HIP(hipMemcpyAsync(&flag, ctr->flags, sizeof(uint32_t), hipMemcpyDeviceToHost, ctr->ctx->stream));
    KT_HIP(hipStreamSynchronize(ctr->ctx->stream));
    if (flag & 2u)  // (set by the range build that writes straight into the export target, kt_bulk.hip)
        return kt::fail(KT_ERR_ARG, "kt_ctr_export_target: the arrays are smaller than the table (its contents are lost: "
                                    "kt_ctr_clear, then count again with larger arrays or without a target)");
    if (flag) return kt::fail(KT_ERR_FULL, "k-mer table is full: raise capacity_slots");
    return KT_OK;
}

// The probing image, whatever form the table is in.  Clearing is deferred: the bulk build (kt_bulk.hip) overwrites every
// slot, so a clear that is followed by a whole-batch kt_ctr_add_reads never has to touch the table.
int ensure_cleared(kt_ctr *ctr) {
    switch (ctr->form()) {
    case TableForm::Stale:
        if (int rc = ktl::table_wipe(ctr)) return rc;
        ctr->imaged();
        return KT_OK;
    case TableForm::Image: return KT_OK;
    default: return kt_table_image(ctr);
    }
}

// a Target-form table's pairs, *ctr->distinct of them, through the probing path into the cleared slots (the rare road: a
// table that was counted into its export arrays and is then added to or probed after all)
int load_target_pairs(kt_ctr *ctr) {
    kt_ctx *ctx = ctr->ctx;
    if (int rc = ctx->use()) return rc;
    uint64_t n = 0;
    KT_HIP(hipMemcpyAsync(&n, ctr->distinct, 8, hipMemcpyDeviceToHost, ctx->stream));
    KT_HIP(hipStreamSynchronize(ctx->stream));
    if (int rc = check_overflow(ctr)) return rc;  // (arrays that were too small hold nothing usable)
    if (int rc = ktl::table_wipe(ctr)) return rc;
    KT_HIP(hipMemsetAsync(ctr->distinct, 0, 8, ctx->stream));
    if (n == 0) return KT_OK;
    return ktl::add_pairs(ctr, ktl::writable_of(ctr), ctr->xt_keys, ctr->xt_counts, n);
}

}  // namespace

int ktl::table_wipe(kt_ctr *ctr) {
    return launch(table_clear_kernel, dim3(grid_for(ctr->ctx, (ctr->cap + BLOCK - 1) / BLOCK, 8)), dim3(BLOCK), 0, ctr->ctx->stream,
                  (Slot *)ctr->slots, ctr->cap);
}

int ktl::table_ready(kt_ctr *ctr) {
    if (int rc = ensure_cleared(ctr)) return rc;
    return check_overflow(ctr);
}

int ktl::table_write(kt_ctr *ctr, kttab::TableRef *t) {
    ctr->stage.drop();  // the table changes: what was staged is no longer the table (kt_ctr_export_fetch says so)
    ctr->written();
    if (int rc = ensure_cleared(ctr)) return rc;
    *t = writable_of(ctr);
    return KT_OK;
}

// the probing image of a Dense table (in place) or a Target-form one (from the target's pairs); no-op otherwise
int kt_table_image(kt_ctr *ctr) {
    kt_ctx *ctx = ctr->ctx;
    switch (ctr->form()) {
    case TableForm::Target:
        // the entries are the caller's export arrays: back into the emptied slots, as (key, count) pairs.  The arrays are the
        // caller's to reuse from here on - whether or not the load succeeds - so a stage that points at them goes with them: a
        // fetch must not hand out what the caller has put there since (kt_ctr_export_fetch says "stage first")
        ctr->imaged();
        if (ctr->stage.aliases(ctr->xt_keys)) ctr->stage.drop();
        return load_target_pairs(ctr);
    case TableForm::Dense: {
        const uint32_t RS = ktl::geom_of(ctr).range_slots();
        const uint64_t n_ranges = ctr->cap / RS;
        uint64_t g = (uint64_t)ctx->n_cu * 4;
        if (g > n_ranges) g = n_ranges;
        if (int rc = ktl::launch(materialize_kernel, dim3((uint32_t)g), dim3(BUILD_T), (size_t)RS * 12, ctx->stream, (Slot *)ctr->slots,
                                 RS, n_ranges, ctr->shift, ctr->m8, ctr->kbits, ctr->range_counts))
            return rc;
        ctr->imaged();
        return KT_OK;
    }
    default: return KT_OK;
    }
}

namespace {

struct Pairs { uint64_t *keys; uint32_t *counts; uint64_t room; };  // device arrays and the entries they have room for
constexpr uint64_t WHOLE_TABLE = ~0ull;

// Export by form: the table's entries with lo <= occurrences <= hi, from whatever form the table is in, into device
// arrays; *n = how many there are (those beyond the arrays' room are not written).  `dest(bound, &arrays)` names the
// arrays, asked once and only when something will be written: bound = the most entries that can come, where the form
// tells before the copy (WHOLE_TABLE: up to the table's size).  `in_place`: a caller that only needs the entries
// somewhere in device memory - a Target-form table asked for all of them then answers with the target's own arrays in
// *at and copies nothing; otherwise *at = what dest named.  `size`: the table's size where the caller has read it (null:
// a Target-form table reads it here).
template <class Dest>
int export_entries(kt_ctr *ctr, const uint64_t *size, uint32_t lo, uint32_t hi, bool in_place, Dest &&dest, Pairs *at, uint64_t *n) {
    kt_ctx *ctx = ctr->ctx;
    hipStream_t st = ctx->stream;
    const bool all = lo <= 1u && hi == 0xFFFFFFFFu;
    if (all) lo = 1u;
    *at = Pairs{};
    switch (ctr->form()) {
    case TableForm::Target: {  // entries [0, *distinct) of the export target
        uint64_t held = size ? *size : 0;
        if (!size) {
            KT_HIP(hipMemcpyAsync(&held, ctr->distinct, 8, hipMemcpyDeviceToHost, st));
            KT_HIP(hipStreamSynchronize(st));
        }
        if (all) {  // nothing to do where the caller wants them there, a plain copy otherwise
            *n = held;
            *at = Pairs{ctr->xt_keys, ctr->xt_counts, held};
            if (in_place) return KT_OK;
            if (int rc = dest(held, at)) return rc;
            const uint64_t w = held < at->room ? held : at->room;
            if (w && at->keys != ctr->xt_keys) KT_HIP(hipMemcpyAsync(at->keys, ctr->xt_keys, w * 8, hipMemcpyDeviceToDevice, st));
            if (w && at->counts != ctr->xt_counts) KT_HIP(hipMemcpyAsync(at->counts, ctr->xt_counts, w * 4, hipMemcpyDeviceToDevice, st));
            KT_HIP(hipStreamSynchronize(st));
            return KT_OK;
        }
        // counted first, so that the arrays need room for the kept entries only; then compacted
        const dim3 grid(ktl::grid_for(ctx, (held + XTILE - 1) / XTILE, 8));
        KT_HIP(hipMemsetAsync(ctr->cursor, 0, 8, st));
        if (int rc = ktl::launch(pairs_filter_kernel, grid, dim3(BLOCK), 0, st, ctr->xt_keys, ctr->xt_counts, held, lo, hi, nullptr,
                                 nullptr, 0ull, ctr->cursor))
            return rc;
        KT_HIP(hipMemcpyAsync(n, ctr->cursor, 8, hipMemcpyDeviceToHost, st));
        KT_HIP(hipStreamSynchronize(st));
        if (!*n) return KT_OK;
        if (int rc = dest(*n, at)) return rc;
        KT_HIP(hipMemsetAsync(ctr->cursor, 0, 8, st));
        if (int rc = ktl::launch(pairs_filter_kernel, grid, dim3(BLOCK), 0, st, ctr->xt_keys, ctr->xt_counts, held, lo, hi, at->keys,
                                 at->counts, at->room, ctr->cursor))
            return rc;
        KT_HIP(hipStreamSynchronize(st));
        return KT_OK;
    }
    case TableForm::Dense: {
        // packed ranges: tile sums of the ranges' entries (filtered: a counting pass, kept per range), the tile scan, a coalesced
        // copy.  Scratch: the tile offsets and, filtered, one u32 per range behind them, in the context's AUX0.
        if (int rc = dest(WHOLE_TABLE, at)) return rc;
        const uint32_t RS = ktl::geom_of(ctr).range_slots();
        const uint64_t n_ranges = ctr->cap / RS, n_tiles = (n_ranges + XT - 1) / XT;
        const dim3 tiles_grid((uint32_t)n_tiles);
        uint64_t *tiles = nullptr;
        if (int rc = ctx->claim(kt::AUX0, (n_tiles + 1) * 8 + (all ? 0 : n_ranges * 4), all ? "kt_table_dense_export" : "kt_table_dense_export_range", &tiles))
            return rc;
        uint32_t *kept = all ? nullptr : (uint32_t *)(tiles + n_tiles + 1);
        const Slot *slots = (const Slot *)ctr->slots;
        if (int rc = all ? ktl::launch(tile_sums_kernel, tiles_grid, dim3(XT), 0, st, ctr->range_counts, n_ranges, tiles)
                         : ktl::launch(dense_kept_kernel, tiles_grid, dim3(XT), 0, st, slots, RS, n_ranges, ctr->range_counts, lo, hi, kept, tiles))
            return rc;
        if (int rc = ktl::launch(tile_scan_kernel, dim3(1), dim3(1024), 0, st, tiles, n_tiles)) return rc;
        if (at->room)
            if (int rc = ktl::launch(all ? dense_export_kernel<false> : dense_export_kernel<true>, tiles_grid, dim3(XT), 0, st, slots, RS,
                                     n_ranges, ctr->range_counts, tiles, at->keys, at->counts, at->room, kept, lo, hi))
                return rc;
        KT_HIP(hipMemcpyAsync(n, tiles + n_tiles, 8, hipMemcpyDeviceToHost, st));
        KT_HIP(hipStreamSynchronize(st));
        return KT_OK;
    }
    default:  // the probing image (a deferred clear first): the export ballot, with the predicate in it when filtered
        if (int rc = ensure_cleared(ctr)) return rc;
        if (int rc = dest(WHOLE_TABLE, at)) return rc;
        KT_HIP(hipMemsetAsync(ctr->cursor, 0, 8, st));
        if (int rc = ktl::launch(all ? table_export_kernel<false> : table_export_kernel<true>, dim3(ktl::grid_for(ctx, (ctr->cap + XTILE - 1) / XTILE, 8)),
                                 dim3(BLOCK), 0, st, (const Slot *)ctr->slots, ctr->cap, at->keys, at->counts, at->room, ctr->cursor,
                                 lo, hi))
            return rc;
        KT_HIP(hipMemcpyAsync(n, ctr->cursor, 8, hipMemcpyDeviceToHost, st));
        KT_HIP(hipStreamSynchronize(st));
        return KT_OK;
    }
}

}  // namespace

using namespace ktl;

extern "C" {

int kt_ctr_create(kt_ctx *ctx, int k, uint64_t capacity_slots, kt_ctr **out) {
    if (!ctx || !out) return kt::fail(KT_ERR_ARG, "kt_ctr_create: null");
    *out = nullptr;
    if (k < 1 || k > 31) return kt::fail(KT_ERR_ARG, "kt_ctr_create: k must be in 1..31");
    if (int rc = ctx->use()) return rc;
    const kttab::Geom geom = kttab::make_geom(capacity_slots, k);
    const uint64_t cap = geom.cap;
    kt_ctr *c = new (std::nothrow) kt_ctr();
    if (!c) return kt::fail(KT_ERR_NOMEM, "kt_ctr_create: host alloc");
    c->ctx = ctx;
    c->k = k;
    c->cap = cap;
    c->shift = geom.shift;
    c->m8 = geom.m8;
    c->kbits = geom.kbits;
    hipError_t e = hipMalloc((void **)&c->slots, cap * sizeof(Slot));
    if (e == hipSuccess) e = hipMalloc((void **)&c->flags, 64);
    if (e == hipSuccess) e = hipMalloc((void **)&c->cursor, 64);
    if (e == hipSuccess) e = hipMalloc((void **)&c->distinct, 64);
    if (e == hipSuccess) e = hipMalloc((void **)&c->range_counts, (cap / geom.range_slots() + 1) * sizeof(uint32_t));
    if (e != hipSuccess) {
        kt_ctr_destroy(c);
        return kt::fail(KT_ERR_NOMEM, std::string("kt_ctr_create: hipMalloc: ") + hipGetErrorString(e));
    }
    *out = c;
    return kt_ctr_clear(c);
}

int kt_ctr_destroy(kt_ctr *ctr) {
    if (!ctr) return KT_OK;
    if (ctr->ctx) {
        (void)hipSetDevice(ctr->ctx->device);
        (void)hipStreamSynchronize(ctr->ctx->stream);
    }
    for (void *p : {ctr->slots, (void *)ctr->flags, (void *)ctr->cursor, (void *)ctr->distinct, (void *)ctr->range_counts})
        if (p) (void)hipFree(p);
    for (kt::Scratch *b : {&ctr->b_ext, &ctr->b_stage_k, &ctr->b_stage_c, &ctr->b_keys1, &ctr->b_keys2, &ctr->b_meta, &ctr->b_desc, &ctr->b_pack})
        b->release();
    kt_bulk_job_free(ctr->job);
    delete ctr;
    return KT_OK;
}

int kt_ctr_clear(kt_ctr *ctr) {
    if (!ctr) return kt::fail(KT_ERR_ARG, "kt_ctr_clear: null");
    if (int rc = ctr->ctx->use()) return rc;
    KT_HIP(hipMemsetAsync(ctr->flags, 0, 64, ctr->ctx->stream));
    KT_HIP(hipMemsetAsync(ctr->distinct, 0, 8, ctr->ctx->stream));
    ctr->cleared();
    ctr->stage.drop();  // (what kt_ctr_export_stage staged is gone with the table's contents)
    return KT_OK;
}

int kt_ctr_export_target(kt_ctr *ctr, uint64_t *keys_dev, uint32_t *counts_dev, uint64_t max_out) {
    if (!ctr) return kt::fail(KT_ERR_ARG, "kt_ctr_export_target: null ctr");
    if ((keys_dev == nullptr) != (counts_dev == nullptr))
        return kt::fail(KT_ERR_ARG, "kt_ctr_export_target: both arrays or neither");
    if (int rc = ctr->ctx->use()) return rc;
    // a table whose entries live in the current target gets its own copy (the probing image) before the target moves
    if (ctr->form() == TableForm::Target && (keys_dev != ctr->xt_keys || counts_dev != ctr->xt_counts))
        if (int rc = kt_table_image(ctr)) return rc;
    ctr->xt_keys = keys_dev;
    ctr->xt_counts = counts_dev;
    ctr->xt_max = keys_dev ? max_out : 0;
    ctr->stage.drop();  // (what was staged may have been the old target's arrays; dropped for the same arrays too)
    return KT_OK;
}

int kt_ctr_capacity(kt_ctr *ctr, uint64_t *slots) {
    if (!ctr || !slots) return kt::fail(KT_ERR_ARG, "kt_ctr_capacity: null");
    *slots = ctr->cap;
    return KT_OK;
}

int kt_ctr_size(kt_ctr *ctr, uint64_t *distinct) {
    if (!ctr || !distinct) return kt::fail(KT_ERR_ARG, "kt_ctr_size: null");
    kt_ctx *ctx = ctr->ctx;
    if (int rc = ctx->use()) return rc;
    // every insert path keeps the count of occupied slots (claims in the probing kernels, placed keys in the range
    // builds), so the size is one 8-byte read - not a scan of the table
    KT_HIP(hipMemcpyAsync(distinct, ctr->distinct, 8, hipMemcpyDeviceToHost, ctx->stream));
    KT_HIP(hipStreamSynchronize(ctx->stream));
    return check_overflow(ctr);
}

int kt_ctr_export(kt_ctr *ctr, uint64_t *keys, uint32_t *counts, uint64_t max_out, uint64_t *n_out, int mem) {
    if (!ctr || !n_out) return kt::fail(KT_ERR_ARG, "kt_ctr_export: null");
    kt_ctx *ctx = ctr->ctx;
    Call call(ctx, mem, "kt_ctr_export");
    if (int rc = call.enter()) return rc;
    if (max_out && (!keys || !counts)) return call.fail("null output");
    if (int rc = check_overflow(ctr)) return rc;
    Pairs mine{keys, counts, max_out}, at{};
    if (call.host() && max_out) {  // (what comes back is the entries written, known only after the pass)
        if (int rc = call.scratch(kt::AUX1, max_out * 8, &mine.keys)) return rc;
        if (int rc = call.scratch(kt::AUX2, max_out * 4, &mine.counts)) return rc;
    }
    // (to host memory a Target-form table is copied straight from its target: the build's output IS the export)
    uint64_t n = 0;
    auto dest = [&](uint64_t, Pairs *d) { return *d = mine, (int)KT_OK; };
    if (int rc = export_entries(ctr, nullptr, 1u, 0xFFFFFFFFu, call.host(), dest, &at, &n)) return rc;
    const uint64_t written = n < max_out ? n : max_out;
    call.back(keys, (const uint64_t *)at.keys, written);
    call.back(counts, (const uint32_t *)at.counts, written);
    if (int rc = call.finish()) return rc;
    *n_out = written;
    if (n > max_out) return call.fail("max_out smaller than the table's size");
    return KT_OK;
}

// The table's entries in pieces (out-of-core callers: the host never holds more than one piece).  kt_ctr_export_stage[_range]
// puts those with min_count <= occurrences <= max_count into a device-side staging area of the library and reports how
// many; kt_ctr_export_fetch copies entries [first, first + count) to host arrays.  The staging area is the table's own
// stage buffers - of the table's size, or, filtered from a Target-form table, of what is kept - (not the context's
// scratch, which any other call on the context re-reserves); all the entries of a Target-form table are staged where they are.
int kt_ctr_export_stage_range(kt_ctr *ctr, uint32_t min_count, uint32_t max_count, uint64_t *n_out) {
    if (!ctr || !n_out) return kt::fail(KT_ERR_ARG, "kt_ctr_export_stage_range: null");
    if (min_count > max_count) return kt::fail(KT_ERR_ARG, "kt_ctr_export_stage_range: min_count > max_count");
    kt_ctx *ctx = ctr->ctx;
    kt::ClaimScope scope(ctx);
    if (int rc = ctx->use()) return rc;
    uint64_t n = 0;
    if (int rc = kt_ctr_size(ctr, &n)) return rc;
    ctr->stage.drop();
    uint64_t kept = 0;
    if (n) {
        Pairs at{};
        auto own = [&](uint64_t bound, Pairs *d) {
            const uint64_t room = bound == WHOLE_TABLE ? n : bound;
            if (int rc = ctr->b_stage_k.reserve(room * 8)) return rc;
            if (int rc = ctr->b_stage_c.reserve(room * 4)) return rc;
            *d = Pairs{(uint64_t *)ctr->b_stage_k.p, (uint32_t *)ctr->b_stage_c.p, room};
            return (int)KT_OK;
        };
        // (all the entries of a table that holds them itself used to go through kt_ctr_export, which reads the overflow flag once
        // more: redundant behind kt_ctr_size, kept so that the refactor changes no traffic at all, the runtime's copies included)
        if (min_count <= 1u && max_count == 0xFFFFFFFFu && ctr->form() != TableForm::Target)
            if (int rc = check_overflow(ctr)) return rc;
        if (int rc = export_entries(ctr, &n, min_count, max_count, true, own, &at, &kept)) return rc;
        if (kept > n) return kt::fail(KT_ERR_ARG, "kt_ctr_export_stage_range: more entries than the table's size");
        if (kept) ctr->stage.set(at.keys, at.counts, kept);
    }
    *n_out = kept;
    return KT_OK;
}

int kt_ctr_export_stage(kt_ctr *ctr, uint64_t *n_out) {
    if (!ctr || !n_out) return kt::fail(KT_ERR_ARG, "kt_ctr_export_stage: null");
    return kt_ctr_export_stage_range(ctr, 1u, 0xFFFFFFFFu, n_out);
}

int kt_ctr_export_fetch(kt_ctr *ctr, uint64_t first, uint64_t count, uint64_t *keys_host, uint32_t *counts_host) {
    if (!ctr) return kt::fail(KT_ERR_ARG, "kt_ctr_export_fetch: null");
    const kt::Stage &stage = ctr->stage;
    if (first > stage.n() || count > stage.n() - first)
        return kt::fail(KT_ERR_ARG, "kt_ctr_export_fetch: beyond the staged entries (call kt_ctr_export_stage first)");
    if (!count) return KT_OK;
    if (!keys_host || !counts_host) return kt::fail(KT_ERR_ARG, "kt_ctr_export_fetch: null output");
    kt_ctx *ctx = ctr->ctx;
    if (int rc = ctx->use()) return rc;
    KT_HIP(hipMemcpyAsync(keys_host, stage.keys() + first, count * 8, hipMemcpyDeviceToHost, ctx->stream));
    KT_HIP(hipMemcpyAsync(counts_host, stage.counts() + first, count * 4, hipMemcpyDeviceToHost, ctx->stream));
    KT_HIP(hipStreamSynchronize(ctx->stream));
    return KT_OK;
}

}  // extern "C"
