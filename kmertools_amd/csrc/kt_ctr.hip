// kt_ctr.hip - canonical k-mer counting in an HBM-resident table, plus the stand-alone hash
// partition of a batch's k-mers (kt_ctr_route: what the out-of-core passes split by), plus the
// debug k-mer generator surface (kt_kmers).
//
// Replaces CountComputer::count_chunk / merge (reference counter/src/lib.rs:92-234):
// the reference's n_parts concurrent hash maps, chunked spill to text files and
// per-partition re-merge collapse into one open-addressing table that stays in HBM
// (16-byte slots {u64 key, u32 count, pad}: the 64-bit CAS that claims a slot and the 32-bit
// atomic add that counts it touch the same 64-byte line, which halves the DRAM lines moved
// per insert compared with separate key/count arrays - profiles/r1_ctr_*).  HBM-bound
// random access; no MFMA.
#include <type_traits>
#include <vector>

#include "kt_internal.hpp"
#include "kt_launch.hpp"
#include "kt_segment.hpp"
#include "kt_table.hpp"

namespace {

using ktseg::SegArgs;
using ktseg::SegShared;

constexpr int BLOCK = ktseg::BLOCK;

// ---- table primitives: kt_table.hpp -------------------------------------------------

using kttab::Slot;
using kttab::TableRef;
using kttab::table_add;
using kttab::TileShared;  // (the tile reservation of erase_survivors_kernel, shared with kt_table.hip's export kernels)
using kttab::XPT;
using kttab::XTILE;
static_assert(BLOCK == kttab::BLOCK, "the tile reservation's workgroup");

// new keys claimed by the thread -> the table's distinct counter: one atomic per wave, at the end of the kernel
__device__ __forceinline__ void publish_fresh(uint32_t fresh, uint64_t *distinct) {
    fresh = ktd::wave_sum(fresh);
    if ((threadIdx.x & 63) == 0 && fresh)
        atomicAdd(reinterpret_cast<unsigned long long *>(distinct), (unsigned long long)fresh);
}

// keep(m): whether the canonical k-mer m is counted at all (ktpf::KeepAll; ktpf::KeepSeenTwice: kt_ctr_add_reads_filtered)
template <class Keep>
__global__ __launch_bounds__(BLOCK) void count_reads_kernel(SegArgs a, TableRef t, uint32_t n_parts, uint32_t part,
                                                            uint64_t *__restrict__ distinct, Keep keep) {
    __shared__ SegShared sm;
    uint32_t fresh = 0;
    for (uint64_t g = blockIdx.x; g < a.n_seg; g += gridDim.x) {
        ktseg::for_each_kmer(a, g, sm, [&](uint64_t f, uint64_t r, uint64_t) {
            const uint64_t m = f < r ? f : r;  // counter/src/lib.rs:124
            if (n_parts > 1 && ktd::owner_of(m, n_parts) != part) return;  // another pass counts this one
            if (!keep(m)) return;
            const uint32_t st = table_add(t, m, 1u);
            if (st == 0u) atomicOr(t.flags, 1u);
            fresh += st == 2u;
        });
    }
    publish_fresh(fresh, distinct);
}

__global__ __launch_bounds__(BLOCK) void add_pairs_kernel(const uint64_t *__restrict__ keys,
                                                          const uint32_t *__restrict__ counts, uint64_t n,
                                                          TableRef t, uint64_t *__restrict__ distinct) {
    uint32_t fresh = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t key = keys[i];
        const uint32_t c = counts ? counts[i] : 1u;
        if (key == KT_EMPTY_KEY || c == 0u) continue;  // adding 0 adds nothing: a claimed slot would mean "seen once"
        const uint32_t st = table_add(t, key, c);
        if (st == 0u) atomicOr(t.flags, 1u);
        fresh += st == 2u;
    }
    publish_fresh(fresh, distinct);
}

// ---- kt_ctr_erase: flag the slots of the keys to remove, compact the others, build the image again from them -------------
// A slot cannot simply be freed: the keys behind it in its probe chain (which may wrap at the end of the range) would be cut
// off, and a stored count has no spare value for a tombstone.  So the slots to drop are flagged in a bitmask beside the
// table (bit s of dead[]: slot s goes), the surviving pairs are compacted into scratch and the image is made anew from them.

// one thread per erase key: the key's slot in the probing image, if it has one, is flagged; the first to flag a slot counts it
__global__ __launch_bounds__(BLOCK) void erase_flag_kernel(const uint64_t *__restrict__ keys, uint64_t n, kttab::Probed t,
                                                           uint64_t key_limit, uint32_t *__restrict__ dead,
                                                           uint64_t *__restrict__ n_erased) {
    uint32_t hit = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t key = keys[i];
        if (key == KT_EMPTY_KEY || key >= key_limit) continue;
        kttab::Probe p = kttab::probe_of(key, t.g);
        for (uint32_t probe = 0; probe < p.rs; probe++) {
            const uint64_t s = p.slot();
            const uint64_t cur = t.slots[s].key;
            if (cur == KT_EMPTY_KEY) break;
            if (cur == key) {
                const uint32_t bit = 1u << (uint32_t)(s & 31u);
                hit += !(atomicOr(dead + (s >> 5), bit) & bit);
                break;
            }
            p.next();
        }
    }
    publish_fresh(hit, n_erased);
}

// table_export_kernel over the slots whose bit in dead[] is clear
__global__ __launch_bounds__(BLOCK) void erase_survivors_kernel(const Slot *__restrict__ slots, uint64_t cap,
                                                                const uint32_t *__restrict__ dead, uint64_t *__restrict__ out_keys,
                                                                uint32_t *__restrict__ out_counts, uint64_t max_out,
                                                                uint64_t *__restrict__ cursor) {
    __shared__ TileShared sm;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint64_t n_tiles = (cap + XTILE - 1) / XTILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint4 v[XPT];
        uint64_t bal[XPT];
#pragma unroll
        for (uint32_t j = 0; j < XPT; j++) {
            const uint64_t i = tile * XTILE + (uint64_t)j * BLOCK + tid;
            v[j] = i < cap ? reinterpret_cast<const uint4 *>(slots)[i] : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);
            const bool gone = i < cap && (dead[i >> 5] >> (uint32_t)(i & 31u) & 1u);
            bal[j] = __ballot((v[j].x & v[j].y) != 0xFFFFFFFFu && !gone);
        }
        const uint64_t base = sm.reserve(bal, cursor);
#pragma unroll
        for (uint32_t j = 0; j < XPT; j++) {
            if ((bal[j] >> lane) & 1ull) {
                const uint64_t pos = sm.pos(base, bal[j], j);
                if (pos < max_out) {
                    out_keys[pos] = ((uint64_t)v[j].y << 32) | v[j].x;
                    out_counts[pos] = v[j].z + 1u;  // stored value is occurrences - 1
                }
            }
        }
        ktd::lds_barrier();  // the reservation's LDS is rewritten by the next tile
    }
}

// ---- a table's entries in the form they are in (view_of builds it; the walks of spectrum, compare, setop, graph and hetmers read it) ---------
// The form is the kernels' template argument; the view holds what they read.
enum Form { FORM_PROBE = 0, FORM_DENSE = 1, FORM_PAIRS = 2 };
struct TableView {
    const void *src;         // FORM_PROBE: the slots [n) (16-byte slots; stored count = occurrences - 1, KT_EMPTY_KEY free);
                             // FORM_DENSE: the n ranges of a dense table, RS slots each, range r's range_counts[r] keys from its
                             // start and counts (occurrences - 1) from byte 8 * RS on; FORM_PAIRS: n keys (an export target's)
    const uint32_t *counts;  // FORM_PAIRS: the keys' occurrences, from anywhere (a caller's array): `head` = how many
                             // counts of its first aligned 16 bytes lie before the array
    uint64_t n;
    uint32_t RS, head;
    const uint32_t *range_counts;
};

// The entry walk: every thread of the workgroup calls it, and `step` gets the lane's next UNROLL (key, occurrences) pairs -
// KT_EMPTY_KEY: no entry - until the grid has covered the table.  The flat forms go by grid-stride tiles of BLOCK * UNROLL
// slots / pairs; a dense table is walked a wave per range, BLOCK / 64 consecutive ranges per workgroup step, coalesced.
// UNIFORM: every wave takes the steps of the longest of the workgroup's ranges (for a `step` with barriers in it; the flat
// forms are uniform anyway); otherwise a wave takes its own range's steps only.  The uniform walk reads range_counts
// through the scalar cache (ktd::load_uniform), so nothing may write range_counts while the kernel runs - a kernel that
// walks a table must not change that table (its stores would also keep a plain uniform load off the scalar unit).
template <int FORM, uint32_t UNROLL, bool UNIFORM, class Step>
__device__ __forceinline__ void walk_entries(const TableView &t, Step &&step) {
    const uint32_t tid = threadIdx.x;
    uint64_t key[UNROLL];
    uint32_t cnt[UNROLL];
    if constexpr (FORM == FORM_DENSE) {
        constexpr uint32_t WAVES = BLOCK / 64;
        const uint32_t lane = tid & 63u, wave = tid >> 6;
        for (uint64_t r0 = (uint64_t)blockIdx.x * WAVES; r0 < t.n; r0 += (uint64_t)gridDim.x * WAVES) {
            uint32_t D = 0, D_max = 0;  // the entries of this wave's range, and how far the wave steps
            if constexpr (UNIFORM) {     // (loads through the scalar cache: the step count stays on the scalar unit)
#pragma unroll
                for (uint32_t w = 0; w < WAVES; w++) {
                    const uint32_t d = r0 + w < t.n ? ktd::load_uniform(t.range_counts + r0 + w) : 0u;
                    D = w == wave ? d : D;
                    D_max = d > D_max ? d : D_max;
                }
            } else {
                D = D_max = r0 + wave < t.n ? t.range_counts[r0 + wave] : 0u;
            }
            const char *base = reinterpret_cast<const char *>(t.src) + (r0 + wave) * t.RS * 16ull;  // (read only below D)
            const uint64_t *keys = reinterpret_cast<const uint64_t *>(base);
            const uint32_t *cnts = reinterpret_cast<const uint32_t *>(base + t.RS * 8ull);
            for (uint32_t e0 = 0; e0 < D_max; e0 += 64u * UNROLL) {
#pragma unroll
                for (uint32_t u = 0; u < UNROLL; u++) {
                    const uint32_t e = e0 + u * 64u + lane;
                    key[u] = e < D ? keys[e] : KT_EMPTY_KEY;
                    cnt[u] = e < D ? cnts[e] + 1u : 0u;
                }
                step(key, cnt);
            }
        }
    } else {
        constexpr uint32_t TILE = BLOCK * UNROLL;
        for (uint64_t i0 = (uint64_t)blockIdx.x * TILE; i0 < t.n; i0 += (uint64_t)gridDim.x * TILE) {
#pragma unroll
            for (uint32_t u = 0; u < UNROLL; u++) {
                const uint64_t i = i0 + u * BLOCK + tid;
                if constexpr (FORM == FORM_PROBE) {
                    const uint4 v = i < t.n ? reinterpret_cast<const uint4 *>(t.src)[i] : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);
                    key[u] = ((uint64_t)v.y << 32) | v.x;
                    cnt[u] = v.z + 1u;
                } else {
                    key[u] = i < t.n ? reinterpret_cast<const uint64_t *>(t.src)[i] : KT_EMPTY_KEY;
                    cnt[u] = i < t.n ? t.counts[i] : 0u;
                }
            }
            step(key, cnt);
        }
    }
}

// bit u = key[u] is an entry
template <uint32_t N>
__device__ __forceinline__ uint32_t present(const uint64_t (&key)[N]) {
    uint32_t m = 0;
#pragma unroll
    for (uint32_t u = 0; u < N; u++) m |= (key[u] != KT_EMPTY_KEY ? 1u : 0u) << u;
    return m;
}

// ---- the abundance spectrum (kt_ctr_spectrum) ---------------------------------------------------------------------
// One pass over what the table's form keeps, counts only (+ the keys where emptiness is in them): hist[min(c, top)] += 1
// per entry of c occurrences.  The spectrum is skewed - nearly every entry of uniform random reads has c = 1, of reads
// sampled from a genome c near the coverage - so a same-address atomic per entry would serialise a wave on one bin.
// Counts 1..SPEC_REG are tallied in registers (an unrolled compare, no dynamic indexing) and reduced once per wave at the
// end; SPEC_REG < c < SPEC_LDS go to a workgroup histogram in LDS (no-return adds, the bins of a coverage peak spread
// the lanes over many addresses); c >= SPEC_LDS to 64-bit global atomics (rare: the repeats).  Every workgroup merges
// its non-zero bins once, at the end.  The register and LDS tallies are u32: a workgroup's share of the entries is
// bounded below 2^31 by the grid (launch_walk).
constexpr uint32_t SPEC_REG = 8, SPEC_LDS = 4096, SPEC_UNROLL = 4;

struct SpecTally {
    uint32_t reg[SPEC_REG] = {};
    uint32_t n = 0;
    uint64_t occ = 0;
    __device__ __forceinline__ void add(uint32_t c, uint32_t top, uint32_t *lds, uint64_t *hist) {
        n++;
        occ += c;
        const uint32_t b = c < top ? c : top;
#pragma unroll
        for (uint32_t j = 0; j < SPEC_REG; j++) reg[j] += b == j + 1u;
        if (b > SPEC_REG) {
            if (b < SPEC_LDS) atomicAdd(&lds[b], 1u);  // (the result is unused: a no-return ds_add)
            else atomicAdd(reinterpret_cast<unsigned long long *>(hist + b), 1ull);
        }
    }
};

// Reads the view with loads of its own, not walk_entries': it needs no key where emptiness is not in the key, so the
// dense and pairs forms read the counts alone, 4 bytes per entry as aligned 16-byte quads.
template <int FORM>
__global__ __launch_bounds__(BLOCK) void spectrum_kernel(TableView tv, uint64_t *__restrict__ hist, uint32_t n_bins,
                                                         uint64_t *__restrict__ totals) {
    const uint64_t n = tv.n;
    __shared__ uint32_t lds[SPEC_LDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t top = n_bins - 1u, lds_bins = n_bins < SPEC_LDS ? n_bins : SPEC_LDS;
    for (uint32_t b = tid; b < lds_bins; b += BLOCK) lds[b] = 0u;
    ktd::lds_barrier();
    SpecTally t;
    if constexpr (FORM == FORM_PROBE) {
        const uint4 *slots = reinterpret_cast<const uint4 *>(tv.src);
        constexpr uint32_t TILE = BLOCK * SPEC_UNROLL;
        for (uint64_t i0 = (uint64_t)blockIdx.x * TILE; i0 < n; i0 += (uint64_t)gridDim.x * TILE) {
            uint4 v[SPEC_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < SPEC_UNROLL; u++) {
                const uint64_t i = i0 + u * BLOCK + tid;
                v[u] = i < n ? slots[i] : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);
            }
#pragma unroll
            for (uint32_t u = 0; u < SPEC_UNROLL; u++)
                if ((v[u].x & v[u].y) != 0xFFFFFFFFu) t.add(v[u].z + 1u, top, lds, hist);
        }
    } else if constexpr (FORM == FORM_DENSE) {
        // a wave per range: the range's counts as quads, SPEC_UNROLL 16-byte loads in flight per lane
        const uint32_t wave = tid >> 6;
        const uint64_t waves = (uint64_t)gridDim.x * (BLOCK / 64);
        for (uint64_t r = (uint64_t)blockIdx.x * (BLOCK / 64) + wave; r < n; r += waves) {
            const uint32_t D = tv.range_counts[r];
            const uint4 *q = reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(tv.src) + r * tv.RS * 16ull + tv.RS * 8ull);
            const uint32_t nq = (D + 3u) / 4u;
            for (uint32_t q0 = 0; q0 < nq; q0 += 64u * SPEC_UNROLL) {
                uint4 v[SPEC_UNROLL];
#pragma unroll
                for (uint32_t u = 0; u < SPEC_UNROLL; u++) {
                    const uint32_t qi = q0 + u * 64u + lane;
                    v[u] = qi < nq ? q[qi] : make_uint4(0u, 0u, 0u, 0u);
                }
#pragma unroll
                for (uint32_t u = 0; u < SPEC_UNROLL; u++) {
                    const uint32_t e = (q0 + u * 64u + lane) * 4u;
                    if (e < D) t.add(v[u].x + 1u, top, lds, hist);
                    if (e + 1u < D) t.add(v[u].y + 1u, top, lds, hist);
                    if (e + 2u < D) t.add(v[u].z + 1u, top, lds, hist);
                    if (e + 3u < D) t.add(v[u].w + 1u, top, lds, hist);
                }
            }
        }
    } else {
        const uint32_t head = tv.head;
        const uint4 *q = reinterpret_cast<const uint4 *>(tv.counts - head);
        const uint64_t end = n + head, nq = (end + 3u) / 4u;
        constexpr uint32_t TILE = BLOCK * SPEC_UNROLL;
        for (uint64_t q0 = (uint64_t)blockIdx.x * TILE; q0 < nq; q0 += (uint64_t)gridDim.x * TILE) {
            uint4 v[SPEC_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < SPEC_UNROLL; u++) {
                const uint64_t qi = q0 + u * BLOCK + tid;
                v[u] = qi < nq ? q[qi] : make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (uint32_t u = 0; u < SPEC_UNROLL; u++) {
                const uint64_t e = (q0 + u * BLOCK + tid) * 4u;
                if (e >= head && e < end) t.add(v[u].x, top, lds, hist);
                if (e + 1u >= head && e + 1u < end) t.add(v[u].y, top, lds, hist);
                if (e + 2u >= head && e + 2u < end) t.add(v[u].z, top, lds, hist);
                if (e + 3u >= head && e + 3u < end) t.add(v[u].w, top, lds, hist);
            }
        }
    }
    // the register tallies: one wave reduction per bin, lane 0 adds the wave's sums to the LDS bins
#pragma unroll
    for (uint32_t j = 0; j < SPEC_REG; j++) {
        const uint32_t s = ktd::wave_sum(t.reg[j]);
        if (lane == 0 && s) atomicAdd(&lds[j + 1u], s);  // (j + 1 <= top < lds_bins whenever s != 0)
    }
    if (totals) {
        uint64_t n_e = t.n, occ = t.occ;
        ktd::wave_sums(n_e, occ);
        if (lane == 0 && n_e) {
            atomicAdd(reinterpret_cast<unsigned long long *>(totals), (unsigned long long)n_e);
            atomicAdd(reinterpret_cast<unsigned long long *>(totals + 1), (unsigned long long)occ);
        }
    }
    ktd::lds_barrier();
    for (uint32_t b = 1u + tid; b < lds_bins; b += BLOCK)
        if (const uint32_t v = lds[b]) atomicAdd(reinterpret_cast<unsigned long long *>(hist + b), (unsigned long long)v);
}

// ---- the comparison matrix of two tables (kt_ctr_compare) ------------------------------------------------------------
// The entry walk of table A, read-only, in whatever form A is in (walk_entries); for every entry (key, a) the key is probed
// in B (B's probing image, B's geometry: kttab::Probed) for its count b (0: absent), and cell (min(a, R - 1),
// min(b, C - 1)) gets one.  The pass is bound by the random 16-byte reads into B: a lane first loads CMP_UNROLL entries of
// A, then issues the B home-slot loads of all of them, and only then resolves them (a walk past the home slot is rare).
// The matrix is skewed as the spectrum is - uniform reads put nearly everything into (1, 0) or (1, 1), reads sampled from
// a genome into a spot around (coverage, coverage) or (coverage, 1) - so the cells are tallied in three tiers: rows 1..4 x
// columns 0..1 in registers (an unrolled compare, reduced once per wave), a low corner of tile_rows x tile_cols (up to
// CMP_LDS cells, at least 128 x 64 or the whole matrix) in LDS with no-return adds, the rest in 64-bit global atomics.
// Every workgroup merges its non-zero LDS cells once, at the end; u32 tallies as in the spectrum (launch_walk bounds a
// workgroup's share below 2^31).  Column 0 (B's k-mers absent from A) is not probed for: compare_row0_kernel takes it from
// B's spectrum with the same saturation, minus this call's column sums over rows >= 1.
#ifndef KT_CMP_UNROLL
#define KT_CMP_UNROLL 8
#endif
constexpr uint32_t CMP_UNROLL = KT_CMP_UNROLL, CMP_LDS = 8192, CMP_REG = 8, CMP_TILE_COLS = 64;

struct CmpArgs {
    kttab::Probed b;      // B's probing image
    uint64_t *cells;      // this call's n_rows x n_cols cells (zeroed; row 0 is left to compare_row0_kernel)
    uint64_t *totals;     // distinct_a, occurrences_a, shared, shared_min
    uint32_t n_rows, n_cols, tile_rows, tile_cols;
};

struct CmpTally {
    uint32_t reg[CMP_REG] = {};  // cell (j / 2 + 1, j % 2)
    uint32_t n = 0, shared = 0;
    uint64_t occ = 0, smin = 0;
    __device__ __forceinline__ void add(uint32_t ca, uint32_t cb, const CmpArgs &c, uint32_t *lds) {
        n++;
        occ += ca;
        if (cb) {
            shared++;
            smin += ca < cb ? ca : cb;
        }
        const uint32_t r = ca < c.n_rows - 1u ? ca : c.n_rows - 1u;  // >= 1: an entry of A occurs at least once
        const uint32_t col = cb < c.n_cols - 1u ? cb : c.n_cols - 1u;
        const uint32_t id = r <= CMP_REG / 2 && col <= 1u ? (r - 1u) * 2u + col : CMP_REG;
#pragma unroll
        for (uint32_t j = 0; j < CMP_REG; j++) reg[j] += id == j;
        if (id == CMP_REG) {
            if (r < c.tile_rows && col < c.tile_cols) atomicAdd(&lds[r * c.tile_cols + col], 1u);  // (no-return ds_add)
            else atomicAdd(reinterpret_cast<unsigned long long *>(c.cells + (uint64_t)r * c.n_cols + col), 1ull);
        }
    }
};

// a: table A's view, FORM = its form
template <int FORM>
__global__ __launch_bounds__(BLOCK) void compare_kernel(TableView a, CmpArgs c) {
    __shared__ uint32_t lds[CMP_LDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t tile = c.tile_rows * c.tile_cols;
    for (uint32_t b = tid; b < tile; b += BLOCK) lds[b] = 0u;
    ktd::lds_barrier();
    CmpTally t;
    // (a wave of a dense table walks its range on its own: nothing below waits for the other waves)
    walk_entries<FORM, CMP_UNROLL, false>(a, [&](const uint64_t (&key)[CMP_UNROLL], const uint32_t (&ca)[CMP_UNROLL]) {
        c.b.counts(key, present(key), [&](uint32_t u, uint32_t cb) { t.add(ca[u], cb, c, lds); });
    });
    // the register cells: one wave reduction each, lane 0 adds the wave's sums to the LDS cells (a non-zero register cell
    // is a cell of the matrix, and rows <= 4, columns <= 1 of the matrix lie inside the tile)
#pragma unroll
    for (uint32_t j = 0; j < CMP_REG; j++) {
        const uint32_t s = ktd::wave_sum(t.reg[j]);
        if (lane == 0 && s) atomicAdd(&lds[(j / 2u + 1u) * c.tile_cols + (j & 1u)], s);
    }
    {
        uint64_t n_e = t.n, occ = t.occ, sh = t.shared, smin = t.smin;
        ktd::wave_sums(n_e, occ, sh, smin);
        if (lane == 0 && n_e) {
            atomicAdd(reinterpret_cast<unsigned long long *>(c.totals), (unsigned long long)n_e);
            atomicAdd(reinterpret_cast<unsigned long long *>(c.totals + 1), (unsigned long long)occ);
            if (sh) {
                atomicAdd(reinterpret_cast<unsigned long long *>(c.totals + 2), (unsigned long long)sh);
                atomicAdd(reinterpret_cast<unsigned long long *>(c.totals + 3), (unsigned long long)smin);
            }
        }
    }
    ktd::lds_barrier();
    for (uint32_t b = tid; b < tile; b += BLOCK)
        if (const uint32_t v = lds[b])
            atomicAdd(reinterpret_cast<unsigned long long *>(c.cells + (uint64_t)(b / c.tile_cols) * c.n_cols + b % c.tile_cols),
                      (unsigned long long)v);
}

// this call's cells S, rows >= 1: their column sums into colsum, and (out != nullptr) S added into the caller's out.  A
// thread per column of a block of BLOCK columns (blockIdx.y) over CMP_FIN_ROWS rows (blockIdx.x): coalesced row by row,
// every cell read by one thread.
constexpr uint32_t CMP_FIN_ROWS = 64;
__global__ __launch_bounds__(BLOCK) void compare_colsum_kernel(const uint64_t *__restrict__ S, uint32_t n_rows, uint32_t n_cols,
                                                               uint64_t *__restrict__ colsum, uint64_t *__restrict__ out) {
    const uint32_t col = blockIdx.y * BLOCK + threadIdx.x;
    if (col >= n_cols) return;
    const uint32_t r0 = 1u + blockIdx.x * CMP_FIN_ROWS, r1 = r0 + CMP_FIN_ROWS < n_rows ? r0 + CMP_FIN_ROWS : n_rows;
    uint64_t s = 0;
    for (uint32_t r = r0; r < r1; r++) {
        const uint64_t i = (uint64_t)r * n_cols + col, v = S[i];
        s += v;
        if (out && v) out[i] += v;
    }
    if (s) atomicAdd(reinterpret_cast<unsigned long long *>(colsum + col), (unsigned long long)s);
}

// row 0 of the matrix: row0[c] += specB[c] - colsum[c] for 1 <= c < n_cols (B's k-mers of column c that A does not hold;
// [0][0] is not touched), and the six totals (totals_out may be null)
__global__ __launch_bounds__(BLOCK) void compare_row0_kernel(const uint64_t *__restrict__ spec_b, const uint64_t *__restrict__ colsum,
                                                             uint32_t n_cols, uint64_t *__restrict__ row0,
                                                             const uint64_t *__restrict__ tot_a, const uint64_t *__restrict__ tot_b,
                                                             uint64_t *__restrict__ totals_out) {
    const uint64_t c = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (c >= 1 && c < n_cols) row0[c] += spec_b[c] - colsum[c];
    if (c == 0 && totals_out) {
        totals_out[0] += tot_a[0];  // distinct_a
        totals_out[1] += tot_b[0];  // distinct_b
        totals_out[2] += tot_a[2];  // shared
        totals_out[3] += tot_a[1];  // occurrences_a
        totals_out[4] += tot_b[1];  // occurrences_b
        totals_out[5] += tot_a[3];  // shared_min
    }
}

// ---- routing (multi-GPU ownership) ------------------------------------------------------

constexpr int MAX_OWNERS = 64;

// ---- set operations of two tables (kt_ctr_setop) ---------------------------------------------------------------------
// One table walked read-only in the form it is in (walk_entries), every key resolved against the other table's probing
// image with the home-slot loads of SET_UNROLL entries in flight together (kttab::Probed), as compare_kernel does; what
// this adds: every entry is decided - membership of both sides under their count ranges, the operation, the count rule - and
// the kept (key, count) pairs are compacted as the export kernels compact: a ballot per entry, the workgroup's waves add
// up their popcounts and ONE cursor atomic reserves the tile's output range (BLOCK x SET_UNROLL entries; every store
// instruction writes one contiguous run).  The cursor is the limit to watch: same-address atomics retire at ~12 ns each,
// and a first version that took one per wave (512 entries) was bound by them, not by the probes - 13.2 ms against
// compare's 7.3 ms on the full-size pair, 87 ms for a union that walks two probing images.  A dense table is
// walked with uniform steps (every wave runs the steps of the longest of the workgroup's four ranges) so that all reach
// the barriers.  max_out = 0 only counts: the position test keeps every store away.
constexpr uint32_t SET_UNROLL = CMP_UNROLL;

struct SetArgs {
    kttab::Probed probed;  // the other table's probing image
    uint32_t op, rule;   // KT_SET_*, KT_SETCNT_*
    uint32_t lo_w, hi_w; // the walked table's count range
    uint32_t lo_p, hi_p; // the probed table's (lo_p >= 1: an absent key is never a member)
    uint64_t *out_keys;
    uint32_t *out_counts;
    uint64_t max_out;
    uint64_t *cursor;    // entries that qualify so far (both walks of union / xor add to it)
};

// the count to emit for an entry of the walked table (cw >= 1 occurrences there, cp in the probed table, 0: absent), or 0
// when it is not emitted.  SECOND: the second walk of union / xor - B walked, A probed: only keys absent from A's table,
// and every rule of (0, b') is b'.
template <bool SECOND>
__device__ __forceinline__ uint32_t set_decide(const SetArgs &s, uint32_t cw, uint32_t cp) {
    const uint32_t w = cw >= s.lo_w && cw <= s.hi_w ? cw : 0u;
    if constexpr (SECOND) return cp ? 0u : w;
    const uint32_t p = cp >= s.lo_p && cp <= s.hi_p ? cp : 0u;
    const bool in = s.op == KT_SET_INTERSECT ? (w && p) : s.op == KT_SET_SUBTRACT ? (w && !p) : s.op == KT_SET_UNION ? (w || p) : ((w != 0u) != (p != 0u));
    if (!in) return 0u;
    if (!w || !p) return w | p;  // one side only: every rule gives that side's count
    if (s.rule == KT_SETCNT_FIRST) return w;
    if (s.rule == KT_SETCNT_MIN) return w < p ? w : p;
    if (s.rule == KT_SETCNT_MAX) return w > p ? w : p;
    const uint64_t sum = (uint64_t)w + p;
    return sum > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)sum;
}

struct SetShared {
    uint32_t wave_total[2][BLOCK / 64];  // [step parity]: a step's sums are read while the fastest wave writes the next step's
    uint64_t tile_base[2];
};

// the workgroup's tile: the entries whose bit is set in `keep` are kept, store(u, pos) writes entry u to its place `pos` of the
// output (the payload is the caller's: setop's and graph's u32, hetmers' second key).  Every thread of the workgroup must be
// here, `step` counting the calls (two barriers a call; the parity keeps a step's LDS words apart from its neighbours').
// N: the walk's unroll.
template <uint32_t N, class Store>
__device__ __forceinline__ void tile_emit(uint64_t *cursor, uint32_t keep, SetShared &sm, uint32_t &step, Store &&store) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, par = step++ & 1u;
    uint64_t bal[N];
    uint32_t total = 0;
#pragma unroll
    for (uint32_t u = 0; u < N; u++) {
        bal[u] = __ballot((keep >> u) & 1u);
        total += (uint32_t)__popcll(bal[u]);
    }
    if (lane == 0) sm.wave_total[par][wave] = total;
    ktd::lds_barrier();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < BLOCK / 64; w++) {
        const uint32_t t = sm.wave_total[par][w];
        before += w < wave ? t : 0u;
        all += t;
    }
    if (threadIdx.x == 0 && all)
        sm.tile_base[par] = atomicAdd(reinterpret_cast<unsigned long long *>(cursor), (unsigned long long)all);
    ktd::lds_barrier();
    if (!total) return;
    uint64_t base = sm.tile_base[par] + before;
#pragma unroll
    for (uint32_t u = 0; u < N; u++) {
        if ((bal[u] >> lane) & 1ull) store(u, base + __popcll(bal[u] & ((1ull << lane) - 1ull)));
        base += (uint32_t)__popcll(bal[u]);
    }
}

// ... with a u32 payload: entries with out[u] != 0 are kept as (key[u], out[u]), nothing at or past s.max_out is written
template <uint32_t N>
__device__ __forceinline__ void set_emit(const SetArgs &s, const uint64_t (&key)[N], const uint32_t (&out)[N], SetShared &sm,
                                         uint32_t &step) {
    uint32_t keep = 0;
#pragma unroll
    for (uint32_t u = 0; u < N; u++) keep |= (out[u] != 0u ? 1u : 0u) << u;
    tile_emit<N>(s.cursor, keep, sm, step, [&](uint32_t u, uint64_t pos) {
        if (pos < s.max_out) {
            s.out_keys[pos] = key[u];
            s.out_counts[pos] = out[u];
        }
    });
}

// w: the walked table's view, FORM = its form
template <int FORM, bool SECOND>
__global__ __launch_bounds__(BLOCK) void setop_kernel(TableView w, SetArgs s) {
    __shared__ SetShared sm;
    uint32_t step = 0;
    walk_entries<FORM, SET_UNROLL, true>(w, [&](const uint64_t (&key)[SET_UNROLL], const uint32_t (&cw)[SET_UNROLL]) {
        uint32_t out[SET_UNROLL] = {};
        s.probed.counts(key, present(key), [&](uint32_t u, uint32_t cp) { out[u] = set_decide<SECOND>(s, cw[u], cp); });
        set_emit(s, key, out, sm, step);
    });
}

// ---- de Bruijn adjacency of a table's k-mers (kt_ctr_graph) -----------------------------------------------------------
// The table walked read-only in the form it is in (walk_entries) and probed in its own probing image: an entry whose count
// lies in [lo, hi] is a node, and its 14 related k-mers - the 4 right and 4 left neighbours of its forward string F (the
// canonical word itself) and the 3 + 3 other k-mers that enter those neighbours from the same side - are all functions of
// F alone, so their home-slot loads go out together (kttab::Probed::counts, 14 x 16 bytes in flight per node).  A related
// k-mer's reverse complement comes from R = rev_comp(F) by the mirrored shift, so one bit reversal serves all 14.  The info
// words are compacted as setop compacts its counts (set_emit: info != 0 for every node); the census is tallied in registers
// (the seven sums and cell (1, 1), where the nodes of a genome's unitigs fall), the other degree cells in LDS, and every
// workgroup adds its non-zero cells to the caller's 32 once, at the end.
// The unroll is the walk's and the emit tile's only (BLOCK x GRAPH_UNROLL entries per cursor atomic); the nodes of a step
// are resolved one after the other, 14 loads in flight each.  The compiler reports 119 VGPRs at 2 (4 waves per SIMD) and
// 133 at 4 (3 waves): 2 keeps the fourth wave, and at 14 probes per node the cursor is far from binding.
#ifndef KT_GRAPH_UNROLL
#define KT_GRAPH_UNROLL 2
#endif
constexpr uint32_t GRAPH_UNROLL = KT_GRAPH_UNROLL, GRAPH_KEYS = 14, GRAPH_SUMS = 7, GRAPH_CELLS = 25;
static_assert(GRAPH_SUMS + GRAPH_CELLS == KT_GRAPH_CENSUS, "the census layout");

struct GraphArgs {
    SetArgs s;          // probed: the table itself; lo_w / hi_w: the solid range; the (key, info) output and its cursor
    uint64_t *census;   // KT_GRAPH_CENSUS cells, added into (null: no census)
    uint32_t k;
};

// the info word of node F (canonical, k bases): bits 0..3 right neighbours, 4..7 left neighbours, 8 right end, 9 left end
__device__ __forceinline__ uint32_t graph_info(const GraphArgs &g, uint64_t F) {
    const uint32_t top = 2u * g.k - 2u;                    // where a k-mer's first base sits (<= 60)
    const uint64_t mask = (1ull << (2u * g.k)) - 1ull;     // 2k <= 62
    const uint64_t low = mask >> 2;                        // the last k - 1 bases
    const uint64_t R = ktd::rev_comp(F, (int)g.k);
    const uint64_t first = F >> top, last = F & 3ull;
    uint64_t key[GRAPH_KEYS];
#pragma unroll
    for (uint64_t x = 0; x < 4; x++) {
        // F[1..k) + x and its reverse complement comp(x) + R[0..k-1)
        const uint64_t rf = ((F << 2) & mask) | x, rr = (R >> 2) | ((3ull - x) << top);
        // x + F[0..k-1) and R[1..k) + comp(x)
        const uint64_t lf = (F >> 2) | (x << top), lr = ((R << 2) & mask) | (3ull - x);
        key[x] = rf < rr ? rf : rr;
        key[4 + x] = lf < lr ? lf : lr;
    }
#pragma unroll
    for (uint64_t j = 0; j < 3; j++) {
        // y + F[1..k) for the three y != F[0] (what else enters the right neighbours), reverse complement R[0..k-1) + comp(y)
        const uint64_t yr = j + (j >= first ? 1ull : 0ull);
        const uint64_t sf = (F & low) | (yr << top), sr = (R & ~3ull) | (3ull - yr);
        // F[0..k-1) + y for the three y != F[k-1], reverse complement comp(y) + R[1..k)
        const uint64_t yl = j + (j >= last ? 1ull : 0ull);
        const uint64_t tf = (F & ~3ull) | yl, tr = (R & low) | ((3ull - yl) << top);
        key[8 + j] = sf < sr ? sf : sr;
        key[11 + j] = tf < tr ? tf : tr;
    }
    uint32_t solid = 0;
    g.s.probed.counts(key, (1u << GRAPH_KEYS) - 1u, [&](uint32_t u, uint32_t c) {
        solid |= (c >= g.s.lo_w && c <= g.s.hi_w ? 1u : 0u) << u;
    });
    const uint32_t dR = __popc(solid & 0xFu), dL = __popc(solid & 0xF0u);
    const uint32_t sibR = 1u + __popc(solid & 0x700u), sibL = 1u + __popc(solid & 0x3800u);
    return (solid & 0xFFu) | (dR != 1u || sibR != 1u ? 0x100u : 0u) | (dL != 1u || sibL != 1u ? 0x200u : 0u);
}

struct GraphTally {
    uint32_t n = 0, deg = 0, ends = 0, isolated = 0, tips = 0, branching = 0, c11 = 0;
    uint64_t occ = 0;
    __device__ __forceinline__ void add(uint32_t info, uint32_t c, uint32_t *cells) {
        const uint32_t dR = __popc(info & 0xFu), dL = __popc(info & 0xF0u);
        n++;
        occ += c;
        deg += dL + dR;
        ends += __popc(info & 0x300u);
        isolated += dL == 0u && dR == 0u;
        tips += (dL == 0u) != (dR == 0u);
        branching += dL > 1u || dR > 1u;
        if (dL == 1u && dR == 1u) c11++;
        else atomicAdd(&cells[5u * dL + dR], 1u);  // (no-return ds_add)
    }
};

// w: the table's view, FORM = its form
template <int FORM>
__global__ __launch_bounds__(BLOCK) void graph_kernel(TableView w, GraphArgs g) {
    __shared__ SetShared sm;
    __shared__ uint32_t cells[GRAPH_CELLS];
    __shared__ unsigned long long sums[GRAPH_SUMS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if (tid < GRAPH_CELLS) cells[tid] = 0u;
    if (tid < GRAPH_SUMS) sums[tid] = 0ull;
    ktd::lds_barrier();
    GraphTally t;
    uint32_t step = 0;
    walk_entries<FORM, GRAPH_UNROLL, true>(w, [&](const uint64_t (&key)[GRAPH_UNROLL], const uint32_t (&cw)[GRAPH_UNROLL]) {
        uint32_t out[GRAPH_UNROLL] = {};
#pragma unroll
        for (uint32_t u = 0; u < GRAPH_UNROLL; u++) {
            // (a lane without an entry, or whose entry is not a node, issues no probe)
            if (key[u] != KT_EMPTY_KEY && cw[u] >= g.s.lo_w && cw[u] <= g.s.hi_w) {
                out[u] = graph_info(g, key[u]);
                t.add(out[u], cw[u], cells);
            }
        }
        set_emit(g.s, key, out, sm, step);
    });
    if (!g.census) return;
    // the register tallies: one wave reduction each, lane 0 adds the wave's sums to the workgroup's
    {
        uint64_t v[GRAPH_SUMS] = {t.n, t.occ, t.deg, t.ends, t.isolated, t.tips, t.branching};
#pragma unroll
        for (uint32_t j = 0; j < GRAPH_SUMS; j++) v[j] = ktd::wave_sum(v[j]);
        const uint32_t c11 = ktd::wave_sum(t.c11);
        if (lane == 0 && v[0]) {
#pragma unroll
            for (uint32_t j = 0; j < GRAPH_SUMS; j++)
                if (v[j]) atomicAdd(&sums[j], (unsigned long long)v[j]);
            if (c11) atomicAdd(&cells[5u * 1u + 1u], c11);
        }
    }
    ktd::lds_barrier();
    if (tid < GRAPH_SUMS) {
        if (const unsigned long long v = sums[tid]) atomicAdd(reinterpret_cast<unsigned long long *>(g.census + tid), v);
    } else if (tid < GRAPH_SUMS + GRAPH_CELLS) {
        if (const uint32_t v = cells[tid - GRAPH_SUMS])
            atomicAdd(reinterpret_cast<unsigned long long *>(g.census + tid), (unsigned long long)v);
    }
}

// ---- heterozygous k-mer pairs of a table (kt_ctr_hetmers) -------------------------------------------------------------
// The rule is in the header.  Three kernels, so that every lane that probes has a k-mer to probe for:
//   nodes   the table walked read-only in the form it is in (walk_entries), its nodes compacted into an array of keys by
//           tile_emit, one cursor atomic per workgroup tile; nodes and their occurrences tallied.  A first version scanned
//           in this walk, as graph_kernel does its 14 probes: with counts from 2 up on a 30x read set one slot in 19 holds a
//           node, and the few lanes of a wave that had one went through up to 93 probes while the others stood idle - 0.11 ns
//           per probe against 0.035 with every entry a node.  Whether the graph's 14 probes would pay for a
//           compaction nobody has measured; these 3k do.
//   scan    one lane per node, probing the table's probing image.  A node's 3 |P| one-substitution variants are functions of F
//           alone: with R = rev_comp(F), the variant
//           of position i and d in 1..3 is min(F ^ (d << 2(k-1-i)), R ^ (d << 2i)) - the complement of a substituted base is
//           the same XOR at the mirrored position, so one bit reversal serves them all.  They go through Probed::counts in
//           groups of HET_POS positions (below); the lane keeps the first solid neighbour n1 and one flag, "a solid variant other
//           than n1 was seen" (deg >= 2), and stops issuing groups at the flag: the census needs the classes 0 / 1 / >= 2 only.
//           A variant equal to F is not probed (self-substitution); one equal to n1 does not raise the flag (double reach).
//           Lanes with deg == 1 and F < n1 are compacted as candidates (F, n1) by tile_emit, one cursor atomic per tile.
//   verify  one lane per candidate runs the same scan from n1, with F already in hand as its first neighbour: the flag is
//           then "n1 has a solid neighbour other than F".  (F itself turns up by the rule's symmetry; were the table changed
//           under the call it might not, and the pair would still be reported - there is no device assert for that.)
//           Survivors are compacted into the output; their two counts are probed here for the sums and the matrix.
// The numbers of nodes and candidates stay on the device: scan and verify read the cursor of the kernel before them and run
// on a grid of the device's size, every workgroup taking the same number of steps over it, so that all reach the emit's
// barriers.  The group is HET_POS = 5 positions = 15 keys in flight per lane, one more than graph_kernel's 14: the compiler
// reports 120 VGPRs for het_scan_kernel and 125 for het_verify_kernel (4 waves per SIMD; graph_kernel: 119); 4 positions
// take 98 / 104, which is still 4 waves, and 6 take 141 / 146 and cost the fourth.  So 5 it is, from the register report
// alone: 4 against 5 on the clock nobody has measured (-DKT_HET_POS=4 builds the
// other).  A group is also the grain of the early stop: a lane whose flag rises issues no further group.  The census classes
// are tallied in registers and reduced as in graph_kernel.  The pairs' matrix cells are plain 64-bit global atomics, one per
// pair: pairs are a small share of the nodes and spread over the smudges' cells, but nobody has measured a table where they
// are not; the three pair sums are register tallies.
#ifndef KT_HET_POS
#define KT_HET_POS 5
#endif
constexpr uint32_t HET_UNROLL = 4, HET_POS = KT_HET_POS, HET_KEYS = 3 * HET_POS, HET_NODE_SUMS = 2, HET_DEG_SUMS = 3, HET_PAIR_SUMS = 3;
static_assert(HET_NODE_SUMS + HET_DEG_SUMS + HET_PAIR_SUMS == KT_HET_CENSUS, "the census layout");

struct HetArgs {
    kttab::Probed probed;       // the table itself
    uint32_t lo, hi;            // the solid range
    uint32_t k, p_lo, p_hi;     // the positions [p_lo, p_hi): 0..k, or the middle one
    uint64_t *nodes;            // the nodes' keys, room for every entry of the table
    uint64_t *n_nodes;          // their cursor
    uint64_t *cand_a, *cand_b;  // the candidates (F, n1), room for every entry of the table
    uint64_t *n_cand;           // their cursor
    uint64_t *census;           // KT_HET_CENSUS cells, added into (null: no census)
};

struct HetScan {
    uint64_t n1;       // the first solid neighbour
    bool have, multi;  // n1 is set; a solid neighbour other than n1 was seen
};

// the solid neighbours of node F, into `s` (stops at s.multi)
__device__ __forceinline__ void het_scan(const HetArgs &h, uint64_t F, HetScan &s) {
    const uint64_t R = ktd::rev_comp(F, (int)h.k);
    const uint32_t top = 2u * h.k - 2u;  // where a k-mer's first base sits (<= 60)
    for (uint32_t i0 = h.p_lo; i0 < h.p_hi && !s.multi; i0 += HET_POS) {
        uint64_t key[HET_KEYS];
        uint32_t want = 0;
#pragma unroll
        for (uint32_t j = 0; j < HET_POS; j++) {
            const bool in = i0 + j < h.p_hi;
            const uint32_t sr = in ? 2u * (i0 + j) : 0u, sf = top - sr;  // position i in R's word and in F's
#pragma unroll
            for (uint32_t d = 1; d <= 3u; d++) {
                const uint64_t f = F ^ ((uint64_t)d << sf), r = R ^ ((uint64_t)d << sr);
                const uint64_t c = f < r ? f : r;
                key[3u * j + d - 1u] = c;
                want |= (in && c != F ? 1u : 0u) << (3u * j + d - 1u);
            }
        }
        h.probed.counts(key, want, [&](uint32_t u, uint32_t c) {
            if (c >= h.lo && c <= h.hi) {
                if (!s.have) s.n1 = key[u], s.have = true;
                else if (key[u] != s.n1) s.multi = true;
            }
        });
    }
}

// the lanes' tallies v[M] into the caller's cells: one wave reduction each, the workgroup's sums in LDS (zeroed, M cells),
// one global atomic per non-zero cell.  Every thread of the workgroup must be here.
template <uint32_t M>
__device__ __forceinline__ void het_add_sums(uint64_t (&v)[M], unsigned long long *sums, uint64_t *cells) {
#pragma unroll
    for (uint32_t j = 0; j < M; j++) v[j] = ktd::wave_sum(v[j]);
    if ((threadIdx.x & 63u) == 0) {
#pragma unroll
        for (uint32_t j = 0; j < M; j++)
            if (v[j]) atomicAdd(&sums[j], (unsigned long long)v[j]);
    }
    ktd::lds_barrier();
    if (threadIdx.x < M)
        if (const unsigned long long t = sums[threadIdx.x]) atomicAdd(reinterpret_cast<unsigned long long *>(cells + threadIdx.x), t);
}

// w: the table's view, FORM = its form
template <int FORM>
__global__ __launch_bounds__(BLOCK) void het_nodes_kernel(TableView w, HetArgs h) {
    __shared__ SetShared sm;
    __shared__ unsigned long long sums[HET_NODE_SUMS];
    if (threadIdx.x < HET_NODE_SUMS) sums[threadIdx.x] = 0ull;
    ktd::lds_barrier();
    uint32_t n = 0, step = 0;
    uint64_t occ = 0;
    walk_entries<FORM, HET_UNROLL, true>(w, [&](const uint64_t (&key)[HET_UNROLL], const uint32_t (&cw)[HET_UNROLL]) {
        uint32_t keep = 0;
#pragma unroll
        for (uint32_t u = 0; u < HET_UNROLL; u++) {
            if (key[u] != KT_EMPTY_KEY && cw[u] >= h.lo && cw[u] <= h.hi) {
                keep |= 1u << u;
                n++;
                occ += cw[u];
            }
        }
        // (the nodes' room is the table's entries: every position is inside it)
        tile_emit<HET_UNROLL>(h.n_nodes, keep, sm, step, [&](uint32_t u, uint64_t pos) { h.nodes[pos] = key[u]; });
    });
    if (!h.census) return;
    uint64_t v[HET_NODE_SUMS] = {n, occ};
    het_add_sums(v, sums, h.census);
}

// one lane per node, grid-stride by workgroup tiles; *h.n_nodes is het_nodes_kernel's
__global__ __launch_bounds__(BLOCK) void het_scan_kernel(HetArgs h) {
    __shared__ SetShared sm;
    __shared__ unsigned long long sums[HET_DEG_SUMS];
    if (threadIdx.x < HET_DEG_SUMS) sums[threadIdx.x] = 0ull;
    ktd::lds_barrier();
    const uint64_t n = *h.n_nodes;  // (the same for every thread: the loop is uniform, all reach the emit's barriers)
    uint32_t d0 = 0, d1 = 0, d2 = 0, step = 0;
    for (uint64_t i0 = (uint64_t)blockIdx.x * BLOCK; i0 < n; i0 += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t i = i0 + threadIdx.x;
        uint64_t F = 0ull;
        HetScan s{0ull, false, false};
        uint32_t keep = 0;
        if (i < n) {
            F = h.nodes[i];
            het_scan(h, F, s);
            d0 += !s.have;
            d1 += s.have && !s.multi;
            d2 += s.multi;
            keep = s.have && !s.multi && F < s.n1 ? 1u : 0u;
        }
        // (the candidates' room is the table's entries: every position is inside it)
        tile_emit<1>(h.n_cand, keep, sm, step, [&](uint32_t, uint64_t pos) {
            h.cand_a[pos] = F;
            h.cand_b[pos] = s.n1;
        });
    }
    if (!h.census) return;
    uint64_t v[HET_DEG_SUMS] = {d0, d1, d2};
    het_add_sums(v, sums, h.census + HET_NODE_SUMS);
}

struct HetOut {
    uint64_t *keys_a, *keys_b;  // the pairs, a < b
    uint32_t *index;            // index[pos] = pos, for the sort to carry (null: unsorted)
    uint64_t max_out;
    uint64_t *cursor;           // pairs so far
    uint64_t *matrix;           // n_rows x n_cols, added into (null: no matrix)
    uint32_t n_rows, n_cols;
};

// one lane per candidate, grid-stride by workgroup tiles; *h.n_cand is het_scan_kernel's
__global__ __launch_bounds__(BLOCK) void het_verify_kernel(HetArgs h, HetOut o) {
    __shared__ SetShared sm;
    __shared__ unsigned long long sums[HET_PAIR_SUMS];
    if (threadIdx.x < HET_PAIR_SUMS) sums[threadIdx.x] = 0ull;
    ktd::lds_barrier();
    const uint64_t n = *h.n_cand;  // (the same for every thread: the loop is uniform, all reach the emit's barriers)
    uint64_t pairs = 0, minor = 0, major = 0;
    uint32_t step = 0;
    for (uint64_t i0 = (uint64_t)blockIdx.x * BLOCK; i0 < n; i0 += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t i = i0 + threadIdx.x;
        uint64_t ab[2] = {0ull, 0ull};
        uint32_t keep = 0;
        if (i < n) {
            ab[0] = h.cand_a[i], ab[1] = h.cand_b[i];
            HetScan s{ab[0], true, false};
            het_scan(h, ab[1], s);
            if (!s.multi) {
                uint32_t c[2] = {0u, 0u};
                h.probed.counts(ab, 3u, [&](uint32_t u, uint32_t cc) { c[u] = cc; });
                const uint32_t mn = c[0] < c[1] ? c[0] : c[1], mx = c[0] < c[1] ? c[1] : c[0];
                keep = 1u;
                pairs++;
                minor += mn;
                major += mx;
                if (o.matrix) {
                    const uint32_t r = mn < o.n_rows - 1u ? mn : o.n_rows - 1u, cl = mx < o.n_cols - 1u ? mx : o.n_cols - 1u;
                    atomicAdd(reinterpret_cast<unsigned long long *>(o.matrix + (uint64_t)r * o.n_cols + cl), 1ull);
                }
            }
        }
        tile_emit<1>(o.cursor, keep, sm, step, [&](uint32_t, uint64_t pos) {
            if (pos < o.max_out) {
                o.keys_a[pos] = ab[0];
                o.keys_b[pos] = ab[1];
                if (o.index) o.index[pos] = (uint32_t)pos;
            }
        });
    }
    if (!h.census) return;
    uint64_t v[HET_PAIR_SUMS] = {pairs, minor, major};
    het_add_sums(v, sums, h.census + HET_NODE_SUMS + HET_DEG_SUMS);
}

// dst[i] = src[index[i]]: the second keys follow the sort of the first
__global__ __launch_bounds__(BLOCK) void het_gather_kernel(const uint64_t *__restrict__ src, const uint32_t *__restrict__ index,
                                                           uint64_t n, uint64_t *__restrict__ dst) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLOCK) dst[i] = src[index[i]];
}

// ---- the scaled sketch of a table's entries (kt_ctr_scaled) ---------------------------------------------------------------
// The table walked read-only in the form it is in (walk_entries), twice: the first walk counts - the entries whose count lies
// in [lo, hi], their occurrences, and those of them whose hash mix64(key ^ seed) is at or below max_hash -, the second one,
// with room for exactly that many, compacts the kept ones as (hash, count) by tile_emit.  Their order is the cursor's, which
// does not matter: kt::scaled_finish sorts them, and a table's keys are distinct.
constexpr uint32_t SCALED_UNROLL = 4, SCALED_SUMS = 3;

struct ScaledWalk {
    uint32_t lo, hi;
    uint64_t seed, max_hash;
};

template <int FORM>
__global__ __launch_bounds__(BLOCK) void scaled_count_kernel(TableView w, ScaledWalk s, uint64_t *__restrict__ cells) {
    __shared__ unsigned long long sums[SCALED_SUMS];
    if (threadIdx.x < SCALED_SUMS) sums[threadIdx.x] = 0ull;
    ktd::lds_barrier();
    uint32_t kept = 0, n = 0;
    uint64_t occ = 0;
    walk_entries<FORM, SCALED_UNROLL, false>(w, [&](const uint64_t (&key)[SCALED_UNROLL], const uint32_t (&cw)[SCALED_UNROLL]) {
#pragma unroll
        for (uint32_t u = 0; u < SCALED_UNROLL; u++) {
            if (key[u] == KT_EMPTY_KEY || cw[u] < s.lo || cw[u] > s.hi) continue;
            n++;
            occ += cw[u];
            kept += ktd::mix64(key[u] ^ s.seed) <= s.max_hash ? 1u : 0u;
        }
    });
    uint64_t v[SCALED_SUMS] = {kept, n, occ};
    het_add_sums(v, sums, cells);
}

template <int FORM>
__global__ __launch_bounds__(BLOCK) void scaled_emit_kernel(TableView w, ScaledWalk s, uint64_t *cursor, uint64_t room,
                                                            uint64_t *__restrict__ hashes, uint32_t *__restrict__ counts) {
    __shared__ SetShared sm;
    uint32_t step = 0;
    walk_entries<FORM, SCALED_UNROLL, true>(w, [&](const uint64_t (&key)[SCALED_UNROLL], const uint32_t (&cw)[SCALED_UNROLL]) {
        uint64_t h[SCALED_UNROLL];
        uint32_t keep = 0;
#pragma unroll
        for (uint32_t u = 0; u < SCALED_UNROLL; u++) {
            h[u] = ktd::mix64(key[u] ^ s.seed);
            keep |= (key[u] != KT_EMPTY_KEY && cw[u] >= s.lo && cw[u] <= s.hi && h[u] <= s.max_hash ? 1u : 0u) << u;
        }
        tile_emit<SCALED_UNROLL>(cursor, keep, sm, step, [&](uint32_t u, uint64_t pos) {
            if (pos < room) hashes[pos] = h[u], counts[pos] = cw[u];
        });
    });
}

__global__ __launch_bounds__(BLOCK) void route_count_kernel(SegArgs a, uint32_t n_owners,
                                                            uint64_t *__restrict__ owner_counts) {
    __shared__ SegShared sm;
    __shared__ uint32_t cnt[MAX_OWNERS];
    if (threadIdx.x < MAX_OWNERS) cnt[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t g = blockIdx.x; g < a.n_seg; g += gridDim.x) {
        ktseg::for_each_kmer(a, g, sm, [&](uint64_t f, uint64_t r, uint64_t) {
            const uint64_t m = f < r ? f : r;
            atomicAdd(&cnt[ktd::owner_of(m, n_owners)], 1u);
        });
        if (threadIdx.x < n_owners && cnt[threadIdx.x]) {
            atomicAdd(reinterpret_cast<unsigned long long *>(&owner_counts[threadIdx.x]),
                      (unsigned long long)cnt[threadIdx.x]);
            cnt[threadIdx.x] = 0;
        }
        __syncthreads();
    }
}

// cursors[o] starts at the exclusive prefix of owner_counts; each workgroup reserves a
// contiguous range per owner for its segment, then its lanes fill the range.
__global__ __launch_bounds__(BLOCK) void route_scatter_kernel(SegArgs a, uint32_t n_owners,
                                                              uint64_t *__restrict__ cursors,
                                                              uint64_t *__restrict__ keys_out) {
    __shared__ SegShared sm;
    __shared__ uint32_t cnt[MAX_OWNERS];
    __shared__ uint64_t base[MAX_OWNERS];
    if (threadIdx.x < MAX_OWNERS) cnt[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t g = blockIdx.x; g < a.n_seg; g += gridDim.x) {
        ktseg::for_each_kmer(a, g, sm, [&](uint64_t f, uint64_t r, uint64_t) {
            const uint64_t m = f < r ? f : r;
            atomicAdd(&cnt[ktd::owner_of(m, n_owners)], 1u);
        });
        if (threadIdx.x < n_owners) {
            const uint32_t c = cnt[threadIdx.x];
            base[threadIdx.x] = c ? atomicAdd(reinterpret_cast<unsigned long long *>(&cursors[threadIdx.x]),
                                              (unsigned long long)c)
                                  : 0;
            cnt[threadIdx.x] = 0;
        }
        __syncthreads();
        ktseg::for_each_kmer(a, g, sm, [&](uint64_t f, uint64_t r, uint64_t) {
            const uint64_t m = f < r ? f : r;
            const uint32_t o = ktd::owner_of(m, n_owners);
            const uint32_t slot = atomicAdd(&cnt[o], 1u);
            keys_out[base[o] + slot] = m;
        });
        if (threadIdx.x < MAX_OWNERS) cnt[threadIdx.x] = 0;
        __syncthreads();
    }
}

__global__ void route_prefix_kernel(const uint64_t *__restrict__ owner_counts, uint32_t n_owners,
                                    uint64_t *__restrict__ cursors) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        uint64_t acc = 0;
        for (uint32_t o = 0; o < n_owners; o++) {
            cursors[o] = acc;
            acc += owner_counts[o];
        }
    }
}

// ---- debug surface -------------------------------------------------------------------------

__global__ __launch_bounds__(BLOCK) void kmers_kernel(SegArgs a, uint64_t *__restrict__ fwd,
                                                      uint64_t *__restrict__ rev, uint8_t *__restrict__ valid) {
    __shared__ SegShared sm;
    for (uint64_t g = blockIdx.x; g < a.n_seg; g += gridDim.x) {
        ktseg::for_each_kmer(a, g, sm, [&](uint64_t f, uint64_t r, uint64_t end) {
            fwd[end] = f;
            rev[end] = r;
            valid[end] = 1;
        });
    }
}

}  // namespace

using namespace ktl;

extern "C" {

int kt_ctr_add_reads(kt_ctr *ctr, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int mem) {
    return kt_ctr_add_reads_part(ctr, bases, offsets, n_reads, mem, 1, 0);
}

int kt_ctr_add_reads_part(kt_ctr *ctr, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int mem,
                          uint32_t n_parts, uint32_t part) {
    if (!ctr) return kt::fail(KT_ERR_ARG, "kt_ctr_add_reads: null ctr");
    if (part >= n_parts) return kt::fail(KT_ERR_ARG, "kt_ctr_add_reads_part: need part < n_parts");
    kt_ctx *ctx = ctr->ctx;
    Call call(ctx, mem, "kt_ctr_add_reads");
    if (int rc = call.enter()) return rc;
    if (n_reads == 0) return KT_OK;
    // the table is about to change: what kt_ctr_export_stage staged is no longer the table (fetch says so).  Here, not only
    // in the gates below: a batch of reads without a base has ended the stage since the stage exists
    ctr->stage.drop();
    if (!offsets) return call.fail("null offsets");
    if (int rc = call.batch(bases, offsets, n_reads)) return rc;
    if (call.total == 0) return KT_OK;
    if (int rc = call.stage()) return rc;
    {
        // a whole batch: partition by hash prefix + one LDS build per range of the table, no global atomics.  Into a
        // table that holds data the ranges are rebuilt from what they have + the batch (worth it for large batches)
        int done = 0;
        if (int rc = kt_bulk_build(ctr, call.bases, call.offsets, n_reads, call.total, n_parts, part, &done)) return rc;
        if (done) return call.finish();
    }
    TableRef t;
    if (int rc = table_write(ctr, &t)) return rc;
    SegArgs a;
    if (int rc = make_seg_args(ctx, call.bases, call.offsets, n_reads, call.total, ctr->k, &a)) return rc;
    hipLaunchKernelGGL(count_reads_kernel<ktpf::KeepAll>, dim3(grid_for(ctx, a.n_seg, 8)), dim3(BLOCK), 0, ctx->stream, a, t, n_parts,
                       part, ctr->distinct, ktpf::KeepAll());
    KT_HIP(hipGetLastError());
    return call.finish();
}

int kt_ctr_add_reads_filtered(kt_ctr *ctr, kt_prefilter *filter, const uint8_t *bases, const uint64_t *offsets,
                              uint64_t n_reads, int mem, uint32_t n_parts, uint32_t part) {
    if (!ctr) return kt::fail(KT_ERR_ARG, "kt_ctr_add_reads_filtered: null ctr");
    kt_ctx *ctx = ctr->ctx;
    Call call(ctx, mem, "kt_ctr_add_reads_filtered");
    if (!filter) return call.fail("null filter");
    if (filter->ctx != ctx) return call.fail("the filter belongs to another context");
    if (filter->k != ctr->k) return call.fail("the filter's k is not the table's");
    if (int rc = call.check_part(n_parts, part)) return rc;
    if (int rc = call.enter()) return rc;
    if (n_reads == 0) return KT_OK;
    ctr->stage.drop();  // (as in kt_ctr_add_reads_part)
    if (!offsets) return call.fail("null offsets");
    if (int rc = call.batch(bases, offsets, n_reads)) return rc;
    if (call.total == 0) return KT_OK;
    if (int rc = call.stage()) return rc;
    TableRef t;
    if (int rc = table_write(ctr, &t)) return rc;
    SegArgs a;
    if (int rc = make_seg_args(ctx, call.bases, call.offsets, n_reads, call.total, ctr->k, &a)) return rc;
    const ktpf::KeepSeenTwice keep{view_of(filter)};
    if (int rc = launch(count_reads_kernel<ktpf::KeepSeenTwice>, dim3(grid_for(ctx, a.n_seg, 8)), dim3(BLOCK), 0, ctx->stream, a, t,
                        n_parts, part, ctr->distinct, keep))
        return rc;
    return call.finish();
}

int kt_ctr_add_pairs(kt_ctr *ctr, const uint64_t *keys, const uint32_t *counts, uint64_t n, int mem) {
    if (!ctr) return kt::fail(KT_ERR_ARG, "kt_ctr_add_pairs: null ctr");
    kt_ctx *ctx = ctr->ctx;
    Call call(ctx, mem, "kt_ctr_add_pairs");
    if (int rc = call.enter()) return rc;
    if (n == 0) return KT_OK;
    if (!keys) return call.fail("null keys");
    ctr->stage.drop();  // (before anything below can fail, as in kt_ctr_add_reads_part)
    const uint64_t *d_keys = nullptr;
    const uint32_t *d_counts = nullptr;
    if (int rc = call.in(kt::AUX1, keys, n, &d_keys)) return rc;
    if (counts)
        if (int rc = call.in(kt::AUX2, counts, n, &d_counts)) return rc;
    if (!d_counts) {
        // raw k-mers (routed from other GPUs): the bulk build, no global atomics (it takes AUX2 for its census, which
        // the counts do not hold on this branch)
        int done = 0;
        if (int rc = kt_bulk_build_keys(ctr, d_keys, n, &done)) return rc;
        if (done) return call.finish();
    }
    TableRef t;
    if (int rc = table_write(ctr, &t)) return rc;
    if (int rc = add_pairs(ctr, t, d_keys, d_counts, n)) return rc;
    return call.finish();
}

}  // extern "C"

// n > 0 device pairs through the probing path (kt_ctr_add_pairs, kt_ctr_erase's survivors, kt_table.hip's load of a target's pairs)
int ktl::add_pairs(kt_ctr *ctr, const TableRef &t, const uint64_t *d_keys, const uint32_t *d_counts, uint64_t n) {
    return launch(add_pairs_kernel, dim3(grid_for(ctr->ctx, (n + BLOCK - 1) / BLOCK, 8)), dim3(BLOCK), 0, ctr->ctx->stream, d_keys,
                  d_counts, n, t, ctr->distinct);
}

// Scratch: AUX1 = the surviving pairs (12 bytes an entry of the table), AUX2 = the bitmask (one bit a slot), host keys in
// OFFSETS - all claimed before the first write into the table.  One wait for the stream tells how many slots were flagged;
// none: the table is left as it is.
extern "C" int kt_ctr_erase(kt_ctr *ctr, const uint64_t *keys, uint64_t n, uint64_t *n_erased, int mem) {
    if (!ctr) return kt::fail(KT_ERR_ARG, "kt_ctr_erase: null table");
    kt_ctx *ctx = ctr->ctx;
    Call call(ctx, mem, "kt_ctr_erase");
    if (int rc = call.refuse_shard(ctr)) return rc;
    if (int rc = call.enter()) return rc;
    if (n && !keys) return call.fail("null keys");
    uint64_t n_t = 0;
    if (int rc = kt_ctr_size(ctr, &n_t)) return rc;  // (KT_ERR_FULL for an overflowed table)
    // the keys are looked up by probing: the probing image first (a dense table is imaged, an export target's pairs are
    // loaded and its arrays are the caller's again, whatever n is) - the content stays what it was
    if (int rc = table_ready(ctr)) return rc;
    if (n == 0 || n_t == 0) {
        if (n_erased) *n_erased = 0;
        return KT_OK;
    }
    const uint64_t words = (ctr->cap + 31) / 32;
    const size_t o_counts = (n_t * 8 + 15) & ~(size_t)15;
    uint8_t *pairs = nullptr;
    uint32_t *dead = nullptr;
    const uint64_t *d_keys = nullptr;
    if (int rc = call.scratch(kt::AUX1, o_counts + n_t * 4, &pairs)) return rc;
    if (int rc = call.scratch(kt::AUX2, words * 4, &dead)) return rc;
    if (int rc = call.in(kt::OFFSETS, keys, n, &d_keys)) return rc;
    uint64_t *live_keys = (uint64_t *)pairs;
    uint32_t *live_counts = (uint32_t *)(pairs + o_counts);
    hipStream_t st = ctx->stream;
    uint64_t *cursor = ctr->cursor;  // [0]: flagged slots, [1]: the survivors' cursor
    KT_HIP(hipMemsetAsync(cursor, 0, 16, st));
    KT_HIP(hipMemsetAsync(dead, 0, words * 4, st));
    hipLaunchKernelGGL(erase_flag_kernel, dim3(grid_for(ctx, (n + BLOCK - 1) / BLOCK, 8)), dim3(BLOCK), 0, st, d_keys, n,
                       probed_of(ctr), 1ull << (2 * ctr->k), dead, cursor);
    KT_HIP(hipGetLastError());
    uint64_t gone = 0;
    KT_HIP(hipMemcpyAsync(&gone, cursor, 8, hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
    if (gone > n_t) return kt::fail(KT_ERR_HIP, "kt_ctr_erase: internal: more slots flagged than the table holds");
    if (gone) {
        hipLaunchKernelGGL(erase_survivors_kernel, dim3(grid_for(ctx, (ctr->cap + XTILE - 1) / XTILE, 8)), dim3(BLOCK), 0, st,
                           (const Slot *)ctr->slots, ctr->cap, (const uint32_t *)dead, live_keys, live_counts, n_t - gone, cursor + 1);
        KT_HIP(hipGetLastError());
        // from here on the table changes (the gate finds the image table_ready left): the slots emptied, the survivors back in
        TableRef t;
        if (int rc = table_write(ctr, &t)) return rc;
        if (int rc = table_wipe(ctr)) return rc;
        KT_HIP(hipMemsetAsync(ctr->distinct, 0, 8, st));
        if (n_t - gone)
            if (int rc = add_pairs(ctr, t, live_keys, live_counts, n_t - gone)) return rc;
    }
    if (int rc = call.finish()) return rc;
    if (n_erased) *n_erased = gone;
    return KT_OK;
}

static int launch_spectrum(kt_ctr *ctr, uint64_t n, uint64_t *d_hist, uint32_t n_bins, uint64_t *d_totals);

extern "C" {

int kt_ctr_spectrum(kt_ctr *ctr, uint64_t *hist, uint32_t n_bins, uint64_t *totals, int mem) {
    if (!ctr || !hist) return kt::fail(KT_ERR_ARG, "kt_ctr_spectrum: null");
    kt_ctx *ctx = ctr->ctx;
    Call call(ctx, mem, "kt_ctr_spectrum");
    if (n_bins < 2 || n_bins > (1u << 24)) return call.fail("n_bins must be in 2..2^24");
    if (int rc = call.enter()) return rc;
    uint64_t n = 0;
    if (int rc = kt_ctr_size(ctr, &n)) return rc;  // (KT_ERR_FULL for an overflowed table)
    if (!n) return KT_OK;                           // nothing to add (a table pending its clear is empty too)
    uint64_t *d_hist = hist, *d_totals = totals;
    if (call.host()) {  // this call's bins are made on the device from zero and added to the caller's
        if (int rc = call.scratch(kt::AUX1, ((size_t)n_bins + 2) * 8, &d_hist)) return rc;
        d_totals = totals ? d_hist + n_bins : nullptr;
        KT_HIP(hipMemsetAsync(d_hist, 0, ((size_t)n_bins + 2) * 8, ctx->stream));
    }
    if (int rc = launch_spectrum(ctr, n, d_hist, n_bins, d_totals)) return rc;
    if (call.host()) {
        std::unique_ptr<uint64_t[]> h;
        if (int rc = call.fetch((const uint64_t *)d_hist, (uint64_t)n_bins + 2, &h)) return rc;
        for (uint32_t b = 1; b < n_bins; b++) hist[b] += h[b];
        if (totals) {
            totals[0] += h[n_bins];
            totals[1] += h[(size_t)n_bins + 1];
        }
    }
    return KT_OK;
}

}  // extern "C"

// the table's n > 0 entries as the kernels walk them, in the form they are in now: the form, the view the kernels read
// and what a launch's workgroups share out (the slots of a probing image, else the entries)
struct TableWalk {
    Form form;
    TableView v;
    uint64_t entries;
};
static TableWalk view_of(const kt_ctr *ctr, uint64_t n) {
    switch (ctr->form()) {
    case kt::TableForm::Target:
        return {FORM_PAIRS, {ctr->xt_keys, ctr->xt_counts, n, 0u, (uint32_t)(((uintptr_t)ctr->xt_counts & 15u) / 4u), nullptr}, n};
    case kt::TableForm::Dense: {
        const uint32_t RS = geom_of(ctr).range_slots();
        return {FORM_DENSE, {ctr->slots, nullptr, ctr->cap / RS, RS, 0u, ctr->range_counts}, n};
    }
    default:  // (n > 0: not a Stale table)
        return {FORM_PROBE, {ctr->slots, nullptr, ctr->cap, 0u, 0u, nullptr}, ctr->cap};
    }
}

// One launch over a table: launch(the form as a compile-time constant, the grid).  A flat form is shared out in tiles of
// `tile` of its `flat_items` (what a workgroup takes per step: BLOCK x the kernel's unroll, in slots or pairs - v.n of them
// - or in whatever else the kernel reads a flat form by); a dense table goes four ranges per workgroup.  ~4 workgroups per
// CU, and enough that no workgroup's share reaches 2^31 entries (the kernels' u32 tallies).
template <class Launch>
static int launch_walk(kt_ctx *ctx, const TableWalk &w, uint64_t flat_items, uint64_t tile, Launch &&launch) {
    const uint64_t work_items = w.form == FORM_DENSE ? (w.v.n + 3) / 4 : (flat_items + tile - 1) / tile;
    uint64_t g = (uint64_t)ctx->n_cu * 4;
    if (g > work_items) g = work_items;
    if (g < (w.entries >> 31) + 1) g = (w.entries >> 31) + 1;
    const dim3 grid((uint32_t)g);
    if (w.form == FORM_PAIRS) launch(std::integral_constant<int, FORM_PAIRS>{}, grid);
    else if (w.form == FORM_DENSE) launch(std::integral_constant<int, FORM_DENSE>{}, grid);
    else launch(std::integral_constant<int, FORM_PROBE>{}, grid);
    KT_HIP(hipGetLastError());
    return KT_OK;
}

// the spectrum launch of a table of n > 0 entries, in the form it is in, into device arrays (kt_ctr_spectrum, kt_ctr_compare)
static int launch_spectrum(kt_ctr *ctr, uint64_t n, uint64_t *d_hist, uint32_t n_bins, uint64_t *d_totals) {
    const TableWalk w = view_of(ctr, n);
    // (the kernel reads the counts of the pairs form as aligned 16-byte quads)
    const uint64_t flat_items = w.form == FORM_PAIRS ? (w.v.n + w.v.head + 3) / 4 : w.v.n;
    return launch_walk(ctr->ctx, w, flat_items, (uint64_t)BLOCK * SPEC_UNROLL, [&](auto form, dim3 grid) {
        hipLaunchKernelGGL(spectrum_kernel<decltype(form)::value>, grid, dim3(BLOCK), 0, ctr->ctx->stream, w.v, d_hist, n_bins, d_totals);
    });
}

extern "C" int kt_ctr_compare(kt_ctr *a, kt_ctr *b, uint64_t *matrix, uint32_t n_rows, uint32_t n_cols, uint64_t *totals, int mem) {
    if (!a || !b || !matrix) return kt::fail(KT_ERR_ARG, "kt_ctr_compare: null");
    if (a->k != b->k) return kt::fail(KT_ERR_ARG, "kt_ctr_compare: the tables have different k");
    if (a->ctx != b->ctx) return kt::fail(KT_ERR_ARG, "kt_ctr_compare: the tables are on different contexts");
    kt_ctx *ctx = a->ctx;
    Call call(ctx, mem, "kt_ctr_compare");
    if (a->n_owners > 1 || b->n_owners > 1) return call.fail("a table is one shard of a sharded table - shards are not supported");
    if (n_rows < 2 || n_cols < 2) return call.fail("n_rows and n_cols must be >= 2");
    if ((uint64_t)n_rows * n_cols > (1ull << 24)) return call.fail("n_rows * n_cols must be <= 2^24");
    if (int rc = call.enter()) return rc;
    uint64_t n_a = 0, n_b = 0;
    if (int rc = kt_ctr_size(a, &n_a)) return rc;  // (KT_ERR_FULL for an overflowed table)
    if (int rc = kt_ctr_size(b, &n_b)) return rc;
    if (!n_a && !n_b) return KT_OK;
    // B is probed: its probing image first.  A's form is read only after that - with a == b, or a B whose image was built
    // from A's arrays, A is walked as it is now
    if (int rc = table_ready(b)) return rc;
    // scratch (u64): this call's cells | B's spectrum | column sums | A's totals (4) | B's totals (2) | the six totals
    const uint64_t cells = (uint64_t)n_rows * n_cols, words = cells + 2ull * n_cols + 12;
    uint64_t *S = nullptr;
    if (int rc = call.scratch(kt::AUX1, words * 8, &S)) return rc;
    uint64_t *spec_b = S + cells, *colsum = spec_b + n_cols, *tot_a = colsum + n_cols,
             *tot_b = tot_a + 4, *tot6 = tot_b + 2;
    KT_HIP(hipMemsetAsync(S, 0, words * 8, ctx->stream));
    if (n_a) {
        const uint32_t tile_cols = n_cols < CMP_TILE_COLS ? n_cols : CMP_TILE_COLS;
        const uint32_t tile_rows = n_rows < CMP_LDS / tile_cols ? n_rows : CMP_LDS / tile_cols;
        const CmpArgs c{probed_of(b), S, tot_a, n_rows, n_cols, tile_rows, tile_cols};
        const TableWalk w = view_of(a, n_a);
        if (int rc = launch_walk(ctx, w, w.v.n, (uint64_t)BLOCK * CMP_UNROLL, [&](auto form, dim3 grid) {
                hipLaunchKernelGGL(compare_kernel<decltype(form)::value>, grid, dim3(BLOCK), 0, ctx->stream, w.v, c);
            }))
            return rc;
    }
    if (n_b)
        if (int rc = launch_spectrum(b, n_b, spec_b, n_cols, tot_b)) return rc;
    const bool host = call.host();
    hipLaunchKernelGGL(compare_colsum_kernel, dim3((n_rows - 1 + CMP_FIN_ROWS - 1) / CMP_FIN_ROWS, (n_cols + BLOCK - 1) / BLOCK),
                       dim3(BLOCK), 0, ctx->stream, (const uint64_t *)S, n_rows, n_cols, colsum, host ? nullptr : matrix);
    hipLaunchKernelGGL(compare_row0_kernel, dim3((n_cols + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, ctx->stream,
                       (const uint64_t *)spec_b, (const uint64_t *)colsum, n_cols, host ? S : matrix, (const uint64_t *)tot_a,
                       (const uint64_t *)tot_b, host ? tot6 : totals);
    KT_HIP(hipGetLastError());
    if (host) {
        std::unique_ptr<uint64_t[]> h;
        if (int rc = call.fetch((const uint64_t *)S, words, &h)) return rc;
        for (uint64_t i = 1; i < cells; i++) matrix[i] += h[i];
        if (totals)
            for (int j = 0; j < 6; j++) totals[j] += h[cells + 2ull * n_cols + 6 + j];
    }
    return KT_OK;
}

// one walk of kt_ctr_setop: table `t` (n_w > 0 entries) in the form it is in, probing s.probed
template <bool SECOND>
static int launch_setop(kt_ctr *t, uint64_t n_w, const SetArgs &s) {
    const TableWalk w = view_of(t, n_w);
    return launch_walk(t->ctx, w, w.v.n, (uint64_t)BLOCK * SET_UNROLL, [&](auto form, dim3 grid) {
        hipLaunchKernelGGL((setop_kernel<decltype(form)::value, SECOND>), grid, dim3(BLOCK), 0, t->ctx->stream, w.v, s);
    });
}

extern "C" int kt_ctr_setop(kt_ctr *a, kt_ctr *b, int op, int count_rule, uint32_t min_a, uint32_t max_a, uint32_t min_b,
                            uint32_t max_b, uint64_t *keys, uint32_t *counts, uint64_t max_out, uint64_t *n_out, int mem,
                            int sorted) {
    if (!a || !b || !n_out) return kt::fail(KT_ERR_ARG, "kt_ctr_setop: null");
    if (a->k != b->k) return kt::fail(KT_ERR_ARG, "kt_ctr_setop: the tables have different k");
    if (a->ctx != b->ctx) return kt::fail(KT_ERR_ARG, "kt_ctr_setop: the tables are on different contexts");
    kt_ctx *ctx = a->ctx;
    Call call(ctx, mem, "kt_ctr_setop");
    if (a->n_owners > 1 || b->n_owners > 1) return call.fail("a table is one shard of a sharded table - shards are not supported");
    if (op < KT_SET_INTERSECT || op > KT_SET_XOR) return call.fail("unknown op");
    if (count_rule < KT_SETCNT_FIRST || count_rule > KT_SETCNT_SUM) return call.fail("unknown count_rule");
    if (min_a == 0 || min_b == 0) return call.fail("min_a and min_b must be >= 1");
    if (min_a > max_a || min_b > max_b) return call.fail("a count range with min > max");
    if (int rc = call.enter()) return rc;
    if (max_out && (!keys || !counts)) return call.fail("null output");
    uint64_t n_a = 0, n_b = 0;
    if (int rc = kt_ctr_size(a, &n_a)) return rc;  // (KT_ERR_FULL for an overflowed table)
    if (int rc = kt_ctr_size(b, &n_b)) return rc;
    *n_out = 0;
    const bool two = (op == KT_SET_UNION || op == KT_SET_XOR) && n_b;  // B's entries that A's table lacks: a second walk
    if (!n_a && !two) return KT_OK;
    // a probed table gets its probing image first (B before A's walk, A before B's); the form of the walked table is read
    // only after that - with a == b, or an image built from the other table's arrays, a table is walked as it is now
    if (n_a)
        if (int rc = table_ready(b)) return rc;
    uint64_t *d_keys = keys;
    uint32_t *d_counts = counts;
    if (call.host() && max_out) {  // (what comes back is the entries written, known only after the walks)
        if (int rc = call.scratch(kt::AUX1, max_out * 8, &d_keys)) return rc;
        if (int rc = call.scratch(kt::AUX2, max_out * 4, &d_counts)) return rc;
    }
    uint64_t *cursor = a->cursor;
    KT_HIP(hipMemsetAsync(cursor, 0, 8, ctx->stream));
    SetArgs s{probed_of(b), (uint32_t)op, (uint32_t)count_rule, min_a, max_a, min_b, max_b, d_keys, d_counts, max_out, cursor};
    if (n_a) {
        if (int rc = launch_setop<false>(a, n_a, s)) return rc;
    }
    if (two) {
        if (int rc = table_ready(a)) return rc;  // (behind A's walk on the stream; uses neither the cursor nor the context's scratch)
        s.probed = probed_of(a);
        s.lo_w = min_b, s.hi_w = max_b;
        if (int rc = launch_setop<true>(b, n_b, s)) return rc;
    }
    uint64_t n = 0;
    KT_HIP(hipMemcpyAsync(&n, cursor, 8, hipMemcpyDeviceToHost, ctx->stream));
    KT_HIP(hipStreamSynchronize(ctx->stream));
    *n_out = n;
    const uint64_t written = n < max_out ? n : max_out;
    if (sorted && written == n)  // (a result that did not fit is not a result: the caller repeats the call)
        if (int rc = kt_sort_pairs(ctx, d_keys, d_counts, n, 2u * (uint32_t)a->k)) return rc;
    call.back(keys, (const uint64_t *)d_keys, written);
    call.back(counts, (const uint32_t *)d_counts, written);
    if (int rc = call.finish()) return rc;
    if (max_out && n > max_out) return call.fail("max_out smaller than the result (*n_out entries)");
    return KT_OK;
}

extern "C" int kt_ctr_graph(kt_ctr *table, uint32_t min_count, uint32_t max_count, uint64_t *keys, uint32_t *info,
                            uint32_t *counts, uint64_t max_out, uint64_t *n_out, uint64_t *census, int mem, int sorted) {
    if (!table || !n_out) return kt::fail(KT_ERR_ARG, "kt_ctr_graph: null");
    kt_ctx *ctx = table->ctx;
    Call call(ctx, mem, "kt_ctr_graph");
    if (int rc = call.refuse_shard(table)) return rc;
    if (min_count == 0) return call.fail("min_count must be >= 1");
    if (min_count > max_count) return call.fail("min_count > max_count");
    if (int rc = call.enter()) return rc;
    if (max_out && (!keys || !info)) return call.fail("null output");
    uint64_t n_t = 0;
    if (int rc = kt_ctr_size(table, &n_t)) return rc;  // (KT_ERR_FULL for an overflowed table)
    *n_out = 0;
    if (!n_t) return KT_OK;
    // the table is probed: its probing image first; its form is read only after that (it is walked as it is now)
    if (int rc = table_ready(table)) return rc;
    // host: this call's results are made in scratch - AUX1: keys | census, AUX2: info | counts
    uint64_t *d_keys = keys, *d_census = census;
    uint32_t *d_info = info, *d_counts = counts;
    if (call.host()) {
        if (int rc = call.scratch(kt::AUX1, (max_out + KT_GRAPH_CENSUS) * 8, &d_keys)) return rc;
        d_census = census ? d_keys + max_out : nullptr;
        if (census) KT_HIP(hipMemsetAsync(d_census, 0, KT_GRAPH_CENSUS * 8, ctx->stream));
        if (max_out) {
            if (int rc = call.scratch(kt::AUX2, max_out * 8, &d_info)) return rc;
            d_counts = counts ? d_info + max_out : nullptr;
        }
    }
    uint64_t *cursor = table->cursor;
    KT_HIP(hipMemsetAsync(cursor, 0, 8, ctx->stream));
    const GraphArgs g{SetArgs{probed_of(table), 0u, 0u, min_count, max_count, 1u, 0xFFFFFFFFu, d_keys, d_info, max_out, cursor},
                      d_census, (uint32_t)table->k};
    const TableWalk w = view_of(table, n_t);
    if (int rc = launch_walk(ctx, w, w.v.n, (uint64_t)BLOCK * GRAPH_UNROLL, [&](auto form, dim3 grid) {
            hipLaunchKernelGGL(graph_kernel<decltype(form)::value>, grid, dim3(BLOCK), 0, ctx->stream, w.v, g);
        }))
        return rc;
    uint64_t n = 0;
    KT_HIP(hipMemcpyAsync(&n, cursor, 8, hipMemcpyDeviceToHost, ctx->stream));
    KT_HIP(hipStreamSynchronize(ctx->stream));
    *n_out = n;
    const uint64_t written = n < max_out ? n : max_out;
    if (sorted && written == n)  // (a result that did not fit is not a result: the caller repeats the call)
        if (int rc = kt_sort_pairs(ctx, d_keys, d_info, n, 2u * (uint32_t)table->k)) return rc;
    // the counts of the emitted keys, in the order they are left in: they need not ride through the sort
    if (d_counts && written)
        if (int rc = lookup_counts(table, d_keys, written, d_counts)) return rc;
    call.back(keys, (const uint64_t *)d_keys, written);
    call.back(info, (const uint32_t *)d_info, written);
    call.back(counts, (const uint32_t *)d_counts, written);
    if (call.host() && census) {
        std::unique_ptr<uint64_t[]> h;
        if (int rc = call.fetch((const uint64_t *)d_census, (uint64_t)KT_GRAPH_CENSUS, &h)) return rc;
        for (int j = 0; j < KT_GRAPH_CENSUS; j++) census[j] += h[j];
    }
    if (int rc = call.finish()) return rc;
    if (max_out && n > max_out) return call.fail("max_out smaller than the result (*n_out nodes)");
    return KT_OK;
}

extern "C" int kt_ctr_hetmers(kt_ctr *table, uint32_t min_count, uint32_t max_count, int positions, uint64_t *keys_a,
                              uint64_t *keys_b, uint32_t *counts_a, uint32_t *counts_b, uint64_t max_out, uint64_t *n_out,
                              uint64_t *matrix, uint32_t n_rows, uint32_t n_cols, uint64_t *census, int mem, int sorted) {
    if (!table || !n_out) return kt::fail(KT_ERR_ARG, "kt_ctr_hetmers: null");
    kt_ctx *ctx = table->ctx;
    Call call(ctx, mem, "kt_ctr_hetmers");
    if (int rc = call.refuse_shard(table)) return rc;
    if (min_count == 0) return call.fail("min_count must be >= 1");
    if (min_count > max_count) return call.fail("min_count > max_count");
    if (positions != KT_HET_ALL && positions != KT_HET_MIDDLE) return call.fail("unknown positions");
    if (positions == KT_HET_MIDDLE && table->k % 2 == 0) return call.fail("KT_HET_MIDDLE needs an odd k");
    if (matrix) {
        if (n_rows < 2 || n_cols < 2) return call.fail("n_rows and n_cols must be >= 2");
        if ((uint64_t)n_rows * n_cols > (1ull << 24)) return call.fail("n_rows * n_cols must be <= 2^24");
    }
    if (int rc = call.enter()) return rc;
    if (max_out && (!keys_a || !keys_b)) return call.fail("null output");
    uint64_t n_t = 0;
    if (int rc = kt_ctr_size(table, &n_t)) return rc;  // (KT_ERR_FULL for an overflowed table)
    // every node is in at most one pair, and the sort carries a pair's index as its u32 payload
    const bool sort = sorted && max_out;
    if (sort && n_t / 2 > 0xFFFFFFFFull) return call.fail("a table of 2^33 entries or more cannot be sorted");
    *n_out = 0;
    if (!n_t) return KT_OK;
    // the table is probed: its probing image first; its form is read only after that (it is walked as it is now)
    if (int rc = table_ready(table)) return rc;
    // scratch - BASES: the nodes' keys | the candidates' two keys; OFFSETS: the two cursors | sorted: the second keys before
    // the gather | the index; host: this call's results - AUX1: keys_a | keys_b | census | matrix, AUX2: counts_a | counts_b
    const uint64_t cells = matrix ? (uint64_t)n_rows * n_cols : 0;
    uint64_t *nodes = nullptr, *words = nullptr;
    if (int rc = call.scratch(kt::BASES, n_t * 24, &nodes)) return rc;
    if (int rc = call.scratch(kt::OFFSETS, 16 + (sort ? max_out * 12 : 0), &words)) return rc;
    uint64_t *n_cand = words, *n_nodes = words + 1, *b_unsorted = words + 2;
    uint32_t *index = sort ? reinterpret_cast<uint32_t *>(b_unsorted + max_out) : nullptr;
    uint64_t *d_a = keys_a, *d_b = keys_b, *d_census = census, *d_matrix = matrix;
    uint32_t *d_ca = counts_a, *d_cb = counts_b;
    if (call.host()) {
        if (int rc = call.scratch(kt::AUX1, (2 * max_out + KT_HET_CENSUS + cells) * 8, &d_a)) return rc;
        d_b = d_a + max_out;
        uint64_t *sums = d_b + max_out;
        KT_HIP(hipMemsetAsync(sums, 0, (KT_HET_CENSUS + cells) * 8, ctx->stream));
        d_census = census ? sums : nullptr;
        d_matrix = matrix ? sums + KT_HET_CENSUS : nullptr;
        if (max_out) {
            if (int rc = call.scratch(kt::AUX2, max_out * 8, &d_ca)) return rc;
            d_cb = counts_b ? d_ca + max_out : nullptr;
            if (!counts_a) d_ca = nullptr;
        }
    }
    uint64_t *cursor = table->cursor;
    KT_HIP(hipMemsetAsync(cursor, 0, 8, ctx->stream));
    KT_HIP(hipMemsetAsync(words, 0, 16, ctx->stream));
    const uint32_t k = (uint32_t)table->k, mid = (k - 1u) / 2u;
    const HetArgs h{probed_of(table), min_count, max_count, k, positions == KT_HET_MIDDLE ? mid : 0u,
                    positions == KT_HET_MIDDLE ? mid + 1u : k, nodes, n_nodes, nodes + n_t, nodes + 2 * n_t, n_cand, d_census};
    const TableWalk w = view_of(table, n_t);
    if (int rc = launch_walk(ctx, w, w.v.n, (uint64_t)BLOCK * HET_UNROLL, [&](auto form, dim3 grid) {
            hipLaunchKernelGGL(het_nodes_kernel<decltype(form)::value>, grid, dim3(BLOCK), 0, ctx->stream, w.v, h);
        }))
        return rc;
    // (the nodes and the candidates are counted on the device only: the grid is the device's, whatever their number)
    const dim3 grid(grid_for(ctx, (n_t + BLOCK - 1) / BLOCK, 4));
    hipLaunchKernelGGL(het_scan_kernel, grid, dim3(BLOCK), 0, ctx->stream, h);
    const HetOut o{d_a, sort ? b_unsorted : d_b, index, max_out, cursor, d_matrix, n_rows, n_cols};
    hipLaunchKernelGGL(het_verify_kernel, grid, dim3(BLOCK), 0, ctx->stream, h, o);
    KT_HIP(hipGetLastError());
    uint64_t n = 0;
    KT_HIP(hipMemcpyAsync(&n, cursor, 8, hipMemcpyDeviceToHost, ctx->stream));
    KT_HIP(hipStreamSynchronize(ctx->stream));
    *n_out = n;
    const uint64_t written = n < max_out ? n : max_out;
    if (sort && written) {
        // (a result that did not fit is not a result: the caller repeats the call; its second keys still go to their array)
        if (written == n)
            if (int rc = kt_sort_pairs(ctx, d_a, index, n, 2u * k)) return rc;
        hipLaunchKernelGGL(het_gather_kernel, dim3(grid_for(ctx, (written + BLOCK - 1) / BLOCK, 8)), dim3(BLOCK), 0, ctx->stream,
                           (const uint64_t *)b_unsorted, (const uint32_t *)index, written, d_b);
        KT_HIP(hipGetLastError());
    }
    // the counts of the emitted keys, in the order they are left in: they need not ride through the sort
    if (d_ca && written)
        if (int rc = lookup_counts(table, d_a, written, d_ca)) return rc;
    if (d_cb && written)
        if (int rc = lookup_counts(table, d_b, written, d_cb)) return rc;
    call.back(keys_a, (const uint64_t *)d_a, written);
    call.back(keys_b, (const uint64_t *)d_b, written);
    call.back(counts_a, (const uint32_t *)d_ca, written);
    call.back(counts_b, (const uint32_t *)d_cb, written);
    if (call.host() && (census || matrix)) {
        std::unique_ptr<uint64_t[]> s;
        if (int rc = call.fetch((const uint64_t *)(d_b + max_out), KT_HET_CENSUS + cells, &s)) return rc;
        if (census)
            for (int j = 0; j < KT_HET_CENSUS; j++) census[j] += s[j];
        for (uint64_t i = 0; i < cells; i++) matrix[i] += s[KT_HET_CENSUS + i];
    }
    if (int rc = call.finish()) return rc;
    if (max_out && n > max_out) return call.fail("max_out smaller than the result (*n_out pairs)");
    return KT_OK;
}

extern "C" int kt_ctr_scaled(kt_ctr *table, uint32_t min_count, uint32_t max_count, uint64_t scaled, uint64_t seed, uint64_t *hashes,
                             uint32_t *abunds, uint64_t max_out, uint64_t *n_out, uint64_t *totals, int mem) {
    if (!table || !n_out) return kt::fail(KT_ERR_ARG, "kt_ctr_scaled: null");
    kt_ctx *ctx = table->ctx;
    Call call(ctx, mem, "kt_ctr_scaled");
    if (int rc = call.refuse_shard(table)) return rc;
    if (min_count == 0) return call.fail("min_count must be >= 1");
    if (min_count > max_count) return call.fail("min_count > max_count");
    if (scaled == 0) return call.fail("scaled must be >= 1");
    if (int rc = call.enter()) return rc;
    if (max_out && !hashes) return call.fail("null output");
    uint64_t n_t = 0;
    if (int rc = kt_ctr_size(table, &n_t)) return rc;  // (KT_ERR_FULL for an overflowed table)
    // this call's sums: [0] kept entries, [1] entries in the count range, [2] their occurrences
    uint64_t *d_sums = nullptr, sums[SCALED_SUMS] = {0, 0, 0};
    if (int rc = call.scratch(kt::BASES, SCALED_SUMS * 8, &d_sums)) return rc;
    KT_HIP(hipMemsetAsync(d_sums, 0, SCALED_SUMS * 8, ctx->stream));
    const ScaledWalk s{min_count, max_count, seed, kt_scaled_max_hash(scaled)};
    if (n_t) {  // the table is walked in the form it is in: nothing here brings it to its probing image
        const TableWalk w = view_of(table, n_t);
        if (int rc = launch_walk(ctx, w, w.v.n, (uint64_t)BLOCK * SCALED_UNROLL, [&](auto form, dim3 grid) {
                hipLaunchKernelGGL(scaled_count_kernel<decltype(form)::value>, grid, dim3(BLOCK), 0, ctx->stream, w.v, s, d_sums);
            }))
            return rc;
        KT_HIP(hipMemcpyAsync(sums, d_sums, SCALED_SUMS * 8, hipMemcpyDeviceToHost, ctx->stream));
        KT_HIP(hipStreamSynchronize(ctx->stream));
    }
    const uint64_t kept = sums[0];
    if (kept >= (1ull << 32)) return call.fail("2^32 kept entries or more (a larger scaled, or a narrower count range)");
    uint64_t *el_h = nullptr;
    uint32_t *el_c = nullptr;
    if (kept) {
        if (int rc = carve(call, kt::AUX1, &el_h, kept, &el_c, kept)) return rc;
        uint64_t *cursor = table->cursor;
        KT_HIP(hipMemsetAsync(cursor, 0, 8, ctx->stream));
        const TableWalk w = view_of(table, n_t);
        if (int rc = launch_walk(ctx, w, w.v.n, (uint64_t)BLOCK * SCALED_UNROLL, [&](auto form, dim3 grid) {
                hipLaunchKernelGGL(scaled_emit_kernel<decltype(form)::value>, grid, dim3(BLOCK), 0, ctx->stream, w.v, s, cursor, kept, el_h, el_c);
            }))
            return rc;
    }
    const kt::ScaledElems e{el_h, el_c, nullptr, kept, 1};
    const kt::ScaledOut o{hashes, abunds, max_out, nullptr, n_out, mem};
    if (int rc = kt::scaled_finish(ctx, "kt_ctr_scaled", e, o)) return rc;
    if (totals)
        KT_HIP(hipMemcpyAsync(totals, d_sums + 1, 16, call.host() ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
    return call.finish();
}

extern "C" {

int kt_ctr_route(kt_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int k,
                 int n_owners, uint64_t *keys_out, uint64_t *owner_counts, int mem) {
    if (!ctx || !owner_counts) return kt::fail(KT_ERR_ARG, "kt_ctr_route: null");
    if (k < 1 || k > 31) return kt::fail(KT_ERR_ARG, "kt_ctr_route: k must be in 1..31");
    if (n_owners < 1 || n_owners > MAX_OWNERS) return kt::fail(KT_ERR_ARG, "kt_ctr_route: n_owners must be in 1..64");
    Call call(ctx, mem, "kt_ctr_route");
    if (int rc = call.enter()) return rc;
    // device scalars: [0..63] owner counts, [64..127] cursors
    uint64_t *d_counts = nullptr;
    if (int rc = call.scratch(kt::AUX2, 2 * MAX_OWNERS * 8, &d_counts)) return rc;
    uint64_t *d_cursors = d_counts + MAX_OWNERS;
    KT_HIP(hipMemsetAsync(d_counts, 0, 2 * MAX_OWNERS * 8, ctx->stream));
    if (n_reads) {
        if (!offsets) return call.fail("null offsets");
        if (int rc = call.batch(bases, offsets, n_reads, nullptr)) return rc;
    }
    uint64_t *d_keys = keys_out;
    if (call.total) {
        if (!bases || !keys_out) return call.fail("null buffer");
        if (int rc = call.stage()) return rc;
        if (call.host())  // (what comes back is the keys routed, known only after the count pass)
            if (int rc = call.scratch(kt::AUX1, call.total * 8, &d_keys)) return rc;
        SegArgs a;
        if (int rc = make_seg_args(ctx, call.bases, call.offsets, n_reads, call.total, k, &a)) return rc;
        const uint32_t grid = grid_for(ctx, a.n_seg, 8);
        hipLaunchKernelGGL(route_count_kernel, dim3(grid), dim3(BLOCK), 0, ctx->stream, a, (uint32_t)n_owners, d_counts);
        hipLaunchKernelGGL(route_prefix_kernel, dim3(1), dim3(64), 0, ctx->stream, d_counts, (uint32_t)n_owners, d_cursors);
        hipLaunchKernelGGL(route_scatter_kernel, dim3(grid), dim3(BLOCK), 0, ctx->stream, a, (uint32_t)n_owners,
                           d_cursors, d_keys);
        KT_HIP(hipGetLastError());
    }
    if (mem == KT_MEM_DEVICE) {
        KT_HIP(hipMemcpyAsync(owner_counts, d_counts, n_owners * 8, hipMemcpyDeviceToDevice, ctx->stream));
        return KT_OK;
    }
    call.back(owner_counts, (const uint64_t *)d_counts, (uint64_t)n_owners);
    if (int rc = call.finish()) return rc;
    uint64_t n_keys = 0;
    for (int o = 0; o < n_owners; o++) n_keys += owner_counts[o];
    if (!n_keys) return KT_OK;
    call.back(keys_out, (const uint64_t *)d_keys, n_keys);
    return call.finish();
}

int kt_kmers(kt_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads, int k, uint64_t *fwd,
             uint64_t *rev, uint8_t *valid, int mem) {
    if (!ctx) return kt::fail(KT_ERR_ARG, "kt_kmers: null ctx");
    if (k < 1 || k > 31) return kt::fail(KT_ERR_ARG, "kt_kmers: k must be in 1..31");
    Call call(ctx, mem, "kt_kmers");
    if (int rc = call.enter()) return rc;
    if (n_reads == 0) return KT_OK;
    if (!offsets) return call.fail("null offsets");
    if (int rc = call.batch(bases, offsets, n_reads, nullptr)) return rc;
    const uint64_t total = call.total;
    if (total == 0) return KT_OK;
    if (!bases || !fwd || !rev || !valid) return call.fail("null buffer");
    if (int rc = call.stage()) return rc;
    uint64_t *d_fwd = fwd, *d_rev = rev;
    uint8_t *d_valid = valid;
    if (call.host()) {  // fwd | rev | valid in one buffer
        if (int rc = call.scratch(kt::OUT, total * 17, &d_fwd)) return rc;
        d_rev = d_fwd + total;
        d_valid = (uint8_t *)(d_rev + total);
        call.back(fwd, (const uint64_t *)d_fwd, total);
        call.back(rev, (const uint64_t *)d_rev, total);
        call.back(valid, (const uint8_t *)d_valid, total);
    }
    KT_HIP(hipMemsetAsync(d_valid, 0, total, ctx->stream));
    SegArgs a;
    if (int rc = make_seg_args(ctx, call.bases, call.offsets, n_reads, total, k, &a)) return rc;
    hipLaunchKernelGGL(kmers_kernel, dim3(grid_for(ctx, a.n_seg, 8)), dim3(BLOCK), 0, ctx->stream, a, d_fwd, d_rev,
                       d_valid);
    KT_HIP(hipGetLastError());
    return call.finish();
}

}  // extern "C"
